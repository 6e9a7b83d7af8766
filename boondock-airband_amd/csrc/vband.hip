// vband.hip -- the voice band stage: a per-row 511-tap highpass / lowpass FIR over the demodulator's audio.
//   highpass / lowpass keys           defaults 100 / 2500 Hz, checked                       src/config.cpp:327-328, :336-338
//   airlame_init                      lame_set_highpassfreq / lame_set_lowpassfreq          src/output.cpp:147-171
// The reference shapes the band inside its MP3 encoder; the device chain has none, so the two keys act here.  The taps, the order of
// the sum, the clamp and the state blob are in include/mi_airband.h.  A post-stage of its own like the PCM stage: two launches on
// the caller's stream, no atomics.  It writes a plane in the layout of the one it reads.  mi_vband_plan_host (poststage_host.cpp) is
// the host twin.  The handle's base and the bodies of the entry points every stage repeats are in poststage.hpp, the lead's load
// and the tails kernel in carry.hpp.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "../../include/mi_airband.h"
#include "carry.hpp"
#include "poststage.hpp"

constexpr char kName[] = "voice band stage";

struct mi_vband : mi::RowStage {
    mi_vband() : RowStage(kName, 2) {}
    size_t classes_cap = 0;                  // classes d_taps has room for
    mi::DevBuf<uint32_t> d_class;            // [rows]: the row's class of settings
    mi::DevBuf<float> d_taps;                // [classes][512]: the 511 taps of a class and a zero
    mi::DevBuf<mi::VbandRowState> d_state;   // [rows]: the checkpoint blob as it is
};

namespace {

using mi::as_flags;
using mi::fail;
constexpr int kThreads = 256;
constexpr int kBatch = mi::kWaveBatch;   // 2000 floats = 500 float4
constexpr int kTaps = MI_VBAND_TAPS;     // 511
constexpr int kLead = 512;               // floats staged in front of the block: two that are not used, then the 510 of the history
constexpr int kRun = 8;                  // consecutive outputs of one thread
constexpr int kOwners = kBatch / kRun;   // 250 threads own outputs
constexpr int kChunks = kTaps / kRun;    // 63 whole chunks of 8 taps; 7 taps behind them
constexpr unsigned kMaxGrid = 2048;      // 8 workgroups on each of 256 CUs; a workgroup strides on from there
static_assert(kLead % 8 == 0 && kBatch % kRun == 0 && kOwners <= kThreads && kRun == 8, "a thread's run is two float4");
static_assert(kLead - kRun * (kChunks + 1) >= 0 && kTaps - kRun * kChunks == 7 && mi::kVbandTapRow == 512 && kChunks % 2 == 1,
              "the last chunk's window begins at the lead's first float");
static_assert(mi::kVbandTapRow / 4 <= kThreads && MI_VBAND_HISTORY <= 2 * kThreads, "one float4 of taps per lane; the tails in two trips");

// Taps 8m .. 8m + kN - 1 into the eight running sums: output j takes sample 8 + j - i of the sixteen in {lo, hi} for tap i, which is
// x[n_j - (8m + i)].  Every product and every sum rounds on its own, and a sum's taps come in ascending order.
template <int kN>
__device__ __forceinline__ void chunk(float (&acc)[kRun], const float* __restrict__ h, const float4 lo0, const float4 lo1, const float4 hi0, const float4 hi1) {
    const float w[2 * kRun] = {lo0.x, lo0.y, lo0.z, lo0.w, lo1.x, lo1.y, lo1.z, lo1.w, hi0.x, hi0.y, hi0.z, hi0.w, hi1.x, hi1.y, hi1.z, hi1.w};
    const float4 t0 = reinterpret_cast<const float4*>(h)[0], t1 = reinterpret_cast<const float4*>(h)[1];  // (one address for the whole wave)
    const float tap[kRun] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w};
#pragma unroll
    for (int i = 0; i < kN; ++i)
#pragma unroll
        for (int j = 0; j < kRun; ++j)
            acc[j] = __fadd_rn(acc[j], __fmul_rn(tap[i], w[kRun + j - i]));
}

// Launch 1.  One workgroup per block (row, batch) of an enabled row (a workgroup strides on where the grid is shorter).  The class's
// 512 tap floats and the block's 2000 samples behind the 512 in front of them -- out of the row's previous batch, or the carried
// samples at batch 0 -- go into LDS.  Thread t < 250 owns outputs 8t .. 8t + 7: it keeps sixteen consecutive samples in registers,
// takes eight taps at a time and slides the window down by eight, so two float4 of samples and two of taps feed 64 products.  Where
// every staged sample compares equal to zero the sums are +0.0f whatever the taps, and the workgroup writes that.
__global__ __launch_bounds__(kThreads) void k_vband_filter(const uint8_t* __restrict__ enabled, const uint32_t* __restrict__ class_of,
                                                           const float* __restrict__ taps, const float* __restrict__ wave, const size_t row_stride,
                                                           const uint32_t rows, const uint32_t nbatches, const mi::VbandRowState* __restrict__ state,
                                                           float* __restrict__ out, const size_t out_stride) {
    __shared__ __align__(16) float xs[kLead + kBatch];
    __shared__ __align__(16) float hs[mi::kVbandTapRow];
    const int t = threadIdx.x;
    const uint32_t total = rows * nbatches;  // (below 2^24)
    for (uint32_t k = blockIdx.x; k < total; k += gridDim.x) {  // (the same trips for the whole workgroup)
        const uint32_t row = k / nbatches, batch = k - row * nbatches;
        if (!enabled[row])  // (the whole workgroup)
            continue;
        const float* const blk = wave + static_cast<size_t>(row) * row_stride + static_cast<size_t>(batch) * kBatch;
        float4* const dst = reinterpret_cast<float4*>(out + static_cast<size_t>(row) * out_stride + static_cast<size_t>(batch) * kBatch);
        if (t < mi::kVbandTapRow / 4)
            reinterpret_cast<float4*>(hs)[t] = reinterpret_cast<const float4*>(taps + static_cast<size_t>(class_of[row]) * mi::kVbandTapRow)[t];
        int live = 0;
        for (int q = t; q < (kLead + kBatch) / 4; q += kThreads) {
            float4 v = mi::load_lead4<kLead>(blk, state[row], q, batch == 0);
            if (q == 0)  // (no output reaches the lead's first two floats)
                v.x = v.y = 0.0f;
            live |= (v.x != 0.0f || v.y != 0.0f || v.z != 0.0f || v.w != 0.0f) ? 1 : 0;
            reinterpret_cast<float4*>(xs)[q] = v;
        }
        if (!__syncthreads_or(live)) {  // (the whole workgroup; the barrier is the one behind the staging)
            for (int q = t; q < kBatch / 4; q += kThreads)
                dst[q] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            continue;  // (nothing read the LDS: the next trip may write it)
        }
        if (t < kOwners) {
            float acc[kRun] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
            // x[n_j - k] for output j and tap k is xs[kLead + 8t + j - k]; chunk m's sixteen begin at p - 8m
            const float4* p = reinterpret_cast<const float4*>(xs + kLead + kRun * t - kRun);
            float4 a0 = p[2], a1 = p[3], b0 = p[0], b1 = p[1];
#pragma unroll 1
            for (int m = 0; m < kChunks - 1; m += 2) {
                chunk<kRun>(acc, hs + kRun * m, b0, b1, a0, a1);
                a0 = p[-2], a1 = p[-1];
                chunk<kRun>(acc, hs + kRun * m + kRun, a0, a1, b0, b1);
                b0 = p[-4], b1 = p[-3];
                p -= 4;
            }
            chunk<kRun>(acc, hs + kRun * (kChunks - 1), b0, b1, a0, a1);
            a0 = p[-2], a1 = p[-1];  // (t = 0: the lead's first eight floats)
            chunk<kTaps - kRun * kChunks>(acc, hs + kRun * kChunks, a0, a1, b0, b1);
#pragma unroll
            for (int j = 0; j < kRun; ++j)
                acc[j] = fminf(fmaxf(acc[j], -1.0f), 1.0f);
            dst[2 * t] = make_float4(acc[0], acc[1], acc[2], acc[3]);
            dst[2 * t + 1] = make_float4(acc[4], acc[5], acc[6], acc[7]);
        }
        __syncthreads();  // (the next trip writes the LDS this one read)
    }
}

// Launch 2.  mi::k_carry_tails (carry.hpp): the last 510 input samples of the call are an enabled row's new carried samples.

// the classes' taps and the rows' classes onto the device (the caller has completed queued work where a call may read them)
int upload_settings(mi_vband* v, const std::vector<uint32_t>& class_of, const std::vector<mi_vband_row>& classes) {
    std::vector<float> table(classes.size() * mi::kVbandTapRow, 0.0f);
    for (size_t c = 0; c < classes.size(); ++c)
        mi::vband_taps(classes[c], table.data() + c * mi::kVbandTapRow);
    if (classes.size() > v->classes_cap) {
        if (dalloc_copy(v->d_taps, table) != hipSuccess)
            return fail(MI_ERR_HIP, "voice band stage: device allocation failed");
        v->classes_cap = classes.size();
    } else if (hipMemcpy(v->d_taps.get(), table.data(), table.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
        return fail(MI_ERR_HIP, "voice band stage: uploading the rows failed");
    }
    if (hipMemcpy(v->d_class.get(), class_of.data(), class_of.size() * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess)
        return fail(MI_ERR_HIP, "voice band stage: uploading the rows failed");
    return MI_OK;
}

}  // namespace

extern "C" {

int mi_vband_create(const mi_vband_row* row_cfg, const uint8_t* row_enabled, int rows, int max_batches, int gpu, mi_vband** out) {
    if (!row_enabled || !out)
        return fail(MI_ERR_INVALID, "NULL argument");
    if (const int rc = mi::batch_geometry_ok(kName, rows, max_batches))
        return rc;
    std::vector<uint32_t> class_of;
    std::vector<mi_vband_row> classes;
    const size_t n = static_cast<size_t>(rows);
    if (const int rc = mi::vband_classes(row_cfg, n, class_of, classes))
        return rc;
    if (const int rc = mi::check_gpu(gpu, "no HIP device: the voice band stage runs on the GPU only"))
        return rc;
    mi_vband* v = new mi_vband();
    v->gpu = gpu;
    v->rows = rows;
    v->max_batches = max_batches;
    if (hipSetDevice(gpu) != hipSuccess || dalloc_copy(v->d_enabled, as_flags(row_enabled, n)) != hipSuccess || dalloc_zero(v->d_state, n) != hipSuccess ||
        dalloc_zero(v->d_class, n) != hipSuccess || upload_settings(v, class_of, classes) != MI_OK || hipDeviceSynchronize() != hipSuccess) {
        delete v;
        return fail(MI_ERR_HIP, "voice band stage: device allocation failed");
    }
    *out = v;
    return MI_OK;
}

void mi_vband_destroy(mi_vband* v) {
    mi::destroy(v);
}

int mi_vband_set_rows(mi_vband* v, const mi_vband_row* row_cfg, const uint8_t* row_enabled) {
    if (!v || (!row_cfg && !row_enabled))
        return fail(MI_ERR_INVALID, "NULL argument");
    const size_t n = static_cast<size_t>(v->rows);
    std::vector<uint32_t> class_of;
    std::vector<mi_vband_row> classes;
    if (row_cfg)
        if (const int rc = mi::vband_classes(row_cfg, n, class_of, classes))
            return rc;
    // (a call still queued reads the rows and the taps it was made with)
    if (hipSetDevice(v->gpu) != hipSuccess || hipDeviceSynchronize() != hipSuccess)
        return fail(MI_ERR_HIP, "voice band stage: uploading the rows failed");
    if (row_cfg)
        if (const int rc = upload_settings(v, class_of, classes))
            return rc;
    if (row_enabled) {
        const std::vector<uint8_t> flags = as_flags(row_enabled, n);
        if (hipMemcpy(v->d_enabled.get(), flags.data(), flags.size(), hipMemcpyHostToDevice) != hipSuccess)
            return fail(MI_ERR_HIP, "voice band stage: uploading the rows failed");
    }
    return MI_OK;
}

int mi_vband_process_device(mi_vband* v, const float* d_waveout, size_t row_stride, int nbatches, float* d_out, size_t out_stride, void* hip_stream) {
    if (const int rc = mi::plane_call_ok(v, d_waveout, row_stride, nbatches, d_out, out_stride, "audio buffer"))
        return rc;
    if (hipSetDevice(v->gpu) != hipSuccess)
        return fail(MI_ERR_HIP, "hipSetDevice failed");
    hipStream_t q = static_cast<hipStream_t>(hip_stream);
    const unsigned rows = static_cast<unsigned>(v->rows), call = rows * static_cast<unsigned>(nbatches);
    v->timing.stamp(0, q);
    hipLaunchKernelGGL(k_vband_filter, dim3(call < kMaxGrid ? call : kMaxGrid), dim3(kThreads), 0, q, v->d_enabled.get(), v->d_class.get(), v->d_taps.get(),
                       d_waveout, row_stride, rows, static_cast<uint32_t>(nbatches), v->d_state.get(), d_out, out_stride);
    v->timing.stamp(1, q);
    mi::launch_carry_tails<MI_VBAND_HISTORY>(q, v->d_enabled.get(), d_waveout, row_stride, rows, nbatches, v->d_state.get());
    v->timing.stamp(2, q);
    if (hipGetLastError() != hipSuccess)
        return fail(MI_ERR_HIP, "voice band stage kernel launch failed");
    v->called = true;
    return MI_OK;
}

int mi_vband_set_timing(mi_vband* v, int on) {
    return mi::set_timing(v, on);
}

int mi_vband_last_launch_ms(mi_vband* v, float* ms) {
    return mi::last_launch_ms(v, ms, "mi_vband_process_device");
}

size_t mi_vband_state_size(const mi_vband* v) {
    return mi::state_size(v, &mi_vband::d_state);
}

int mi_vband_get_state(mi_vband* v, void* buf, size_t len) {
    return mi::get_state(kName, v, &mi_vband::d_state, buf, len);
}

int mi_vband_set_state(mi_vband* v, const void* buf, size_t len) {
    return mi::set_state(kName, v, &mi_vband::d_state, buf, len);
}

}  // extern "C"
