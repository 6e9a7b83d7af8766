// limit.hip -- the peak limiter stage: a per-row look-ahead gain that keeps the audio inside a ceiling without clipping it.
// Nothing else behind the demodulator does: the mixer adds its open inputs unclamped (the reference leaves that to LAME), ampfactor
// (src/config.cpp:623) is multiplied in before the demodulator's hard clamp, and the PCM stage's quantiser saturates.  The window
// maximum, the gain, the order of its 64-term mean, the clamp and the state blob are in include/mi_airband.h.  A post-stage like the
// voice band stage: two launches on the caller's stream, no atomics.  It writes a plane in the layout of the one it reads.
// mi_limit_plan_host (poststage_host.cpp) is the host twin.  The handle's base and the bodies of the entry points every stage repeats
// are in poststage.hpp, the tails kernel in carry.hpp (whose load of the lead k_limit restates: see there).
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "../../include/mi_airband.h"
#include "carry.hpp"
#include "poststage.hpp"

constexpr char kName[] = "limiter stage";

struct mi_limit : mi::RowStage {
    mi_limit() : RowStage(kName, 2) {}
    mi::DevBuf<mi_limit_row> d_cfg;          // [rows]
    mi::DevBuf<mi::LimitRowState> d_state;   // [rows]: the checkpoint blob as it is
};

namespace {

using mi::as_flags;
using mi::fail;
constexpr int kThreads = 256;
constexpr int kBatch = mi::kWaveBatch;        // 2000 floats = 500 float4
constexpr int kLook = MI_LIMIT_LOOKAHEAD;     // 63
constexpr int kLead = 1088;                   // floats staged in front of the block: two that are not used, then the 1086 of the history
constexpr int kStage = kLead + kBatch;        // 3088
constexpr int kTrips = (kStage + kThreads - 1) / kThreads;  // 13 staged values per thread in a doubling pass
constexpr int kFirst = kLead - kLook;         // 1025: the staged index of the sample output 0 carries, and of the first gain it adds
constexpr int kGains = kBatch + kLook;        // 2063 gains feed a block's outputs
constexpr int kRun = 8;                       // consecutive outputs of one thread
constexpr int kOwners = kBatch / kRun;        // 250 threads own outputs
constexpr unsigned kMaxGrid = 2048;           // 8 workgroups on each of 256 CUs; a workgroup strides on from there
static_assert(kLead >= MI_LIMIT_HISTORY && kLead - MI_LIMIT_HISTORY == 2 && kLead % 4 == 0 && kLead <= kBatch, "the lead is whole float4 inside the previous batch");
static_assert(kFirst - (MI_LIMIT_WINDOW - 1) == 2, "the oldest value a gain's window reaches is the lead's third float");
static_assert(kBatch % kRun == 0 && kOwners <= kThreads && kRun == 8 && (kLook + 1) % kRun == 0, "a thread's run is two float4, the 64 gains eight chunks");
static_assert(kRun * (kOwners - 1) + kLook + 2 * kRun == kGains + kRun && kGains + kRun <= kStage && kFirst + kGains == kStage,
              "the last owner's last sixteen end a float behind the gains, inside the array");
static_assert(MI_LIMIT_WINDOW == 1024, "ten doublings");

// Launch 1.  One workgroup per block (row, batch) of an enabled row (a workgroup strides on where the grid is shorter).  The block's
// 2000 samples behind the 1088 in front of them -- out of the row's previous batch, or the carried samples at batch 0 --, times the
// pregain, go into LDS as us[].  Where none of them is over the ceiling every gain is 1.0f and the block is us[] moved by 63.
// Otherwise ms[i] becomes the maximum of |us| over the 1024 values that end at i by ten doublings (windows of 1, 2, 4 .. 512 joined
// with the one that ends a window's width earlier; lane t works on i = t + 256 j, so both reads and the write have unit stride over
// the lanes and meet no bank twice); the last doubling writes the gain of staged index 1025 + j at ms[j], which puts an owner's
// windows on float4.  Thread t < 250 owns outputs 8t .. 8t + 7: it keeps sixteen consecutive gains in registers, adds eight to each
// of its sums and slides on by eight, every sum in the definition's order and none shared between outputs.
__global__ __launch_bounds__(kThreads) void k_limit(const uint8_t* __restrict__ enabled, const mi_limit_row* __restrict__ cfg, const float* __restrict__ wave,
                                                    const size_t row_stride, const uint32_t rows, const uint32_t nbatches,
                                                    const mi::LimitRowState* __restrict__ state, float* __restrict__ out, const size_t out_stride) {
    __shared__ __align__(16) float us[kStage];
    __shared__ __align__(16) float ms[kStage];
    const int t = threadIdx.x;
    const uint32_t total = rows * nbatches;  // (below 2^24)
    for (uint32_t k = blockIdx.x; k < total; k += gridDim.x) {  // (the same trips for the whole workgroup)
        const uint32_t row = k / nbatches, batch = k - row * nbatches;
        if (!enabled[row])  // (the whole workgroup)
            continue;
        const float pregain = cfg[row].pregain, ceiling = cfg[row].ceiling;
        const float* const blk = wave + static_cast<size_t>(row) * row_stride + static_cast<size_t>(batch) * kBatch;
        float4* const dst = reinterpret_cast<float4*>(out + static_cast<size_t>(row) * out_stride + static_cast<size_t>(batch) * kBatch);
        int over = 0;
        for (int q = t; q < kStage / 4; q += kThreads) {
            float4 v;  // (mi::load_lead4 of carry.hpp, kept as the stage had it: with the shared one the transparent path measured 2 % off)
            if (q >= kLead / 4 || batch != 0) {
                v = reinterpret_cast<const float4*>(blk - kLead)[q];
            } else {  // floats 4q .. 4q + 3 of the lead are carried samples 4q - 2 .. 4q + 1
                const float* const c = state[row].x + 4 * q;
                const float2 a = q ? *reinterpret_cast<const float2*>(c - 2) : make_float2(0.0f, 0.0f);
                const float2 b = *reinterpret_cast<const float2*>(c);
                v = make_float4(a.x, a.y, b.x, b.y);
            }
            if (q == 0)  // (no output reaches the lead's first two floats)
                v.x = v.y = 0.0f;
            v = make_float4(__fmul_rn(v.x, pregain), __fmul_rn(v.y, pregain), __fmul_rn(v.z, pregain), __fmul_rn(v.w, pregain));
            over |= (fabsf(v.x) > ceiling || fabsf(v.y) > ceiling || fabsf(v.z) > ceiling || fabsf(v.w) > ceiling) ? 1 : 0;
            reinterpret_cast<float4*>(us)[q] = v;
        }
        if (!__syncthreads_or(over)) {  // (the whole workgroup; the barrier is the one behind the staging)
            for (int q = t; q < kBatch / 4; q += kThreads) {
                const float* const u = us + kFirst + 4 * q;
                dst[q] = make_float4(u[0], u[1], u[2], u[3]);
            }
        } else {
            float v[kTrips];
#pragma unroll
            for (int j = 0; j < kTrips; ++j) {  // windows of 2 out of us[]
                const int i = t + kThreads * j;
                if (i < kStage)
                    ms[i] = fmaxf(fabsf(us[i]), i ? fabsf(us[i - 1]) : 0.0f);
            }
            __syncthreads();
#pragma unroll 1
            for (int w = 2; w < MI_LIMIT_WINDOW / 2; w *= 2) {  // windows of 4 .. 512 (shorter where the array begins: no output reads those)
#pragma unroll
                for (int j = 0; j < kTrips; ++j) {
                    const int i = t + kThreads * j;
                    if (i < kStage)
                        v[j] = i >= w ? fmaxf(ms[i], ms[i - w]) : ms[i];
                }
                __syncthreads();
#pragma unroll
                for (int j = 0; j < kTrips; ++j) {
                    const int i = t + kThreads * j;
                    if (i < kStage)
                        ms[i] = v[j];
                }
                __syncthreads();
            }
#pragma unroll
            for (int j = 0; j < kTrips; ++j) {  // windows of 1024, and their gains
                const int i = t + kThreads * j;
                if (i >= kFirst && i < kStage) {
                    const float p = fmaxf(ms[i], ms[i - MI_LIMIT_WINDOW / 2]);
                    v[j] = p > ceiling ? __fdiv_rn(ceiling, p) : 1.0f;
                }
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < kTrips; ++j) {
                const int i = t + kThreads * j;
                if (i >= kFirst && i < kStage)
                    ms[i - kFirst] = v[j];
            }
            __syncthreads();
            if (t < kOwners) {
                float acc[kRun] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
                // the gain of sample n - 63 + m, output n's m-th, is ms[n + m]; chunk c's sixteen begin at ms[8t + 8c]
                const float4* p = reinterpret_cast<const float4*>(ms + kRun * t);
                float4 lo0 = p[0], lo1 = p[1];
#pragma unroll
                for (int c = 0; c < (kLook + 1) / kRun; ++c) {
                    const float4 hi0 = p[2], hi1 = p[3];  // (the last chunk's hi1 reaches a float behind the gains; its last float is not used)
                    const float g[2 * kRun] = {lo0.x, lo0.y, lo0.z, lo0.w, lo1.x, lo1.y, lo1.z, lo1.w, hi0.x, hi0.y, hi0.z, hi0.w, hi1.x, hi1.y, hi1.z, hi1.w};
#pragma unroll
                    for (int i = 0; i < kRun; ++i)
#pragma unroll
                        for (int j = 0; j < kRun; ++j)
                            acc[j] = __fadd_rn(acc[j], g[i + j]);
                    lo0 = hi0, lo1 = hi1;
                    p += 2;
                }
                const float* const u = us + kFirst + kRun * t;
#pragma unroll
                for (int j = 0; j < kRun; ++j) {
                    const float y = __fmul_rn(u[j], __fmul_rn(acc[j], 0.015625f));
                    acc[j] = fminf(fmaxf(y, -ceiling), ceiling);
                }
                dst[2 * t] = make_float4(acc[0], acc[1], acc[2], acc[3]);
                dst[2 * t + 1] = make_float4(acc[4], acc[5], acc[6], acc[7]);
            }
        }
        __syncthreads();  // (the next trip writes the LDS this one read)
    }
}

// Launch 2.  mi::k_carry_tails (carry.hpp): the last 1086 input samples of the call are an enabled row's new carried samples.

}  // namespace

extern "C" {

int mi_limit_create(const mi_limit_row* row_cfg, const uint8_t* row_enabled, int rows, int max_batches, int gpu, mi_limit** out) {
    if (!row_enabled || !out)
        return fail(MI_ERR_INVALID, "NULL argument");
    if (const int rc = mi::batch_geometry_ok(kName, rows, max_batches))
        return rc;
    const size_t n = static_cast<size_t>(rows);
    std::vector<mi_limit_row> cfg;
    if (const int rc = mi::limit_rows(row_cfg, n, cfg))
        return rc;
    if (const int rc = mi::check_gpu(gpu, "no HIP device: the limiter stage runs on the GPU only"))
        return rc;
    mi_limit* l = new mi_limit();
    l->gpu = gpu;
    l->rows = rows;
    l->max_batches = max_batches;
    if (hipSetDevice(gpu) != hipSuccess || dalloc_copy(l->d_enabled, as_flags(row_enabled, n)) != hipSuccess || dalloc_zero(l->d_state, n) != hipSuccess ||
        dalloc_copy(l->d_cfg, cfg) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
        delete l;
        return fail(MI_ERR_HIP, "limiter stage: device allocation failed");
    }
    *out = l;
    return MI_OK;
}

void mi_limit_destroy(mi_limit* l) {
    mi::destroy(l);
}

int mi_limit_set_rows(mi_limit* l, const mi_limit_row* row_cfg, const uint8_t* row_enabled) {
    if (!l || (!row_cfg && !row_enabled))
        return fail(MI_ERR_INVALID, "NULL argument");
    const size_t n = static_cast<size_t>(l->rows);
    std::vector<mi_limit_row> cfg;
    if (row_cfg)
        if (const int rc = mi::limit_rows(row_cfg, n, cfg))
            return rc;
    // (a call still queued reads the rows and the settings it was made with)
    if (hipSetDevice(l->gpu) != hipSuccess || hipDeviceSynchronize() != hipSuccess)
        return fail(MI_ERR_HIP, "limiter stage: uploading the rows failed");
    if (row_cfg && hipMemcpy(l->d_cfg.get(), cfg.data(), n * sizeof(mi_limit_row), hipMemcpyHostToDevice) != hipSuccess)
        return fail(MI_ERR_HIP, "limiter stage: uploading the rows failed");
    if (row_enabled) {
        const std::vector<uint8_t> flags = as_flags(row_enabled, n);
        if (hipMemcpy(l->d_enabled.get(), flags.data(), flags.size(), hipMemcpyHostToDevice) != hipSuccess)
            return fail(MI_ERR_HIP, "limiter stage: uploading the rows failed");
    }
    return MI_OK;
}

int mi_limit_process_device(mi_limit* l, const float* d_in, size_t row_stride, int nbatches, float* d_out, size_t out_stride, void* hip_stream) {
    if (const int rc = mi::plane_call_ok(l, d_in, row_stride, nbatches, d_out, out_stride, "input plane"))
        return rc;
    if (hipSetDevice(l->gpu) != hipSuccess)
        return fail(MI_ERR_HIP, "hipSetDevice failed");
    hipStream_t q = static_cast<hipStream_t>(hip_stream);
    const unsigned rows = static_cast<unsigned>(l->rows), call = rows * static_cast<unsigned>(nbatches);
    l->timing.stamp(0, q);
    hipLaunchKernelGGL(k_limit, dim3(call < kMaxGrid ? call : kMaxGrid), dim3(kThreads), 0, q, l->d_enabled.get(), l->d_cfg.get(), d_in, row_stride, rows,
                       static_cast<uint32_t>(nbatches), l->d_state.get(), d_out, out_stride);
    l->timing.stamp(1, q);
    mi::launch_carry_tails<MI_LIMIT_HISTORY>(q, l->d_enabled.get(), d_in, row_stride, rows, nbatches, l->d_state.get());
    l->timing.stamp(2, q);
    if (hipGetLastError() != hipSuccess)
        return fail(MI_ERR_HIP, "limiter stage kernel launch failed");
    l->called = true;
    return MI_OK;
}

int mi_limit_set_timing(mi_limit* l, int on) {
    return mi::set_timing(l, on);
}

int mi_limit_last_launch_ms(mi_limit* l, float* ms) {
    return mi::last_launch_ms(l, ms, "mi_limit_process_device");
}

size_t mi_limit_state_size(const mi_limit* l) {
    return mi::state_size(l, &mi_limit::d_state);
}

int mi_limit_get_state(mi_limit* l, void* buf, size_t len) {
    return mi::get_state(kName, l, &mi_limit::d_state, buf, len);
}

int mi_limit_set_state(mi_limit* l, const void* buf, size_t len) {
    return mi::set_state(kName, l, &mi_limit::d_state, buf, len);
}

}  // extern "C"
