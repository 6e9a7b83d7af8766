// pcm.hip -- the PCM stage: the blocks the output gate lets travel, as 8 kHz or 16 kHz int16 or WAV-container IMA ADPCM.
//   airlame_init                      in WAVE_RATE 16000, out MP3_RATE 8000                 src/output.cpp:147-171
//   lame_encode_buffer_ieee_float     what the reference does with a travelling batch       src/output.cpp:478, :534
// MP3 stays with the host; this is the arithmetic whose every byte can be defined.  The filter, the quantiser, the encoder step and
// the state blob are in include/mi_airband.h.  A post-stage of its own like the gate and the splitter: two launches on the caller's
// stream, no atomics.  It reads the gate's index and counts where the gate left them, in device memory.  mi_pcm_plan_host
// (poststage_host.cpp) is the host twin.  The handle's base and the bodies of the entry points every stage repeats are in
// poststage.hpp, the lead's load and the tails kernel in carry.hpp.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "../../include/mi_airband.h"
#include "carry.hpp"
#include "poststage.hpp"

constexpr char kName[] = "PCM stage";

struct mi_pcm : mi::RowStage {
    mi_pcm() : RowStage(kName, 2) {}
    uint32_t max_blocks = 0;
    mi::PcmGeometry geo{};
    mi::PcmLiveTaps taps{};
    mi::DevBuf<mi::PcmRowState> d_state;    // [rows]: the checkpoint blob as it is
    mi::PinnedBuf<uint32_t> h_count;        // [2], landing place of the counts in mi_pcm_download
    // what the last mi_pcm_process_device was given (what mi_pcm_download reads)
    const void* last_out = nullptr;
    const uint32_t* last_count = nullptr;
};

namespace {

using mi::aligned;
using mi::as_flags;
using mi::fail;
constexpr int kThreads = 256;
constexpr int kBatch = mi::kWaveBatch;        // 2000 floats = 500 float4
constexpr int kLead = 64;                     // floats loaded in front of the block: the 62 of the history behind two that are not used
constexpr int kHalf = (kLead + kBatch) / 2;   // 1032 even and as many odd samples
constexpr int kImaS = MI_PCM_IMA_SAMPLES, kImaB = MI_PCM_IMA_BYTES;
static_assert((kLead + kBatch) % 4 == 0, "what is loaded is whole float4s");
static_assert(kBatch / kImaS <= kThreads && kImaB == 16 && (kImaS - 1) % 8 == 0, "one lane per sub-block, one uint4 each");

__constant__ int kStepTable[mi::kImaSteps] = {
    7,     8,     9,     10,    11,    12,    13,    14,    16,    17,    19,    21,    23,    25,    28,    31,    34,    37,
    41,    45,    50,    55,    60,    66,    73,    80,    88,    97,    107,   118,   130,   143,   157,   173,   190,   209,
    230,   253,   279,   307,   337,   371,   408,   449,   494,   544,   598,   658,   724,   796,   876,   963,   1060,  1166,
    1282,  1411,  1552,  1707,  1878,  2066,  2272,  2499,  2749,  3024,  3327,  3660,  4026,  4428,  4871,  5358,  5894,  6484,
    7132,  7845,  8630,  9493,  10442, 11487, 12635, 13899, 15289, 16818, 18500, 20350, 22385, 24623, 27086, 29794, 32767};

__device__ __forceinline__ int quantise(const float y) {
    float v = __fmul_rn(y, 32767.0f);
    v = fminf(fmaxf(v, -32767.0f), 32767.0f);
    return static_cast<int>(rintf(v));  // v_rndne_f32: to nearest, ties to even
}

__device__ __forceinline__ uint32_t pack2(const int a, const int b) {
    return (static_cast<uint32_t>(a) & 0xFFFFu) | (static_cast<uint32_t>(b) << 16);
}

// One sub-block by one lane: the 25 samples out of LDS, the 24-step recurrence, 16 bytes as one uint4.
__device__ __forceinline__ uint4 ima_subblock(const int16_t* __restrict__ s, const int* __restrict__ steps) {
    const int s0 = s[0], s1 = s[1];
    const int d4 = 4 * (s1 > s0 ? s1 - s0 : s0 - s1);
    int index = 0;  // the steps ascend: the smallest i with 7 T[i] >= 4 d is the number of steps below that
    for (int i = 0; i < mi::kImaSteps; ++i)
        index += 7 * steps[i] < d4 ? 1 : 0;
    index = index > mi::kImaSteps - 1 ? mi::kImaSteps - 1 : index;
    uint32_t w[4] = {(static_cast<uint32_t>(s0) & 0xFFFFu) | (static_cast<uint32_t>(index) << 16), 0u, 0u, 0u};
    int p = s0;
#pragma unroll
    for (int n = 0; n < kImaS - 1; ++n) {
        int step = steps[index], diff = s[n + 1] - p;
        const bool neg = diff < 0;
        diff = neg ? -diff : diff;
        int vp = step >> 3, code = 0;
        if (diff >= step) {
            code = 4;
            diff -= step;
            vp += step;
        }
        step >>= 1;
        if (diff >= step) {
            code |= 2;
            diff -= step;
            vp += step;
        }
        step >>= 1;
        if (diff >= step) {
            code |= 1;
            vp += step;
        }
        p = neg ? p - vp : p + vp;
        p = p < -32768 ? -32768 : (p > 32767 ? 32767 : p);
        index += code < 4 ? -1 : 2 * (code - 3);
        index = index < 0 ? 0 : (index > mi::kImaSteps - 1 ? mi::kImaSteps - 1 : index);
        w[1 + n / 8] |= static_cast<uint32_t>(code | (neg ? 8 : 0)) << (4 * (n % 8));  // the earlier sample in the low nibble
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// Launch 1.  One workgroup per block k of the index (a workgroup strides on where the grid is shorter than the count).  kDecimate: the
// block's 500 float4 and the 16 in front of them -- out of the row's previous batch, or the carried samples at batch 0 -- go into
// LDS split into even and odd samples, so that the lanes' reads of one tap are consecutive words; thread t sums outputs t, t + 256,
// ... over the 33 taps that are not exactly zero, in the order of the definition.  Otherwise a thread quantises its float4 as it
// comes.  The int16 samples meet in LDS; from there they leave as uint4, or lanes 0 .. S / 25 - 1 run one sub-block each.
template <bool kDecimate, bool kIma>
__global__ __launch_bounds__(kThreads) void k_pcm_encode(const float* __restrict__ wave, const size_t row_stride, const uint32_t rows, const uint32_t nbatches,
                                                         const mi_gate_block* __restrict__ index, const uint32_t* __restrict__ count,
                                                         const uint32_t max_blocks, const mi::PcmRowState* __restrict__ state, const mi::PcmLiveTaps taps,
                                                         uint4* __restrict__ out) {
    constexpr int kS = kDecimate ? kBatch / 2 : kBatch;
    constexpr int kOut4 = kIma ? kS / kImaS : kS / 8;  // uint4 of one encoded block
    __shared__ float ev[kDecimate ? kHalf : 2], od[kDecimate ? kHalf : 2];
    __shared__ __align__(16) int16_t s16[kS];
    __shared__ int steps[kIma ? mi::kImaSteps : 1];
    const int t = threadIdx.x;
    if (kIma && t < mi::kImaSteps)
        steps[t] = kStepTable[t];
    const uint32_t stored = count[1], limit = stored < max_blocks ? stored : max_blocks;
    for (uint32_t k = blockIdx.x; k < limit; k += gridDim.x) {  // (the same trips for the whole workgroup)
        const uint2 e = *reinterpret_cast<const uint2*>(index + k);
        const uint32_t row = e.x, batch = e.y;
        uint4* const dst = out + static_cast<size_t>(k) * kOut4;
        if (row >= rows || batch >= nbatches) {  // (the whole workgroup) not an entry of this call: a zero block, nothing read
            if (t < kOut4)
                dst[t] = make_uint4(0u, 0u, 0u, 0u);
            continue;
        }
        const float* const blk = wave + static_cast<size_t>(row) * row_stride + static_cast<size_t>(batch) * kBatch;
        if (kDecimate) {
            for (int q = t; q < (kLead + kBatch) / 4; q += kThreads) {
                const float4 v = mi::load_lead4<kLead>(blk, state[row], q, batch == 0);
                *reinterpret_cast<float2*>(ev + 2 * q) = make_float2(v.x, v.z);
                *reinterpret_cast<float2*>(od + 2 * q) = make_float2(v.y, v.w);
            }
            __syncthreads();
            for (int m = t; m < kS; m += kThreads) {
                // sample 2m - k of the block is float kLead + 2m - k of what was loaded: even k = 2j reads ev[32 + m - j], k = 31 od[16 + m]
                const float* const x = ev + kLead / 2 + m;
                float y = 0.0f;
#pragma unroll
                for (int j = 0; j < 16; ++j)
                    y = __fadd_rn(y, __fmul_rn(taps.h[j], x[-j]));
                y = __fadd_rn(y, __fmul_rn(taps.h[16], od[kLead / 2 - 16 + m]));
#pragma unroll
                for (int j = 16; j < 32; ++j)
                    y = __fadd_rn(y, __fmul_rn(taps.h[j + 1], x[-j]));
                s16[m] = static_cast<int16_t>(quantise(y));
            }
        } else {
            for (int q = t; q < kBatch / 4; q += kThreads) {
                const float4 v = reinterpret_cast<const float4*>(blk)[q];
                *reinterpret_cast<uint2*>(s16 + 4 * q) = make_uint2(pack2(quantise(v.x), quantise(v.y)), pack2(quantise(v.z), quantise(v.w)));
            }
        }
        __syncthreads();
        if (t < kOut4)
            dst[t] = kIma ? ima_subblock(s16 + kImaS * t, steps) : reinterpret_cast<const uint4*>(s16)[t];
        __syncthreads();  // (the next trip writes the LDS this one read)
    }
}

// Launch 2.  mi::k_carry_tails (carry.hpp): the last 62 samples of the call are an enabled row's new carried samples.

template <bool kDecimate, bool kIma>
void launch_encode(const mi_pcm* p, hipStream_t q, unsigned grid, const float* d_waveout, size_t row_stride, int nbatches, const mi_gate_block* d_index,
                   const uint32_t* d_count, void* d_out) {
    hipLaunchKernelGGL((k_pcm_encode<kDecimate, kIma>), dim3(grid), dim3(kThreads), 0, q, d_waveout, row_stride, static_cast<uint32_t>(p->rows),
                       static_cast<uint32_t>(nbatches), d_index, d_count, p->max_blocks, p->d_state.get(), p->taps, static_cast<uint4*>(d_out));
}

}  // namespace

extern "C" {

int mi_pcm_create(const mi_pcm_cfg* cfg, const uint8_t* row_enabled, int rows, int max_batches, size_t max_blocks, int gpu, mi_pcm** out) {
    if (!row_enabled || !out)
        return fail(MI_ERR_INVALID, "NULL argument");
    mi::PcmGeometry geo;
    if (const int rc = mi::pcm_geometry(cfg, &geo))
        return rc;
    if (const int rc = mi::batch_geometry_ok(kName, rows, max_batches))
        return rc;
    if (const int rc = mi::check_gpu(gpu, "no HIP device: the PCM stage runs on the GPU only"))
        return rc;
    mi_pcm* p = new mi_pcm();
    p->gpu = gpu;
    p->rows = rows;
    p->max_batches = max_batches;
    p->geo = geo;
    p->taps = mi::pcm_live_taps();
    const size_t n = static_cast<size_t>(rows), all = n * static_cast<size_t>(max_batches);
    p->max_blocks = static_cast<uint32_t>(max_blocks && max_blocks < all ? max_blocks : all);  // (the gate stores no more blocks than `all`)
    if (hipSetDevice(gpu) != hipSuccess || dalloc_copy(p->d_enabled, as_flags(row_enabled, n)) != hipSuccess || dalloc_zero(p->d_state, n) != hipSuccess ||
        hipHostMalloc(reinterpret_cast<void**>(p->h_count.put()), 2 * sizeof(uint32_t)) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
        delete p;
        return fail(MI_ERR_HIP, "PCM stage: device allocation failed");
    }
    *out = p;
    return MI_OK;
}

void mi_pcm_destroy(mi_pcm* p) {
    mi::destroy(p);
}

int mi_pcm_set_rows(mi_pcm* p, const uint8_t* row_enabled) {
    return mi::set_enabled(kName, p, row_enabled);
}

int mi_pcm_process_device(mi_pcm* p, const float* d_waveout, size_t row_stride, int nbatches, const mi_gate_block* d_index, const uint32_t* d_count,
                          void* d_out, void* hip_stream) {
    if (!p || !d_waveout || !d_index || !d_count || !d_out)
        return fail(MI_ERR_INVALID, "NULL argument");
    if (nbatches < 1 || nbatches > p->max_batches)
        return fail(MI_ERR_INVALID, "nbatches outside 1 .. max_batches");
    if (row_stride < static_cast<size_t>(nbatches) * mi::kWaveBatch)
        return fail(MI_ERR_INVALID, "a row stride is shorter than the call");
    if (row_stride % 4 != 0 || !aligned(d_waveout, 16) || !aligned(d_index, 8) || !aligned(d_count, 4) || !aligned(d_out, 16))
        return fail(MI_ERR_INVALID,
                    "the audio buffer and the output must be 16-byte aligned with a row stride that is a multiple of 4 floats; the index 8-byte aligned");
    if (hipSetDevice(p->gpu) != hipSuccess)
        return fail(MI_ERR_HIP, "hipSetDevice failed");
    hipStream_t q = static_cast<hipStream_t>(hip_stream);
    const unsigned rows = static_cast<unsigned>(p->rows);
    const uint64_t call = static_cast<uint64_t>(rows) * static_cast<uint64_t>(nbatches);  // the most blocks a gate stores in this call
    const unsigned grid = static_cast<unsigned>(call < p->max_blocks ? call : p->max_blocks);
    const bool decimate = p->geo.rate == 8000, ima = p->geo.format == MI_PCM_IMA4;
    p->timing.stamp(0, q);
    if (decimate && ima)
        launch_encode<true, true>(p, q, grid, d_waveout, row_stride, nbatches, d_index, d_count, d_out);
    else if (decimate)
        launch_encode<true, false>(p, q, grid, d_waveout, row_stride, nbatches, d_index, d_count, d_out);
    else if (ima)
        launch_encode<false, true>(p, q, grid, d_waveout, row_stride, nbatches, d_index, d_count, d_out);
    else
        launch_encode<false, false>(p, q, grid, d_waveout, row_stride, nbatches, d_index, d_count, d_out);
    p->timing.stamp(1, q);
    mi::launch_carry_tails<MI_PCM_HISTORY>(q, p->d_enabled.get(), d_waveout, row_stride, rows, nbatches, p->d_state.get());
    p->timing.stamp(2, q);
    if (hipGetLastError() != hipSuccess)
        return fail(MI_ERR_HIP, "PCM stage kernel launch failed");
    p->called = true;
    p->last_out = d_out;
    p->last_count = d_count;
    return MI_OK;
}

int mi_pcm_download(mi_pcm* p, void* hip_stream, void* out, uint32_t* count) {
    if (!p || !count)
        return fail(MI_ERR_INVALID, "NULL argument");
    if (!p->last_count)
        return fail(MI_ERR_INVALID, "no mi_pcm_process_device call to download");
    hipStream_t q = static_cast<hipStream_t>(hip_stream);
    if (!mi::land_counts(p->gpu, q, p->h_count, p->last_count, count))
        return fail(MI_ERR_HIP, "PCM stage: reading the counts failed");
    count[1] = count[1] < p->max_blocks ? count[1] : p->max_blocks;
    const size_t k = count[1];
    if (out && k &&
        (hipMemcpyAsync(out, p->last_out, k * p->geo.block_bytes, hipMemcpyDeviceToHost, q) != hipSuccess || hipStreamSynchronize(q) != hipSuccess))
        return fail(MI_ERR_HIP, "PCM stage: download failed");
    return MI_OK;
}

int mi_pcm_set_timing(mi_pcm* p, int on) {
    return mi::set_timing(p, on);
}

int mi_pcm_last_launch_ms(mi_pcm* p, float* ms) {
    return mi::last_launch_ms(p, ms, "mi_pcm_process_device");
}

size_t mi_pcm_state_size(const mi_pcm* p) {
    return mi::state_size(p, &mi_pcm::d_state);
}

int mi_pcm_get_state(mi_pcm* p, void* buf, size_t len) {
    return mi::get_state(kName, p, &mi_pcm::d_state, buf, len);
}

int mi_pcm_set_state(mi_pcm* p, const void* buf, size_t len) {
    return mi::set_state(kName, p, &mi_pcm::d_state, buf, len);
}

}  // extern "C"
