// denoise.hip -- the noise reduction stage: a spectral gate per row over a plane of audio.  512-point spectra of 500-sample frames at a
// hop of 250, a noise floor per bin from the minima of the row's last eight batches, a gain per frame and bin, the conjugate
// transform and the overlap-add.  The reference has nothing of the kind: it hands waveout to LAME as it is (src/output.cpp:147-171).
// The frames, the order of every sum, the gain, the clamp and the state blob are in include/mi_airband.h.  A post-stage of its own
// like the voice band stage: three launches on the caller's stream, no atomics.  It writes a plane in the layout of the one it reads.
// mi_denoise_plan_host (poststage_host.cpp) is the host twin.  The handle's base and the bodies of the entry points every stage
// repeats are in poststage.hpp, the passes of the transform in fft_radix8.hpp.
//
// Compile with -ffp-contract=off (the FFT spec).
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

#include "../../include/mi_airband.h"
#include "fft_radix8.hpp"
#include "poststage.hpp"

constexpr char kName[] = "noise reduction stage";

struct mi_denoise : mi::RowStage {
    mi_denoise() : RowStage(kName, 3) {}
    mi::DevBuf<mi::DenoiseGains> d_cfg;        // [rows]
    mi::DevBuf<float> d_window;                // [500]
    mi::DevBuf<float> d_tw;                    // [256] x {re, im}
    mi::DevBuf<float> d_floor;                 // [rows][max_batches][257]: M of the call's blocks
    mi::DevBuf<mi::DenoiseRowState> d_state;   // [rows]: the checkpoint blob as it is
};

namespace mi {
namespace {

constexpr int kL = MI_DENOISE_FFT_LOG;
using Gm = FftGeom<kL>;
constexpr int kBatch = kWaveBatch;             // 2000 floats = 500 float4
constexpr int kHop = MI_DENOISE_HOP, kFrame = MI_DENOISE_FRAME, kN = MI_DENOISE_FFT, kBins = MI_DENOISE_BINS, kDepth = MI_DENOISE_DEPTH;
constexpr int kFrames = kBatch / kHop + 1;     // 9 frames make a block: one wave each
constexpr int kThreads = 64 * kFrames;         // 576
constexpr int kStaged = kFrame + kBatch;       // the block behind the 500 samples before it
constexpr int kBinRow = 260;                   // floats of one frame's row of P or S
constexpr unsigned kMaxGrid = 512;             // two workgroups (about 62 KB of LDS each) on each of 256 CUs; a workgroup strides on from there
static_assert(Gm::TPF == 64 && Gm::NPASS == 3 && kStaged % 4 == 0 && kFrame % 4 == 0 && kBatch / 4 <= kThreads && kBins <= kThreads && kBins <= kBinRow &&
                  kBins == 4 * 64 + 1 && kFrames * kBinRow <= kStaged,
              "one wave per transform, 64 lanes x 8 points; a lane forms P of four bins and lane 0 of bin 256 as well");

// What a lane keeps for every transform it takes part in.
struct Lane {
    int nidx[8];               // bitrev_9(8 tau + r): where the lane's 8 inputs lie
    float w[8];                // the window there, 0.0f from 500 on
    float2 w8, w83;
    float2 twr[Gm::NPASS][7];
};

__device__ __forceinline__ void lane_setup(Lane& l, const int tau, const float* __restrict__ window, const float* __restrict__ twf) {
    const int nrev = static_cast<int>(__brev(static_cast<unsigned>(tau)) >> (32 - (kL - 3)));
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int rev3 = ((r & 1) << 2) | (r & 2) | ((r >> 2) & 1);
        l.nidx[r] = rev3 * Gm::TPF + nrev;
        l.w[r] = l.nidx[r] < kFrame ? window[l.nidx[r]] : 0.0f;
    }
    const float2* tw = reinterpret_cast<const float2*>(twf);
    l.w8 = tw[kN / 8];
    l.w83 = tw[3 * kN / 8];
    load_all_tw<kL, 1>(tau, tw, l.twr);
}

// the spec's graph over the lane's 8 inputs: pass 0 in registers, the later passes through the wave's exchange slot, which holds the
// natural-order result behind the last pass's fence
__device__ __forceinline__ void transform(float2 (&x)[8], const Lane& l, float2* __restrict__ xch, const int tau) {
    pass0(x, l.w8, l.w83);
#pragma unroll
    for (int r = 0; r < 8; ++r)
        xch[xpad(tau * 8 + r)] = x[r];
    fft_sync<kL>();
    later_passes<kL, 1>(x, l.twr, xch, tau);
}

// Frame `frame` of the staged block by one wave: X into the wave's slot, P[0 .. 256] into prow.  Returns whether the frame is silent
// (the same value in every lane).
__device__ __forceinline__ bool frame_forward(const float* __restrict__ xs, const int frame, const Lane& l, float2* __restrict__ xch,
                                              float* __restrict__ prow, const int tau) {
    float2 x[8];
    int live = 0;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const float s = l.nidx[r] < kFrame ? xs[kHop * frame + l.nidx[r]] : 0.0f;
        live |= s != 0.0f ? 1 : 0;
        x[r] = make_float2(__fmul_rn(s, l.w[r]), 0.0f);
    }
    transform(x, l, xch, tau);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float2 v = xch[xpad(tau + 64 * j)];
        prow[tau + 64 * j] = __fadd_rn(__fmul_rn(v.x, v.x), __fmul_rn(v.y, v.y));
    }
    if (tau == 0) {
        const float2 v = xch[xpad(kN / 2)];
        prow[kN / 2] = __fadd_rn(__fmul_rn(v.x, v.x), __fmul_rn(v.y, v.y));
    }
    return !__any(live);
}

// S_f[k] from the rows of P of frames f - 1 and f
__device__ __forceinline__ float smoothed(const float* __restrict__ p0, const float* __restrict__ p1, const int k) {
    const int lo = k ? k - 1 : 1, hi = k < kBins - 1 ? k + 1 : kBins - 2;
    const float t0 = __fadd_rn(__fadd_rn(p0[lo], p0[k]), p0[hi]), t1 = __fadd_rn(__fadd_rn(p1[lo], p1[k]), p1[hi]);
    return __fadd_rn(t0, t1);
}

// the block's 2000 samples behind the 500 before them -- out of the row's previous batch, or the carried samples at the call's first
// batch -- into xs (the blob's rows are 4-byte aligned only: the carried samples come one float at a time)
__device__ __forceinline__ void stage_block(float* __restrict__ xs, const float* __restrict__ blk, const DenoiseRowState& carried, const bool first_batch,
                                            const int t) {
    for (int q = t; q < kStaged / 4; q += kThreads) {
        float4 v;
        if (q >= kFrame / 4 || !first_batch) {
            v = reinterpret_cast<const float4*>(blk - kFrame)[q];
        } else {
            const float* const c = carried.x + 4 * q;
            v = make_float4(c[0], c[1], c[2], c[3]);
        }
        reinterpret_cast<float4*>(xs)[q] = v;
    }
}

// Launch 1.  One workgroup per block (row, batch) of an enabled row (a workgroup strides on where the grid is shorter).  Wave j
// transforms frame j of the staged block and leaves P of it in LDS; then thread k < 257 forms S of frames 1 .. 8 at bin k and writes
// the minimum over the counting ones, M, to the scratch.
__global__ __launch_bounds__(kThreads) void k_denoise_floor(const uint8_t* __restrict__ enabled, const float* __restrict__ in, const size_t row_stride,
                                                            const uint32_t rows, const uint32_t nbatches, const uint32_t max_batches,
                                                            const DenoiseRowState* __restrict__ state, const float* __restrict__ window,
                                                            const float* __restrict__ twf, float* __restrict__ floors) {
    __shared__ __align__(16) float xs[kStaged];
    __shared__ __align__(16) float2 xch[kFrames][Gm::XN];
    __shared__ float pw[kFrames][kBinRow];
    __shared__ int silent[kFrames];
    const int t = threadIdx.x, tau = t & 63, wave = t >> 6;
    Lane l;
    lane_setup(l, tau, window, twf);
    const uint32_t total = rows * nbatches;  // (below 2^24)
    for (uint32_t k = blockIdx.x; k < total; k += gridDim.x) {  // (the same trips for the whole workgroup)
        const uint32_t row = k / nbatches, batch = k - row * nbatches;
        if (!enabled[row])  // (the whole workgroup)
            continue;
        stage_block(xs, in + static_cast<size_t>(row) * row_stride + static_cast<size_t>(batch) * kBatch, state[row], batch == 0, t);
        __syncthreads();
        const bool quiet = frame_forward(xs, wave, l, xch[wave], pw[wave], tau);
        if (tau == 0)
            silent[wave] = quiet ? 1 : 0;
        __syncthreads();
        if (t < kBins) {
            float m = INFINITY;
            for (int j = 1; j < kFrames; ++j)
                if (!silent[j - 1] && !silent[j])
                    m = fminf(m, smoothed(pw[j - 1], pw[j], t));
            floors[(static_cast<size_t>(row) * max_batches + batch) * kBins + t] = m;
        }
        // (the next trip writes xs behind this barrier's readers, and pw, xch and silent behind its own first barrier)
    }
}

// Launch 2.  One workgroup per block.  The nine frames are transformed again -- the same bits as in launch 1 --, S of every frame and
// the noise estimate of the block's batch go into LDS (m from the scratch rows of the call and the carried rows), then wave j takes
// frame j's spectrum out of its slot at the bit-reversed places, times the gains and conjugated, runs the same graph and leaves z in
// the slot; the overlap-add reads two slots per output.
__global__ __launch_bounds__(kThreads) void k_denoise_apply(const uint8_t* __restrict__ enabled, const DenoiseGains* __restrict__ cfg,
                                                            const float* __restrict__ in, const size_t row_stride, const uint32_t rows,
                                                            const uint32_t nbatches, const uint32_t max_batches, const DenoiseRowState* __restrict__ state,
                                                            const float* __restrict__ window, const float* __restrict__ twf,
                                                            const float* __restrict__ floors, float* __restrict__ out, const size_t out_stride) {
    __shared__ __align__(16) float xs[kStaged];
    __shared__ __align__(16) float2 xch[kFrames][Gm::XN];
    __shared__ float pw[kFrames][kBinRow];
    __shared__ float noise[kBinRow];
    __shared__ float ws[kFrame];
    const int t = threadIdx.x, tau = t & 63, wave = t >> 6;
    float(&sm)[kFrames][kBinRow] = *reinterpret_cast<float(*)[kFrames][kBinRow]>(xs);  // S lies over the staged block, dead once P is formed
    Lane l;
    lane_setup(l, tau, window, twf);
    if (t < kFrame)
        ws[t] = window[t];
    const uint32_t total = rows * nbatches;  // (below 2^24)
    for (uint32_t k = blockIdx.x; k < total; k += gridDim.x) {  // (the same trips for the whole workgroup)
        const uint32_t row = k / nbatches, batch = k - row * nbatches;
        if (!enabled[row])  // (the whole workgroup)
            continue;
        const float g_min = cfg[row].g_min, over = cfg[row].over;
        stage_block(xs, in + static_cast<size_t>(row) * row_stride + static_cast<size_t>(batch) * kBatch, state[row], batch == 0, t);
        __syncthreads();
        (void)frame_forward(xs, wave, l, xch[wave], pw[wave], tau);
        __syncthreads();
        for (int e = t; e < (kFrames - 1) * kBins; e += kThreads) {
            const int j = 1 + e / kBins, bin = e - (j - 1) * kBins;
            const float s = smoothed(pw[j - 1], pw[j], bin);
            sm[j][bin] = s;
            if (j == 1)  // the block's first frame takes S of the frame behind it
                sm[0][bin] = s;
        }
        if (t < kBins) {
            float m = INFINITY;
            for (int d = 0; d < kDepth; ++d) {  // batches batch - 7 .. batch: carried rows in front of the call's
                const int c = static_cast<int>(batch) - (kDepth - 1) + d;
                m = fminf(m, c < 0 ? state[row].m[kDepth - 1 + c][t] : floors[(static_cast<size_t>(row) * max_batches + static_cast<uint32_t>(c)) * kBins + t]);
            }
            noise[t] = isinf(m) ? 0.0f : __fmul_rn(over, m);
        }
        __syncthreads();
        for (int bin = tau; bin < kBins; bin += 64) {  // the frame's gains in the place of its S: one division a bin, not one a point
            const float n = noise[bin], s = sm[wave][bin];
            sm[wave][bin] = n >= s ? g_min : fmaxf(g_min, __fsub_rn(1.0f, __fdiv_rn(n, s)));
        }
        fft_sync<kL>();  // (the wave alone reads and writes its row of sm from here on)
        {
            float2 x[8];
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const float g = sm[wave][l.nidx[r] <= kN / 2 ? l.nidx[r] : kN - l.nidx[r]];
                const float2 v = xch[wave][xpad(l.nidx[r])];
                x[r] = make_float2(__fmul_rn(g, v.x), -__fmul_rn(g, v.y));
            }
            fft_sync<kL>();  // (every lane holds its inputs: the slot becomes the exchange's)
            transform(x, l, xch[wave], tau);
        }
        __syncthreads();
        if (t < kBatch / 4) {
            float y[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int n = 4 * t + e, q = n / kHop, i = n - q * kHop;  // the older frame q of the block, the newer one q + 1
                const float a = __fmul_rn(__fmul_rn(xch[q][xpad(kHop + i)].x, 1.0f / kN), ws[kHop + i]);
                const float b = __fmul_rn(__fmul_rn(xch[q + 1][xpad(i)].x, 1.0f / kN), ws[i]);
                y[e] = fminf(fmaxf(__fadd_rn(a, b), -1.0f), 1.0f);
            }
            reinterpret_cast<float4*>(out + static_cast<size_t>(row) * out_stride + static_cast<size_t>(batch) * kBatch)[t] = make_float4(y[0], y[1], y[2], y[3]);
        }
        __syncthreads();  // (the next trip writes the LDS this one read)
    }
}

// Launch 3, behind the two that read the old state.  One workgroup per enabled row: the last 500 input samples of the call are the
// row's new carried samples, and the last seven M -- carried rows, then the call's -- its new carried minima.  A thread walks one bin
// upwards through the seven rows, so that it reads a carried row before it writes it.
__global__ __launch_bounds__(256) void k_denoise_tails(const uint8_t* __restrict__ enabled, const float* __restrict__ in, const size_t row_stride,
                                                       const uint32_t rows, const uint32_t nbatches, const uint32_t max_batches,
                                                       const float* __restrict__ floors, DenoiseRowState* __restrict__ state) {
    const uint32_t row = blockIdx.x;
    if (row >= rows || !enabled[row])
        return;
    const float* const tail = in + static_cast<size_t>(row) * row_stride + static_cast<size_t>(nbatches) * kBatch - kFrame;
    for (int j = threadIdx.x; j < kFrame; j += 256)
        state[row].x[j] = tail[j];
    for (int bin = threadIdx.x; bin < kBins; bin += 256)
        for (int i = 0; i < kDepth - 1; ++i) {
            const int c = i + static_cast<int>(nbatches) - (kDepth - 1);  // the batch of the call, or a carried row where negative
            state[row].m[i][bin] = c < 0 ? state[row].m[i + nbatches][bin] : floors[(static_cast<size_t>(row) * max_batches + static_cast<uint32_t>(c)) * kBins + bin];
        }
}

// the rows' settings onto the device (the caller has completed queued work where a call may read them)
int upload_settings(mi_denoise* d, const std::vector<DenoiseGains>& cfg) {
    if (hipMemcpy(d->d_cfg.get(), cfg.data(), cfg.size() * sizeof(DenoiseGains), hipMemcpyHostToDevice) != hipSuccess)
        return fail(MI_ERR_HIP, "noise reduction stage: uploading the rows failed");
    return MI_OK;
}

}  // namespace
}  // namespace mi

using mi::as_flags;
using mi::fail;

extern "C" {

int mi_denoise_create(const mi_denoise_row* row_cfg, const uint8_t* row_enabled, int rows, int max_batches, int gpu, mi_denoise** out) {
    if (!row_enabled || !out)
        return fail(MI_ERR_INVALID, "NULL argument");
    if (const int rc = mi::batch_geometry_ok(kName, rows, max_batches))
        return rc;
    const size_t n = static_cast<size_t>(rows);
    std::vector<mi::DenoiseGains> cfg;
    if (const int rc = mi::denoise_rows(row_cfg, n, cfg))
        return rc;
    std::vector<float> tw, window(mi::kFrame);
    if (const int rc = mi::spec_twiddles(mi::kL, tw))
        return rc;
    mi::denoise_window(window.data());
    if (const int rc = mi::check_gpu(gpu, "no HIP device: the noise reduction stage runs on the GPU only"))
        return rc;
    std::vector<mi::DenoiseRowState> fresh(n);
    mi::denoise_fresh(fresh.data(), n);
    mi_denoise* d = new mi_denoise();
    d->gpu = gpu;
    d->rows = rows;
    d->max_batches = max_batches;
    if (hipSetDevice(gpu) != hipSuccess || dalloc_copy(d->d_enabled, as_flags(row_enabled, n)) != hipSuccess || dalloc_copy(d->d_state, fresh) != hipSuccess ||
        dalloc_copy(d->d_cfg, cfg) != hipSuccess || dalloc_copy(d->d_window, window) != hipSuccess || dalloc_copy(d->d_tw, tw) != hipSuccess ||
        dalloc(d->d_floor, n * static_cast<size_t>(max_batches) * mi::kBins) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
        delete d;
        return fail(MI_ERR_HIP, "noise reduction stage: device allocation failed");
    }
    *out = d;
    return MI_OK;
}

void mi_denoise_destroy(mi_denoise* d) {
    mi::destroy(d);
}

int mi_denoise_set_rows(mi_denoise* d, const mi_denoise_row* row_cfg, const uint8_t* row_enabled) {
    if (!d || (!row_cfg && !row_enabled))
        return fail(MI_ERR_INVALID, "NULL argument");
    const size_t n = static_cast<size_t>(d->rows);
    std::vector<mi::DenoiseGains> cfg;
    if (row_cfg)
        if (const int rc = mi::denoise_rows(row_cfg, n, cfg))
            return rc;
    // (a call still queued reads the rows it was made with)
    if (hipSetDevice(d->gpu) != hipSuccess || hipDeviceSynchronize() != hipSuccess)
        return fail(MI_ERR_HIP, "noise reduction stage: uploading the rows failed");
    if (row_cfg)
        if (const int rc = mi::upload_settings(d, cfg))
            return rc;
    if (row_enabled) {
        const std::vector<uint8_t> flags = as_flags(row_enabled, n);
        if (hipMemcpy(d->d_enabled.get(), flags.data(), flags.size(), hipMemcpyHostToDevice) != hipSuccess)
            return fail(MI_ERR_HIP, "noise reduction stage: uploading the rows failed");
    }
    return MI_OK;
}

int mi_denoise_process_device(mi_denoise* d, const float* d_in, size_t row_stride, int nbatches, float* d_out, size_t out_stride, void* hip_stream) {
    if (const int rc = mi::plane_call_ok(d, d_in, row_stride, nbatches, d_out, out_stride, "input plane"))
        return rc;
    if (hipSetDevice(d->gpu) != hipSuccess)
        return fail(MI_ERR_HIP, "hipSetDevice failed");
    hipStream_t q = static_cast<hipStream_t>(hip_stream);
    const unsigned rows = static_cast<unsigned>(d->rows), call = rows * static_cast<unsigned>(nbatches), grid = call < mi::kMaxGrid ? call : mi::kMaxGrid;
    const uint32_t nb = static_cast<uint32_t>(nbatches), mb = static_cast<uint32_t>(d->max_batches);
    d->timing.stamp(0, q);
    hipLaunchKernelGGL(mi::k_denoise_floor, dim3(grid), dim3(mi::kThreads), 0, q, d->d_enabled.get(), d_in, row_stride, rows, nb, mb, d->d_state.get(),
                       d->d_window.get(), d->d_tw.get(), d->d_floor.get());
    d->timing.stamp(1, q);
    hipLaunchKernelGGL(mi::k_denoise_apply, dim3(grid), dim3(mi::kThreads), 0, q, d->d_enabled.get(), d->d_cfg.get(), d_in, row_stride, rows, nb, mb,
                       d->d_state.get(), d->d_window.get(), d->d_tw.get(), d->d_floor.get(), d_out, out_stride);
    d->timing.stamp(2, q);
    hipLaunchKernelGGL(mi::k_denoise_tails, dim3(rows), dim3(256), 0, q, d->d_enabled.get(), d_in, row_stride, rows, nb, mb, d->d_floor.get(), d->d_state.get());
    d->timing.stamp(3, q);
    if (hipGetLastError() != hipSuccess)
        return fail(MI_ERR_HIP, "noise reduction stage kernel launch failed");
    d->called = true;
    return MI_OK;
}

int mi_denoise_set_timing(mi_denoise* d, int on) {
    return mi::set_timing(d, on);
}

int mi_denoise_last_launch_ms(mi_denoise* d, float* ms) {
    return mi::last_launch_ms(d, ms, "mi_denoise_process_device");
}

size_t mi_denoise_state_size(const mi_denoise* d) {
    return mi::state_size(d, &mi_denoise::d_state);
}

int mi_denoise_get_state(mi_denoise* d, void* buf, size_t len) {
    return mi::get_state(kName, d, &mi_denoise::d_state, buf, len);
}

int mi_denoise_set_state(mi_denoise* d, const void* buf, size_t len) {
    return mi::set_state(kName, d, &mi_denoise::d_state, buf, len);
}

}  // extern "C"
