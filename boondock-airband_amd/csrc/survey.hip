// survey.hip -- the band survey: for every FFT bin of a device-resident capture, the mean and the peak magnitude over each run of
// windows_per_cell consecutive windows (a "cell"; by default one audio batch).  It is the pass that comes before a channel plan: the
// demodulator evaluates only the bins its plan picks, this stage looks at all of them and keeps 2 * fft_size floats per cell.
//
// A post-stage of its own like the output gate (outgate.hip): its own handle, two launches on the caller's stream, no atomics.
//   k_survey       one workgroup = one tile of consecutive windows of one (stream, cell).  The windows are stage 1's: its span load, level table and
//                  lane setup by its own text (iq_front.hpp), the same conversion x window and radix-8 passes (fft_radix8.hpp), so
//                  a bin's magnitude has the bits of the oracle's ao_fft_forward.  Behind the last pass, where stage 1 picks its
//                  channel bins, every lane takes the 8 bins tau + j * N/8 of the natural-order spectrum in the exchange slot and
//                  keeps a running float max and float64 sum of sqrtf(re * re + im * im) in registers across all the windows it
//                  sees.  A tile is walked TW windows of span at a time, so its length is not bounded by the LDS, and it never
//                  straddles a cell: a cell that is no multiple of the tile ends in a short one.  One partial {sum, max} per
//                  (stream, cell, tile, bin) leaves the kernel.
//   k_survey_fold  folds the partials of a cell in tile order: mean = (float)(S / windows_per_cell), peak = the max.
// Order of the float64 sum S of a bin (fixed, so two runs give the same bytes): within a tile, FFT group f of the workgroup (F groups
// run side by side: 8 at N = 256, 4 at 512, 2 at 1024, else 1) adds the windows f, f + F, f + 2F, ... of every TW-window piece in
// turn; the groups' sums are added in group order, then the tiles' in tile order.
//
// Compile with -ffp-contract=off (the FFT spec).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "../../include/mi_airband.h"
#include "iq_front.hpp"
#include "poststage.hpp"

struct mi_survey : mi::IqFront {
    mi_survey() : IqFront("band survey", 2) {}
    uint32_t tile_windows = 0;  // windows per tile, a multiple of the kernel's TW
    uint32_t tiles = 0;         // tiles per cell
    int nenabled = 0;
    mi::DevBuf<int> d_streams;   // [nstreams], the first nenabled: the enabled streams, ascending
    mi::DevBuf<double> d_psum;   // [nstreams][max_cells][tiles][fft_size]
    mi::DevBuf<float> d_pmax;    // the same
};

namespace mi {
namespace {

constexpr uint32_t kMaxTilesPerCell = 4;  // partials written per cell and bin: enough workgroups for one stream, little to fold

struct SurveyArgs : IqArgs {
    uint32_t wpc, tile_windows, tiles;
    const int* streams;  // [gridDim.z] the stream each z takes
    double* psum;        // [gridDim.z][gridDim.x][tiles][N]
    float* pmax;
};

// The dynamic LDS a k_survey workgroup needs: the tile walk's, or the groups' partials that lie over it at the end.  mi_survey_create
// refuses a geometry whose need exceeds kLdsLimit and mi_survey_process_device launches with it: one function, so the two cannot
// drift.  hop_bytes <= 2^20 (mi_survey_create), so nothing here wraps.  0: no such kernel instance.
size_t survey_lds_bytes(int log2n, int sfmt, unsigned hop_bytes) {
    return dispatch_log2n(log2n, size_t{0}, [&](auto l) {
        using Gm = FftGeom<l()>;
        const size_t work = tile_lds_bytes<l()>(iq_bps2(sfmt), hop_bytes);
        const size_t fold = Gm::F > 1 ? static_cast<size_t>(Gm::F) * Gm::N * 12 : 0;
        return work > fold ? work : fold;
    });
}

template <int L, int SFMT>
__global__ __launch_bounds__(FftGeom<L>::BLOCK) void k_survey(const SurveyArgs a) {
    using Gm = FftGeom<L>;
    constexpr int N = Gm::N, TPF = Gm::TPF, F = Gm::F, TW = Gm::TW, XN = Gm::XN, BLOCK = Gm::BLOCK;
    constexpr int BPS2 = iq_bps2(SFMT);  // bytes per complex sample
    constexpr bool kTwInRegs = L <= 11;

    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int tid = threadIdx.x;
    const unsigned cell = blockIdx.x, tile = blockIdx.y;
    const int stream = a.streams[blockIdx.z];
    const unsigned t0 = tile * a.tile_windows;                                       // first window of the tile within its cell
    const int nt = static_cast<int>(min(a.tile_windows, a.wpc - t0));                // its windows: the last tile of a cell may be short
    const long long wfirst = static_cast<long long>(cell) * a.wpc + t0;             // ... counted from the stream's base

    const unsigned span_bytes = span_alloc<L>(BPS2, a.hop_bytes);
    unsigned char* span = lds;
    float* lut = reinterpret_cast<float*>(lds + span_bytes);
    float2* xch_all = reinterpret_cast<float2*>(lds + span_bytes + 1024);
    load_levels<SFMT, BLOCK>(lut, a.levels, tid);

    // ---- per-lane constants: window coefficients of the 8 samples this lane converts, twiddles ----
    const int f = tid / TPF;
    const int tau = tid - f * TPF;
    float2* xch = xch_all + f * XN;
    const float2* tw = reinterpret_cast<const float2*>(a.tw);
    const FftLane ln = fft_lane<L>(tau, a.window, tw);
    [[maybe_unused]] float2 twr[kTwInRegs ? Gm::NPASS : 1][7];
    if constexpr (kTwInRegs)
        load_all_tw<L, 1>(tau, tw, twr);

    // the lane's bins tau + j * TPF: running max and float64 sum of the magnitude over the windows of FFT group f
    float mx[8];
    double sm[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        mx[j] = 0.0f;
        sm[j] = 0.0;
    }

    const unsigned char* gbase = a.iq + static_cast<size_t>(stream) * a.stream_stride;
    for (int s0 = 0; s0 < nt; s0 += TW) {  // the tile, TW windows of span at a time
        const int nw = min(TW, nt - s0);
        if (s0)
            __syncthreads();  // every FFT of the piece before has converted its samples
        const unsigned mis = load_span<BLOCK>(span, gbase, (wfirst + s0) * static_cast<long long>(a.hop_bytes), nw, a.hop_bytes, N * BPS2, a.valid_bytes, tid);
        __syncthreads();

        // ---- FFTs: F windows at a time ----
        for (int it = 0; it * F < nw; ++it) {
            const int wi = it * F + f;
            const bool active = wi < nw;
            float2 x[8];
            const int wbyte = static_cast<int>(mis) + (active ? wi : 0) * static_cast<int>(a.hop_bytes);
#pragma unroll
            for (int r = 0; r < 8; ++r)
                x[r] = fetch_sample<SFMT>(span, wbyte + ln.nidx[r] * BPS2, lut, a.conv_scale, ln.wreg[r]);
            pass0(x, ln.w8, ln.w83);
#pragma unroll
            for (int r = 0; r < 8; ++r)
                xch[xpad(tau * 8 + r)] = x[r];
            fft_sync<L>();
            if constexpr (kTwInRegs)
                later_passes<L, 1>(x, twr, xch, tau);
            else
                later_passes_tw<L, 1>(x, tw, xch, tau);
            // natural-order spectrum now sits in xch: every bin's magnitude, as stage 1 takes a picked one (rtl_airband.cpp:505-511)
            if (active) {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float2 v = xch[xpad(tau + j * TPF)];
                    const float m = sqrtf(v.x * v.x + v.y * v.y);
                    mx[j] = fmaxf(mx[j], m);
                    sm[j] += static_cast<double>(m);
                }
            }
            fft_sync<L>();  // the slot is rewritten by the next window's pass 0
        }
    }

    // ---- one partial per bin: the F groups' in group order ----
    const size_t pbase = ((static_cast<size_t>(blockIdx.z) * gridDim.x + cell) * a.tiles + tile) * N;
    if constexpr (F == 1) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            a.psum[pbase + tau + j * TPF] = sm[j];
            a.pmax[pbase + tau + j * TPF] = mx[j];
        }
    } else {
        __syncthreads();  // span and exchange slots are dead: the groups' partials go over them
        double* fs = reinterpret_cast<double*>(lds);
        float* fm = reinterpret_cast<float*>(lds + static_cast<size_t>(F) * N * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            fs[f * N + tau + j * TPF] = sm[j];
            fm[f * N + tau + j * TPF] = mx[j];
        }
        __syncthreads();
        for (int k = tid; k < N; k += BLOCK) {
            double s = fs[k];
            float m = fm[k];
#pragma unroll
            for (int g = 1; g < F; ++g) {
                s += fs[g * N + k];
                m = fmaxf(m, fm[g * N + k]);
            }
            a.psum[pbase + k] = s;
            a.pmax[pbase + k] = m;
        }
    }
}

// One lane = four consecutive bins of one (stream, cell): the tiles' partials in tile order.
__global__ __launch_bounds__(64) void k_survey_fold(const double* __restrict__ psum, const float* __restrict__ pmax, const int* __restrict__ streams,
                                                    const int n, const int tiles, const double wpc, float* __restrict__ mean,
                                                    float* __restrict__ peak) {
    const int bin = (blockIdx.y * 64 + threadIdx.x) * 4;
    if (bin >= n)
        return;
    const size_t cell = blockIdx.x, ncells = gridDim.x;
    const size_t pb = (static_cast<size_t>(blockIdx.z) * ncells + cell) * tiles * n + bin;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    float m[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int t = 0; t < tiles; ++t) {
        const double2 s01 = *reinterpret_cast<const double2*>(psum + pb + static_cast<size_t>(t) * n);
        const double2 s23 = *reinterpret_cast<const double2*>(psum + pb + static_cast<size_t>(t) * n + 2);
        const float4 mm = *reinterpret_cast<const float4*>(pmax + pb + static_cast<size_t>(t) * n);
        s[0] += s01.x, s[1] += s01.y, s[2] += s23.x, s[3] += s23.y;
        m[0] = fmaxf(m[0], mm.x), m[1] = fmaxf(m[1], mm.y), m[2] = fmaxf(m[2], mm.z), m[3] = fmaxf(m[3], mm.w);
    }
    const size_t ob = (static_cast<size_t>(streams[blockIdx.z]) * ncells + cell) * n + bin;
    *reinterpret_cast<float4*>(mean + ob) = make_float4(static_cast<float>(s[0] / wpc), static_cast<float>(s[1] / wpc), static_cast<float>(s[2] / wpc),
                                                        static_cast<float>(s[3] / wpc));
    *reinterpret_cast<float4*>(peak + ob) = make_float4(m[0], m[1], m[2], m[3]);
}

hipError_t launch_survey(const SurveyArgs& a, int log2n, int sfmt, bool conv_arith, int ncells, int nenabled, hipStream_t s) {
    return dispatch_fft(log2n, sfmt, conv_arith, hipErrorInvalidValue, [&](auto l, auto f) {
        return launch_lds(k_survey<l(), f()>, dim3(ncells, a.tiles, nenabled), dim3(FftGeom<l()>::BLOCK), survey_lds_bytes(l(), f(), a.hop_bytes), s, a);
    });
}

}  // namespace
}  // namespace mi

using mi::aligned;
using mi::fail;

extern "C" {

int mi_survey_create(const mi_device_cfg* dev, int nstreams, int max_cells, int windows_per_cell, int gpu, mi_survey** out) {
    mi::Plan plan;
    if (const int rc = mi::iq_front_plan("band survey", dev, out, nstreams, max_cells, windows_per_cell, mi::survey_lds_bytes, mi::kLdsLimit, plan))
        return rc;
    mi_survey* s = nullptr;
    if (const int rc = mi::iq_front_new("band survey", plan, nstreams, max_cells, windows_per_cell, gpu, &s))
        return rc;
    // tiles: whole multiples of the kernel's TW windows, at most kMaxTilesPerCell of them to a cell
    const uint32_t tw = mi::dispatch_log2n(s->log2n, 0u, [](auto l) { return static_cast<uint32_t>(mi::FftGeom<l()>::TW); });
    const uint32_t want = std::min((s->wpc + tw - 1) / tw, mi::kMaxTilesPerCell);
    s->tile_windows = ((s->wpc + want - 1) / want + tw - 1) / tw * tw;
    s->tiles = (s->wpc + s->tile_windows - 1) / s->tile_windows;
    const size_t partials = static_cast<size_t>(nstreams) * static_cast<size_t>(max_cells) * s->tiles * static_cast<size_t>(s->fft_size);
    std::vector<int> all(static_cast<size_t>(nstreams));
    for (int i = 0; i < nstreams; ++i)
        all[static_cast<size_t>(i)] = i;
    s->nenabled = nstreams;
    if (hipSetDevice(gpu) != hipSuccess || iq_front_upload(s, plan) != hipSuccess || dalloc_copy(s->d_streams, all) != hipSuccess ||
        dalloc(s->d_psum, partials) != hipSuccess || dalloc(s->d_pmax, partials) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
        delete s;
        return fail(MI_ERR_HIP, "band survey: device allocation failed");
    }
    *out = s;
    return MI_OK;
}

void mi_survey_destroy(mi_survey* s) {
    mi::destroy(s);
}

int mi_survey_set_streams(mi_survey* s, const uint8_t* stream_enabled) {
    if (!s)
        return fail(MI_ERR_INVALID, "NULL argument");
    std::vector<int> list;
    for (int i = 0; i < s->nstreams; ++i)
        if (!stream_enabled || stream_enabled[i])
            list.push_back(i);
    if (list.empty())
        return fail(MI_ERR_INVALID, "band survey: no stream enabled");
    // (a call still queued reads the list it was made with)
    if (!mi::sync_copy(s->gpu, s->d_streams, list.data(), list.size() * sizeof(int), hipMemcpyHostToDevice))
        return fail(MI_ERR_HIP, "band survey: uploading the stream list failed");
    s->nenabled = static_cast<int>(list.size());
    return MI_OK;
}

size_t mi_survey_bytes_needed(const mi_survey* s, int ncells) {
    return mi::iq_bytes_needed(s, ncells);
}

int mi_survey_process_device(mi_survey* s, const void* d_iq, size_t stream_stride_bytes, int ncells, float* d_mean, float* d_peak, void* hip_stream) {
    if (!s || !d_iq || !d_mean || !d_peak)
        return fail(MI_ERR_INVALID, "NULL argument");
    if (const int rc = mi::iq_call_ok(s, d_iq, stream_stride_bytes, ncells, aligned(d_mean, 16) && aligned(d_peak, 16), "d_mean and d_peak must be 16-byte aligned"))
        return rc;
    if (hipSetDevice(s->gpu) != hipSuccess)
        return fail(MI_ERR_HIP, "hipSetDevice failed");
    hipStream_t q = static_cast<hipStream_t>(hip_stream);
    mi::SurveyArgs a{};
    mi::iq_args(a, s, d_iq, stream_stride_bytes, ncells);
    a.wpc = s->wpc;
    a.tile_windows = s->tile_windows;
    a.tiles = s->tiles;
    a.streams = s->d_streams;
    a.psum = s->d_psum;
    a.pmax = s->d_pmax;
    s->timing.stamp(0, q);
    if (mi::launch_survey(a, s->log2n, s->sfmt, s->conv_arith, ncells, s->nenabled, q) != hipSuccess)
        return fail(MI_ERR_HIP, "band survey kernel launch failed");
    s->timing.stamp(1, q);
    hipLaunchKernelGGL(mi::k_survey_fold, dim3(static_cast<unsigned>(ncells), static_cast<unsigned>(s->fft_size / 256), static_cast<unsigned>(s->nenabled)),
                       dim3(64), 0, q, s->d_psum.get(), s->d_pmax.get(), s->d_streams.get(), s->fft_size, static_cast<int>(s->tiles),
                       static_cast<double>(s->wpc), d_mean, d_peak);
    s->timing.stamp(2, q);
    if (hipGetLastError() != hipSuccess)
        return fail(MI_ERR_HIP, "band survey kernel launch failed");
    s->called = s->timing.on;  // (a stamped call: last_launch_ms refuses after any other)
    return MI_OK;
}

int mi_survey_set_timing(mi_survey* s, int on) {
    return mi::set_timing(s, on);
}

int mi_survey_last_launch_ms(mi_survey* s, float* ms) {
    return mi::last_launch_ms(s, ms, "mi_survey_process_device");
}

}  // extern "C"
