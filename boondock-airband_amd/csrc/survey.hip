// survey.hip -- the band survey: for every FFT bin of a device-resident capture, the mean and the peak magnitude over each run of
// windows_per_cell consecutive windows (a "cell"; by default one audio batch).  It is the pass that comes before a channel plan: the
// demodulator evaluates only the bins its plan picks, this stage looks at all of them and keeps 2 * fft_size floats per cell.
//
// A post-stage of its own like the output gate (outgate.hip): its own handle, two launches on the caller's stream, no atomics.
//   k_survey       one workgroup = one tile of consecutive windows of one (stream, cell).  The windows are stage 1's: the same span
//                  load, conversion x window and radix-8 passes (fft_radix8.hpp), so a bin's magnitude has the bits of the oracle's
//                  ao_fft_forward.  Behind the last pass, where stage 1 picks its channel bins, every lane takes the 8 bins
//                  tau + j * N/8 of the natural-order spectrum in the exchange slot and keeps a running float max and float64 sum of
//                  sqrtf(re * re + im * im) in registers across all the windows it sees.  A tile is walked TW windows of span at a
//                  time, so its length is not bounded by the LDS, and it never straddles a cell: a cell that is no multiple of the
//                  tile ends in a short one.  One partial {sum, max} per (stream, cell, tile, bin) leaves the kernel.
//   k_survey_fold  folds the partials of a cell in tile order: mean = (float)(S / windows_per_cell), peak = the max.
// Order of the float64 sum S of a bin (fixed, so two runs give the same bytes): within a tile, FFT group f of the workgroup (F groups
// run side by side: 8 at N = 256, 4 at 512, 2 at 1024, else 1) adds the windows f, f + F, f + 2F, ... of every TW-window piece in
// turn; the groups' sums are added in group order, then the tiles' in tile order.
//
// Compile with -ffp-contract=off (the FFT spec).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <string>
#include <vector>

#include "../../include/mi_airband.h"
#include "fft_radix8.hpp"
#include "poststage.hpp"

struct mi_survey : mi::Stage {
    mi_survey() : Stage("band survey", 2) {}
    int nstreams = 0;
    int max_cells = 0;
    uint32_t wpc = 0;           // windows per cell
    uint32_t tile_windows = 0;  // windows per tile, a multiple of the kernel's TW
    uint32_t tiles = 0;         // tiles per cell
    int log2n = 0, fft_size = 0, sfmt = 0, sample_bytes = 0;  // sample_bytes: one complex sample
    bool conv_arith = false;
    float conv_scale = 0.0f;
    size_t hop_bytes = 0;
    int nenabled = 0;
    mi::DevBuf<float> d_window, d_tw, d_levels;
    mi::DevBuf<int> d_streams;   // [nstreams], the first nenabled: the enabled streams, ascending
    mi::DevBuf<double> d_psum;   // [nstreams][max_cells][tiles][fft_size]
    mi::DevBuf<float> d_pmax;    // the same
};

namespace mi {
namespace {

constexpr uint32_t kMaxTilesPerCell = 4;  // partials written per cell and bin: enough workgroups for one stream, little to fold

struct SurveyArgs {
    const unsigned char* iq;  // stream s at iq + s*stream_stride
    size_t stream_stride;
    size_t valid_bytes;       // readable bytes per stream starting at its base
    uint32_t hop_bytes;
    uint32_t wpc, tile_windows, tiles;
    const float* window;
    const float* tw;
    const float* levels;
    float conv_scale;
    const int* streams;  // [gridDim.z] the stream each z takes
    double* psum;        // [gridDim.z][gridDim.x][tiles][N]
    float* pmax;
};

constexpr size_t kSurveyLdsLimit = 160 * 1024;  // what one workgroup may ask for on gfx950: the CU's whole LDS

// bytes per complex sample of a kernel instance's format
constexpr int survey_bps2(int sfmt) {
    return sfmt == MI_SFMT_S16 ? 4 : (sfmt == MI_SFMT_F32 ? 8 : 2);
}

// The span of one TW-window piece in LDS: its bytes, up to 15 in front of them (the piece starts at a 16-byte line) and a line's
// rounding.  k_survey lays its LDS out with it and survey_lds_bytes sizes the launch with it.
template <int L>
__host__ __device__ constexpr unsigned survey_span_alloc(int bps2, unsigned hop_bytes) {
    return (static_cast<unsigned>(FftGeom<L>::TW - 1) * hop_bytes + static_cast<unsigned>(FftGeom<L>::N * bps2) + 16 + 15) & ~15u;
}

template <int L>
constexpr size_t survey_lds_bytes_of(int bps2, unsigned hop_bytes) {
    using Gm = FftGeom<L>;
    const size_t work = static_cast<size_t>(survey_span_alloc<L>(bps2, hop_bytes)) + 1024 + static_cast<size_t>(Gm::F) * Gm::XN * 8;
    const size_t fold = Gm::F > 1 ? static_cast<size_t>(Gm::F) * Gm::N * 12 : 0;  // the groups' partials lie over the working set
    return work > fold ? work : fold;
}

// The dynamic LDS a k_survey workgroup needs.  mi_survey_create refuses a geometry whose need exceeds kSurveyLdsLimit and
// launch_survey_one launches with it: one function, so the two cannot drift.  hop_bytes <= 2^20 (mi_survey_create), so nothing here
// wraps.  0: no such kernel instance.
size_t survey_lds_bytes(int log2n, int sfmt, unsigned hop_bytes) {
    const int bps2 = survey_bps2(sfmt);
    switch (log2n) {
        case 8: return survey_lds_bytes_of<8>(bps2, hop_bytes);
        case 9: return survey_lds_bytes_of<9>(bps2, hop_bytes);
        case 10: return survey_lds_bytes_of<10>(bps2, hop_bytes);
        case 11: return survey_lds_bytes_of<11>(bps2, hop_bytes);
        case 12: return survey_lds_bytes_of<12>(bps2, hop_bytes);
        case 13: return survey_lds_bytes_of<13>(bps2, hop_bytes);
    }
    return 0;
}

template <int L, int SFMT>
__global__ __launch_bounds__(FftGeom<L>::BLOCK) void k_survey(const SurveyArgs a) {
    using Gm = FftGeom<L>;
    constexpr int N = Gm::N, TPF = Gm::TPF, F = Gm::F, TW = Gm::TW, XN = Gm::XN, BLOCK = Gm::BLOCK;
    constexpr int BPS2 = survey_bps2(SFMT);  // bytes per complex sample
    constexpr bool kTwInRegs = L <= 11;

    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int tid = threadIdx.x;
    const unsigned cell = blockIdx.x, tile = blockIdx.y;
    const int stream = a.streams[blockIdx.z];
    const unsigned t0 = tile * a.tile_windows;                                       // first window of the tile within its cell
    const int nt = static_cast<int>(min(a.tile_windows, a.wpc - t0));                // its windows: the last tile of a cell may be short
    const long long wfirst = static_cast<long long>(cell) * a.wpc + t0;             // ... counted from the stream's base

    const unsigned span_alloc = survey_span_alloc<L>(BPS2, a.hop_bytes);
    unsigned char* span = lds;
    float* lut = reinterpret_cast<float*>(lds + span_alloc);
    float2* xch_all = reinterpret_cast<float2*>(lds + span_alloc + 1024);
    if constexpr (SFMT == MI_SFMT_U8 || SFMT == MI_SFMT_S8) {
        for (int i = tid; i < 256; i += BLOCK)
            lut[i] = a.levels[i];
    }

    // ---- per-lane constants: window coefficients of the 8 samples this lane converts, twiddles ----
    const int f = tid / TPF;
    const int tau = tid - f * TPF;
    float2* xch = xch_all + f * XN;
    const int nrev = (L > 3) ? static_cast<int>(__brev(static_cast<unsigned>(tau)) >> (32 - (L - 3))) : 0;
    int nidx[8];
    float wreg[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int rev3 = ((r & 1) << 2) | (r & 2) | ((r >> 2) & 1);
        nidx[r] = rev3 * TPF + nrev;  // natural sample index = bitrev_L(8 tau + r)
        wreg[r] = a.window[nidx[r]];
    }
    const float2* tw = reinterpret_cast<const float2*>(a.tw);
    const float2 w8 = tw[N / 8], w83 = tw[3 * N / 8];
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
        // ---- HBM -> LDS: the byte span of this piece, each byte read once, 16 B per lane ----
        const long long b0 = (wfirst + s0) * static_cast<long long>(a.hop_bytes);
        const unsigned mis = static_cast<unsigned>(reinterpret_cast<uintptr_t>(gbase + b0) & 15);
        const unsigned need = static_cast<unsigned>(nw - 1) * a.hop_bytes + N * BPS2;
        const unsigned nchunks = (mis + need + 15) >> 4;
        for (unsigned c = tid; c < nchunks; c += BLOCK) {
            const long long off = b0 - mis + 16ll * c;
            uint4 v;
            if (off >= 0 && off + 16 <= static_cast<long long>(a.valid_bytes)) {
                v = *reinterpret_cast<const uint4*>(gbase + off);
            } else {  // the 16-byte lines around the first and the last byte of the call: nothing outside them is touched
                unsigned char tmp[16];
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const long long o = off + i;
                    tmp[i] = (o >= 0 && o < static_cast<long long>(a.valid_bytes)) ? gbase[o] : 0;
                }
                v = *reinterpret_cast<uint4*>(tmp);
            }
            *reinterpret_cast<uint4*>(span + 16 * c) = v;
        }
        __syncthreads();

        // ---- FFTs: F windows at a time ----
        for (int it = 0; it * F < nw; ++it) {
            const int wi = it * F + f;
            const bool active = wi < nw;
            float2 x[8];
            const int wbyte = static_cast<int>(mis) + (active ? wi : 0) * static_cast<int>(a.hop_bytes);
#pragma unroll
            for (int r = 0; r < 8; ++r)
                x[r] = fetch_sample<SFMT>(span, wbyte + nidx[r] * BPS2, lut, a.conv_scale, wreg[r]);
            pass0(x, w8, w83);
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

template <int L, int SFMT>
hipError_t launch_survey_one(const SurveyArgs& a, int ncells, int nenabled, hipStream_t s) {
    using Gm = FftGeom<L>;
    const size_t lds = survey_lds_bytes(L, SFMT, a.hop_bytes);
    if (lds > kSurveyLdsLimit)  // (mi_survey_create has refused such a geometry)
        return hipErrorInvalidValue;
    auto kern = k_survey<L, SFMT>;
    if (lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));
        if (e != hipSuccess)
            return e;
    }
    hipLaunchKernelGGL(kern, dim3(ncells, a.tiles, nenabled), dim3(Gm::BLOCK), lds, s, a);
    return hipGetLastError();
}

template <int L>
hipError_t launch_survey_fmt(const SurveyArgs& a, int sfmt, bool conv_arith, int ncells, int nenabled, hipStream_t s) {
    switch (sfmt) {
        case MI_SFMT_U8:
            return conv_arith ? launch_survey_one<L, kSfmtU8Arith>(a, ncells, nenabled, s) : launch_survey_one<L, MI_SFMT_U8>(a, ncells, nenabled, s);
        case MI_SFMT_S8: return launch_survey_one<L, MI_SFMT_S8>(a, ncells, nenabled, s);
        case MI_SFMT_S16: return launch_survey_one<L, MI_SFMT_S16>(a, ncells, nenabled, s);
        case MI_SFMT_F32: return launch_survey_one<L, MI_SFMT_F32>(a, ncells, nenabled, s);
    }
    return hipErrorInvalidValue;
}

hipError_t launch_survey(const SurveyArgs& a, int log2n, int sfmt, bool conv_arith, int ncells, int nenabled, hipStream_t s) {
    switch (log2n) {
        case 8: return launch_survey_fmt<8>(a, sfmt, conv_arith, ncells, nenabled, s);
        case 9: return launch_survey_fmt<9>(a, sfmt, conv_arith, ncells, nenabled, s);
        case 10: return launch_survey_fmt<10>(a, sfmt, conv_arith, ncells, nenabled, s);
        case 11: return launch_survey_fmt<11>(a, sfmt, conv_arith, ncells, nenabled, s);
        case 12: return launch_survey_fmt<12>(a, sfmt, conv_arith, ncells, nenabled, s);
        case 13: return launch_survey_fmt<13>(a, sfmt, conv_arith, ncells, nenabled, s);
    }
    return hipErrorInvalidValue;
}

int kernel_tw(int log2n) {  // FftGeom<L>::TW
    return log2n <= 10 ? 64 : (log2n == 11 ? 32 : (log2n == 12 ? 16 : 8));
}
static_assert(FftGeom<10>::TW == 64 && FftGeom<11>::TW == 32 && FftGeom<12>::TW == 16 && FftGeom<13>::TW == 8, "kernel_tw restates FftGeom::TW");

}  // namespace
}  // namespace mi

using mi::aligned;
using mi::fail;

extern "C" {

int mi_survey_create(const mi_device_cfg* dev, int nstreams, int max_cells, int windows_per_cell, int gpu, mi_survey** out) {
    if (!dev || !out)
        return fail(MI_ERR_INVALID, "NULL argument");
    *out = nullptr;
    if (nstreams < 1 || nstreams > 65535 || max_cells < 1 || max_cells >= (1 << 24) || windows_per_cell < 0 || windows_per_cell > (1 << 20))
        return fail(MI_ERR_INVALID, "band survey needs 1 <= nstreams < 2^16, 1 <= max_cells < 2^24 and 0 <= windows_per_cell <= 2^20");
    mi::Plan plan;
    if (const int rc = mi::device_plan(*dev, plan))
        return rc;
    if (plan.hop_bytes == 0 || plan.hop_bytes > (1u << 20))
        return fail(MI_ERR_INVALID, "band survey: the hop (sample_rate / 16000 samples) is out of range");
    if (const size_t lds = mi::survey_lds_bytes(plan.log2n, plan.dev.sfmt, static_cast<unsigned>(plan.hop_bytes)); lds > mi::kSurveyLdsLimit)
        return fail(MI_ERR_INVALID, "band survey: a workgroup would need " + std::to_string(lds) + " bytes of LDS at this fft_size, sample format and hop (" +
                                        std::to_string(plan.hop_bytes) + " bytes), over the limit of " + std::to_string(mi::kSurveyLdsLimit) +
                                        " (160 KiB): lower the sample rate");
    if (const int rc = mi::check_gpu(gpu, "no HIP device: the band survey runs on the GPU only"))
        return rc;
    mi_survey* s = new (std::nothrow) mi_survey();
    if (!s)
        return fail(MI_ERR_NOMEM, "host allocation failed");
    s->gpu = gpu;
    s->nstreams = nstreams;
    s->max_cells = max_cells;
    s->wpc = static_cast<uint32_t>(windows_per_cell ? windows_per_cell : MI_WAVE_BATCH);
    s->log2n = plan.log2n;
    s->fft_size = plan.fft_size;
    s->sfmt = plan.dev.sfmt;
    s->sample_bytes = 2 * plan.bytes_per_sample;
    s->conv_arith = plan.conv_arith;
    s->conv_scale = plan.conv_scale;
    s->hop_bytes = plan.hop_bytes;
    // tiles: whole multiples of the kernel's TW windows, at most kMaxTilesPerCell of them to a cell
    const uint32_t tw = static_cast<uint32_t>(mi::kernel_tw(s->log2n));
    const uint32_t want = std::min((s->wpc + tw - 1) / tw, mi::kMaxTilesPerCell);
    s->tile_windows = ((s->wpc + want - 1) / want + tw - 1) / tw * tw;
    s->tiles = (s->wpc + s->tile_windows - 1) / s->tile_windows;
    const size_t partials = static_cast<size_t>(nstreams) * static_cast<size_t>(max_cells) * s->tiles * static_cast<size_t>(s->fft_size);
    std::vector<int> all(static_cast<size_t>(nstreams));
    for (int i = 0; i < nstreams; ++i)
        all[static_cast<size_t>(i)] = i;
    s->nenabled = nstreams;
    if (hipSetDevice(gpu) != hipSuccess || dalloc_copy(s->d_window, plan.window) != hipSuccess || dalloc_copy(s->d_tw, plan.tw) != hipSuccess ||
        dalloc_copy(s->d_levels, plan.levels) != hipSuccess || dalloc_copy(s->d_streams, all) != hipSuccess ||
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
    if (!s || ncells < 1)
        return 0;
    return (static_cast<size_t>(ncells) * s->wpc - 1) * s->hop_bytes + static_cast<size_t>(s->sample_bytes) * static_cast<size_t>(s->fft_size);
}

int mi_survey_process_device(mi_survey* s, const void* d_iq, size_t stream_stride_bytes, int ncells, float* d_mean, float* d_peak, void* hip_stream) {
    if (!s || !d_iq || !d_mean || !d_peak)
        return fail(MI_ERR_INVALID, "NULL argument");
    if (ncells < 1 || ncells > s->max_cells)
        return fail(MI_ERR_INVALID, "ncells outside 1 .. max_cells");
    if (!aligned(d_mean, 16) || !aligned(d_peak, 16))
        return fail(MI_ERR_INVALID, "band survey: d_mean and d_peak must be 16-byte aligned");
    if (!aligned(d_iq, static_cast<uintptr_t>(s->sample_bytes)) || stream_stride_bytes % static_cast<size_t>(s->sample_bytes) != 0)
        return fail(MI_ERR_INVALID, "band survey: d_iq and the stream stride must be aligned to one complex sample");
    if (hipSetDevice(s->gpu) != hipSuccess)
        return fail(MI_ERR_HIP, "hipSetDevice failed");
    hipStream_t q = static_cast<hipStream_t>(hip_stream);
    mi::SurveyArgs a{};
    a.iq = static_cast<const unsigned char*>(d_iq);
    a.stream_stride = stream_stride_bytes;
    a.valid_bytes = mi_survey_bytes_needed(s, ncells);
    a.hop_bytes = static_cast<uint32_t>(s->hop_bytes);
    a.wpc = s->wpc;
    a.tile_windows = s->tile_windows;
    a.tiles = s->tiles;
    a.window = s->d_window;
    a.tw = s->d_tw;
    a.levels = s->d_levels;
    a.conv_scale = s->conv_scale;
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
