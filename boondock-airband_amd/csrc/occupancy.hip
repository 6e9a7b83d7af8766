// occupancy.hip -- the channel finder: from the band survey's planes (survey.hip: mean and peak per stream, cell and bin) to a record
// per bin -- noise floor, threshold, which cells are active -- and to channel candidates, the maximal runs of occupied bins in
// frequency order.  include/mi_airband.h "channel finder" holds the definition; mi_occupancy_plan_host (poststage_host.cpp) is the host
// twin, and the device equals it byte for byte.
//
// A post-stage of its own like the band survey: its own handle, four launches on the caller's stream, no floating-point atomics.
//   k_occ_bins   one workgroup = 64 consecutive bins of one stream x kOccWaves waves.  Lane l of every wave owns bin b0 + l; wave w
//                owns the cells [w * seg, (w + 1) * seg), seg = ceil(ncells / kOccWaves), and reads one cell's 64 floats at a time, a
//                coalesced 256-byte line.  The floor is an exact radix select on the float's bits (non-negative floats order as their
//                bit patterns do): four rounds of 8 bits from the top, each one pass over the column that counts, with integer LDS
//                atomics, the digits of the values still matching the prefix found so far -- hist[digit][bin], so the 64 lanes of a
//                wave hit 64 distinct counters -- and then picks per bin the digit that holds rank k.  Counts are order-free, so the
//                result does not depend on which wave adds first.  A fifth pass takes each wave's segment in cell order: active
//                count, first, last, runs, the two maxima, and whether the segment's first and last cell are active; wave 0 joins the
//                segments in order (two runs that touch across a boundary are one) and writes the 32-byte record.
//   k_occ_mark   one workgroup per stream walks the positions p = (bin + N / 2) % N in tiles of 256: a position is a run start when it
//                is occupied and the one below is not.  rank[stream][p] = the start's number within the stream (-1: no start), and the
//                stream's count.
//   launch_row_scan (poststage.hip), rows = streams: d_stream_first and d_count.
//   k_occ_write  one lane per position; the lane of a run start walks its run and writes the candidate at stream_first + rank unless
//                that is at or beyond the capacity.  The all-occupied band is one lane walking N positions.
//
// Compile with -ffp-contract=off: threshold = floor * ratio is one float32 multiply.
#include <hip/hip_runtime.h>

#include <cmath>
#include <new>
#include <string>
#include <vector>

#include "../../include/mi_airband.h"
#include "poststage.hpp"

struct mi_occupancy : mi::Stage {
    mi_occupancy() : Stage("channel finder", 4) {}
    int nstreams = 0;
    int max_cells = 0;
    int log2n = 0, fft_size = 0;
    mi_occ_cfg cfg{};
    uint32_t max_candidates = 0;
    mi::DevBuf<uint8_t> d_enabled;        // [nstreams] 0 / 1
    mi::DevBuf<int> d_rank;               // [nstreams][fft_size]: a run start's number within its stream, -1 elsewhere
    mi::DevBuf<uint32_t> d_stream_count;  // [nstreams]
    mi::PinnedBuf<uint32_t> h_count;      // [2], landing place of the counts in mi_occupancy_download
    // destinations of the last mi_occupancy_process_device (what mi_occupancy_download reads)
    const mi_occ_bin* last_bins = nullptr;
    const mi_occ_candidate* last_cands = nullptr;
    const uint32_t* last_stream_first = nullptr;
    const uint32_t* last_count = nullptr;
};

namespace {

using mi::aligned;
using mi::fail;

constexpr int kOccBins = 64;                       // bins per workgroup: one per lane
constexpr int kOccWaves = 16;                      // cell segments per workgroup
constexpr int kOccBlock = kOccBins * kOccWaves;    // 1024
constexpr int kOccDigits = 256;                    // 8 bits a round
constexpr int kOccLoads = 4;                       // cells a wave has in flight
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr size_t kOccLdsBytes = sizeof(uint32_t) * (kOccDigits + kOccWaves + 2) * kOccBins;  // 70144 of the CU's 160 KB
static_assert(kOccDigits % kOccWaves == 0, "every wave sums the same number of digits");

// a wave's view of its segment in the fifth pass
struct Segment {
    uint32_t active, first, last, runs;
    uint32_t max_mean, max_peak;  // float bits: non-negative floats order as their bit patterns do, whatever the denormal mode
    uint32_t ends;  // bit 0: the segment's first cell is active, bit 1: its last cell is
};

__global__ __launch_bounds__(kOccBlock) void k_occ_bins(const uint8_t* __restrict__ enabled, const float* __restrict__ mean, const float* __restrict__ peak,
                                                        const int n, const int ncells, const uint32_t kth, const float ratio,
                                                        mi_occ_bin* __restrict__ bins) {
    const int stream = blockIdx.y;
    if (!enabled[stream])
        return;
    // hist [256][64] counters (behind the select the segments' partials lie over them), part [waves][64] = the counts of a wave's 16
    // digits, then the prefix and the rank per bin: kOccLdsBytes of dynamic LDS, as survey.hip asks for its own
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    uint32_t* hist = lds;
    uint32_t(*part)[kOccBins] = reinterpret_cast<uint32_t(*)[kOccBins]>(lds + kOccDigits * kOccBins);
    uint32_t* s_prefix = lds + (kOccDigits + kOccWaves) * kOccBins;
    uint32_t* s_rank = s_prefix + kOccBins;
    static_assert(sizeof(Segment) * kOccWaves * kOccBins <= sizeof(uint32_t) * kOccDigits * kOccBins, "the partials fit the histogram's space");

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int bin = blockIdx.x * kOccBins + lane;  // < n: n is a multiple of 64
    const int seg = (ncells + kOccWaves - 1) / kOccWaves;
    const int c0 = min(wave * seg, ncells), c1 = min(c0 + seg, ncells);
    const float* col = mean + static_cast<size_t>(stream) * ncells * n + bin;
    const float* pcol = peak + static_cast<size_t>(stream) * ncells * n + bin;

    if (wave == 0) {
        s_prefix[lane] = 0;
        s_rank[lane] = kth;
    }
    // ---- the floor: rank kth of the column, 8 bits a round from the top ----
    for (int round = 0; round < 4; ++round) {
        const int shift = 24 - 8 * round;
        for (int i = tid; i < kOccDigits * kOccBins; i += kOccBlock)
            hist[i] = 0;
        __syncthreads();
        const uint32_t prefix = s_prefix[lane];
        const uint32_t himask = round ? ~0u << (shift + 8) : 0u;  // the bits the earlier rounds settled
        for (int c = c0; c < c1; c += kOccLoads) {
            uint32_t v[kOccLoads];
#pragma unroll
            for (int j = 0; j < kOccLoads; ++j)
                v[j] = c + j < c1 ? __float_as_uint(col[static_cast<size_t>(c + j) * n]) : 0u;
#pragma unroll
            for (int j = 0; j < kOccLoads; ++j)
                if (c + j < c1 && (v[j] & himask) == prefix)
                    atomicAdd(&hist[((v[j] >> shift) & 255u) * kOccBins + lane], 1u);
        }
        __syncthreads();
        // wave w: the counts of digits 16 w .. 16 w + 15 of every bin
        uint32_t sum = 0;
#pragma unroll
        for (int d = 0; d < kOccDigits / kOccWaves; ++d)
            sum += hist[(wave * (kOccDigits / kOccWaves) + d) * kOccBins + lane];
        part[wave][lane] = sum;
        __syncthreads();
        if (wave == 0) {  // the digit whose counter holds rank r: it exists, the counters of a bin add up to more than r
            uint32_t r = s_rank[lane];
            int w = 0;
            while (w < kOccWaves - 1 && r >= part[w][lane]) {
                r -= part[w][lane];
                ++w;
            }
            int d = w * (kOccDigits / kOccWaves);
            const int dlast = d + kOccDigits / kOccWaves - 1;
            while (d < dlast && r >= hist[d * kOccBins + lane]) {
                r -= hist[d * kOccBins + lane];
                ++d;
            }
            s_rank[lane] = r;
            s_prefix[lane] = prefix | (static_cast<uint32_t>(d) << shift);
        }
        __syncthreads();
    }
    const float floor_v = __uint_as_float(s_prefix[lane]);
    const float threshold = __fmul_rn(floor_v, ratio);

    // ---- the bin record: every wave its segment in cell order ----
    const uint32_t tbits = __float_as_uint(threshold);
    Segment sg{0, kNone, kNone, 0, 0u, 0u, 0};
    bool before = false;
    for (int c = c0; c < c1; c += kOccLoads) {
        uint32_t m[kOccLoads], p[kOccLoads];
#pragma unroll
        for (int j = 0; j < kOccLoads; ++j) {
            const bool in = c + j < c1;
            m[j] = in ? __float_as_uint(col[static_cast<size_t>(c + j) * n]) : 0u;
            p[j] = in ? __float_as_uint(pcol[static_cast<size_t>(c + j) * n]) : 0u;
        }
#pragma unroll
        for (int j = 0; j < kOccLoads; ++j) {
            if (c + j >= c1)
                break;
            const bool active = m[j] > tbits;
            if (active) {
                sg.active += 1;
                sg.first = sg.first == kNone ? static_cast<uint32_t>(c + j) : sg.first;
                sg.last = static_cast<uint32_t>(c + j);
                sg.runs += before ? 0u : 1u;
                sg.max_mean = max(sg.max_mean, m[j]);
                sg.max_peak = max(sg.max_peak, p[j]);
                if (c + j == c0)
                    sg.ends |= 1u;
            }
            before = active;
        }
    }
    if (before)
        sg.ends |= 2u;  // (an empty segment leaves `before` false)
    Segment* segs = reinterpret_cast<Segment*>(hist);  // the last round's select is behind a barrier
    segs[wave * kOccBins + lane] = sg;
    __syncthreads();
    if (wave == 0) {
        Segment t = sg;  // segment 0 is never empty: ncells >= 1
        for (int w = 1; w < kOccWaves; ++w) {
            if (min(w * seg, ncells) >= ncells)  // empty, as are all behind it
                break;
            const Segment u = segs[w * kOccBins + lane];
            t.runs += u.runs - (((t.ends & 2u) && (u.ends & 1u)) ? 1u : 0u);
            t.active += u.active;
            t.first = t.first == kNone ? u.first : t.first;
            t.last = u.last == kNone ? t.last : u.last;
            t.max_mean = max(t.max_mean, u.max_mean);
            t.max_peak = max(t.max_peak, u.max_peak);
            t.ends = (t.ends & 1u) | (u.ends & 2u);
        }
        uint4* out = reinterpret_cast<uint4*>(bins + static_cast<size_t>(stream) * n + bin);
        out[0] = make_uint4(__float_as_uint(floor_v), __float_as_uint(threshold), t.active, t.first);
        out[1] = make_uint4(t.last, t.runs, t.max_mean, t.max_peak);
    }
}

__device__ __forceinline__ bool occupied_at(const mi_occ_bin* __restrict__ sb, const int n, const int p, const uint32_t min_cells) {
    return sb[(p + n / 2) & (n - 1)].active_cells >= min_cells;
}

// One workgroup per stream: run starts in position order, their numbers, their count.
__global__ __launch_bounds__(mi::kScanTile) void k_occ_mark(const uint8_t* __restrict__ enabled, const mi_occ_bin* __restrict__ bins, const int n,
                                                            const uint32_t min_cells, int* __restrict__ rank, uint32_t* __restrict__ stream_count) {
    __shared__ uint32_t wave_sum[mi::kScanTile / 64];
    const int stream = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (!enabled[stream]) {  // (the whole workgroup)
        if (t == 0)
            stream_count[stream] = 0;
        return;
    }
    const mi_occ_bin* sb = bins + static_cast<size_t>(stream) * n;
    uint32_t running = 0;
    for (int p0 = 0; p0 < n; p0 += mi::kScanTile) {  // n is a multiple of 256
        const int p = p0 + t;
        const bool start = occupied_at(sb, n, p, min_cells) && (p == 0 || !occupied_at(sb, n, p - 1, min_cells));
        const unsigned long long m = __ballot(start);
        if (lane == 0)
            wave_sum[wave] = static_cast<uint32_t>(__popcll(m));
        __syncthreads();
        uint32_t below = 0, tile = 0;
        for (int w = 0; w < mi::kScanTile / 64; ++w) {
            const uint32_t s = wave_sum[w];
            below += w < wave ? s : 0u;
            tile += s;
        }
        rank[static_cast<size_t>(stream) * n + p] = start ? static_cast<int>(running + below + __popcll(m & ((1ull << lane) - 1ull))) : -1;
        running += tile;
        __syncthreads();  // wave_sum is rewritten by the next tile
    }
    if (t == 0)
        stream_count[stream] = running;
}

// One lane per position of one stream; a run start's lane walks the run.
__global__ __launch_bounds__(256) void k_occ_write(const uint8_t* __restrict__ enabled, const mi_occ_bin* __restrict__ bins, const int* __restrict__ rank,
                                                   const uint32_t* __restrict__ stream_first, const int n, const uint32_t min_cells,
                                                   const uint32_t max_candidates, mi_occ_candidate* __restrict__ cands) {
    const int stream = blockIdx.y, p = blockIdx.x * 256 + threadIdx.x;  // p < n: n is a multiple of 256
    if (!enabled[stream])
        return;
    const int r = rank[static_cast<size_t>(stream) * n + p];
    if (r < 0)
        return;
    const uint32_t k = stream_first[stream] + static_cast<uint32_t>(r);
    if (k >= max_candidates)
        return;
    const mi_occ_bin* sb = bins + static_cast<size_t>(stream) * n;
    const int half = n / 2, mask = n - 1;
    int best = (p + half) & mask, q = p + 1;
    uint32_t best_mean = __float_as_uint(sb[best].max_mean);  // compared as bits, as k_occ_bins does
    for (; q < n; ++q) {
        const mi_occ_bin& b = sb[(q + half) & mask];
        if (b.active_cells < min_cells)
            break;
        if (__float_as_uint(b.max_mean) > best_mean) {  // ties stay with the lowest position
            best_mean = __float_as_uint(b.max_mean);
            best = (q + half) & mask;
        }
    }
    const mi_occ_bin& bb = sb[best];
    uint2* out = reinterpret_cast<uint2*>(cands + k);
    out[0] = make_uint2(static_cast<uint32_t>(stream), static_cast<uint32_t>(best));
    out[1] = make_uint2(static_cast<uint32_t>((p + half) & mask), static_cast<uint32_t>((q - 1 + half) & mask));
    out[2] = make_uint2(static_cast<uint32_t>(q - p), bb.active_cells);
    out[3] = make_uint2(bb.first_cell, bb.last_cell);
    out[4] = make_uint2(__float_as_uint(bb.max_mean), __float_as_uint(bb.max_peak));
}

std::vector<uint8_t> stream_flags(const uint8_t* stream_enabled, int nstreams) {
    std::vector<uint8_t> f(static_cast<size_t>(nstreams), 1);
    for (int i = 0; stream_enabled && i < nstreams; ++i)
        f[static_cast<size_t>(i)] = stream_enabled[i] ? 1 : 0;
    return f;
}

}  // namespace

extern "C" {

int mi_occupancy_create(const mi_device_cfg* dev, const mi_occ_cfg* cfg, int nstreams, int max_cells, size_t max_candidates, int gpu,
                        mi_occupancy** out) {
    if (!dev || !out)
        return fail(MI_ERR_INVALID, "NULL argument");
    *out = nullptr;
    if (nstreams < 1 || nstreams > 65535 || max_cells < 1 || max_cells >= (1 << 24))
        return fail(MI_ERR_INVALID, "channel finder needs 1 <= nstreams < 2^16 and 1 <= max_cells < 2^24");
    mi_occ_cfg c;
    int log2n = 0;
    if (const int rc = mi::occ_settings(dev, cfg, &c, &log2n))
        return rc;
    if (c.min_cells > static_cast<uint32_t>(max_cells))
        return fail(MI_ERR_INVALID, "channel finder: min_cells must be at most max_cells");
    if (const int rc = mi::check_gpu(gpu, "no HIP device: the channel finder runs on the GPU only"))
        return rc;
    mi_occupancy* o = new (std::nothrow) mi_occupancy();
    if (!o)
        return fail(MI_ERR_NOMEM, "host allocation failed");
    o->gpu = gpu;
    o->nstreams = nstreams;
    o->max_cells = max_cells;
    o->log2n = log2n;
    o->fft_size = 1 << log2n;
    o->cfg = c;
    const size_t most = static_cast<size_t>(nstreams) * static_cast<size_t>(o->fft_size) / 2;  // (below 2^28)
    o->max_candidates = static_cast<uint32_t>(max_candidates && max_candidates < most ? max_candidates : most);
    const std::vector<uint8_t> all = stream_flags(nullptr, nstreams);
    if (hipSetDevice(gpu) != hipSuccess ||
        hipFuncSetAttribute(reinterpret_cast<const void*>(k_occ_bins), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(kOccLdsBytes)) !=
            hipSuccess ||
        dalloc_copy(o->d_enabled, all) != hipSuccess ||
        dalloc(o->d_rank, static_cast<size_t>(nstreams) * static_cast<size_t>(o->fft_size)) != hipSuccess ||
        dalloc(o->d_stream_count, static_cast<size_t>(nstreams)) != hipSuccess ||
        hipHostMalloc(reinterpret_cast<void**>(o->h_count.put()), 2 * sizeof(uint32_t)) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
        delete o;
        return fail(MI_ERR_HIP, "channel finder: device allocation failed");
    }
    *out = o;
    return MI_OK;
}

void mi_occupancy_destroy(mi_occupancy* o) {
    mi::destroy(o);
}

int mi_occupancy_set_streams(mi_occupancy* o, const uint8_t* stream_enabled) {
    if (!o)
        return fail(MI_ERR_INVALID, "NULL argument");
    const std::vector<uint8_t> f = stream_flags(stream_enabled, o->nstreams);
    bool any = false;
    for (const uint8_t v : f)
        any = any || v;
    if (!any)
        return fail(MI_ERR_INVALID, "channel finder: no stream enabled");
    // (a call still queued reads the mask it was made with)
    if (!mi::sync_copy(o->gpu, o->d_enabled, f.data(), f.size(), hipMemcpyHostToDevice))
        return fail(MI_ERR_HIP, "channel finder: uploading the stream mask failed");
    return MI_OK;
}

int mi_occupancy_process_device(mi_occupancy* o, const float* d_mean, const float* d_peak, int ncells, mi_occ_bin* d_bins, mi_occ_candidate* d_cands,
                                uint32_t* d_stream_first, uint32_t* d_count, void* hip_stream) {
    if (!o || !d_mean || !d_peak || !d_bins || !d_cands || !d_stream_first || !d_count)
        return fail(MI_ERR_INVALID, "NULL argument");
    if (ncells < 1 || ncells > o->max_cells)
        return fail(MI_ERR_INVALID, "ncells outside 1 .. max_cells");
    if (!aligned(d_mean, 16) || !aligned(d_peak, 16) || !aligned(d_bins, 16) || !aligned(d_cands, 8) || !aligned(d_stream_first, 4) ||
        !aligned(d_count, 4))
        return fail(MI_ERR_INVALID, "channel finder: d_mean, d_peak and d_bins must be 16-byte aligned, d_cands 8-byte aligned");
    if (hipSetDevice(o->gpu) != hipSuccess)
        return fail(MI_ERR_HIP, "hipSetDevice failed");
    hipStream_t q = static_cast<hipStream_t>(hip_stream);
    const int n = o->fft_size;
    const unsigned ns = static_cast<unsigned>(o->nstreams);
    const uint32_t kth = static_cast<uint32_t>(static_cast<uint64_t>(ncells - 1) * o->cfg.floor_permille / 1000);
    o->timing.stamp(0, q);
    hipLaunchKernelGGL(k_occ_bins, dim3(static_cast<unsigned>(n / kOccBins), ns), dim3(kOccBlock), kOccLdsBytes, q, o->d_enabled.get(), d_mean, d_peak, n, ncells, kth,
                       o->cfg.ratio, d_bins);
    o->timing.stamp(1, q);
    hipLaunchKernelGGL(k_occ_mark, dim3(ns), dim3(mi::kScanTile), 0, q, o->d_enabled.get(), d_bins, n, o->cfg.min_cells, o->d_rank.get(),
                       o->d_stream_count.get());
    o->timing.stamp(2, q);
    mi::launch_row_scan(q, o->d_stream_count, o->nstreams, o->max_candidates, d_stream_first, d_count);
    o->timing.stamp(3, q);
    hipLaunchKernelGGL(k_occ_write, dim3(static_cast<unsigned>(n / 256), ns), dim3(256), 0, q, o->d_enabled.get(), d_bins, o->d_rank.get(), d_stream_first, n,
                       o->cfg.min_cells, o->max_candidates, d_cands);
    o->timing.stamp(4, q);
    if (hipGetLastError() != hipSuccess)
        return fail(MI_ERR_HIP, "channel finder kernel launch failed");
    o->called = o->timing.on;  // (a stamped call: last_launch_ms refuses after any other)
    o->last_bins = d_bins;
    o->last_cands = d_cands;
    o->last_stream_first = d_stream_first;
    o->last_count = d_count;
    return MI_OK;
}

int mi_occupancy_download(mi_occupancy* o, void* hip_stream, mi_occ_bin* bins, mi_occ_candidate* cands, uint32_t* stream_first, uint32_t* count) {
    if (!o || !count)
        return fail(MI_ERR_INVALID, "NULL argument");
    if (!o->last_count)
        return fail(MI_ERR_INVALID, "no mi_occupancy_process_device call to download");
    hipStream_t q = static_cast<hipStream_t>(hip_stream);
    if (!mi::land_counts(o->gpu, q, o->h_count, o->last_count, count))
        return fail(MI_ERR_HIP, "channel finder: reading the counts failed");
    const size_t k = count[1];
    bool ok = true;
    if (bins)
        ok = ok && hipMemcpyAsync(bins, o->last_bins, static_cast<size_t>(o->nstreams) * static_cast<size_t>(o->fft_size) * sizeof(mi_occ_bin),
                                  hipMemcpyDeviceToHost, q) == hipSuccess;
    if (cands && k)
        ok = ok && hipMemcpyAsync(cands, o->last_cands, k * sizeof(mi_occ_candidate), hipMemcpyDeviceToHost, q) == hipSuccess;
    if (stream_first)
        ok = ok && hipMemcpyAsync(stream_first, o->last_stream_first, (static_cast<size_t>(o->nstreams) + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost,
                                  q) == hipSuccess;
    if (!ok || hipStreamSynchronize(q) != hipSuccess)
        return fail(MI_ERR_HIP, "channel finder: download failed");
    return MI_OK;
}

int mi_occupancy_set_timing(mi_occupancy* o, int on) {
    return mi::set_timing(o, on);
}

int mi_occupancy_last_launch_ms(mi_occupancy* o, float* ms) {
    return mi::last_launch_ms(o, ms, "mi_occupancy_process_device");
}

}  // extern "C"
