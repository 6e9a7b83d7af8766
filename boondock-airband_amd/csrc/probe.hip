// probe.hip -- the channel probe: for a caller-given list of targets {stream, bin}, envelope and phase statistics of that bin over
// each run of windows_per_cell consecutive windows (a cell).  It is the step between the channel finder and a channel plan: the
// survey's planes keep magnitudes, and what tells an AM carrier from a constant-envelope NFM one, and where in its bin a carrier
// sits, is the phase and how the envelope moves from window to window.  Definition: include/mi_airband.h "channel probe".
//
// A post-stage of its own like the band survey (survey.hip): its own handle, two launches on the caller's stream, no atomics.
//   k_probe         one workgroup = one tile of consecutive windows of one stream that has targets.  The windows are the survey's and
//                   stage 1's: their level table and lane setup by their own text (iq_front.hpp), the same conversion x window
//                   and radix-8 passes (fft_radix8.hpp), so a bin's value has the bits of the oracle's ao_fft_forward.  The span
//                   load is iq_front.hpp's load_span written out here: called as the function, the N = 8192 instances spill 16
//                   bytes more.  Behind the last pass, where k_survey takes all bins, lane tau of an FFT
//                   takes the bins of the stream's targets tau, tau + N/8, ... (a stream has at most N) from the natural-order
//                   spectrum in the exchange slot and stores {re, im} at z[target][window], the scratch plane in the handle.
//                   Tiles cut the call's windows, not the cells: the plane makes a window's predecessor a plain load, whatever
//                   tile or cell it lies in.  A tile is walked TW windows of span at a time, as in k_survey.
//   k_probe_reduce  one workgroup of 256 lanes = one (target, cell).
// Order of the four float64 sums of a (target, cell) (fixed, so two runs give the same bytes): lane t adds the terms of the cell's
// windows t, t + 256, t + 512, ... in turn; the 256 lanes' sums are then added by the halving tree -- lane t takes lane t + d for
// d = 128, 64, ... 1.  The term of window w in r_re and r_im is formed from z[w] and z[w - 1]; window 0 of the call has none.
//
// Compile with -ffp-contract=off (the FFT spec; the float64 terms are sums of exact products and do not depend on it).
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/mi_airband.h"
#include "iq_front.hpp"
#include "poststage.hpp"

namespace mi {
namespace {

// a stream that has targets: its slice of the sorted target list
struct ProbeStream {
    int stream, first, count;
};

}  // namespace
}  // namespace mi

struct mi_probe : mi::IqFront {
    mi_probe() : IqFront("channel probe", 2) {}
    int max_targets = 0;
    int ntargets = 0;  // 0 until mi_probe_set_targets
    int nactive = 0;   // streams that have a target
    mi::DevBuf<mi_probe_target> d_targets;  // [max_targets], the first ntargets
    mi::DevBuf<mi::ProbeStream> d_active;   // [nstreams], the first nactive
    mi::DevBuf<float2> d_z;                 // [max_targets][max_cells * wpc], the scratch plane
    // the last mi_probe_process_device (what mi_probe_download reads)
    const mi_probe_cell* last_cells = nullptr;
    size_t last_records = 0;
};

namespace mi {
namespace {

constexpr int kProbeTilePieces = 2;  // a tile is this many TW-window pieces: enough workgroups for one stream, lane setup paid once per tile
constexpr int kReduceBlock = 256;

// The dynamic LDS a k_probe workgroup needs: the tile walk's.  mi_probe_create refuses a geometry whose need exceeds kLdsLimit and
// launch_probe launches with it: one function, so the two cannot drift.  hop_bytes <= 2^20 (mi_probe_create), so nothing here
// wraps.  0: no such kernel instance.
size_t probe_lds_bytes(int log2n, int sfmt, unsigned hop_bytes) {
    return dispatch_log2n(log2n, size_t{0}, [&](auto l) { return tile_lds_bytes<l()>(iq_bps2(sfmt), hop_bytes); });
}

struct ProbeArgs : IqArgs {
    uint32_t nwindows;        // of the call, per stream
    uint32_t tile_windows;    // kProbeTilePieces * TW, set by the launcher
    const ProbeStream* active;        // [gridDim.z]
    const mi_probe_target* targets;
    float2* z;                        // [targets][zstride]
    size_t zstride;
};

template <int L, int SFMT>
__global__ __launch_bounds__(FftGeom<L>::BLOCK) void k_probe(const ProbeArgs a) {
    using Gm = FftGeom<L>;
    constexpr int N = Gm::N, TPF = Gm::TPF, F = Gm::F, TW = Gm::TW, XN = Gm::XN, BLOCK = Gm::BLOCK;
    constexpr int BPS2 = iq_bps2(SFMT);  // bytes per complex sample
    constexpr bool kTwInRegs = L <= 11;

    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int tid = threadIdx.x;
    const ProbeStream as = a.active[blockIdx.z];
    const unsigned wfirst = blockIdx.x * a.tile_windows;                         // first window of the tile, counted from the stream's base
    const int nt = static_cast<int>(min(a.tile_windows, a.nwindows - wfirst));   // its windows: the last tile of the call may be short

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
    // the lane's targets are numbers tau, tau + TPF, ... of the stream's slice (count <= N = 8 TPF, so at most 8): their bins are read
    // where they are used, a few cached loads beside a whole FFT: eight more registers a lane would add to what N = 8192 spills
    const mi_probe_target* tg = a.targets + as.first;
    float2* zrows = a.z + static_cast<size_t>(as.first) * a.zstride;

    const unsigned char* gbase = a.iq + static_cast<size_t>(as.stream) * a.stream_stride;
    for (int s0 = 0; s0 < nt; s0 += TW) {  // the tile, TW windows of span at a time
        const int nw = min(TW, nt - s0);
        if (s0)
            __syncthreads();  // every FFT of the piece before has converted its samples
        // ---- HBM -> LDS: the byte span of this piece, each byte read once, 16 B per lane (load_span, written out) ----
        const long long b0 = (static_cast<long long>(wfirst) + s0) * static_cast<long long>(a.hop_bytes);
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
            // natural-order spectrum now sits in xch: the targets' bins, as stage 1 takes a picked one (rtl_airband.cpp:505-511)
            if (active) {
                const size_t w = static_cast<size_t>(wfirst) + static_cast<size_t>(s0 + wi);  // < nwindows <= zstride
                for (int k = tau; k < as.count; k += TPF)
                    zrows[static_cast<size_t>(k) * a.zstride + w] = xch[xpad(static_cast<int>(tg[k].bin))];
            }
            fft_sync<L>();  // the slot is rewritten by the next window's pass 0
        }
    }
}

// One workgroup = one (target, cell): blockIdx.x = target * ncells + cell.  The order of the sums is the file's head comment.
__global__ __launch_bounds__(kReduceBlock) void k_probe_reduce(const float2* __restrict__ z, const size_t zstride, const uint32_t wpc,
                                                              const uint32_t ncells, mi_probe_cell* __restrict__ cells) {
    __shared__ double sh[4][kReduceBlock];
    const int t = threadIdx.x;
    const uint32_t target = blockIdx.x / ncells, cell = blockIdx.x - target * ncells;
    const float2* row = z + static_cast<size_t>(target) * zstride;
    const size_t w0 = static_cast<size_t>(cell) * wpc;
    double s1 = 0.0, s2 = 0.0, rr = 0.0, ri = 0.0;
    for (uint32_t i = t; i < wpc; i += kReduceBlock) {
        const size_t w = w0 + i;
        const float2 c = row[w];
        const float m = sqrtf(c.x * c.x + c.y * c.y);
        const double md = static_cast<double>(m);
        s1 += md;
        s2 += md * md;
        if (w > 0) {
            const float2 p = row[w - 1];
            const double cr = c.x, ci = c.y, pr = p.x, pi = p.y;
            rr += cr * pr + ci * pi;
            ri += ci * pr - cr * pi;
        }
    }
    sh[0][t] = s1, sh[1][t] = s2, sh[2][t] = rr, sh[3][t] = ri;
    __syncthreads();
    for (int d = kReduceBlock / 2; d >= 1; d >>= 1) {
        if (t < d) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                sh[k][t] += sh[k][t + d];
        }
        __syncthreads();
    }
    if (t == 0) {
        mi_probe_cell r;
        r.s1 = sh[0][0], r.s2 = sh[1][0], r.r_re = sh[2][0], r.r_im = sh[3][0];
        r.windows = wpc;
        r.pairs = wpc - (cell == 0 ? 1u : 0u);
        cells[blockIdx.x] = r;
    }
}

hipError_t launch_probe(ProbeArgs a, int log2n, int sfmt, bool conv_arith, int nactive, hipStream_t s) {
    return dispatch_fft(log2n, sfmt, conv_arith, hipErrorInvalidValue, [&](auto l, auto f) {
        using Gm = FftGeom<l()>;
        a.tile_windows = kProbeTilePieces * Gm::TW;
        const unsigned tiles = (a.nwindows + a.tile_windows - 1) / a.tile_windows;
        return launch_lds(k_probe<l(), f()>, dim3(tiles, 1, nactive), dim3(Gm::BLOCK), probe_lds_bytes(l(), f(), a.hop_bytes), s, a);
    });
}

}  // namespace
}  // namespace mi

using mi::aligned;
using mi::fail;

extern "C" {

int mi_probe_create(const mi_device_cfg* dev, int nstreams, int max_cells, int windows_per_cell, int max_targets, int gpu, mi_probe** out) {
    mi::Plan plan;
    if (const int rc = mi::iq_front_plan("channel probe", dev, out, nstreams, max_cells, windows_per_cell, mi::probe_lds_bytes, mi::kLdsLimit, plan))
        return rc;
    const uint64_t wpc = static_cast<uint64_t>(windows_per_cell ? windows_per_cell : MI_WAVE_BATCH);
    if (max_targets < 1 || static_cast<int64_t>(max_targets) > static_cast<int64_t>(nstreams) * plan.fft_size ||
        static_cast<uint64_t>(max_targets) * static_cast<uint64_t>(max_cells) >= (uint64_t{1} << 31))
        return fail(MI_ERR_INVALID, "channel probe needs 1 <= max_targets <= nstreams * fft_size and max_targets * max_cells < 2^31");
    if (static_cast<uint64_t>(max_cells) * wpc >= (uint64_t{1} << 32))
        return fail(MI_ERR_INVALID, "channel probe: max_cells * windows_per_cell does not fit the 32-bit window count");
    mi_probe* p = nullptr;
    if (const int rc = mi::iq_front_new("channel probe", plan, nstreams, max_cells, windows_per_cell, gpu, &p))
        return rc;
    p->max_targets = max_targets;
    const size_t zlen = static_cast<size_t>(max_targets) * static_cast<size_t>(max_cells) * p->wpc;
    if (hipSetDevice(gpu) != hipSuccess || iq_front_upload(p, plan) != hipSuccess || dalloc(p->d_targets, static_cast<size_t>(max_targets)) != hipSuccess ||
        dalloc(p->d_active, static_cast<size_t>(nstreams)) != hipSuccess || dalloc(p->d_z, zlen) != hipSuccess ||
        hipDeviceSynchronize() != hipSuccess) {
        delete p;
        return fail(MI_ERR_HIP, "channel probe: device allocation failed");
    }
    *out = p;
    return MI_OK;
}

void mi_probe_destroy(mi_probe* p) {
    mi::destroy(p);
}

int mi_probe_set_targets(mi_probe* p, const mi_probe_target* targets, int ntargets) {
    if (!p || !targets)
        return fail(MI_ERR_INVALID, "NULL argument");
    if (ntargets < 1 || ntargets > p->max_targets)
        return fail(MI_ERR_INVALID, "channel probe: ntargets outside 1 .. max_targets");
    std::vector<mi::ProbeStream> active;
    for (int i = 0; i < ntargets; ++i) {
        const mi_probe_target& t = targets[i];
        if (t.stream >= static_cast<uint32_t>(p->nstreams) || t.bin >= static_cast<uint32_t>(p->fft_size))
            return fail(MI_ERR_INVALID, "channel probe: a target's stream or bin is out of range");
        if (i && (t.stream < targets[i - 1].stream || (t.stream == targets[i - 1].stream && t.bin <= targets[i - 1].bin)))
            return fail(MI_ERR_INVALID, "channel probe: the targets must be strictly ascending by (stream, bin)");
        if (active.empty() || active.back().stream != static_cast<int>(t.stream))
            active.push_back(mi::ProbeStream{static_cast<int>(t.stream), i, 0});
        active.back().count += 1;
    }
    // (a call still queued reads the lists it was made with)
    if (!mi::sync_copy(p->gpu, p->d_targets, targets, static_cast<size_t>(ntargets) * sizeof(mi_probe_target), hipMemcpyHostToDevice) ||
        hipMemcpy(p->d_active, active.data(), active.size() * sizeof(mi::ProbeStream), hipMemcpyHostToDevice) != hipSuccess) {
        p->ntargets = 0;  // the device lists may be torn: a call is refused until a list has been set
        return fail(MI_ERR_HIP, "channel probe: uploading the target list failed");
    }
    p->ntargets = ntargets;
    p->nactive = static_cast<int>(active.size());
    return MI_OK;
}

size_t mi_probe_bytes_needed(const mi_probe* p, int ncells) {
    return mi::iq_bytes_needed(p, ncells);
}

int mi_probe_process_device(mi_probe* p, const void* d_iq, size_t stream_stride_bytes, int ncells, mi_probe_cell* d_cells, void* hip_stream) {
    if (!p || !d_iq || !d_cells)
        return fail(MI_ERR_INVALID, "NULL argument");
    if (p->ntargets < 1)
        return fail(MI_ERR_INVALID, "channel probe: no target list set (mi_probe_set_targets)");
    if (const int rc = mi::iq_call_ok(p, d_iq, stream_stride_bytes, ncells, aligned(d_cells, 8), "d_cells must be 8-byte aligned"))
        return rc;
    if (hipSetDevice(p->gpu) != hipSuccess)
        return fail(MI_ERR_HIP, "hipSetDevice failed");
    hipStream_t q = static_cast<hipStream_t>(hip_stream);
    mi::ProbeArgs a{};
    mi::iq_args(a, p, d_iq, stream_stride_bytes, ncells);
    a.nwindows = static_cast<uint32_t>(ncells) * p->wpc;
    a.active = p->d_active;
    a.targets = p->d_targets;
    a.z = p->d_z;
    a.zstride = static_cast<size_t>(p->max_cells) * p->wpc;
    p->timing.stamp(0, q);
    if (mi::launch_probe(a, p->log2n, p->sfmt, p->conv_arith, p->nactive, q) != hipSuccess)
        return fail(MI_ERR_HIP, "channel probe kernel launch failed");
    p->timing.stamp(1, q);
    const size_t records = static_cast<size_t>(p->ntargets) * static_cast<size_t>(ncells);  // < 2^31 (mi_probe_create)
    hipLaunchKernelGGL(mi::k_probe_reduce, dim3(static_cast<unsigned>(records)), dim3(mi::kReduceBlock), 0, q, p->d_z.get(), a.zstride, p->wpc,
                       static_cast<uint32_t>(ncells), d_cells);
    p->timing.stamp(2, q);
    if (hipGetLastError() != hipSuccess)
        return fail(MI_ERR_HIP, "channel probe kernel launch failed");
    p->called = p->timing.on;  // (a stamped call: last_launch_ms refuses after any other)
    p->last_cells = d_cells;
    p->last_records = records;
    return MI_OK;
}

int mi_probe_download(mi_probe* p, void* hip_stream, mi_probe_cell* cells) {
    if (!p || !cells)
        return fail(MI_ERR_INVALID, "NULL argument");
    if (!p->last_cells)
        return fail(MI_ERR_INVALID, "no mi_probe_process_device call to download");
    hipStream_t q = static_cast<hipStream_t>(hip_stream);
    if (hipSetDevice(p->gpu) != hipSuccess ||
        hipMemcpyAsync(cells, p->last_cells, p->last_records * sizeof(mi_probe_cell), hipMemcpyDeviceToHost, q) != hipSuccess ||
        hipStreamSynchronize(q) != hipSuccess)
        return fail(MI_ERR_HIP, "channel probe: download failed");
    return MI_OK;
}

int mi_probe_set_timing(mi_probe* p, int on) {
    return mi::set_timing(p, on);
}

int mi_probe_last_launch_ms(mi_probe* p, float* ms) {
    return mi::last_launch_ms(p, ms, "mi_probe_process_device");
}

}  // extern "C"
