// channelize_l64.hip -- ahead-of-time instance and launcher of the lane-resident stage 1 (l64_kernel.h).
//
// The kernel takes its pruning masks at compile time.  Built here: the full graph (any plan at N = 512, 1024 or 2048 with a
// supported hop).
// A plan's own instance -- exactly its butterflies, straight-line -- is compiled by hipRTC when the handle is created
// (l64_jit.cpp) and launched through the module API; if that is not possible the full-graph instance below runs instead.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.hpp"
#include "l64_kernel.h"

namespace mi {
namespace {

struct FullMasks {
    static constexpr unsigned long long n[6] = {0x3ull, 0xfull, 0xffull, 0xffffull, 0xffffffffull, ~0ull};
};

template <int HOP, int LOG2N, bool MASKED>
__global__ __launch_bounds__(256, 2) void k_channelize_l64(const L64Args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char l64_lds[];
    mi_l64::l64_body<HOP, FullMasks, LOG2N, MASKED>(a, l64_lds);
}

using Kern = void (*)(const L64Args);
template <bool MASKED>
Kern full_instance(int log2n, unsigned hop) {
    switch (log2n) {
        case 9: return hop == 160 ? k_channelize_l64<160, 9, MASKED> : k_channelize_l64<128, 9, MASKED>;
        case 10: return hop == 160 ? k_channelize_l64<160, 10, MASKED> : k_channelize_l64<128, 10, MASKED>;
        case 11: return hop == 160 ? k_channelize_l64<160, 11, MASKED> : k_channelize_l64<128, 11, MASKED>;
    }
    return nullptr;
}

// the kernel's geometry of one FFT size (mi_l64::Geo) as run-time values: the host sizes LDS by the constants the kernel addresses with
struct GeoRt {
    unsigned n, tile, zrow, padw;
    int round_windows;
};
template <int LOG2N>
GeoRt geo_rt(int m6) {
    using G = mi_l64::Geo<LOG2N>;
    return {static_cast<unsigned>(G::kN), static_cast<unsigned>(G::kTile), static_cast<unsigned>(G::kZRow), G::kPadW, G::round_windows(m6)};
}
GeoRt geo_of(int log2n, int m6) {
    return log2n == 9 ? geo_rt<9>(m6) : (log2n == 10 ? geo_rt<10>(m6) : geo_rt<11>(m6));
}

}  // namespace

// windows of a wave that go through the exchange buffer per round
int l64_round_windows(int log2n, int m6) {
    return geo_of(log2n, m6).round_windows;
}
int l64_zstride(int log2n, int m6) {
    int zs = m6 * static_cast<int>(geo_of(log2n, m6).zrow);
    while ((zs / 4) % 32 != 16)  // consecutive windows 16 write banks apart
        zs += 16;
    return zs;
}

bool l64_supported(int log2n, size_t hop_bytes, int bytes_per_sample) {
    const size_t hop = hop_bytes / (2 * static_cast<size_t>(bytes_per_sample));
    return log2n >= 9 && log2n <= 11 && (hop == 160 || hop == 128);
}

// dynamic LDS of a workgroup: the span (or the exchange buffer over it), window table, level table, ticket word, output rows
size_t l64_lds_bytes(int log2n, unsigned hop, int m6, int nch, int n_iq_rows, unsigned* region_bytes) {
    const GeoRt g = geo_of(log2n, m6);
    const unsigned n = g.n, tile = g.tile, padw = g.padw;
    const unsigned nsamp = (tile - 1) * hop + n;
    const unsigned padb = 4u * ((padw - 2u * hop) & 63u);
    const unsigned span = (8u * nsamp + padb * ((nsamp + hop - 1) / hop) + 15u) & ~15u;
    const unsigned zbuf = (4u * static_cast<unsigned>(g.round_windows) * static_cast<unsigned>(l64_zstride(log2n, m6)) + 15u) & ~15u;
    const unsigned region = std::max(span, zbuf);
    if (region_bytes)
        *region_bytes = region;
    return static_cast<size_t>(region) + 4 * n + 1024 + 16 + static_cast<size_t>(nch) * tile * 4 + static_cast<size_t>(n_iq_rows) * tile * 8;
}

hipError_t launch_channelize_l64(const ChannelizeArgs& c, int log2n, int sfmt, int nstreams, hipStream_t s) {
    const unsigned bps2 = sfmt == MI_SFMT_S16 ? 4u : (sfmt == MI_SFMT_F32 ? 8u : 2u);
    const unsigned hop = c.hop_bytes / bps2;
    if (!l64_supported(log2n, c.hop_bytes, static_cast<int>(bps2 / 2u)))
        return hipErrorInvalidValue;
    const L64Jit* jit = c.l64_jit;  // the plan's own instance, if it could be compiled (of a launch with a stream list: the one that takes it)
    const int m6 = jit ? c.l64.m6 : 64;
    const unsigned tile = geo_of(log2n, m6).tile;
    L64Args a{};
    a.iq = c.iq;
    a.stream_stride = c.stream_stride;
    a.valid_bytes = c.valid_bytes;
    a.nfft = c.nfft;
    a.plane_off = c.plane_off;
    a.mag = c.mag;
    a.cplx = reinterpret_cast<float*>(c.cplx);
    a.plane_stride = c.plane_stride;
    a.window = c.window;
    a.levels = c.levels;
    a.conv_scale = c.conv_scale;
    a.nch = c.nch;
    a.n_iq_rows = c.n_iq_rows;
    a.xmax = c.xmax;
    a.chan = jit ? c.l64_chan : c.l64_chan_full;
    a.nb_pad = c.l64.nb_pad;
    a.zstride = static_cast<unsigned>(l64_zstride(log2n, m6));
    // (the exchange buffer of the combining stages, 4 waves x round windows x zstride, lies over the span; with every class
    // live at N = 2048 it is the larger of the two)
    const size_t lds = l64_lds_bytes(log2n, hop, m6, c.nch, c.n_iq_rows, &a.span_bytes);
    a.ntiles = (c.nfft + tile - 1) / tile;
    a.sfmt = sfmt;
    a.linear_tiles = c.l64.linear_tiles;
    if (c.streams)  // a launch over some of the handle's streams
        nstreams = c.nactive;
    if (lds > 160 * 1024 || static_cast<unsigned long long>(a.ntiles) * static_cast<unsigned>(nstreams) >= (1ull << 32))
        return hipErrorInvalidValue;
    a.nstreams = static_cast<unsigned>(nstreams);
    a.streams = c.streams;
    // persistent workgroups that draw runs of contiguous tiles from a ticket counter (l64_kernel.h): as many as the machine
    // holds at once when this launch has it to itself -- fewer are resident when other kernels of the pipeline run alongside,
    // the rest then find the tickets gone
    const unsigned long long ttotal = static_cast<unsigned long long>(a.ntiles) * a.nstreams;
    static const int cus = [] {  // (a property of the machine, asked once)
        int dev = 0, n = 256;
        if (hipGetDevice(&dev) == hipSuccess)
            (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
        return n > 0 ? n : 256;
    }();
    // a multiple of the workgroups a CU holds at once (3 when the instance was compiled for three waves per SIMD and its LDS
    // allows it, else 2): a remainder would queue behind the resident ones and leave CUs idle at the end
    const int resident = (jit && l64_jit_minwaves(jit) >= 3 && lds * 3 <= 160 * 1024) ? 3 : (lds * 2 <= 160 * 1024 ? 2 : 1);
    const unsigned long long want = static_cast<unsigned long long>(cus) * (c.l64.wg_per_cu > 0 ? c.l64.wg_per_cu : 2 * resident);
    // runs of up to 8 tiles (output cache lines shared by neighbouring tiles stay in one workgroup), shorter when the launch is
    // small: at least ~8 runs per workgroup, so that the last ones to finish are not far behind
    if (!c.l64_tickets || !c.l64_ticket_seq)
        return hipErrorInvalidValue;
    unsigned run = static_cast<unsigned>(ttotal / (want * 8ull));
    run = run < 1u ? 1u : (run > 8u ? 8u : run);
    a.run_tiles = run;
    const unsigned long long nruns = (ttotal + run - 1) / run;
    const unsigned gx = static_cast<unsigned>(nruns < want ? nruns : want);
    a.ticket = c.l64_tickets + (*c.l64_ticket_seq)++ % kL64Tickets;
    {
        hipError_t e = hipMemsetAsync(a.ticket, 0, sizeof(unsigned), s);
        if (e != hipSuccess)
            return e;
    }
    if (jit)
        return l64_jit_launch(jit, a, gx, 1u, lds, s);
    const Kern kern = c.streams ? full_instance<true>(log2n, hop) : full_instance<false>(log2n, hop);
    if (lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));
        if (e != hipSuccess)
            return e;
    }
    hipLaunchKernelGGL(kern, dim3(gx), dim3(256), lds, s, a);
    return hipGetLastError();
}

}  // namespace mi
