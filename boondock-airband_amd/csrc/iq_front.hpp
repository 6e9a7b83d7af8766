// iq_front.hpp -- what the kernels that read raw I/Q share: stage 1 (channelize.hip: k_channelize, k_channelize9p), the band survey
// (survey.hip: k_survey) and the channel probe (probe.hip: k_probe).  It is the arithmetic contract's front end: which bytes of the
// caller's I/Q are read and which are never touched (load_span), the level table (load_levels) and what a lane converts (fft_lane),
// in front of the butterflies of fft_radix8.hpp.  With them the host pieces of a launch: the LDS size of a span, the one LDS limit
// with the launcher that respects it, and the ladders that turn (log2n, sample format, conv_arith) into a kernel instance.  Pieces,
// not a skeleton: a kernel keeps its own order of statements and calls the ones it uses.  Two kernels hold a device piece written
// out instead, because the call cost them a compiler resource or their timing band: k_probe the span load,
// k_channelize all three.  Whoever changes a device piece here changes those copies with it.  Internal linkage: every .hip that
// includes this file gets its own copy.
//
// Compile with -ffp-contract=off (the FFT spec).
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "fft_radix8.hpp"

namespace mi {
namespace {

constexpr size_t kLdsLimit = 160 * 1024;  // what one workgroup may ask for on gfx950: the CU's whole LDS

// bytes per complex sample of a kernel instance's format (kSfmtU8Arith: 2)
constexpr int iq_bps2(int sfmt) {
    return sfmt == MI_SFMT_S16 ? 4 : (sfmt == MI_SFMT_F32 ? 8 : 2);
}

// The span of one TW-window piece in LDS: its bytes, up to 15 in front of them (the piece starts at a 16-byte line) and a line's
// rounding.  A kernel lays its LDS out with it and its launcher sizes the launch with it.
template <int L>
__host__ __device__ constexpr unsigned span_alloc(int bps2, unsigned hop_bytes) {
    return (static_cast<unsigned>(FftGeom<L>::TW - 1) * hop_bytes + static_cast<unsigned>(FftGeom<L>::N * bps2) + 16 + 15) & ~15u;
}

// HBM -> LDS: the byte span of nw windows that starts b0 bytes behind the stream's base gbase, each byte read once, 16 B per lane.
// Returns mis, the bytes in front of the span's first one in LDS: window w of the piece starts at span + mis + w * hop_bytes.
template <int BLOCK>
__device__ __forceinline__ unsigned load_span(unsigned char* span, const unsigned char* gbase, const long long b0, const int nw, const unsigned hop_bytes,
                                              const unsigned window_bytes, const size_t valid_bytes, const int tid) {
    const unsigned mis = static_cast<unsigned>(reinterpret_cast<uintptr_t>(gbase + b0) & 15);
    const unsigned need = static_cast<unsigned>(nw - 1) * hop_bytes + window_bytes;
    const unsigned nchunks = (mis + need + 15) >> 4;
    for (unsigned c = tid; c < nchunks; c += BLOCK) {
        const long long off = b0 - mis + 16ll * c;
        uint4 v;
        if (off >= 0 && off + 16 <= static_cast<long long>(valid_bytes)) {
            v = *reinterpret_cast<const uint4*>(gbase + off);
        } else {  // the 16-byte lines around the first and the last byte of the call: nothing outside them is touched
            unsigned char tmp[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const long long o = off + i;
                tmp[i] = (o >= 0 && o < static_cast<long long>(valid_bytes)) ? gbase[o] : 0;
            }
            v = *reinterpret_cast<uint4*>(tmp);
        }
        *reinterpret_cast<uint4*>(span + 16 * c) = v;
    }
    return mis;
}

// the level table of the 8-bit formats into LDS (the other formats convert without one)
template <int SFMT, int BLOCK>
__device__ __forceinline__ void load_levels(float* lut, const float* levels, const int tid) {
    if constexpr (SFMT == MI_SFMT_U8 || SFMT == MI_SFMT_S8) {
        for (int i = tid; i < 256; i += BLOCK)
            lut[i] = levels[i];
    }
}

// Per-lane constants of lane tau of an N-point FFT: the 8 samples it converts with their window coefficients, pass 0's twiddles.
struct FftLane {
    int nidx[8];
    float wreg[8];
    float2 w8, w83;
};

template <int L>
__device__ __forceinline__ FftLane fft_lane(const int tau, const float* window, const float2* tw) {
    constexpr int N = 1 << L;
    FftLane ln;
    const int nrev = (L > 3) ? static_cast<int>(__brev(static_cast<unsigned>(tau)) >> (32 - (L - 3))) : 0;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int rev3 = ((r & 1) << 2) | (r & 2) | ((r >> 2) & 1);
        ln.nidx[r] = rev3 * (N / 8) + nrev;  // natural sample index = bitrev_L(8 tau + r)
        ln.wreg[r] = window[ln.nidx[r]];
    }
    ln.w8 = tw[N / 8];
    ln.w83 = tw[3 * N / 8];
    return ln;
}

// The LDS of a workgroup that runs whole FFTs, in this order: the span, the level table (1 KiB), F exchange slots.  (Stage 1's
// output rows, and the pruned kernel's own buffers in place of the slots, come behind.)
template <int L>
constexpr size_t tile_lds_bytes(int bps2, unsigned hop_bytes) {
    return static_cast<size_t>(span_alloc<L>(bps2, hop_bytes)) + 1024 + static_cast<size_t>(FftGeom<L>::F) * FftGeom<L>::XN * 8;
}

// A launch with dynamic LDS: refused over the limit (the stage's create call has refused such a geometry), the attribute a request
// above 48 KiB needs, the launch.
template <class Args>
hipError_t launch_lds(void (*kern)(Args), const dim3 grid, const dim3 block, const size_t lds, hipStream_t s, const Args& a) {
    if (lds > kLdsLimit)
        return hipErrorInvalidValue;
    if (lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));
        if (e != hipSuccess)
            return e;
    }
    hipLaunchKernelGGL(kern, grid, block, lds, s, a);
    return hipGetLastError();
}

// The ladders from run-time values to a kernel instance: fn is called with std::integral_constant<int, ...> of the FFT size's log2
// and / or the instance's format; `none` is the answer where there is no such instance.
template <class R, class Fn>
R dispatch_log2n(const int log2n, const R none, Fn&& fn) {
    switch (log2n) {
        case 8: return fn(std::integral_constant<int, 8>{});
        case 9: return fn(std::integral_constant<int, 9>{});
        case 10: return fn(std::integral_constant<int, 10>{});
        case 11: return fn(std::integral_constant<int, 11>{});
        case 12: return fn(std::integral_constant<int, 12>{});
        case 13: return fn(std::integral_constant<int, 13>{});
    }
    return none;
}

template <class R, class Fn>
R dispatch_sfmt(const int sfmt, const bool conv_arith, const R none, Fn&& fn) {
    switch (sfmt) {
        case MI_SFMT_U8:
            return conv_arith ? fn(std::integral_constant<int, kSfmtU8Arith>{}) : fn(std::integral_constant<int, static_cast<int>(MI_SFMT_U8)>{});
        case MI_SFMT_S8: return fn(std::integral_constant<int, static_cast<int>(MI_SFMT_S8)>{});
        case MI_SFMT_S16: return fn(std::integral_constant<int, static_cast<int>(MI_SFMT_S16)>{});
        case MI_SFMT_F32: return fn(std::integral_constant<int, static_cast<int>(MI_SFMT_F32)>{});
    }
    return none;
}

template <class R, class Fn>
R dispatch_fft(const int log2n, const int sfmt, const bool conv_arith, const R none, Fn&& fn) {
    return dispatch_log2n(log2n, none, [&](auto l) { return dispatch_sfmt(sfmt, conv_arith, none, [&](auto f) { return fn(l, f); }); });
}

}  // namespace
}  // namespace mi
