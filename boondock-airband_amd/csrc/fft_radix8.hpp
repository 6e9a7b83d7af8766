// fft_radix8.hpp -- the arithmetic channelize.hip (stage 1), survey.hip (the band survey) and probe.hip (the channel probe) share: the
// geometry of an N-point FFT done by N/8 lanes, the butterflies of the documented FFT spec taken three radix-2 DIT stages
// at a time, the LDS exchange between passes, and the sample conversion x window.  What stands in front of it -- the span load, the
// level table, the lane setup -- and the launch are in iq_front.hpp, which includes this file.  Internal linkage: every .hip that
// includes it gets its own copy.
//
// Compile with -ffp-contract=off: products and sums must round separately except where fma is spelled.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/mi_airband.h"

namespace mi {
namespace {

template <int L>
struct FftGeom {
    static constexpr int N = 1 << L;
    static constexpr int TPF = N / 8;                      // lanes per FFT
    static constexpr int BLOCK = TPF < 256 ? 256 : TPF;    // threads per workgroup
    static constexpr int F = BLOCK / TPF;                  // FFTs in flight per workgroup
    static constexpr int NPASS = (L + 2) / 3;
    static constexpr int TW = L <= 10 ? 64 : (L == 11 ? 32 : (L == 12 ? 16 : 8));  // windows per tile
    static constexpr int XN = N + N / 8;                   // padded exchange length (float2)
};

// Lanes of one FFT exchange data through their slot of `xch`.  Up to N = 512 they all sit in one wave (64 lanes x 8 points;
// N = 256: two FFTs per wave), whose LDS operations execute in order: a wave-level fence orders the exchange, and the four
// waves of a workgroup never wait for each other inside the window loop.  Larger FFTs span waves and need the barrier.
template <int L>
__device__ __forceinline__ void fft_sync() {
    if constexpr ((1 << L) / 8 <= 64) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    } else {
        __syncthreads();
    }
}

__device__ __forceinline__ int xpad(int p) {
    return p + (p >> 3);
}

// generic butterfly (a, b) -> (a + w b, a - w b)
__device__ __forceinline__ void bfly(float2& a, float2& b, const float2 w) {
    const float tr = __builtin_fmaf(-b.y, w.y, b.x * w.x);
    const float ti = __builtin_fmaf(b.y, w.x, b.x * w.y);
    const float2 a0 = a;
    a.x = a0.x + tr;
    a.y = a0.y + ti;
    b.x = a0.x - tr;
    b.y = a0.y - ti;
}
// w = 1
__device__ __forceinline__ void bfly_one(float2& a, float2& b) {
    const float2 a0 = a, b0 = b;
    a.x = a0.x + b0.x;
    a.y = a0.y + b0.y;
    b.x = a0.x - b0.x;
    b.y = a0.y - b0.y;
}
// w = -j : t = (b.im, -b.re)
__device__ __forceinline__ void bfly_negj(float2& a, float2& b) {
    const float2 a0 = a, b0 = b;
    a.x = a0.x + b0.y;
    a.y = a0.y - b0.x;
    b.x = a0.x - b0.y;
    b.y = a0.y + b0.x;
}

// Pass K covers DIT stages 3K+1 .. min(3K+3, L).  A lane owns 8 elements that are closed under those
// stages: groups of G = 2^nst elements at stride S = 8^K.
template <int L, int K>
struct Pass {
    static constexpr int S = 1 << (3 * K);
    static constexpr int NST = (L - 3 * K) >= 3 ? 3 : (L - 3 * K);
    static constexpr int G = 1 << NST;
    static constexpr int GROUPS = 8 / G;
    static constexpr int NTW = GROUPS * (G - 1);  // distinct twiddles a lane needs in this pass (<= 7)

    __device__ static __forceinline__ int pos(int tau, int gi, int ri) {
        const int u = tau * GROUPS + gi;
        const int hi = u >> (3 * K);
        const int lo = u & (S - 1);
        return ((hi * G + ri) << (3 * K)) + lo;
    }
    // twiddle exponent of the butterfly (ri, ri + 2^a), stage 3K+1+a
    __device__ static __forceinline__ int tw_exp(int tau, int gi, int a, int m) {
        const int u = tau * GROUPS + gi;
        const int lo = u & (S - 1);
        return (m * S + lo) * ((1 << L) >> (3 * K + 1 + a));
    }
    __device__ static __forceinline__ void load_tw(int tau, const float2* __restrict__ tw, float2 (&r)[7]) {
#pragma unroll
        for (int gi = 0; gi < GROUPS; ++gi)
#pragma unroll
            for (int a = 0; a < NST; ++a)
#pragma unroll
                for (int m = 0; m < (1 << a); ++m)
                    r[gi * (G - 1) + ((1 << a) - 1) + m] = tw[tw_exp(tau, gi, a, m)];
    }
    __device__ static __forceinline__ void run(float2 (&x)[8], const float2 (&r)[7]) {
#pragma unroll
        for (int gi = 0; gi < GROUPS; ++gi)
#pragma unroll
            for (int a = 0; a < NST; ++a)
#pragma unroll
                for (int ri = 0; ri < G; ++ri)
                    if ((ri & (1 << a)) == 0) {
                        const int m = ri & ((1 << a) - 1);
                        bfly(x[gi * G + ri], x[gi * G + ri + (1 << a)], r[gi * (G - 1) + ((1 << a) - 1) + m]);
                    }
    }
};

// pass 0: S = 1, lo = 0, twiddles are 1, -j, W8 = tw[N/8], W8^3 = tw[3N/8]
__device__ __forceinline__ void pass0(float2 (&x)[8], const float2 w8, const float2 w83) {
    bfly_one(x[0], x[1]);
    bfly_one(x[2], x[3]);
    bfly_one(x[4], x[5]);
    bfly_one(x[6], x[7]);
    bfly_one(x[0], x[2]);
    bfly_negj(x[1], x[3]);
    bfly_one(x[4], x[6]);
    bfly_negj(x[5], x[7]);
    bfly_one(x[0], x[4]);
    bfly(x[1], x[5], w8);
    bfly_negj(x[2], x[6]);
    bfly(x[3], x[7], w83);
}

template <int L, int K>
__device__ __forceinline__ void later_passes(float2 (&x)[8], const float2 (&twr)[FftGeom<L>::NPASS][7], float2* __restrict__ xch, int tau) {
    if constexpr (K < FftGeom<L>::NPASS) {
        using P = Pass<L, K>;
#pragma unroll
        for (int gi = 0; gi < P::GROUPS; ++gi)
#pragma unroll
            for (int ri = 0; ri < P::G; ++ri)
                x[gi * P::G + ri] = xch[xpad(P::pos(tau, gi, ri))];
        P::run(x, twr[K]);
#pragma unroll
        for (int gi = 0; gi < P::GROUPS; ++gi)
#pragma unroll
            for (int ri = 0; ri < P::G; ++ri)
                xch[xpad(P::pos(tau, gi, ri))] = x[gi * P::G + ri];
        fft_sync<L>();
        later_passes<L, K + 1>(x, twr, xch, tau);
    }
}

// The passes behind pass 0 with the lane's twiddles fetched where they are used: for the instantiations that cannot keep four passes
// of them beside what they accumulate (N >= 4096: 1024 lanes a workgroup, 128 registers a lane).  Same butterflies.
template <int L, int K>
__device__ __forceinline__ void later_passes_tw(float2 (&x)[8], const float2* __restrict__ tw, float2* __restrict__ xch, int tau) {
    if constexpr (K < FftGeom<L>::NPASS) {
        using P = Pass<L, K>;
        float2 r[7];
        P::load_tw(tau, tw, r);
#pragma unroll
        for (int gi = 0; gi < P::GROUPS; ++gi)
#pragma unroll
            for (int ri = 0; ri < P::G; ++ri)
                x[gi * P::G + ri] = xch[xpad(P::pos(tau, gi, ri))];
        P::run(x, r);
#pragma unroll
        for (int gi = 0; gi < P::GROUPS; ++gi)
#pragma unroll
            for (int ri = 0; ri < P::G; ++ri)
                xch[xpad(P::pos(tau, gi, ri))] = x[gi * P::G + ri];
        fft_sync<L>();
        later_passes_tw<L, K + 1>(x, tw, xch, tau);
    }
}

template <int L, int K>
__device__ __forceinline__ void load_all_tw(int tau, const float2* __restrict__ tw, float2 (&twr)[FftGeom<L>::NPASS][7]) {
    if constexpr (K < FftGeom<L>::NPASS) {
        Pass<L, K>::load_tw(tau, tw, twr[K]);
        load_all_tw<L, K + 1>(tau, tw, twr);
    }
}

// u8 samples without the level table: (b - 127.5f) / 127.5f as a product with the reciprocal and one fma correction step.  The
// plan checks on the host, for all 256 values, that this reproduces the table the reference builds (rtl_airband.cpp:341-346)
// bit for bit before it selects this instantiation -- a lookup is two random LDS reads per sample in a kernel the LDS bounds.
constexpr int kSfmtU8Arith = 100;
__device__ __forceinline__ float level_u8(float n) {
    constexpr float d = 127.5f, rcp = 1.0f / 127.5f;
    const float q0 = n * rcp;
    return __builtin_fmaf(__builtin_fmaf(-q0, d, n), rcp, q0);
}

template <int SFMT>
__device__ __forceinline__ float2 fetch_sample(const unsigned char* __restrict__ span, int byte_off, const float* __restrict__ lut, float scale,
                                               float w) {
    float2 v;
    if constexpr (SFMT == kSfmtU8Arith) {
        const unsigned short b = *reinterpret_cast<const unsigned short*>(span + byte_off);
        v.x = level_u8(static_cast<float>(b & 0xff) - 127.5f) * w;
        v.y = level_u8(static_cast<float>(b >> 8) - 127.5f) * w;
    } else if constexpr (SFMT == MI_SFMT_U8 || SFMT == MI_SFMT_S8) {
        const unsigned short b = *reinterpret_cast<const unsigned short*>(span + byte_off);
        v.x = lut[b & 0xff] * w;  // rtl_airband.cpp:473-474
        v.y = lut[b >> 8] * w;
    } else if constexpr (SFMT == MI_SFMT_S16) {
        const short2 s = *reinterpret_cast<const short2*>(span + byte_off);
        v.x = scale * static_cast<float>(s.x) * w;  // rtl_airband.cpp:438-439
        v.y = scale * static_cast<float>(s.y) * w;
    } else {
        const float2 s = *reinterpret_cast<const float2*>(span + byte_off);
        v.x = scale * s.x * w;  // rtl_airband.cpp:456-457
        v.y = scale * s.y * w;
    }
    return v;
}

}  // namespace
}  // namespace mi
