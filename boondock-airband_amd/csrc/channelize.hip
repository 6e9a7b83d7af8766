// channelize.hip -- stage 1 of the hot path on gfx950: sample conversion x window, sliding FFT, bin
// pick + magnitude.  Replaces rtl_airband.cpp:424-511 (and the NEON samplefft(), rtl_airband_neon.s:28-83,
// and FFTW3f / hello_fft) for a whole tile of consecutive windows per workgroup.
//
// One workgroup = TW consecutive windows of one stream.  The byte span the TW windows cover
// ((TW-1)*hop + fft_size samples; windows overlap 3.2x at fft 512) is read from HBM ONCE with 16-byte
// coalesced loads into LDS; every window then converts its samples out of LDS.  An FFT of N points is
// done by N/8 lanes, 8 points per lane, as radix-2 DIT stages taken three at a time in registers with
// one LDS exchange between passes.  The arithmetic of every butterfly is the documented FFT spec
// (DESIGN.md): t = w*b as {fma(-b.im, w.im, b.re*w.re), fma(b.im, w.re, b.re*w.im)}, a' = a + t,
// b' = a - t, so the result is bit-identical to the CPU oracle (zero signs aside).  Only the
// channel bins leave the chip: magnitude (and re/im for channels that need raw I/Q), staged per tile
// in LDS and written as contiguous rows of the [stream][channel][time] planes stage 2 reads.
//
// The span load, level table and lane setup are iq_front.hpp's, which the band survey and the channel probe share.  The pruned kernel
// k_channelize9p calls them; k_channelize holds the same text written out, because with the calls its fft 2048 instance left its
// timing band -- a change to load_span, load_levels or fft_lane is made here as well.  Both take the LDS sizes,
// the launcher and the instance ladders from there.
//
// Compile with -ffp-contract=off: products and sums must round separately except where fma is spelled.
#include <hip/hip_runtime.h>

#include "iq_front.hpp"
#include "kernels.hpp"

namespace mi {
namespace {

template <int L, int SFMT>
__global__ __launch_bounds__(FftGeom<L>::BLOCK) void k_channelize(const ChannelizeArgs a) {
    using Gm = FftGeom<L>;
    constexpr int N = Gm::N, TPF = Gm::TPF, F = Gm::F, TW = Gm::TW, XN = Gm::XN, BLOCK = Gm::BLOCK;
    constexpr int BPS2 = iq_bps2(SFMT);  // bytes per complex sample

    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int tid = threadIdx.x;
    const int stream = a.streams ? a.streams[blockIdx.y] : static_cast<int>(blockIdx.y);  // the handle's index: IQ, planes, xmax, st, afc_spec
    const unsigned w0 = blockIdx.x * TW;
    const int nw = min(static_cast<unsigned>(TW), a.nfft - w0);

    const unsigned span_bytes = span_alloc<L>(BPS2, a.hop_bytes);
    unsigned char* span = lds;
    float* lut = reinterpret_cast<float*>(lds + span_bytes);
    float2* xch_all = reinterpret_cast<float2*>(lds + span_bytes + 1024);
    float* out_mag = reinterpret_cast<float*>(xch_all + F * XN);
    float2* out_iq = reinterpret_cast<float2*>(out_mag + a.nch * TW);

    // ---- HBM -> LDS: the byte span of this tile, each byte read once, 16 B per lane (load_span and load_levels, written out) ----
    const unsigned char* gbase = a.iq + static_cast<size_t>(stream) * a.stream_stride;
    const long long b0 = static_cast<long long>(w0) * a.hop_bytes;
    const unsigned mis = static_cast<unsigned>(reinterpret_cast<uintptr_t>(gbase + b0) & 15);
    const unsigned need = static_cast<unsigned>(nw - 1) * a.hop_bytes + N * BPS2;
    const unsigned nchunks = (mis + need + 15) >> 4;
    for (unsigned c = tid; c < nchunks; c += BLOCK) {
        const long long off = b0 - mis + 16ll * c;
        uint4 v;
        if (off >= 0 && off + 16 <= static_cast<long long>(a.valid_bytes)) {
            v = *reinterpret_cast<const uint4*>(gbase + off);
        } else {
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
    if constexpr (SFMT == MI_SFMT_U8 || SFMT == MI_SFMT_S8) {
        for (int i = tid; i < 256; i += BLOCK)
            lut[i] = a.levels[i];
    }

    // ---- per-lane constants: window coefficients of the 8 samples this lane converts, twiddles (fft_lane, written out) ----
    const int f = tid / TPF;
    const int tau = tid - f * TPF;
    float2* xch = xch_all + f * XN;
    const float2* tw = reinterpret_cast<const float2*>(a.tw);
    const int nrev = (L > 3) ? static_cast<int>(__brev(static_cast<unsigned>(tau)) >> (32 - (L - 3))) : 0;
    int nidx[8];
    float wreg[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int rev3 = ((r & 1) << 2) | (r & 2) | ((r >> 2) & 1);
        nidx[r] = rev3 * TPF + nrev;  // natural sample index = bitrev_L(8 tau + r)
        wreg[r] = a.window[nidx[r]];
    }
    const float2 w8 = tw[N / 8], w83 = tw[3 * N / 8];
    float2 twr[Gm::NPASS][7];
    load_all_tw<L, 1>(tau, tw, twr);
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
        later_passes<L, 1>(x, twr, xch, tau);
        // natural-order spectrum now sits in xch: pick the channel bins (rtl_airband.cpp:505-511)
        if (active) {
            for (int c = tau; c < a.nch; c += TPF) {
                const ChanParams& cp = a.cp[c];
                const uint32_t bin = a.st ? a.st[static_cast<size_t>(stream) * a.nch + c].afc_bin : cp.bin;  // dev->bins[j]
                const float2 v = xch[xpad(static_cast<int>(bin))];
                out_mag[c * TW + wi] = sqrtf(v.x * v.x + v.y * v.y);
                if (cp.iq_row >= 0)
                    out_iq[cp.iq_row * TW + wi] = v;
            }
            // AFC reads the spectrum of the last FFT before the batch trigger (rtl_airband.cpp:648-652, square() :186-192)
            if (a.afc_spec && w0 + static_cast<unsigned>(wi) == a.nfft - 1) {
                float* __restrict__ sq = a.afc_spec + static_cast<size_t>(stream) * N;
                for (int k = tau; k < N; k += TPF) {
                    const float2 v = xch[xpad(k)];
                    sq[k] = v.x * v.x + v.y * v.y;
                }
            }
        }
        fft_sync<L>();  // the slot is rewritten by the next window's pass 0
    }
    __syncthreads();  // the staged rows were written by every wave

    // ---- LDS -> HBM: contiguous rows of the planes ----
    for (int idx = tid; idx < a.nch * TW; idx += BLOCK) {
        const int c = idx / TW, i = idx - c * TW;
        if (i < nw)
            a.mag[(static_cast<size_t>(stream) * a.nch + c) * a.plane_stride + a.plane_off + w0 + i] = out_mag[idx];
    }
    if (a.xmax) {  // upper bound the time-parallel stage 2 starts its sandwich from
        for (int c = tid; c < a.nch; c += BLOCK) {
            float m = 0.0f;
            for (int i = 0; i < nw; ++i)
                m = fmaxf(m, out_mag[c * TW + i]);
            atomicMax(a.xmax + static_cast<size_t>(stream) * a.nch + c, __float_as_uint(m));
        }
    }
    for (int idx = tid; idx < a.n_iq_rows * TW; idx += BLOCK) {
        const int c = idx / TW, i = idx - c * TW;
        if (i < nw)
            a.cplx[(static_cast<size_t>(stream) * a.n_iq_rows + c) * a.plane_stride + a.plane_off + w0 + i] = out_iq[idx];
    }
}

// ---- N = 512 with the graph pruned to the picked bins (PrunePlan) ----
// A wave takes kGW windows at a time.  Pass 0 (stages 1-3) is the full one, a window per trip: the conversion x window of all
// 512 samples is needed whatever is picked.  It keeps only the residues R_3 of every block of 8.  Pass 1 (stages 4-6) then
// has 8 * m3 radix-8 work items per window instead of 64 -- (block of 64, residue in R_3) -- and pass 2 (stages 7-9) has m6:
// the items of the kGW windows are packed onto the lanes (class = lane & (classes - 1), so a lane's twiddles and output
// slots never change), each item runs the same Pass<9, K>::run butterflies on the same operands as the full kernel.
// Exchange buffers per window: b0[row ri][block hi * m3 + j] (row stride rs1), b1[row ri][j2] (rs2), b2[rank of the bin].
constexpr int kGW = 2;

template <int SFMT>
__global__ __launch_bounds__(256, 4) void k_channelize9p(const ChannelizeArgs a) {
    constexpr int L = 9, N = 512, TW = FftGeom<9>::TW, BLOCK = 256, NWAVE = 4;
    constexpr int BPS2 = iq_bps2(SFMT);
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    const int stream = a.streams ? a.streams[blockIdx.y] : static_cast<int>(blockIdx.y);  // the handle's index: IQ, planes, xmax, st, afc_spec
    const unsigned w0 = blockIdx.x * TW;
    const int nw = min(static_cast<unsigned>(TW), a.nfft - w0);
    const PrunePlan& pp = a.prune;
    const int m3 = pp.m3, sh3 = pp.sh3, m6 = pp.m6, sh6 = pp.sh6, m9 = pp.m9, rs1 = pp.rs1, rs2 = pp.rs2;
    const int b0len = 8 * rs1, b2len = (m9 + 1) & ~1;  // float2 per window; b1 reuses b0's rows (rs2 <= rs1)
    const int b1len = b0len;
    const int wlen = kGW * (b0len + b2len);  // float2 per wave

    const unsigned span_bytes = span_alloc<L>(BPS2, a.hop_bytes);
    unsigned char* span = lds;
    float* lut = reinterpret_cast<float*>(lds + span_bytes);
    float2* xw = reinterpret_cast<float2*>(lds + span_bytes + 1024) + wave * wlen;
    float* out_mag = reinterpret_cast<float*>(reinterpret_cast<float2*>(lds + span_bytes + 1024) + NWAVE * wlen);
    float2* out_iq = reinterpret_cast<float2*>(out_mag + a.nch * TW);
    float2* b0 = xw;
    float2* b1 = b0;
    float2* b2 = b0 + kGW * b0len;

    // ---- HBM -> LDS: the byte span of this tile ----
    const unsigned char* gbase = a.iq + static_cast<size_t>(stream) * a.stream_stride;
    const unsigned mis = load_span<BLOCK>(span, gbase, static_cast<long long>(w0) * a.hop_bytes, nw, a.hop_bytes, N * BPS2, a.valid_bytes, tid);
    load_levels<SFMT, BLOCK>(lut, a.levels, tid);

    // ---- per-lane constants ----
    const int tau = lane;  // pass 0: lane = block of 8 at stage 3
    const FftLane ln = fft_lane<L>(tau, a.window, reinterpret_cast<const float2*>(a.tw));
    // the lane's item class in pass 1 / pass 2: 7 twiddles and 8 output slots each
    const int j1 = lane & ((1 << sh3) - 1), j2 = lane & ((1 << sh6) - 1);
    float2 t1[7], t2[7];
    unsigned o1[2], o2[2];  // 8 output slots each, a byte per slot (0xff = not needed)
    {
        const float* c1 = a.prune_t1 + static_cast<size_t>(j1) * kPruneClassWords;
        const float* c2 = a.prune_t2 + static_cast<size_t>(j2) * kPruneClassWords;
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            t1[k] = make_float2(c1[2 * k], c1[2 * k + 1]);
            t2[k] = make_float2(c2[2 * k], c2[2 * k + 1]);
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            o1[k] = __float_as_uint(c1[14 + k]);
            o2[k] = __float_as_uint(c2[14 + k]);
        }
    }
    const int ipf1 = 8 << sh3;  // padded items of pass 1 per window (block hi = 0..7, class)
    const int hi1 = (lane & (ipf1 - 1)) >> sh3;
    __syncthreads();

    for (int wbase = wave * kGW; wbase < nw; wbase += NWAVE * kGW) {
        // ---- pass 0, one window per trip ----
#pragma unroll 1
        for (int g = 0; g < kGW; ++g) {
            const int wi = wbase + g;
            const int wbyte = static_cast<int>(mis) + (wi < nw ? wi : 0) * static_cast<int>(a.hop_bytes);
            float2 x[8];
#pragma unroll
            for (int r = 0; r < 8; ++r)
                x[r] = fetch_sample<SFMT>(span, wbyte + ln.nidx[r] * BPS2, lut, a.conv_scale, ln.wreg[r]);
            pass0(x, ln.w8, ln.w83);
            float2* d = b0 + g * b0len + (tau & 7) * rs1 + (tau >> 3) * m3;  // block tau = 8 hi + ri of pass 1
#pragma unroll
            for (int r = 0; r < 8; ++r)
                if (pp.rank3[r] >= 0)
                    d[pp.rank3[r]] = x[r];
        }
        fft_sync<L>();
        // ---- pass 1: kGW * ipf1 items ----
        for (int q = lane; q < kGW * ipf1; q += 64) {
            const int g = q >> (3 + sh3);
            if (j1 < m3) {
                const float2* src = b0 + g * b0len + hi1 * m3 + j1;
                float2 x[8];
#pragma unroll
                for (int ri = 0; ri < 8; ++ri)
                    x[ri] = src[ri * rs1];
                Pass<L, 1>::run(x, t1);
                fft_sync<L>();  // b1 lies over the rows just read
                float2* dst = b1 + g * b1len + hi1 * rs2;  // block hi1 of 64 = row of pass 2
#pragma unroll
                for (int ri = 0; ri < 8; ++ri) {
                    const unsigned o = (o1[ri >> 2] >> (8 * (ri & 3))) & 0xffu;
                    if (o != 0xffu)
                        dst[o] = x[ri];
                }
            }
        }
        fft_sync<L>();
        // ---- pass 2: kGW << sh6 items ----
        for (int q = lane; q < (kGW << sh6); q += 64) {
            const int g = q >> sh6;
            if (j2 < m6) {
                const float2* src = b1 + g * b1len + j2;
                float2 x[8];
#pragma unroll
                for (int ri = 0; ri < 8; ++ri)
                    x[ri] = src[ri * rs2];
                Pass<L, 2>::run(x, t2);
                float2* dst = b2 + g * b2len;
#pragma unroll
                for (int ri = 0; ri < 8; ++ri) {
                    const unsigned o = (o2[ri >> 2] >> (8 * (ri & 3))) & 0xffu;
                    if (o != 0xffu)
                        dst[o] = x[ri];
                }
            }
        }
        fft_sync<L>();
        // ---- the picked bins of the kGW windows (rtl_airband.cpp:505-511) ----
        for (int idx = lane; idx < kGW * a.nch; idx += 64) {
            const int g = idx / a.nch, c = idx - g * a.nch;
            const int wi = wbase + g;
            if (wi < nw) {
                const float2 v = b2[g * b2len + a.prune_rank[c]];
                out_mag[c * TW + wi] = sqrtf(v.x * v.x + v.y * v.y);
                const int iq_row = a.cp[c].iq_row;
                if (iq_row >= 0)
                    out_iq[iq_row * TW + wi] = v;
            }
        }
        fft_sync<L>();
    }
    __syncthreads();  // the staged rows were written by every wave

    // ---- LDS -> HBM: contiguous rows of the planes ----
    for (int idx = tid; idx < a.nch * TW; idx += BLOCK) {
        const int c = idx / TW, i = idx - c * TW;
        if (i < nw)
            a.mag[(static_cast<size_t>(stream) * a.nch + c) * a.plane_stride + a.plane_off + w0 + i] = out_mag[idx];
    }
    if (a.xmax) {
        for (int c = tid; c < a.nch; c += BLOCK) {
            float m = 0.0f;
            for (int i = 0; i < nw; ++i)
                m = fmaxf(m, out_mag[c * TW + i]);
            atomicMax(a.xmax + static_cast<size_t>(stream) * a.nch + c, __float_as_uint(m));
        }
    }
    for (int idx = tid; idx < a.n_iq_rows * TW; idx += BLOCK) {
        const int c = idx / TW, i = idx - c * TW;
        if (i < nw)
            a.cplx[(static_cast<size_t>(stream) * a.n_iq_rows + c) * a.plane_stride + a.plane_off + w0 + i] = out_iq[idx];
    }
}

template <int SFMT>
hipError_t launch_9p(const ChannelizeArgs& a, int nstreams, hipStream_t s) {
    using Gm = FftGeom<9>;
    const size_t wlen = static_cast<size_t>(kGW) * (8 * a.prune.rs1 + ((a.prune.m9 + 1) & ~1));
    const size_t lds = span_alloc<9>(iq_bps2(SFMT), a.hop_bytes) + 1024 + 4 * wlen * 8 + static_cast<size_t>(a.nch) * Gm::TW * 4 +
                       static_cast<size_t>(a.n_iq_rows) * Gm::TW * 8;
    return launch_lds(k_channelize9p<SFMT>, dim3((a.nfft + Gm::TW - 1) / Gm::TW, nstreams), dim3(256), lds, s, a);
}

template <int L, int SFMT>
hipError_t launch_one(const ChannelizeArgs& a, int nstreams, hipStream_t s) {
    using Gm = FftGeom<L>;
    const size_t lds = tile_lds_bytes<L>(iq_bps2(SFMT), a.hop_bytes) + static_cast<size_t>(a.nch) * Gm::TW * 4 + static_cast<size_t>(a.n_iq_rows) * Gm::TW * 8;
    return launch_lds(k_channelize<L, SFMT>, dim3((a.nfft + Gm::TW - 1) / Gm::TW, nstreams), dim3(Gm::BLOCK), lds, s, a);
}

}  // namespace

hipError_t launch_channelize(const ChannelizeArgs& a, int log2n, int sfmt, int nstreams, hipStream_t s) {
    if (a.streams)  // a launch over some of the handle's streams: the grid covers those alone
        nstreams = a.nactive;
    if (a.nfft == 0 || nstreams <= 0)
        return hipSuccess;
    // the pruned graphs have no complete spectrum: AFC launches (they want one) take the full kernel
    if (a.l64.enabled && a.l64_chan && !a.afc_spec && !a.st && l64_supported(log2n, a.hop_bytes, sfmt == MI_SFMT_S16 ? 2 : (sfmt == MI_SFMT_F32 ? 4 : 1)))
        return launch_channelize_l64(a, log2n, sfmt, nstreams, s);
    if (log2n == 9 && a.prune.enabled && a.prune_t1 && a.prune_t2 && a.prune_rank && !a.afc_spec && !a.st)
        return dispatch_sfmt(sfmt, a.conv_arith != 0, hipErrorInvalidValue, [&](auto f) { return launch_9p<f()>(a, nstreams, s); });
    return dispatch_fft(log2n, sfmt, a.conv_arith != 0, hipErrorInvalidValue, [&](auto l, auto f) { return launch_one<l(), f()>(a, nstreams, s); });
}

}  // namespace mi
