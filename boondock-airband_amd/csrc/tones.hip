// tones.hip -- the CTCSS tone finder: one Goertzel detector for each of the reference's 51 standard tones over the audio
// mi_demod_process_device wrote, one record per row and window -- the strongest tone, the runner-up and the mean of the 51 powers.
//   ToneDetector         q0 = coeff * q1 - q2 + x;  power = q1 * q1 + q2 * q2 - q1 * q2 * coeff    src/ctcss.cpp:31-55
//   CTCSS::reset         on the way to CLOSED, here at every MI_NO_SIGNAL batch                    src/ctcss.cpp:165-172, squelch.cpp:287
// The rule, the record, the order of the sum and the state blob are in include/mi_airband.h.  A post-stage of its own like the gate
// and the splitter: three launches on the caller's stream, no atomics.  A window never spans a MI_NO_SIGNAL batch, so it is one
// contiguous range of the row's audio (a PIECE), which may begin in the carried state; what is left behind the last window of a call
// is the row's TAIL piece, whose wave writes the state.  mi_tones_plan_host (poststage_host.cpp) is the host twin.  The handle's base
// and the bodies of the entry points every stage repeats are in poststage.hpp.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "../../include/mi_airband.h"
#include "poststage.hpp"

constexpr char kName[] = "tone finder";

struct mi_tones : mi::RowStage {
    mi_tones() : RowStage(kName, 3) {}
    uint32_t window = 0;
    uint32_t max_records = 0;
    mi::DevBuf<mi::TonesRowState> d_state;    // [rows]: the checkpoint blob as it is
    mi::DevBuf<float> d_coeff;                // [64]: lane t's coefficient, 0 beyond the table
    mi::DevBuf<float> d_carry;                // [rows][2][64]: q1 and q2 as the call found them (the bank reads these, its tails write d_state)
    mi::DevBuf<uint4> d_piece;                // [rows][windows of the call + 1]: {first sample, samples, seq, meta}, the tail last
    mi::DevBuf<uint32_t> d_row_rec_count;     // [rows]
    mi::PinnedBuf<uint32_t> h_count;          // [2], landing place of the counts in mi_tones_download
    // destinations of the last mi_tones_process_device (what mi_tones_download reads)
    const mi_tone_record* last_records = nullptr;
    const float* last_powers = nullptr;
    const uint32_t* last_row_first = nullptr;
    const uint32_t* last_count = nullptr;
};

namespace {

using mi::aligned;
using mi::as_flags;
using mi::fail;
using mi::kRowsPerGroup;
constexpr int kTones = MI_TONES_STANDARD, kLanes = MI_TONES_LANES;
// a piece's meta word: the count the tail leaves in its low bits
constexpr uint32_t kTail = 0x80000000u, kFromCarry = 0x40000000u, kSkip = 0x20000000u, kCountMask = 0x00FFFFFFu;
static_assert(kLanes == 64, "one lane per tone, one wave per piece");

__device__ inline uint32_t uniform(uint32_t v) {
    return static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(v)));
}

__device__ __forceinline__ float lane_read(const float v, const int lane) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// Launch 1.  The row's wave copies the carried q1 / q2 aside, loads 64 flags a trip, one per lane, and walks the ballot mask a
// stretch at a time in wave-uniform code: a stretch of MI_NO_SIGNAL batches resets the count, a stretch of the others completes
// (count + its samples) / window windows, whose pieces the lanes write side by side.  Lane 0 adds the tail.
__global__ __launch_bounds__(256) void k_tones_walk(const uint8_t* __restrict__ enabled, const mi::TonesRowState* __restrict__ state,
                                                    const char* __restrict__ axc, const size_t axc_stride, const int rows, const int nbatches,
                                                    const uint32_t window, const uint32_t slots, float* __restrict__ carry, uint4* __restrict__ piece,
                                                    uint32_t* __restrict__ row_rec_count) {
    const uint32_t lane = threadIdx.x & 63;
    const int row = blockIdx.x * kRowsPerGroup + (threadIdx.x >> 6);
    if (row >= rows)  // (the whole wave)
        return;
    uint4* const pc = piece + static_cast<size_t>(row) * slots;
    if (!enabled[row]) {  // the row sits out: no record, every byte of its state stays
        if (lane == 0) {
            row_rec_count[row] = 0;
            pc[0] = make_uint4(0u, 0u, 0u, kSkip);
        }
        return;
    }
    const mi::TonesRowState* st = state + row;
    carry[static_cast<size_t>(row) * 2 * kLanes + lane] = st->q1[lane];
    carry[static_cast<size_t>(row) * 2 * kLanes + kLanes + lane] = st->q2[lane];
    uint32_t c = uniform(st->count);
    const uint32_t seq0 = uniform(st->seq);
    uint32_t nrec = 0;
    uint32_t cur = 0;        // first sample of the window that is running
    bool from_carry = true;  // ... which began in the carried state
    for (int b0 = 0; b0 < nbatches; b0 += 64) {
        const int b = b0 + static_cast<int>(lane);
        const bool sig = b < nbatches && axc[static_cast<size_t>(row) * axc_stride + b] != MI_NO_SIGNAL;
        const unsigned long long sigmask = __ballot(sig);  // lanes beyond nbatches contribute 0
        const int n = nbatches - b0 < 64 ? nbatches - b0 : 64;
        for (int l = 0; l < n;) {
            const unsigned long long rest = sigmask >> l;
            if (!(rest & 1ull)) {  // CTCSS::reset
                l += rest ? __builtin_ctzll(rest) : n - l;
                c = 0;
                from_carry = false;
                cur = static_cast<uint32_t>(b0 + l) * mi::kWaveBatch;
                continue;
            }
            const unsigned long long gap = ~rest;
            int run = gap ? __builtin_ctzll(gap) : 64;
            run = run < n - l ? run : n - l;
            const uint32_t s0 = static_cast<uint32_t>(b0 + l) * mi::kWaveBatch;
            const uint32_t total = c + static_cast<uint32_t>(run) * mi::kWaveBatch, nw = total / window;
            for (uint32_t k = lane; k < nw; k += 64) {
                const uint32_t end = s0 + (k + 1) * window - c;  // one behind the window's last sample
                const uint32_t start = k == 0 ? cur : end - window;
                if (nrec + k < slots - 1)
                    pc[nrec + k] = make_uint4(start, end - start, seq0 + nrec + k, k == 0 && from_carry ? kFromCarry : 0u);
            }
            if (nw) {
                cur = s0 + nw * window - c;
                from_carry = false;
                nrec += nw;
            }
            c = total - nw * window;
            l += run;
        }
    }
    if (lane == 0) {
        nrec = nrec < slots - 1 ? nrec : slots - 1;
        pc[nrec] = make_uint4(cur, static_cast<uint32_t>(nbatches) * mi::kWaveBatch - cur, seq0 + nrec, kTail | (from_carry ? kFromCarry : 0u) | c);
        row_rec_count[row] = nrec;
    }
}

// Launch 2.  mi::launch_row_scan (poststage.hip): exclusive scan of the rows' record counts, and the two counts.

// Launch 3, the hot path.  One wave per (row, piece), four to a workgroup.  Lane t holds tone t's coefficient, q1 and q2; the wave
// loads 64 consecutive samples at once, one per lane (the next 64 are asked for before these are used), and takes 64 steps, each
// reading its sample out of lane j into a scalar register -- j is a constant after unrolling -- so the loop has no LDS and no memory
// access per sample: three dependent VALU operations and one v_readlane.  A wave alone is bound by that dependency; the SIMD is kept
// busy by the other (row, piece) waves on it, and at a handful of registers as many fit as the hardware takes.
__global__ __launch_bounds__(256) void k_tones_bank(const uint4* __restrict__ piece, const uint32_t slots, const uint32_t* __restrict__ row_rec_count,
                                                    const uint32_t* __restrict__ row_first, const float* __restrict__ coeffs,
                                                    const float* __restrict__ carry, mi::TonesRowState* __restrict__ state,
                                                    const float* __restrict__ wave, const size_t row_stride, const uint32_t rows,
                                                    const uint32_t nsamples, const uint32_t max_records, mi_tone_record* __restrict__ records,
                                                    float* __restrict__ powers) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t w = blockIdx.x * kRowsPerGroup + (threadIdx.x >> 6);
    const uint32_t row = w / slots, j = w % slots;
    if (row >= rows || j > uniform(row_rec_count[row]))  // (the whole wave)
        return;
    const uint4 d = piece[static_cast<size_t>(row) * slots + j];
    const uint32_t start = uniform(d.x), len = uniform(d.y), seq = uniform(d.z), meta = uniform(d.w);
    const bool tail = (meta & kTail) != 0;
    const uint32_t k = uniform(row_first[row]) + j;
    if ((meta & kSkip) || (!tail && k >= max_records) || start > nsamples || len > nsamples - start)
        return;
    const float coeff = coeffs[lane];
    float q1 = 0.0f, q2 = 0.0f;
    if (meta & kFromCarry) {
        q1 = carry[static_cast<size_t>(row) * 2 * kLanes + lane];
        q2 = carry[static_cast<size_t>(row) * 2 * kLanes + kLanes + lane];
    }
    const float* x = wave + static_cast<size_t>(row) * row_stride + start;
    float v = lane < len ? x[lane] : 0.0f;
    uint32_t i = 0;
    for (; i + 64 <= len; i += 64) {
        const float next = i + 64 + lane < len ? x[i + 64 + lane] : 0.0f;
#pragma unroll
        for (int s = 0; s < 64; ++s) {
            const float q0 = coeff * q1 - q2 + lane_read(v, s);
            q2 = q1;
            q1 = q0;
        }
        v = next;
    }
    for (uint32_t s = 0; s < len - i; ++s) {  // the last, short group: the lane index is a loop counter
        const float q0 = coeff * q1 - q2 + lane_read(v, static_cast<int>(s));
        q2 = q1;
        q1 = q0;
    }
    if (lane >= kTones)
        q1 = q2 = 0.0f;
    if (tail) {
        mi::TonesRowState* st = state + row;
        st->q1[lane] = q1;
        st->q2[lane] = q2;
        if (lane == 0)
            *reinterpret_cast<uint2*>(st) = make_uint2(meta & kCountMask, seq);  // {count, seq}, 8-byte aligned
        return;
    }
    // the window's end: the powers read lane by lane in index order, as `total += mag` does in the reference (ctcss.cpp:141-148)
    const float p = lane < kTones ? q1 * q1 + q2 * q2 - q1 * q2 * coeff : 0.0f;
    float total = lane_read(p, 0), bp = total, sp = 0.0f;
    uint32_t best = 0, second = 0xFFFFFFFFu;
#pragma unroll
    for (int t = 1; t < kTones; ++t) {
        const float m = lane_read(p, t);
        total += m;
        if (m > bp) {
            second = best;
            sp = bp;
            best = static_cast<uint32_t>(t);
            bp = m;
        } else if (second == 0xFFFFFFFFu || m > sp) {
            second = static_cast<uint32_t>(t);
            sp = m;
        }
    }
    if (lane == 0) {  // 40 bytes, 8-byte aligned: five 8-byte vector stores
        const uint32_t last = start + len - 1;
        uint2* r = reinterpret_cast<uint2*>(records + k);
        r[0] = make_uint2(row, seq);
        r[1] = make_uint2(last / mi::kWaveBatch, last % mi::kWaveBatch);
        r[2] = make_uint2(best, second);
        r[3] = make_uint2(__float_as_uint(bp), __float_as_uint(sp));
        r[4] = make_uint2(__float_as_uint(total / 51.0f), 0u);
    }
    if (powers)
        powers[static_cast<size_t>(k) * kLanes + lane] = p;
}

}  // namespace

extern "C" {

int mi_tones_create(const mi_tones_cfg* cfg, const uint8_t* row_enabled, int rows, int max_batches, size_t max_records, int gpu, mi_tones** out) {
    if (!row_enabled || !out)
        return fail(MI_ERR_INVALID, "NULL argument");
    const uint32_t window = mi::tones_window(cfg);
    if (!window)
        return MI_ERR_INVALID;
    if (rows < 1 || rows >= (1 << 20) || max_batches < 1 || max_batches > (1 << 20) ||
        static_cast<uint64_t>(rows) * mi::tones_max_windows(window, static_cast<uint64_t>(max_batches)) >= (1ull << 24))
        return fail(MI_ERR_INVALID,
                    "tone finder needs 1 <= rows < 2^20, 1 <= max_batches <= 2^20 and rows * ((window - 1 + 2000 * max_batches) / window) < 2^24");
    if (const int rc = mi::check_gpu(gpu, "no HIP device: the tone finder runs on the GPU only"))
        return rc;
    mi_tones* t = new mi_tones();
    t->gpu = gpu;
    t->rows = rows;
    t->max_batches = max_batches;
    t->window = window;
    const size_t n = static_cast<size_t>(rows), most = n * static_cast<size_t>(mi::tones_max_windows(window, static_cast<uint64_t>(max_batches)));
    t->max_records = static_cast<uint32_t>(max_records && max_records < most ? max_records : most);  // (no call has more records than `most`)
    std::vector<float> coeff(MI_TONES_LANES);
    mi::tones_coeffs(window, coeff.data());
    if (hipSetDevice(gpu) != hipSuccess || dalloc_copy(t->d_enabled, as_flags(row_enabled, n)) != hipSuccess || dalloc_zero(t->d_state, n) != hipSuccess ||
        dalloc_copy(t->d_coeff, coeff) != hipSuccess || dalloc(t->d_carry, n * 2 * MI_TONES_LANES) != hipSuccess || dalloc(t->d_piece, most + n) != hipSuccess ||
        dalloc(t->d_row_rec_count, n) != hipSuccess || hipHostMalloc(reinterpret_cast<void**>(t->h_count.put()), 2 * sizeof(uint32_t)) != hipSuccess ||
        hipDeviceSynchronize() != hipSuccess) {
        delete t;
        return fail(MI_ERR_HIP, "tone finder: device allocation failed");
    }
    *out = t;
    return MI_OK;
}

void mi_tones_destroy(mi_tones* t) {
    mi::destroy(t);
}

int mi_tones_set_rows(mi_tones* t, const uint8_t* row_enabled) {
    return mi::set_enabled(kName, t, row_enabled);
}

int mi_tones_process_device(mi_tones* t, const float* d_waveout, size_t row_stride, const char* d_axc, size_t axc_stride, int nbatches,
                            mi_tone_record* d_records, float* d_powers, uint32_t* d_row_first_record, uint32_t* d_count, void* hip_stream) {
    if (!t || !d_waveout || !d_axc || !d_records || !d_row_first_record || !d_count)
        return fail(MI_ERR_INVALID, "NULL argument");
    if (nbatches < 1 || nbatches > t->max_batches)
        return fail(MI_ERR_INVALID, "nbatches outside 1 .. max_batches");
    if (axc_stride < static_cast<size_t>(nbatches) || row_stride < static_cast<size_t>(nbatches) * mi::kWaveBatch)
        return fail(MI_ERR_INVALID, "a row stride is shorter than the call");
    if (row_stride % 4 != 0 || !aligned(d_waveout, 16) || !aligned(d_records, 8) || !aligned(d_powers, 4) || !aligned(d_row_first_record, 4) ||
        !aligned(d_count, 4))
        return fail(MI_ERR_INVALID, "the audio buffer must be 16-byte aligned with a row stride that is a multiple of 4 floats; records 8-byte aligned");
    if (hipSetDevice(t->gpu) != hipSuccess)
        return fail(MI_ERR_HIP, "hipSetDevice failed");
    hipStream_t q = static_cast<hipStream_t>(hip_stream);
    const unsigned rows = static_cast<unsigned>(t->rows);
    // the windows a row can complete in this call, and its tail: at most what create allocated, as nbatches <= max_batches
    const uint32_t slots = static_cast<uint32_t>(mi::tones_max_windows(t->window, static_cast<uint64_t>(nbatches))) + 1u;
    t->timing.stamp(0, q);
    hipLaunchKernelGGL(k_tones_walk, dim3((rows + kRowsPerGroup - 1) / kRowsPerGroup), dim3(256), 0, q, t->d_enabled.get(), t->d_state.get(), d_axc, axc_stride,
                       t->rows, nbatches, t->window, slots, t->d_carry.get(), t->d_piece.get(), t->d_row_rec_count.get());
    t->timing.stamp(1, q);
    mi::launch_row_scan(q, t->d_row_rec_count, t->rows, t->max_records, d_row_first_record, d_count);
    t->timing.stamp(2, q);
    hipLaunchKernelGGL(k_tones_bank, dim3((rows * slots + kRowsPerGroup - 1) / kRowsPerGroup), dim3(256), 0, q, t->d_piece.get(), slots,
                       t->d_row_rec_count.get(), d_row_first_record, t->d_coeff.get(), t->d_carry.get(), t->d_state.get(), d_waveout, row_stride, rows,
                       static_cast<uint32_t>(nbatches) * mi::kWaveBatch, t->max_records, d_records, d_powers);
    t->timing.stamp(3, q);
    if (hipGetLastError() != hipSuccess)
        return fail(MI_ERR_HIP, "tone finder kernel launch failed");
    t->called = true;
    t->last_records = d_records;
    t->last_powers = d_powers;
    t->last_row_first = d_row_first_record;
    t->last_count = d_count;
    return MI_OK;
}

int mi_tones_download(mi_tones* t, void* hip_stream, mi_tone_record* records, float* powers, uint32_t* row_first_record, uint32_t* count) {
    if (!t || !count)
        return fail(MI_ERR_INVALID, "NULL argument");
    if (!t->last_count)
        return fail(MI_ERR_INVALID, "no mi_tones_process_device call to download");
    if (powers && !t->last_powers)
        return fail(MI_ERR_INVALID, "the last mi_tones_process_device call stored no powers");
    hipStream_t q = static_cast<hipStream_t>(hip_stream);
    if (!mi::land_counts(t->gpu, q, t->h_count, t->last_count, count))
        return fail(MI_ERR_HIP, "tone finder: reading the counts failed");
    const size_t k = count[1];
    bool ok = true;
    if (records && k)
        ok = ok && hipMemcpyAsync(records, t->last_records, k * sizeof(mi_tone_record), hipMemcpyDeviceToHost, q) == hipSuccess;
    if (powers && k)
        ok = ok && hipMemcpyAsync(powers, t->last_powers, k * MI_TONES_LANES * sizeof(float), hipMemcpyDeviceToHost, q) == hipSuccess;
    if (row_first_record)
        ok = ok && hipMemcpyAsync(row_first_record, t->last_row_first, (static_cast<size_t>(t->rows) + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, q) ==
                       hipSuccess;
    if (!ok || hipStreamSynchronize(q) != hipSuccess)
        return fail(MI_ERR_HIP, "tone finder: download failed");
    return MI_OK;
}

int mi_tones_set_timing(mi_tones* t, int on) {
    return mi::set_timing(t, on);
}

int mi_tones_last_launch_ms(mi_tones* t, float* ms) {
    return mi::last_launch_ms(t, ms, "mi_tones_process_device");
}

size_t mi_tones_state_size(const mi_tones* t) {
    return mi::state_size(t, &mi_tones::d_state);
}

int mi_tones_get_state(mi_tones* t, void* buf, size_t len) {
    return mi::get_state(kName, t, &mi_tones::d_state, buf, len);
}

int mi_tones_set_state(mi_tones* t, const void* buf, size_t len) {
    return mi::set_state(kName, t, &mi_tones::d_state, buf, len, [t](const mi::TonesRowState* rows, size_t n) {
        return mi::tones_state_ok(rows, n, t->window) ? nullptr : "malformed blob (count >= window or a padding lane not zero)";
    });
}

}  // extern "C"
