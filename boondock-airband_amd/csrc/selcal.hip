// selcal.hip -- the SELCAL decoder stage: which aircraft was called.  Per row and window of 2000 samples at a hop of 1000, a Goertzel
// bank over the SELCAL tone table, the energy of the window and the decision whether the window names a pair of tones; then, per row,
// a sequential decoder over the windows' pairs that emits one code record per call (two pulses, two tones each).  The reference
// leaves the chirps in the recording.  The windows, the order of every sum, the decision, the decoder's table and the state blob are
// in include/mi_airband.h.  A post-stage in the tone finder's mould: five launches on the caller's stream, no atomics.
// mi_selcal_plan_host (poststage_host.cpp) is the host twin; the decoder's step is one text for both (selcal_step, poststage.hpp).
// The handle's base and the bodies of the entry points every stage repeats are in poststage.hpp, the lead's load and the tails kernel
// in carry.hpp.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "../../include/mi_airband.h"
#include "carry.hpp"
#include "poststage.hpp"

constexpr char kName[] = "SELCAL stage";

struct mi_selcal : mi::RowStage {
    mi_selcal() : RowStage(kName, 5) {}
    mi::SelcalPlan plan{};
    uint32_t max_codes = 0;
    mi::DevBuf<mi::SelcalRowState> d_state;   // [rows]: the checkpoint blob as it is
    mi::DevBuf<float> d_window;               // [2000]
    mi::DevBuf<uint32_t> d_pair;              // [rows][2 * batches of the call]: what each window named
    mi::DevBuf<mi_selcal_code> d_scratch;     // [rows][most codes of a row in the call]: the walk's codes before they are placed
    mi::DevBuf<uint32_t> d_row_code_count;    // [rows]
    mi::PinnedBuf<uint32_t> h_count;          // [2], landing place of the counts in mi_selcal_download
    // destinations of the last mi_selcal_process_device (what mi_selcal_download reads)
    const mi_selcal_code* last_codes = nullptr;
    const mi_selcal_window_record* last_windows = nullptr;
    const uint32_t* last_row_first = nullptr;
    const uint32_t* last_count = nullptr;
    int last_nbatches = 0;
};

namespace {

using mi::aligned;
using mi::as_flags;
using mi::fail;
constexpr int kBatch = mi::kWaveBatch;           // 2000 floats = 500 float4
constexpr int kWin = MI_SELCAL_WINDOW;           // 2000
constexpr int kLead = MI_SELCAL_HISTORY + 2;     // 1004 floats staged in front of the block: two that are not used, then the 1002 of the history
constexpr int kStage = kLead + kBatch;           // 3004
constexpr int kFirstA = kLead - MI_SELCAL_HOP;   // 4: the staged index of window 2b's first sample; window 2b + 1 begins at kLead
constexpr int kMaxTones = MI_SELCAL_MAX_TONES;   // 32
static_assert(kLead % 4 == 0 && kFirstA % 4 == 0 && kFirstA >= 2 && kFirstA + kWin <= kStage && kLead + kWin == kStage && kWin % 4 == 0,
              "both windows are whole float4 of what is staged, and neither reads the lead's first two floats");
static_assert(2 * kMaxTones == 64, "one lane per (window of the block, tone)");

// What the bank is told of the settings.
struct BankArgs {
    float coeff[kMaxTones];  // 0 beyond the table
    uint32_t ntones;
    float min_energy, tc, max_twist, min_separation;
};

__device__ __forceinline__ float lane_read(const float v, const int lane) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// Launch 1, the hot path.  One wave, one workgroup, per (row, batch) block of an enabled row.  The block's 2000 samples behind the
// 1004 in front of them -- out of the row's previous batch, or the carried samples at batch 0 -- go into LDS times the window, once for
// each of the block's two windows (the halves that overlap meet different window coefficients): y[0] for window 2b, y[1] for 2b + 1,
// 16000 bytes.  E of both comes out of the same arrays, lane l summing j = l (mod 64) and an xor butterfly standing for the halving
// one (float addition commutes, so every lane holds the halving tree's element 0).  Lane 32 h + t then runs tone t's recurrence over
// window h: each group of four steps reads one float4 of y[h], one address per half-wave, which LDS broadcasts -- three dependent VALU
// operations a step and a quarter of an LDS read.  A wave alone is bound by that dependency chain; the SIMD is kept busy by the other
// blocks' waves on it, ten to a CU at 16000 bytes of LDS each.  Where both windows are silent (E == 0: a closed batch) the recurrence
// is skipped: the header defines such a window's powers as zero.  The three largest powers of each window are picked in wave-uniform
// code, lane by lane in index order as the definition does, and lane 0 writes both windows' records and decisions.
__global__ __launch_bounds__(64) void k_selcal_bank(const uint8_t* __restrict__ enabled, const mi::SelcalRowState* __restrict__ state,
                                                    const float* __restrict__ plane, const size_t row_stride, const uint32_t nbatches,
                                                    const float* __restrict__ window, const BankArgs a, uint32_t* __restrict__ pair_out,
                                                    mi_selcal_window_record* __restrict__ windows) {
    __shared__ __align__(16) float y[2][kWin];
    const int lane = threadIdx.x;
    const uint32_t row = blockIdx.x / nbatches, batch = blockIdx.x - row * nbatches;  // (the grid is rows * nbatches)
    if (!enabled[row])  // (the whole wave) the row sits out: no record, no decision
        return;
    const float* const blk = plane + static_cast<size_t>(row) * row_stride + static_cast<size_t>(batch) * kBatch;
    const float4* const w4 = reinterpret_cast<const float4*>(window);
    for (int q = lane; q < kStage / 4; q += 64) {
        const float4 v = mi::load_lead4<kLead>(blk, state[row], q, batch == 0);
        if (q >= kFirstA / 4 && q < (kFirstA + kWin) / 4) {
            const float4 c = w4[q - kFirstA / 4];
            reinterpret_cast<float4*>(y[0])[q - kFirstA / 4] = make_float4(v.x * c.x, v.y * c.y, v.z * c.z, v.w * c.w);
        }
        if (q >= kLead / 4) {
            const float4 c = w4[q - kLead / 4];
            reinterpret_cast<float4*>(y[1])[q - kLead / 4] = make_float4(v.x * c.x, v.y * c.y, v.z * c.z, v.w * c.w);
        }
    }
    __syncthreads();
    float e[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        float s = y[h][lane] * y[h][lane];
        for (int j = lane + 64; j < kWin; j += 64)
            s = s + y[h][j] * y[h][j];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1)
            s = s + __shfl_xor(s, d);
        e[h] = s;
    }
    const int half = lane >> 5, tone = lane & 31;
    const float coeff = a.coeff[tone];
    float q1 = 0.0f, q2 = 0.0f;
    if (e[0] != 0.0f || e[1] != 0.0f) {  // (the whole wave)
        const float4* const yp = reinterpret_cast<const float4*>(y[half]);
#pragma unroll 4
        for (int g = 0; g < kWin / 4; ++g) {
            const float4 v = yp[g];
            float q0 = coeff * q1 - q2 + v.x;
            q2 = coeff * q0 - q1 + v.y;
            q1 = coeff * q2 - q0 + v.z;
            q0 = coeff * q1 - q2 + v.w;
            q2 = q1;
            q1 = q0;
        }
    }
    float p = q1 * q1 + q2 * q2 - q1 * q2 * coeff;
    if (e[half] == 0.0f || static_cast<uint32_t>(tone) >= a.ntones)  // a silent window's powers are zero by definition
        p = 0.0f;
    const size_t k0 = (static_cast<size_t>(row) * nbatches + batch) * 2;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        int i0 = 0, i1 = -1, i2 = -1;
        float p0 = lane_read(p, 32 * h), p1 = 0.0f, p2 = 0.0f;
        for (int t = 1; t < static_cast<int>(a.ntones); ++t) {  // (wave-uniform)
            const float m = lane_read(p, 32 * h + t);
            if (m > p0) {
                i2 = i1, p2 = p1;
                i1 = i0, p1 = p0;
                i0 = t, p0 = m;
            } else if (i1 < 0 || m > p1) {
                i2 = i1, p2 = p1;
                i1 = t, p1 = m;
            } else if (i2 < 0 || m > p2) {
                i2 = t, p2 = m;
            }
        }
        if (i2 < 0)
            p2 = 0.0f;
        const float E = e[h];
        const bool named = E >= a.min_energy && p0 + p1 >= a.tc * E && p0 <= a.max_twist * p1 && p1 >= a.min_separation * p2;
        const uint32_t lo = static_cast<uint32_t>(i0 < i1 ? i0 : i1), hi = static_cast<uint32_t>(i0 < i1 ? i1 : i0);
        const uint32_t pair = named ? lo | hi << 8 : MI_SELCAL_NONE;
        if (lane == 0) {
            pair_out[k0 + h] = pair;
            if (windows) {  // 24 bytes, 8-byte aligned: three 8-byte vector stores
                uint2* const r = reinterpret_cast<uint2*>(windows + k0 + h);
                const uint32_t third = i2 < 0 ? static_cast<uint32_t>(MI_SELCAL_NONE8) : static_cast<uint32_t>(i2);
                r[0] = make_uint2(static_cast<uint32_t>(i0) | static_cast<uint32_t>(i1) << 8 | third << 16, __float_as_uint(p0));
                r[1] = make_uint2(__float_as_uint(p1), __float_as_uint(p2));
                r[2] = make_uint2(__float_as_uint(E), pair);
            }
        }
    }
}

// Launch 2.  One lane per row: the decoder over the call's 2 * nbatches decisions in order, its codes into the row's slots of the
// scratch, the row's count, and the decoder's part of the state (the carried samples are the tails kernel's).
__global__ __launch_bounds__(256) void k_selcal_walk(const uint8_t* __restrict__ enabled, mi::SelcalRowState* __restrict__ state,
                                                     const uint32_t* __restrict__ pairs, const uint32_t rows, const uint32_t nwin, const uint32_t slots,
                                                     const uint32_t min_run, const uint32_t max_run, const uint32_t max_gap,
                                                     mi_selcal_code* __restrict__ scratch, uint32_t* __restrict__ row_code_count) {
    const uint32_t row = blockIdx.x * 256 + threadIdx.x;
    if (row >= rows)
        return;
    if (!enabled[row]) {  // the row sits out: no code, every byte of its state stays
        row_code_count[row] = 0;
        return;
    }
    mi::SelcalRowState* const st = state + row;
    const uint32_t n0 = st->window, seq0 = st->seq;
    mi::SelcalDecoder d{st->phase, st->pair1, st->pair2, st->run1, st->run2, st->gap, st->first_window};
    const uint32_t* const pr = pairs + static_cast<size_t>(row) * nwin;
    uint32_t n = 0;
    for (uint32_t i = 0; i < nwin; ++i) {
        if (!mi::selcal_step(d, pr[i], n0 + i, min_run, max_run, max_gap))
            continue;
        if (n < slots) {  // (always: slots is the most a row can emit)
            uint4* const c = reinterpret_cast<uint4*>(scratch + static_cast<size_t>(row) * slots + n);
            const uint32_t tones = (d.pair1 & 0xFFu) | (d.pair1 >> 8) << 8 | (d.pair2 & 0xFFu) << 16 | (d.pair2 >> 8) << 24;
            c[0] = make_uint4(row, seq0 + n, tones, d.first_window);
            c[1] = make_uint4(n0 + i, d.run1, d.gap, i / 2);
            ++n;
        }
    }
    st->window = n0 + nwin;
    st->seq = seq0 + n;
    st->phase = d.phase;
    st->pair1 = d.pair1;
    st->pair2 = d.pair2;
    st->run1 = d.run1;
    st->run2 = d.run2;
    st->gap = d.gap;
    st->first_window = d.first_window;
    row_code_count[row] = n;
}

// Launch 3.  mi::launch_row_scan (poststage.hip): exclusive scan of the rows' code counts, and the two counts.

// Launch 4.  One thread per (row, slot): a code the row emitted goes to its place, unless that is at or beyond the capacity.
__global__ __launch_bounds__(256) void k_selcal_store(const mi_selcal_code* __restrict__ scratch, const uint32_t* __restrict__ row_code_count,
                                                      const uint32_t* __restrict__ row_first, const uint32_t rows, const uint32_t slots,
                                                      const uint32_t max_codes, mi_selcal_code* __restrict__ codes) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    const uint32_t row = i / slots, j = i - row * slots;
    if (row >= rows || j >= row_code_count[row])
        return;
    const uint32_t k = row_first[row] + j;
    if (k >= max_codes)
        return;
    const uint2* const src = reinterpret_cast<const uint2*>(scratch + i);
    uint2* const dst = reinterpret_cast<uint2*>(codes + k);  // 32 bytes, 8-byte aligned: four 8-byte vector stores
#pragma unroll
    for (int m = 0; m < 4; ++m)
        dst[m] = src[m];
}

// Launch 5.  mi::k_carry_tails (carry.hpp): the last 1002 input samples of the call are an enabled row's new carried samples.

}  // namespace

extern "C" {

int mi_selcal_create(const mi_selcal_cfg* cfg, const uint8_t* row_enabled, int rows, int max_batches, size_t max_codes, int gpu, mi_selcal** out) {
    if (!row_enabled || !out)
        return fail(MI_ERR_INVALID, "NULL argument");
    mi::SelcalPlan plan;
    if (const int rc = mi::selcal_plan(cfg, &plan))
        return rc;
    if (const int rc = mi::batch_geometry_ok(kName, rows, max_batches))
        return rc;
    if (const int rc = mi::check_gpu(gpu, "no HIP device: the SELCAL stage runs on the GPU only"))
        return rc;
    mi_selcal* s = new mi_selcal();
    s->gpu = gpu;
    s->rows = rows;
    s->max_batches = max_batches;
    s->plan = plan;
    const size_t n = static_cast<size_t>(rows), most = n * mi::selcal_max_codes(plan.min_run, static_cast<uint64_t>(max_batches));
    s->max_codes = static_cast<uint32_t>(max_codes && max_codes < most ? max_codes : most);  // (no call has more codes than `most`)
    std::vector<float> w(MI_SELCAL_WINDOW);
    mi::selcal_window(w.data());
    if (hipSetDevice(gpu) != hipSuccess || dalloc_copy(s->d_enabled, as_flags(row_enabled, n)) != hipSuccess || dalloc_zero(s->d_state, n) != hipSuccess ||
        dalloc_copy(s->d_window, w) != hipSuccess || dalloc(s->d_pair, n * 2 * static_cast<size_t>(max_batches)) != hipSuccess ||
        dalloc(s->d_scratch, most) != hipSuccess || dalloc(s->d_row_code_count, n) != hipSuccess ||
        hipHostMalloc(reinterpret_cast<void**>(s->h_count.put()), 2 * sizeof(uint32_t)) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
        delete s;
        return fail(MI_ERR_HIP, "SELCAL stage: device allocation failed");
    }
    *out = s;
    return MI_OK;
}

void mi_selcal_destroy(mi_selcal* s) {
    mi::destroy(s);
}

int mi_selcal_set_rows(mi_selcal* s, const uint8_t* row_enabled) {
    return mi::set_enabled(kName, s, row_enabled);
}

int mi_selcal_process_device(mi_selcal* s, const float* d_plane, size_t row_stride, int nbatches, mi_selcal_window_record* d_windows,
                             mi_selcal_code* d_codes, uint32_t* d_row_first_code, uint32_t* d_count, void* hip_stream) {
    if (!s || !d_plane || !d_codes || !d_row_first_code || !d_count)
        return fail(MI_ERR_INVALID, "NULL argument");
    if (nbatches < 1 || nbatches > s->max_batches)
        return fail(MI_ERR_INVALID, "nbatches outside 1 .. max_batches");
    if (row_stride < static_cast<size_t>(nbatches) * mi::kWaveBatch)
        return fail(MI_ERR_INVALID, "a row stride is shorter than the call");
    if (row_stride % 4 != 0 || !aligned(d_plane, 16) || !aligned(d_windows, 8) || !aligned(d_codes, 8) || !aligned(d_row_first_code, 4) || !aligned(d_count, 4))
        return fail(MI_ERR_INVALID, "the plane must be 16-byte aligned with a row stride that is a multiple of 4 floats; window and code records 8-byte aligned");
    if (hipSetDevice(s->gpu) != hipSuccess)
        return fail(MI_ERR_HIP, "hipSetDevice failed");
    hipStream_t q = static_cast<hipStream_t>(hip_stream);
    const unsigned rows = static_cast<unsigned>(s->rows), nb = static_cast<unsigned>(nbatches);
    // the codes a row can emit in this call: at most what create allocated, as nbatches <= max_batches
    const uint32_t slots = mi::selcal_max_codes(s->plan.min_run, nb);
    BankArgs a{};
    std::memcpy(a.coeff, s->plan.coeff, sizeof(a.coeff));
    a.ntones = s->plan.ntones;
    a.min_energy = s->plan.min_energy;
    a.tc = s->plan.tc;
    a.max_twist = s->plan.max_twist;
    a.min_separation = s->plan.min_separation;
    s->timing.stamp(0, q);
    hipLaunchKernelGGL(k_selcal_bank, dim3(rows * nb), dim3(64), 0, q, s->d_enabled.get(), s->d_state.get(), d_plane, row_stride, nb, s->d_window.get(), a,
                       s->d_pair.get(), d_windows);
    s->timing.stamp(1, q);
    hipLaunchKernelGGL(k_selcal_walk, dim3((rows + 255) / 256), dim3(256), 0, q, s->d_enabled.get(), s->d_state.get(), s->d_pair.get(), rows, 2 * nb, slots,
                       s->plan.min_run, s->plan.max_run, s->plan.max_gap, s->d_scratch.get(), s->d_row_code_count.get());
    s->timing.stamp(2, q);
    mi::launch_row_scan(q, s->d_row_code_count, s->rows, s->max_codes, d_row_first_code, d_count);
    s->timing.stamp(3, q);
    hipLaunchKernelGGL(k_selcal_store, dim3((rows * slots + 255) / 256), dim3(256), 0, q, s->d_scratch.get(), s->d_row_code_count.get(), d_row_first_code, rows,
                       slots, s->max_codes, d_codes);
    s->timing.stamp(4, q);
    mi::launch_carry_tails<MI_SELCAL_HISTORY>(q, s->d_enabled.get(), d_plane, row_stride, rows, nbatches, s->d_state.get());
    s->timing.stamp(5, q);
    if (hipGetLastError() != hipSuccess)
        return fail(MI_ERR_HIP, "SELCAL stage kernel launch failed");
    s->called = true;
    s->last_codes = d_codes;
    s->last_windows = d_windows;
    s->last_row_first = d_row_first_code;
    s->last_count = d_count;
    s->last_nbatches = nbatches;
    return MI_OK;
}

int mi_selcal_download(mi_selcal* s, void* hip_stream, mi_selcal_code* codes, mi_selcal_window_record* windows, uint32_t* row_first_code, uint32_t* count) {
    if (!s || !count)
        return fail(MI_ERR_INVALID, "NULL argument");
    if (!s->last_count)
        return fail(MI_ERR_INVALID, "no mi_selcal_process_device call to download");
    if (windows && !s->last_windows)
        return fail(MI_ERR_INVALID, "the last mi_selcal_process_device call stored no window records");
    hipStream_t q = static_cast<hipStream_t>(hip_stream);
    if (!mi::land_counts(s->gpu, q, s->h_count, s->last_count, count))
        return fail(MI_ERR_HIP, "SELCAL stage: reading the counts failed");
    const size_t k = count[1], nw = static_cast<size_t>(s->rows) * 2 * static_cast<size_t>(s->last_nbatches);
    bool ok = true;
    if (codes && k)
        ok = ok && hipMemcpyAsync(codes, s->last_codes, k * sizeof(mi_selcal_code), hipMemcpyDeviceToHost, q) == hipSuccess;
    if (windows)
        ok = ok && hipMemcpyAsync(windows, s->last_windows, nw * sizeof(mi_selcal_window_record), hipMemcpyDeviceToHost, q) == hipSuccess;
    if (row_first_code)
        ok = ok && hipMemcpyAsync(row_first_code, s->last_row_first, (static_cast<size_t>(s->rows) + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, q) ==
                       hipSuccess;
    if (!ok || hipStreamSynchronize(q) != hipSuccess)
        return fail(MI_ERR_HIP, "SELCAL stage: download failed");
    return MI_OK;
}

int mi_selcal_set_timing(mi_selcal* s, int on) {
    return mi::set_timing(s, on);
}

int mi_selcal_last_launch_ms(mi_selcal* s, float* ms) {
    return mi::last_launch_ms(s, ms, "mi_selcal_process_device");
}

size_t mi_selcal_state_size(const mi_selcal* s) {
    return mi::state_size(s, &mi_selcal::d_state);
}

int mi_selcal_get_state(mi_selcal* s, void* buf, size_t len) {
    return mi::get_state(kName, s, &mi_selcal::d_state, buf, len);
}

int mi_selcal_set_state(mi_selcal* s, const void* buf, size_t len) {
    return mi::set_state(kName, s, &mi_selcal::d_state, buf, len,
                         [s](const mi::SelcalRowState* rows, size_t n) { return mi::selcal_state_ok(rows, n, s->plan); });
}

}  // extern "C"
