// elt.hip -- the ELT detector stage: which row carries a distress beacon's swept tone, and since when.  Per row and frame of 256
// samples at a hop of 80, a Goertzel bank over the bins 2 .. 33 of the 256-point transform, the frame's energy and the decision whether
// the frame is tonal and on which bin; then, per row, a sequential walker over the frames' bins that follows sweeps, chains valid ones
// and emits one record when a beacon starts and one when it ends.  The reference leaves the wail in the recording.  The frames, the
// order of every sum, the decision, the walker's rules and the state blob are in include/mi_airband.h.  A post-stage in the SELCAL
// stage's mould: five launches on the caller's stream, no atomics.  mi_elt_plan_host (poststage_host.cpp) is the host twin; the
// walker's step is one text for both (elt_step, poststage.hpp).  The handle's base and the bodies of the entry points every stage
// repeats are in poststage.hpp, the lead's load and the tails kernel in carry.hpp.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "../../include/mi_airband.h"
#include "carry.hpp"
#include "poststage.hpp"

constexpr char kName[] = "ELT stage";

struct mi_elt : mi::RowStage {
    mi_elt() : RowStage(kName, 5) {}
    mi::EltPlan plan{};
    uint32_t max_events = 0;
    mi::DevBuf<mi::EltRowState> d_state;    // [rows]: the checkpoint blob as it is
    mi::DevBuf<float> d_window;             // [256]
    mi::DevBuf<uint8_t> d_bin;              // [rows][batches of the call][32]: what each frame decided, 25 bytes of every 32
    mi::DevBuf<mi_elt_event> d_scratch;     // [rows][most events of a row in the call]: the walk's events before they are placed
    mi::DevBuf<uint32_t> d_row_event_count; // [rows]
    mi::PinnedBuf<uint32_t> h_count;        // [2], landing place of the counts in mi_elt_download
    // destinations of the last mi_elt_process_device (what mi_elt_download reads)
    const mi_elt_event* last_events = nullptr;
    const mi_elt_frame_record* last_frames = nullptr;
    const uint32_t* last_row_first = nullptr;
    const uint32_t* last_count = nullptr;
    int last_nbatches = 0;
};

namespace {

using mi::aligned;
using mi::as_flags;
using mi::fail;
constexpr int kBatch = mi::kWaveBatch;        // 2000 floats = 500 float4
constexpr int kFrame = MI_ELT_FRAME;          // 256
constexpr int kHop = MI_ELT_HOP;              // 80
constexpr int kFrames = MI_ELT_FRAMES;        // 25
constexpr int kBins = MI_ELT_BINS;            // 32
constexpr int kLead = MI_ELT_HISTORY + 2;     // 180 floats staged in front of the block: two that are not used, then the 178 of the history
constexpr int kStage = kLead + kBatch;        // 2180
constexpr int kFirst = kLead - (kFrame - kHop);  // 4: the staged index of frame 0's first sample; frame g begins at kFirst + 80 g
constexpr int kPasses = (kFrames + 1) / 2;    // 13: two frames a pass, one to each half of the wave
constexpr int kBinSlot = 32;                  // bytes of decisions per block, of which 25 are used: two 16-byte loads for the walk
static_assert(kLead % 4 == 0 && kFirst % 4 == 0 && kHop % 4 == 0 && kFirst >= 2 && kFirst + (kFrames - 1) * kHop + kFrame == kStage && kFrame % 64 == 0,
              "every frame is whole float4 of what is staged, none reads the lead's first two floats, and the last ends with the block");
static_assert(2 * kBins == 64 && kFrames <= kBinSlot, "one lane per (frame of the pass, bin)");

// What the bank is told of the settings.
struct BankArgs {
    float min_energy, tc;
    uint32_t band_lo, band_hi;
};

// Launch 1, the hot path.  One wave, one workgroup, per (row, batch) block of an enabled row.  The block's 2000 samples behind the 180
// in front of them -- out of the row's previous batch, or the carried samples at batch 0 -- go into LDS as they are, 9040 bytes with
// the zeros behind them that the idle half of the last pass reads, and the window beside them, 1024: frames overlap by 176 samples and
// each meets the window at another place, so y = x * w is made where it is used.  A block whose staged floats are all +-0 (a closed
// batch) writes its 25 silent records at once.  Otherwise the 25 energies first: lane l sums j = l (mod 64) and an xor butterfly
// stands for the halving one (float addition commutes, so every lane holds the halving tree's element 0).  Then thirteen passes of two
// frames: lane 32 h + t runs bin t + 2's recurrence over frame 2 i + h.  Each group of four steps reads one float4 of x, one address
// per half-wave, and one float4 of w, one address for the wave: LDS broadcasts both.  Four multiplications off the chain and three
// dependent operations a step.  A wave alone is bound by that chain; the SIMD is kept busy by the other blocks' waves on it, sixteen
// to a CU at 10192 bytes of LDS each.  A silent frame's powers are zero by definition.  The largest power of each frame is found by an
// xor butterfly inside the half-wave that carries (power, bin) and prefers the lower bin on a tie, which is the definition's order;
// its neighbours come by two lane reads.  Lanes 0 and 32 write their frame's record and decision.
__global__ __launch_bounds__(64) void k_elt_bank(const uint8_t* __restrict__ enabled, const mi::EltRowState* __restrict__ state,
                                                 const float* __restrict__ plane, const size_t row_stride, const uint32_t nbatches,
                                                 const float* __restrict__ window, const float* __restrict__ coeffs, const BankArgs a,
                                                 uint8_t* __restrict__ bin_out, mi_elt_frame_record* __restrict__ frames) {
    __shared__ __align__(16) float x[kStage + kHop];  // (kStage, and the 80 floats the idle half of the last pass reads: zeros)
    __shared__ __align__(16) float w[kFrame];
    __shared__ float energy[kBinSlot];
    const int lane = threadIdx.x;
    const uint32_t row = blockIdx.x / nbatches, batch = blockIdx.x - row * nbatches;  // (the grid is rows * nbatches)
    if (!enabled[row])  // (the whole wave) the row sits out: no record, no decision
        return;
    const float* const blk = plane + static_cast<size_t>(row) * row_stride + static_cast<size_t>(batch) * kBatch;
    uint32_t any = 0;
    for (int q = lane; q < kStage / 4; q += 64) {
        const float4 v = mi::load_lead4<kLead>(blk, state[row], q, batch == 0);
        reinterpret_cast<float4*>(x)[q] = v;
        any |= (__float_as_uint(v.x) | __float_as_uint(v.y) | __float_as_uint(v.z) | __float_as_uint(v.w)) & 0x7FFFFFFFu;
    }
    if (lane < kHop / 4)
        reinterpret_cast<float4*>(x)[kStage / 4 + lane] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    reinterpret_cast<float4*>(w)[lane] = reinterpret_cast<const float4*>(window)[lane];
    const size_t k0 = (static_cast<size_t>(row) * nbatches + batch) * kFrames;
    uint8_t* const bins = bin_out + (static_cast<size_t>(row) * nbatches + batch) * kBinSlot;
    if (!__any(any != 0)) {  // (the whole wave) digital silence: E = +0.0f, every power +0.0f, best the lowest bin, no decision
        if (lane < kFrames) {
            bins[lane] = MI_ELT_NONE8;
            if (frames) {  // 16 bytes, 8-byte aligned: two 8-byte vector stores
                uint2* const r = reinterpret_cast<uint2*>(frames + k0 + lane);
                r[0] = make_uint2(static_cast<uint32_t>(MI_ELT_BIN0) | static_cast<uint32_t>(MI_ELT_NONE8) << 8, 0u);
                r[1] = make_uint2(0u, 0u);
            }
        }
        return;
    }
    __syncthreads();
    for (int g = 0; g < kFrames; ++g) {
        const float* const xf = x + kFirst + g * kHop;
        float y = xf[lane] * w[lane];
        float s = y * y;
#pragma unroll
        for (int j = 64; j < kFrame; j += 64) {
            y = xf[lane + j] * w[lane + j];
            s = s + y * y;
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1)
            s = s + __shfl_xor(s, d);
        if (lane == 0)
            energy[g] = s;
    }
    __syncthreads();
    const int half = lane >> 5, t = lane & 31;
    const float coeff = coeffs[t];
    const float4* const w4 = reinterpret_cast<const float4*>(w);
    for (int i = 0; i < kPasses; ++i) {
        const int g = 2 * i + half;
        const bool real = g < kFrames;  // (the last pass has one frame; its other half runs over zeros and writes nothing)
        const float E = real ? energy[g] : 0.0f;
        const float4* const xp = reinterpret_cast<const float4*>(x + kFirst + g * kHop);
        float q1 = 0.0f, q2 = 0.0f;
#pragma unroll 4
        for (int n = 0; n < kFrame / 4; ++n) {
            const float4 v = xp[n], c = w4[n];
            float q0 = coeff * q1 - q2 + v.x * c.x;
            q2 = coeff * q0 - q1 + v.y * c.y;
            q1 = coeff * q2 - q0 + v.z * c.z;
            q0 = coeff * q1 - q2 + v.w * c.w;
            q2 = q1;
            q1 = q0;
        }
        float p = q1 * q1 + q2 * q2 - q1 * q2 * coeff;
        if (E == 0.0f)  // a silent frame's powers are zero by definition
            p = 0.0f;
        float pb = p;
        int best = t;
#pragma unroll
        for (int d = 16; d >= 1; d >>= 1) {
            const float po = __shfl_xor(pb, d);
            const int bo = __shfl_xor(best, d);
            if (po > pb || (po == pb && bo < best)) {
                pb = po;
                best = bo;
            }
        }
        const float lo = __shfl(p, 32 * half + (best > 0 ? best - 1 : 0)), hi = __shfl(p, 32 * half + (best < kBins - 1 ? best + 1 : kBins - 1));
        const float p3 = (best > 0 ? lo : 0.0f) + pb + (best < kBins - 1 ? hi : 0.0f);
        const uint32_t bin = static_cast<uint32_t>(best) + MI_ELT_BIN0;
        const bool tonal = E >= a.min_energy && p3 >= a.tc * E && bin >= a.band_lo && bin <= a.band_hi;
        const uint32_t decided = tonal ? bin : static_cast<uint32_t>(MI_ELT_NONE8);
        if (t == 0 && real) {
            bins[g] = static_cast<uint8_t>(decided);
            if (frames) {
                uint2* const r = reinterpret_cast<uint2*>(frames + k0 + g);
                r[0] = make_uint2(bin | decided << 8, __float_as_uint(E));
                r[1] = make_uint2(__float_as_uint(pb), __float_as_uint(p3));
            }
        }
    }
}

// Launch 2.  One lane per row: the walker over the call's 25 * nbatches decisions in order, its events into the row's slots of the
// scratch, the row's count, and the walker's part of the state (the carried samples are the tails kernel's).
__global__ __launch_bounds__(256) void k_elt_walk(const uint8_t* __restrict__ enabled, mi::EltRowState* __restrict__ state,
                                                  const uint8_t* __restrict__ bins, const uint32_t rows, const uint32_t nbatches, const uint32_t slots,
                                                  const mi::EltRules rules, mi_elt_event* __restrict__ scratch, uint32_t* __restrict__ row_event_count) {
    const uint32_t row = blockIdx.x * 256 + threadIdx.x;
    if (row >= rows)
        return;
    if (!enabled[row]) {  // the row sits out: no event, every byte of its state stays
        row_event_count[row] = 0;
        return;
    }
    mi::EltRowState* const st = state + row;
    const uint32_t f0 = st->frame, seq0 = st->seq;
    mi::EltWalker w{st->open, st->start, st->first_bin, st->last_bin, st->last_frame, st->dir, st->drops, st->count, st->chain_dir, st->chain_first,
                    st->last_end, st->alarmed, st->bin_from, st->bin_to};
    const uint4* const br = reinterpret_cast<const uint4*>(bins + static_cast<size_t>(row) * nbatches * kBinSlot);
    uint32_t n = 0;
    for (uint32_t b = 0; b < nbatches; ++b) {
        const uint4 lo = br[2 * b], hi = br[2 * b + 1];
        const uint32_t word[7] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z};
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            uint32_t v = word[k];
#pragma nounroll
            for (int m = 4 * k; m < 4 * k + 4 && m < kFrames; ++m, v >>= 8) {
                const uint32_t f = f0 + b * kFrames + static_cast<uint32_t>(m);
                mi::elt_step(w, rules, v & 0xFFu, f, [&](uint32_t kind) {
                    if (n < slots) {  // (always: slots is the most a row can emit)
                        uint4* const e = reinterpret_cast<uint4*>(scratch + static_cast<size_t>(row) * slots + n);
                        e[0] = make_uint4(row, seq0 + n, mi::elt_event_word2(w, kind), f);
                        e[1] = make_uint4(w.chain_first, w.last_end, w.count, b);
                        ++n;
                    }
                });
            }
        }
    }
    st->frame = f0 + nbatches * kFrames;
    st->seq = seq0 + n;
    st->open = w.open, st->start = w.start, st->first_bin = w.first_bin, st->last_bin = w.last_bin, st->last_frame = w.last_frame, st->dir = w.dir;
    st->drops = w.drops, st->count = w.count, st->chain_dir = w.chain_dir, st->chain_first = w.chain_first, st->last_end = w.last_end;
    st->alarmed = w.alarmed, st->bin_from = w.bin_from, st->bin_to = w.bin_to;
    row_event_count[row] = n;
}

// Launch 3.  mi::launch_row_scan (poststage.hip): exclusive scan of the rows' event counts, and the two counts.

// Launch 4.  One thread per (row, slot): an event the row emitted goes to its place, unless that is at or beyond the capacity.
__global__ __launch_bounds__(256) void k_elt_store(const mi_elt_event* __restrict__ scratch, const uint32_t* __restrict__ row_event_count,
                                                   const uint32_t* __restrict__ row_first, const uint32_t rows, const uint32_t slots,
                                                   const uint32_t max_events, mi_elt_event* __restrict__ events) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    const uint32_t row = i / slots, j = i - row * slots;
    if (row >= rows || j >= row_event_count[row])
        return;
    const uint32_t k = row_first[row] + j;
    if (k >= max_events)
        return;
    const uint2* const src = reinterpret_cast<const uint2*>(scratch + i);
    uint2* const dst = reinterpret_cast<uint2*>(events + k);  // 32 bytes, 8-byte aligned: four 8-byte vector stores
#pragma unroll
    for (int m = 0; m < 4; ++m)
        dst[m] = src[m];
}

// Launch 5.  mi::k_carry_tails (carry.hpp): the last 178 input samples of the call are an enabled row's new carried samples.

}  // namespace

extern "C" {

int mi_elt_create(const mi_elt_cfg* cfg, const uint8_t* row_enabled, int rows, int max_batches, size_t max_events, int gpu, mi_elt** out) {
    if (!row_enabled || !out)
        return fail(MI_ERR_INVALID, "NULL argument");
    mi::EltPlan plan;
    if (const int rc = mi::elt_plan(cfg, &plan))
        return rc;
    if (const int rc = mi::batch_geometry_ok(kName, rows, max_batches))
        return rc;
    if (const int rc = mi::check_gpu(gpu, "no HIP device: the ELT stage runs on the GPU only"))
        return rc;
    mi_elt* s = new mi_elt();
    s->gpu = gpu;
    s->rows = rows;
    s->max_batches = max_batches;
    s->plan = plan;
    const size_t n = static_cast<size_t>(rows), most = n * mi::elt_max_events(plan.min_sweeps, plan.min_len, static_cast<uint64_t>(max_batches));
    s->max_events = static_cast<uint32_t>(max_events && max_events < most ? max_events : most);  // (no call has more events than `most`)
    std::vector<float> w(MI_ELT_FRAME + MI_ELT_BINS);  // the window, and the coefficients behind it
    mi::elt_window(w.data());
    std::memcpy(w.data() + MI_ELT_FRAME, plan.coeff, sizeof(plan.coeff));
    if (hipSetDevice(gpu) != hipSuccess || dalloc_copy(s->d_enabled, as_flags(row_enabled, n)) != hipSuccess || dalloc_zero(s->d_state, n) != hipSuccess ||
        dalloc_copy(s->d_window, w) != hipSuccess || dalloc(s->d_bin, n * kBinSlot * static_cast<size_t>(max_batches)) != hipSuccess ||
        dalloc(s->d_scratch, most) != hipSuccess || dalloc(s->d_row_event_count, n) != hipSuccess ||
        hipHostMalloc(reinterpret_cast<void**>(s->h_count.put()), 2 * sizeof(uint32_t)) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
        delete s;
        return fail(MI_ERR_HIP, "ELT stage: device allocation failed");
    }
    *out = s;
    return MI_OK;
}

void mi_elt_destroy(mi_elt* s) {
    mi::destroy(s);
}

int mi_elt_set_rows(mi_elt* s, const uint8_t* row_enabled) {
    return mi::set_enabled(kName, s, row_enabled);
}

int mi_elt_process_device(mi_elt* s, const float* d_plane, size_t row_stride, int nbatches, mi_elt_frame_record* d_frames, mi_elt_event* d_events,
                          uint32_t* d_row_first_event, uint32_t* d_count, void* hip_stream) {
    if (!s || !d_plane || !d_events || !d_row_first_event || !d_count)
        return fail(MI_ERR_INVALID, "NULL argument");
    if (nbatches < 1 || nbatches > s->max_batches)
        return fail(MI_ERR_INVALID, "nbatches outside 1 .. max_batches");
    if (row_stride < static_cast<size_t>(nbatches) * mi::kWaveBatch)
        return fail(MI_ERR_INVALID, "a row stride is shorter than the call");
    if (row_stride % 4 != 0 || !aligned(d_plane, 16) || !aligned(d_frames, 8) || !aligned(d_events, 8) || !aligned(d_row_first_event, 4) || !aligned(d_count, 4))
        return fail(MI_ERR_INVALID, "the plane must be 16-byte aligned with a row stride that is a multiple of 4 floats; frame and event records 8-byte aligned");
    if (hipSetDevice(s->gpu) != hipSuccess)
        return fail(MI_ERR_HIP, "hipSetDevice failed");
    hipStream_t q = static_cast<hipStream_t>(hip_stream);
    const unsigned rows = static_cast<unsigned>(s->rows), nb = static_cast<unsigned>(nbatches);
    // the events a row can emit in this call: at most what create allocated, as nbatches <= max_batches
    const uint32_t slots = mi::elt_max_events(s->plan.min_sweeps, s->plan.min_len, nb);
    const BankArgs a{s->plan.min_energy, s->plan.tc, s->plan.band_lo, s->plan.band_hi};
    s->timing.stamp(0, q);
    hipLaunchKernelGGL(k_elt_bank, dim3(rows * nb), dim3(64), 0, q, s->d_enabled.get(), s->d_state.get(), d_plane, row_stride, nb, s->d_window.get(),
                       s->d_window.get() + MI_ELT_FRAME, a, s->d_bin.get(), d_frames);
    s->timing.stamp(1, q);
    hipLaunchKernelGGL(k_elt_walk, dim3((rows + 255) / 256), dim3(256), 0, q, s->d_enabled.get(), s->d_state.get(), s->d_bin.get(), rows, nb, slots,
                       mi::elt_rules(s->plan), s->d_scratch.get(), s->d_row_event_count.get());
    s->timing.stamp(2, q);
    mi::launch_row_scan(q, s->d_row_event_count, s->rows, s->max_events, d_row_first_event, d_count);
    s->timing.stamp(3, q);
    hipLaunchKernelGGL(k_elt_store, dim3((rows * slots + 255) / 256), dim3(256), 0, q, s->d_scratch.get(), s->d_row_event_count.get(), d_row_first_event, rows,
                       slots, s->max_events, d_events);
    s->timing.stamp(4, q);
    mi::launch_carry_tails<MI_ELT_HISTORY>(q, s->d_enabled.get(), d_plane, row_stride, rows, nbatches, s->d_state.get());
    s->timing.stamp(5, q);
    if (hipGetLastError() != hipSuccess)
        return fail(MI_ERR_HIP, "ELT stage kernel launch failed");
    s->called = true;
    s->last_events = d_events;
    s->last_frames = d_frames;
    s->last_row_first = d_row_first_event;
    s->last_count = d_count;
    s->last_nbatches = nbatches;
    return MI_OK;
}

int mi_elt_download(mi_elt* s, void* hip_stream, mi_elt_event* events, mi_elt_frame_record* frames, uint32_t* row_first_event, uint32_t* count) {
    if (!s || !count)
        return fail(MI_ERR_INVALID, "NULL argument");
    if (!s->last_count)
        return fail(MI_ERR_INVALID, "no mi_elt_process_device call to download");
    if (frames && !s->last_frames)
        return fail(MI_ERR_INVALID, "the last mi_elt_process_device call stored no frame records");
    hipStream_t q = static_cast<hipStream_t>(hip_stream);
    if (!mi::land_counts(s->gpu, q, s->h_count, s->last_count, count))
        return fail(MI_ERR_HIP, "ELT stage: reading the counts failed");
    const size_t k = count[1], nf = static_cast<size_t>(s->rows) * MI_ELT_FRAMES * static_cast<size_t>(s->last_nbatches);
    bool ok = true;
    if (events && k)
        ok = ok && hipMemcpyAsync(events, s->last_events, k * sizeof(mi_elt_event), hipMemcpyDeviceToHost, q) == hipSuccess;
    if (frames)
        ok = ok && hipMemcpyAsync(frames, s->last_frames, nf * sizeof(mi_elt_frame_record), hipMemcpyDeviceToHost, q) == hipSuccess;
    if (row_first_event)
        ok = ok && hipMemcpyAsync(row_first_event, s->last_row_first, (static_cast<size_t>(s->rows) + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, q) ==
                       hipSuccess;
    if (!ok || hipStreamSynchronize(q) != hipSuccess)
        return fail(MI_ERR_HIP, "ELT stage: download failed");
    return MI_OK;
}

int mi_elt_set_timing(mi_elt* s, int on) {
    return mi::set_timing(s, on);
}

int mi_elt_last_launch_ms(mi_elt* s, float* ms) {
    return mi::last_launch_ms(s, ms, "mi_elt_process_device");
}

size_t mi_elt_state_size(const mi_elt* s) {
    return mi::state_size(s, &mi_elt::d_state);
}

int mi_elt_get_state(mi_elt* s, void* buf, size_t len) {
    return mi::get_state(kName, s, &mi_elt::d_state, buf, len);
}

int mi_elt_set_state(mi_elt* s, const void* buf, size_t len) {
    return mi::set_state(kName, s, &mi_elt::d_state, buf, len, [s](const mi::EltRowState* rows, size_t n) { return mi::elt_state_ok(rows, n, s->plan); });
}

}  // extern "C"
