// acars.hip -- the ACARS decoder stage: which blocks a row's MSK bursts carried.  Per (row, batch), a bank of coherent bit detectors
// under 20 timing hypotheses a third of a sample apart -- 300 change bits and one quality sum each --; then, per row, a sequential
// walker over the slots: the sync compare on every hypothesis while the row is idle, and the frame's bytes, checksum and timing moves
// on the chosen one.  The reference leaves the bursts in the recording.  The grid, the order of every sum, the sync's choice, the
// walker and the state blob are in include/mi_airband.h.  A post-stage in the SELCAL stage's mould: five launches on the caller's
// stream, no atomics.  mi_acars_plan_host (poststage_host.cpp) is the host twin; the bit, the walker's step, the sync's choice and the
// timing move are one text for both (acars_bit, acars_step, acars_pick, acars_retime: poststage.hpp).  The handle's base and the
// bodies of the entry points every stage repeats are in poststage.hpp, the lead's load and the tails kernel in carry.hpp.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "../../include/mi_airband.h"
#include "carry.hpp"
#include "poststage.hpp"

constexpr char kName[] = "ACARS stage";

struct mi_acars : mi::RowStage {
    mi_acars() : RowStage(kName, 5) {}
    mi::AcarsPlan plan{};
    uint32_t max_frames = 0;
    mi::DevBuf<mi::AcarsRowState> d_state;    // [rows]: the checkpoint blob as it is
    mi::DevBuf<float> d_templates;            // [40]: h1, h2
    mi::DevBuf<uint32_t> d_bits;              // [rows][max_batches][20][10]: the change bits of a call without d_bits
    mi::DevBuf<float> d_q;                    // [rows][max_batches][20]
    mi::DevBuf<mi_acars_frame> d_scratch;     // [rows][most frames of a row in the call]: the walk's frames before they are placed
    mi::DevBuf<uint32_t> d_row_frame_count;   // [rows]
    mi::PinnedBuf<uint32_t> h_count;          // [2], landing place of the counts in mi_acars_download
    // destinations of the last mi_acars_process_device (what mi_acars_download reads)
    const mi_acars_frame* last_frames = nullptr;
    const uint32_t* last_row_first = nullptr;
    const uint32_t* last_count = nullptr;
};

namespace {

using mi::aligned;
using mi::as_flags;
using mi::fail;
constexpr int kBatch = mi::kWaveBatch;          // 2000 floats = 500 float4
constexpr int kLead = MI_ACARS_HISTORY + 2;     // 8 floats staged in front of the block: two that are not used, then the 6 of the history
constexpr int kStage = kLead + kBatch;          // 2008
constexpr int kTau = MI_ACARS_HYPOTHESES;       // 20
constexpr int kBits = MI_ACARS_BITS;            // 300
constexpr int kWords = MI_ACARS_BIT_WORDS;      // 10
constexpr int kBlockWords = kTau * kWords;      // 200
constexpr int kFrameParts = sizeof(mi_acars_frame) / 8;  // 34 uint2: three of fields, 31 of bytes
static_assert(kStage % 4 == 0 && kBits == 4 * 64 + 44 && kTau % 4 == 0 && kFrameParts == 3 + MI_ACARS_RAW_BYTES / 8,
              "whole float4 are staged; a hypothesis is five passes of a wave, the last of 44 lanes; a wave of the block takes five hypotheses");

// Launch 1, the hot path.  One workgroup of four waves per (row, batch) block of an enabled row.  The block's 2000 samples behind the
// 8 in front of them -- out of the row's previous batch, or the carried samples at batch 0 -- go into LDS, 8032 bytes, beside the two
// templates.  Wave w takes the hypotheses w, w + 4, .. w + 16; for each, five passes of 64 slots (the last of 44), lane l on slot
// 64 p + l: six or seven multiply-add pairs out of LDS (acars_bit), the ballot of the change bits written as two words by lane 0, and
// q added to the lane's running sum, which is the header's s_l; an xor butterfly stands for the halving one (float addition commutes,
// so every lane holds the halving tree's element 0).  Neighbouring lanes begin 6 or 7 floats apart, so a 32-lane half reads a span
// of about 213 floats through 32 banks: DESIGN.md 5o counts the conflicts.  Where every sample of the block and the six in front of
// it is +-0 the sums are skipped: they would give c = 1 and Q = +0.0f everywhere.
__global__ __launch_bounds__(256) void k_acars_bits(const uint8_t* __restrict__ enabled, const mi::AcarsRowState* __restrict__ state,
                                                    const float* __restrict__ plane, const size_t row_stride, const uint32_t nbatches,
                                                    const float* __restrict__ templates, uint32_t* __restrict__ bits, float* __restrict__ qout) {
    __shared__ __align__(16) float s[kStage];
    __shared__ float h[2 * kTau];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t row = blockIdx.x / nbatches, batch = blockIdx.x - row * nbatches;  // (the grid is rows * nbatches)
    if (!enabled[row])  // (the whole workgroup) the row sits out: nothing is written
        return;
    const float* const blk = plane + static_cast<size_t>(row) * row_stride + static_cast<size_t>(batch) * kBatch;
    int sound = 0;
    for (int q = tid; q < kStage / 4; q += 256) {
        const float4 v = mi::load_lead4<kLead>(blk, state[row], q, batch == 0);
        reinterpret_cast<float4*>(s)[q] = v;
        sound |= (q && (v.x != 0.0f || v.y != 0.0f)) || v.z != 0.0f || v.w != 0.0f;  // (the lead's first two floats are no bit's)
    }
    if (tid < 2 * kTau)
        h[tid] = templates[tid];
    uint32_t* const words = bits + static_cast<size_t>(blockIdx.x) * kBlockWords;
    float* const Q = qout + static_cast<size_t>(blockIdx.x) * kTau;
    if (!__syncthreads_or(sound)) {  // (the whole workgroup) digital silence
        if (tid < kBlockWords)
            words[tid] = tid % kWords == kWords - 1 ? (1u << (kBits - 32 * (kWords - 1))) - 1u : 0xFFFFFFFFu;
        if (tid < kTau)
            Q[tid] = 0.0f;
        return;
    }
    for (int tau = wave; tau < kTau; tau += 4) {
        float acc = 0.0f;
#pragma unroll
        for (int p = 0; p < 5; ++p) {
            const int j = 64 * p + lane;
            uint32_t c = 0;
            if (j < kBits) {
                float q;
                c = mi::acars_bit(s, h, h + kTau, tau, j, &q);
                acc = p ? acc + q : q;
            }
            const unsigned long long vote = __ballot(c);
            if (lane == 0) {
                words[tau * kWords + 2 * p] = static_cast<uint32_t>(vote);
                words[tau * kWords + 2 * p + 1] = static_cast<uint32_t>(vote >> 32);
            }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1)
            acc = acc + __shfl_xor(acc, d);
        if (lane == 0)
            Q[tau] = acc;
    }
}

struct WalkArgs {
    uint32_t sync_errors, keep_bad, hold_timing;
    float min_quality;
};

__device__ __forceinline__ uint32_t uniform(const uint32_t v) {
    return static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(v)));
}

// Launch 2.  One wave, one workgroup, per row; lane tau < 20 holds hypothesis tau's last change bits.  The wave steps through the
// call's 300 * nbatches slots in order, a batch's 200 words and 20 Q in LDS.  Idle: every lane shifts its bit in and counts the
// mismatches against the pattern (a popcount); a ballot says whether any lane hit, and only then the choice among them is made, in
// wave-uniform code over the lanes' counts in LDS (acars_pick).  Inside a frame the chosen lane's bit is broadcast and the walker
// (acars_step) runs on wave-uniform values, the frame's bytes in LDS; a finished frame goes to the row's next slot of the scratch, 34
// lanes storing 8 bytes each.  The walker's part of the state goes back at the end (the carried samples are the tails kernel's).
__global__ __launch_bounds__(64) void k_acars_walk(const uint8_t* __restrict__ enabled, mi::AcarsRowState* __restrict__ state,
                                                   const uint32_t* __restrict__ bits, const float* __restrict__ qin, const uint32_t nbatches,
                                                   const uint32_t slots, const WalkArgs a, mi_acars_frame* __restrict__ scratch,
                                                   uint32_t* __restrict__ row_frame_count) {
    __shared__ __align__(8) uint8_t bytes[MI_ACARS_RAW_BYTES];
    __shared__ uint32_t words[kBlockWords];
    __shared__ float Q[kTau];
    __shared__ uint32_t mism[kTau];
    const int lane = threadIdx.x;
    const uint32_t row = blockIdx.x;
    if (!enabled[row]) {  // (the whole wave) the row sits out: no frame, every byte of its state stays
        if (lane == 0)
            row_frame_count[row] = 0;
        return;
    }
    mi::AcarsRowState* const st = state + row;
    if (lane < MI_ACARS_RAW_BYTES / 8)
        reinterpret_cast<uint2*>(bytes)[lane] = reinterpret_cast<const uint2*>(st->bytes)[lane];
    uint64_t hist = lane < kTau ? st->hist[lane] : 0;
    const uint32_t batch0 = uniform(st->batch);
    mi::AcarsWalker w{uniform(st->phase), uniform(st->u),   uniform(st->prev),          uniform(st->nbits),       uniform(st->cur),
                      uniform(st->nbytes), uniform(st->tail), uniform(st->crc),           uniform(st->parity_errors), uniform(st->start_batch),
                      uniform(st->start_third), uniform(st->tau_sync), uniform(st->mismatches), uniform(st->end)};
    uint32_t n = 0;
    // what a step's answer does in batch b: the record of a finished frame, and the row idle behind it
    const auto event = [&](const int ev, const uint32_t b) {
        if (ev != mi::kAcarsDone)
            return;
        if (w.crc == 0 || a.keep_bad) {
            __syncthreads();  // the frame's last byte is in LDS
            if (n < slots && lane < kFrameParts) {  // (n < slots always: slots is the most a row can end)
                uint2 v;
                if (lane == 0)
                    v = make_uint2(row, w.start_batch);
                else if (lane == 1)
                    v = make_uint2(w.start_third, w.tau_sync | w.u << 8 | w.mismatches << 16 | (w.crc == 0 ? 1u : 0u) << 24);
                else if (lane == 2)
                    v = make_uint2(w.nbytes | w.parity_errors << 16 | w.end << 24, b);
                else
                    v = reinterpret_cast<const uint2*>(bytes)[lane - 3];
                reinterpret_cast<uint2*>(scratch + static_cast<size_t>(row) * slots + n)[lane] = v;
            }
            ++n;
            __syncthreads();  // ... and is read before the row goes idle
        }
        mi::acars_idle(w, bytes);
    };
    for (uint32_t b = 0; b < nbatches; ++b) {
        const size_t blk = static_cast<size_t>(row) * nbatches + b;
        __syncthreads();  // the batch before is done with words and Q
        for (int i = lane; i < kBlockWords; i += 64)
            words[i] = bits[blk * kBlockWords + i];
        if (lane < kTau)
            Q[lane] = qin[blk * kTau + lane];
        __syncthreads();
        bool skip = false;
        if (w.phase == MI_ACARS_FRAME && !a.hold_timing) {
            const uint32_t move = uniform(static_cast<uint32_t>(mi::acars_retime(w, Q)));
            w.u = uniform(w.u);
            skip = move == mi::kAcarsSkip;
            if (move == mi::kAcarsReplay)  // hypothesis 0's last bit of the batch before
                event(mi::acars_step(w, bytes, uniform(static_cast<uint32_t>(__shfl(static_cast<int>(hist & 1u), 0)))), b);
        }
        for (int wi = 0; wi < kWords; ++wi) {
            const uint32_t word = lane < kTau ? words[lane * kWords + wi] : 0u;
            const int nbit = wi < kWords - 1 ? 32 : kBits - 32 * (kWords - 1);
            for (int t = 0; t < nbit; ++t) {
                const uint32_t c = word >> t & 1u;
                const uint64_t h39 = hist << 1 | c;
                hist = h39 & mi::kAcarsMask38;
                if (w.phase == MI_ACARS_FRAME) {  // (wave-uniform)
                    if (skip)
                        skip = false;
                    else
                        event(mi::acars_step(w, bytes, uniform(static_cast<uint32_t>(__shfl(static_cast<int>(c), static_cast<int>(w.u))))), b);
                    continue;
                }
                const uint32_t m = static_cast<uint32_t>(__popcll(h39 ^ mi::kAcarsSync));
                const bool hit = lane < kTau && m <= a.sync_errors && Q[lane < kTau ? lane : 0] >= a.min_quality;
                if (__ballot(hit) == 0)
                    continue;
                if (lane < kTau)
                    mism[lane] = m;
                __syncthreads();
                const int u = static_cast<int>(uniform(static_cast<uint32_t>(mi::acars_pick(mism, Q, a.sync_errors, a.min_quality))));
                mi::acars_open(w, u, uniform(mism[u]), batch0 + b, 32 * wi + t);
                __syncthreads();  // mism is read before the next hit rewrites it
            }
        }
    }
    __syncthreads();
    if (lane < kTau)
        st->hist[lane] = hist;
    if (lane < MI_ACARS_RAW_BYTES / 8)
        reinterpret_cast<uint2*>(st->bytes)[lane] = reinterpret_cast<const uint2*>(bytes)[lane];
    if (lane == 0) {
        st->batch = batch0 + nbatches;
        st->phase = w.phase, st->u = w.u, st->prev = w.prev, st->nbits = w.nbits, st->cur = w.cur, st->nbytes = w.nbytes, st->tail = w.tail;
        st->crc = w.crc, st->parity_errors = w.parity_errors, st->start_batch = w.start_batch, st->start_third = w.start_third;
        st->tau_sync = w.tau_sync, st->mismatches = w.mismatches, st->end = w.end;
        row_frame_count[row] = n;
    }
}

// Launch 3.  mi::launch_row_scan (poststage.hip): exclusive scan of the rows' frame counts, and the two counts.

// Launch 4.  One thread per (row, slot, 8 bytes of the record): a frame the row ended goes to its place, unless that is at or beyond
// the capacity.
__global__ __launch_bounds__(256) void k_acars_store(const mi_acars_frame* __restrict__ scratch, const uint32_t* __restrict__ row_frame_count,
                                                     const uint32_t* __restrict__ row_first, const uint32_t rows, const uint32_t slots,
                                                     const uint32_t max_frames, mi_acars_frame* __restrict__ frames) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    const uint32_t rec = i / kFrameParts, part = i - rec * kFrameParts;
    const uint32_t row = rec / slots, j = rec - row * slots;
    if (row >= rows || j >= row_frame_count[row])
        return;
    const uint32_t k = row_first[row] + j;
    if (k >= max_frames)
        return;
    reinterpret_cast<uint2*>(frames + k)[part] = reinterpret_cast<const uint2*>(scratch + rec)[part];  // 8-byte aligned, as the records are
}

// Launch 5.  mi::k_carry_tails (carry.hpp): the last 6 input samples of the call are an enabled row's new carried samples.

}  // namespace

extern "C" {

int mi_acars_create(const mi_acars_cfg* cfg, const uint8_t* row_enabled, int rows, int max_batches, size_t max_frames, int gpu, mi_acars** out) {
    if (!row_enabled || !out)
        return fail(MI_ERR_INVALID, "NULL argument");
    mi::AcarsPlan plan;
    if (const int rc = mi::acars_plan(cfg, &plan))
        return rc;
    if (const int rc = mi::batch_geometry_ok(kName, rows, max_batches))
        return rc;
    if (const int rc = mi::check_gpu(gpu, "no HIP device: the ACARS stage runs on the GPU only"))
        return rc;
    mi_acars* s = new mi_acars();
    s->gpu = gpu;
    s->rows = rows;
    s->max_batches = max_batches;
    s->plan = plan;
    const size_t n = static_cast<size_t>(rows), blocks = n * static_cast<size_t>(max_batches);
    const size_t most = n * mi::acars_max_frames(static_cast<uint64_t>(max_batches));
    s->max_frames = static_cast<uint32_t>(max_frames && max_frames < most ? max_frames : most);  // (no call has more frames than `most`)
    std::vector<float> h(2 * kTau);
    mi::acars_templates(h.data(), h.data() + kTau);
    if (hipSetDevice(gpu) != hipSuccess || dalloc_copy(s->d_enabled, as_flags(row_enabled, n)) != hipSuccess || dalloc_zero(s->d_state, n) != hipSuccess ||
        dalloc_copy(s->d_templates, h) != hipSuccess || dalloc(s->d_bits, blocks * kBlockWords) != hipSuccess || dalloc(s->d_q, blocks * kTau) != hipSuccess ||
        dalloc(s->d_scratch, most) != hipSuccess || dalloc(s->d_row_frame_count, n) != hipSuccess ||
        hipHostMalloc(reinterpret_cast<void**>(s->h_count.put()), 2 * sizeof(uint32_t)) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
        delete s;
        return fail(MI_ERR_HIP, "ACARS stage: device allocation failed");
    }
    *out = s;
    return MI_OK;
}

void mi_acars_destroy(mi_acars* s) {
    mi::destroy(s);
}

int mi_acars_set_rows(mi_acars* s, const uint8_t* row_enabled) {
    return mi::set_enabled(kName, s, row_enabled);
}

int mi_acars_process_device(mi_acars* s, const float* d_plane, size_t row_stride, int nbatches, uint32_t* d_bits, float* d_q, mi_acars_frame* d_frames,
                            uint32_t* d_row_first_frame, uint32_t* d_count, void* hip_stream) {
    if (!s || !d_plane || !d_frames || !d_row_first_frame || !d_count)
        return fail(MI_ERR_INVALID, "NULL argument");
    if (nbatches < 1 || nbatches > s->max_batches)
        return fail(MI_ERR_INVALID, "nbatches outside 1 .. max_batches");
    if (row_stride < static_cast<size_t>(nbatches) * mi::kWaveBatch)
        return fail(MI_ERR_INVALID, "a row stride is shorter than the call");
    if (row_stride % 4 != 0 || !aligned(d_plane, 16) || !aligned(d_bits, 4) || !aligned(d_q, 4) || !aligned(d_frames, 8) || !aligned(d_row_first_frame, 4) ||
        !aligned(d_count, 4))
        return fail(MI_ERR_INVALID, "the plane must be 16-byte aligned with a row stride that is a multiple of 4 floats; frame records 8-byte aligned");
    if (hipSetDevice(s->gpu) != hipSuccess)
        return fail(MI_ERR_HIP, "hipSetDevice failed");
    hipStream_t q = static_cast<hipStream_t>(hip_stream);
    const unsigned rows = static_cast<unsigned>(s->rows), nb = static_cast<unsigned>(nbatches);
    // the frames a row can end in this call: at most what create allocated, as nbatches <= max_batches
    const uint32_t slots = mi::acars_max_frames(nb);
    uint32_t* const bits = d_bits ? d_bits : s->d_bits.get();
    float* const qs = d_q ? d_q : s->d_q.get();
    const WalkArgs a{s->plan.sync_errors, s->plan.keep_bad, s->plan.hold_timing, s->plan.min_quality};
    s->timing.stamp(0, q);
    hipLaunchKernelGGL(k_acars_bits, dim3(rows * nb), dim3(256), 0, q, s->d_enabled.get(), s->d_state.get(), d_plane, row_stride, nb, s->d_templates.get(),
                       bits, qs);
    s->timing.stamp(1, q);
    hipLaunchKernelGGL(k_acars_walk, dim3(rows), dim3(64), 0, q, s->d_enabled.get(), s->d_state.get(), bits, qs, nb, slots, a, s->d_scratch.get(),
                       s->d_row_frame_count.get());
    s->timing.stamp(2, q);
    mi::launch_row_scan(q, s->d_row_frame_count, s->rows, s->max_frames, d_row_first_frame, d_count);
    s->timing.stamp(3, q);
    hipLaunchKernelGGL(k_acars_store, dim3((rows * slots * kFrameParts + 255) / 256), dim3(256), 0, q, s->d_scratch.get(), s->d_row_frame_count.get(),
                       d_row_first_frame, rows, slots, s->max_frames, d_frames);
    s->timing.stamp(4, q);
    mi::launch_carry_tails<MI_ACARS_HISTORY>(q, s->d_enabled.get(), d_plane, row_stride, rows, nbatches, s->d_state.get());
    s->timing.stamp(5, q);
    if (hipGetLastError() != hipSuccess)
        return fail(MI_ERR_HIP, "ACARS stage kernel launch failed");
    s->called = true;
    s->last_frames = d_frames;
    s->last_row_first = d_row_first_frame;
    s->last_count = d_count;
    return MI_OK;
}

int mi_acars_download(mi_acars* s, void* hip_stream, mi_acars_frame* frames, uint32_t* row_first_frame, uint32_t* count) {
    if (!s || !count)
        return fail(MI_ERR_INVALID, "NULL argument");
    if (!s->last_count)
        return fail(MI_ERR_INVALID, "no mi_acars_process_device call to download");
    hipStream_t q = static_cast<hipStream_t>(hip_stream);
    if (!mi::land_counts(s->gpu, q, s->h_count, s->last_count, count))
        return fail(MI_ERR_HIP, "ACARS stage: reading the counts failed");
    const size_t k = count[1];
    bool ok = true;
    if (frames && k)
        ok = ok && hipMemcpyAsync(frames, s->last_frames, k * sizeof(mi_acars_frame), hipMemcpyDeviceToHost, q) == hipSuccess;
    if (row_first_frame)
        ok = ok && hipMemcpyAsync(row_first_frame, s->last_row_first, (static_cast<size_t>(s->rows) + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, q) ==
                       hipSuccess;
    if (!ok || hipStreamSynchronize(q) != hipSuccess)
        return fail(MI_ERR_HIP, "ACARS stage: download failed");
    return MI_OK;
}

int mi_acars_set_timing(mi_acars* s, int on) {
    return mi::set_timing(s, on);
}

int mi_acars_last_launch_ms(mi_acars* s, float* ms) {
    return mi::last_launch_ms(s, ms, "mi_acars_process_device");
}

size_t mi_acars_state_size(const mi_acars* s) {
    return mi::state_size(s, &mi_acars::d_state);
}

int mi_acars_get_state(mi_acars* s, void* buf, size_t len) {
    return mi::get_state(kName, s, &mi_acars::d_state, buf, len);
}

int mi_acars_set_state(mi_acars* s, const void* buf, size_t len) {
    return mi::set_state(kName, s, &mi_acars::d_state, buf, len, [](const mi::AcarsRowState* rows, size_t n) { return mi::acars_state_ok(rows, n); });
}

}  // extern "C"
