// same.hip -- the SAME decoder stage: which weather-alert headers a row's AFSK bursts carried.  Per (row, batch), a bank of
// non-coherent mark / space detectors under 16 timing hypotheses 48 units (of 1/25 sample) apart -- 65 or 66 bits and one quality
// sum each --; then, per row, a sequential walker over the bit indices: the sync compare on every hypothesis while the row is idle,
// the burst's bytes and timing moves on the chosen one, and the assembler that votes three bursts into a message.  The grid, the
// order of every sum, the bookkeeping at a batch edge, the walker and the state blob are in include/mi_airband.h.  A post-stage in
// the ACARS stage's mould: five launches on the caller's stream, no atomics.  mi_same_plan_host (poststage_host.cpp) is the host
// twin; the bit, the walker's step, the sync's choice, the assembler and the timing move are one text for both (same_bit, same_step,
// same_pick, same_open, same_burst_end, same_close, same_gap, same_retime: poststage.hpp).
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "../../include/mi_airband.h"
#include "carry.hpp"
#include "poststage.hpp"

constexpr char kName[] = "SAME stage";

struct mi_same : mi::RowStage {
    mi_same() : RowStage(kName, 5) {}
    mi::SamePlan plan{};
    uint32_t max_messages = 0;
    mi::DevBuf<mi::SameRowState> d_state;      // [rows]: the checkpoint blob as it is
    mi::DevBuf<float> d_templates;             // [4][768]
    mi::DevBuf<uint32_t> d_bits;               // [rows][max_batches][16][4]: the bits of a call without d_bits
    mi::DevBuf<float> d_q;                     // [rows][max_batches][16]
    mi::DevBuf<mi_same_message> d_scratch;     // [rows][most messages of a row in the call]: the walk's messages before they are placed
    mi::DevBuf<uint32_t> d_row_message_count;  // [rows]
    mi::PinnedBuf<uint32_t> h_count;           // [2], landing place of the counts in mi_same_download
    // destinations of the last mi_same_process_device (what mi_same_download reads)
    const mi_same_message* last_messages = nullptr;
    const uint32_t* last_row_first = nullptr;
    const uint32_t* last_count = nullptr;
};

namespace {

using mi::aligned;
using mi::as_flags;
using mi::fail;
constexpr int kBatch = mi::kWaveBatch;          // 2000 floats = 500 float4
constexpr int kLead = MI_SAME_HISTORY + 2;      // 32 floats staged in front of the block: two that are not used, then the 30 of the history
constexpr int kStage = kLead + kBatch;          // 2032
constexpr int kTau = MI_SAME_HYPOTHESES;        // 16
constexpr int kWords = MI_SAME_BIT_WORDS;       // 4
constexpr int kBlockWords = kTau * kWords;      // 64
constexpr int kUnits = MI_SAME_BIT_UNITS;       // 768
constexpr int kMsgParts = sizeof(mi_same_message) / 8;  // 38 uint2
static_assert(kStage % 4 == 0 && kTau % 4 == 0 && MI_SAME_MAX_BITS == 66 && kMsgParts <= 64 && 3 * MI_SAME_RAW_BYTES / 8 == 102,
              "whole float4 are staged; a hypothesis is one pass of a wave and two bits over; a wave of the block takes four hypotheses");

// Launch 1, the hot path.  One workgroup of four waves per (row, batch) block of an enabled row.  The block's 2000 samples behind the
// 32 in front of them -- out of the row's previous batch, or the carried samples at batch 0 -- go into LDS beside the four templates,
// 8128 + 12288 bytes.  Wave w takes the hypotheses w, w + 4, w + 8, w + 12.  First the bits 64 and 65 of its four hypotheses on lanes
// 0 .. 7, then per hypothesis one pass, lane l on bit l: 30 or 31 samples against four templates out of LDS (same_bit), the ballot of
// the bits written as two words by lane 0, and q -- with q of bit 64 + l behind it on lanes 0 and 1 -- into the xor butterfly that
// stands for the halving tree (float addition commutes).  Neighbouring lanes begin 30 or 31 floats apart: lanes l and l + 25 of a
// 32-lane half read the same bank, a two-way conflict on seven pairs; the templates are read at rho = 0 .. 24 + 25 i, equal or in
// different banks.  Where every sample of the block and the 30 in front of it is +-0 the sums are skipped.
__global__ __launch_bounds__(256) void k_same_bits(const uint8_t* __restrict__ enabled, const mi::SameRowState* __restrict__ state,
                                                   const float* __restrict__ plane, const size_t row_stride, const uint32_t nbatches,
                                                   const float* __restrict__ templates, const float space_gain, uint32_t* __restrict__ bits,
                                                   float* __restrict__ qout) {
    __shared__ __align__(16) float s[kStage];
    __shared__ __align__(16) float T[4 * kUnits];
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
    for (int q = tid; q < kUnits; q += 256)
        reinterpret_cast<float4*>(T)[q] = reinterpret_cast<const float4*>(templates)[q];
    const uint32_t grid = (state[row].grid + 80u * (batch % 48u)) % kUnits;  // (the grid repeats every 48 batches)
    uint32_t* const words = bits + static_cast<size_t>(blockIdx.x) * kBlockWords;
    float* const Q = qout + static_cast<size_t>(blockIdx.x) * kTau;
    if (!__syncthreads_or(sound)) {  // (the whole workgroup) digital silence
        if (tid < kBlockWords) {
            const int cnt = mi::same_count(mi::same_first(grid, tid / kWords)), wi = tid % kWords;
            words[tid] = wi == 3 ? static_cast<uint32_t>(cnt) : wi == 2 ? (1u << (cnt - 64)) - 1u : 0xFFFFFFFFu;
        }
        if (tid < kTau)
            Q[tid] = 0.0f;
        return;
    }
    // bits 64 and 65 of the wave's four hypotheses: lane 2 i + e on bit 64 + e of hypothesis wave + 4 i
    float qx = 0.0f;
    uint32_t cx = 0;
    {
        const int tau = wave + 4 * ((lane >> 1) & 3), j = 64 + (lane & 1);
        const int r0 = mi::same_first(grid, tau);
        if (lane < 8 && j < mi::same_count(r0))
            cx = mi::same_bit(s, T, r0 + kUnits * j, space_gain, &qx);
    }
    const unsigned long long over = __ballot(cx);
    for (int i = 0; i < 4; ++i) {
        const int tau = wave + 4 * i;
        const int r0 = mi::same_first(grid, tau), cnt = mi::same_count(r0);
        float acc;
        const uint32_t c = mi::same_bit(s, T, r0 + kUnits * lane, space_gain, &acc);
        const float more = __shfl(qx, 2 * i + (lane & 1));
        if (lane + 64 < cnt)
            acc = acc + more;
        const unsigned long long vote = __ballot(c);
        if (lane == 0) {
            words[tau * kWords] = static_cast<uint32_t>(vote);
            words[tau * kWords + 1] = static_cast<uint32_t>(vote >> 32);
            words[tau * kWords + 2] = static_cast<uint32_t>(over >> (2 * i)) & 3u;
            words[tau * kWords + 3] = static_cast<uint32_t>(cnt);
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1)
            acc = acc + __shfl_xor(acc, d);
        if (lane == 0)
            Q[tau] = acc;
    }
}

struct WalkArgs {
    uint32_t sync_errors, max_bad, gap_batches, hold_timing;
    float min_quality;
};

__device__ __forceinline__ uint32_t uniform(const uint32_t v) {
    return static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(v)));
}

// Launch 2.  One wave, one workgroup, per row; lane tau < 16 holds hypothesis tau's last 64 bits.  The wave steps through the call's
// bit indices in order, a batch's 64 words and 16 Q in LDS: the gap rule and the timing move at the batch's first index, then cnt(15)
// indices, the hypotheses that are ahead taking their waiting bit at the first.  Idle: every lane counts its mismatches against both
// patterns; a ballot says whether any lane hit, and only then the choice is made in wave-uniform code (same_pick).  Inside a burst the
// chosen lane's bit is broadcast and the walker and the assembler (same_step, same_burst_end) run on wave-uniform values, the row's
// three byte buffers in LDS; a closed message is built in LDS and goes to the row's next slot of the scratch, 38 lanes storing 8 bytes
// each.  The walker's part of the state goes back at the end (the carried samples are the tails kernel's).
__global__ __launch_bounds__(64) void k_same_walk(const uint8_t* __restrict__ enabled, mi::SameRowState* __restrict__ state,
                                                  const uint32_t* __restrict__ bits, const float* __restrict__ qin, const uint32_t nbatches,
                                                  const uint32_t slots, const WalkArgs a, mi_same_message* __restrict__ scratch,
                                                  uint32_t* __restrict__ row_message_count) {
    __shared__ __align__(8) uint8_t bytes[3 * MI_SAME_RAW_BYTES];
    __shared__ __align__(8) mi_same_message msg;
    __shared__ uint32_t words[kBlockWords];
    __shared__ float Q[kTau];
    __shared__ uint32_t mk[kTau];
    const int lane = threadIdx.x;
    const uint32_t row = blockIdx.x;
    if (!enabled[row]) {  // (the whole wave) the row sits out: no message, every byte of its state stays
        if (lane == 0)
            row_message_count[row] = 0;
        return;
    }
    mi::SameRowState* const st = state + row;
    for (int i = lane; i < 3 * MI_SAME_RAW_BYTES / 8; i += 64)
        reinterpret_cast<uint2*>(bytes)[i] = reinterpret_cast<const uint2*>(st->bytes)[i];
    uint64_t hist = lane < kTau ? st->hist[lane] : 0;
    const uint32_t batch0 = uniform(st->batch);
    uint32_t grid = uniform(st->grid);
    mi::SameWalker w;
#pragma unroll
    for (int i = 0; i < mi::kSameWalkerWords; ++i)
        reinterpret_cast<uint32_t*>(&w)[i] = uniform(reinterpret_cast<const uint32_t*>(&st->w)[i]);
    uint32_t n = 0;
    __syncthreads();
    // a closed message goes to the row's next slot
    const auto record = [&](const bool closed) {
        if (!closed)
            return;
        __syncthreads();  // the message is in LDS
        if (n < slots && lane < kMsgParts)  // (n < slots always: slots is the most a row can close)
            reinterpret_cast<uint2*>(scratch + static_cast<size_t>(row) * slots + n)[lane] = reinterpret_cast<const uint2*>(&msg)[lane];
        ++n;
        __syncthreads();  // ... and is read before the next one is built
    };
    const auto step = [&](const uint32_t c, const uint32_t b) {
        uint32_t trunc = 0;
        if (mi::same_step(w, bytes, c, a.max_bad, &trunc))
            record(mi::same_burst_end(w, bytes, trunc, row, b, &msg));
    };
    for (uint32_t b = 0; b < nbatches; ++b) {
        const size_t blk = static_cast<size_t>(row) * nbatches + b;
        __syncthreads();  // the batch before is done with words and Q
        words[lane] = bits[blk * kBlockWords + lane];
        if (lane < kTau)
            Q[lane] = qin[blk * kTau + lane];
        __syncthreads();
        const int ahead = mi::same_ahead(grid);
        const int mine = lane < kTau && lane < ahead;  // this lane's bit of the first index waits in its history
        const int r0 = mi::same_first(grid, lane < kTau ? lane : 0);
        const uint32_t w0 = words[(lane & 15) * kWords], w1 = words[(lane & 15) * kWords + 1], w2 = words[(lane & 15) * kWords + 2];
        const int rounds = static_cast<int>(uniform(words[15 * kWords + 3]));
        record(mi::same_gap(w, bytes, a.gap_batches, row, b, &msg));
        bool skip = false;
        if (w.phase == MI_SAME_BURST && !a.hold_timing) {
            const uint32_t move = uniform(static_cast<uint32_t>(mi::same_retime(w, Q)));
            w.u = uniform(w.u);
            skip = move == mi::kSameSkip;
            if (move == mi::kSameReplay)  // hypothesis 15's newest carried bit
                step(uniform(static_cast<uint32_t>(__shfl(static_cast<int>(hist & 1u), 15))), b);
        }
        for (int i = 0; i < rounds; ++i) {
            const int j = i - mine;
            uint32_t c;
            if (j >= 0) {
                c = (j < 32 ? w0 >> j : j < 64 ? w1 >> (j - 32) : w2 >> (j - 64)) & 1u;
                hist = hist << 1 | c;
            } else {
                c = static_cast<uint32_t>(hist & 1u);
            }
            if (w.phase == MI_SAME_BURST) {  // (wave-uniform)
                if (skip)
                    skip = false;
                else
                    step(uniform(static_cast<uint32_t>(__shfl(static_cast<int>(c), static_cast<int>(w.u)))), b);
                continue;
            }
            if (w.deaf) {
                --w.deaf;
                continue;
            }
            const uint32_t m = mi::same_mismatch(hist);
            const bool hit = lane < kTau && (m & 0xFFu) <= a.sync_errors && Q[lane & 15] >= a.min_quality;
            if (__ballot(hit) == 0)
                continue;
            if (lane < kTau)
                mk[lane] = m;
            __syncthreads();
            const int u = static_cast<int>(uniform(static_cast<uint32_t>(mi::same_pick(mk, Q, a.sync_errors, a.min_quality))));
            const uint32_t kind = uniform(mk[u] >> 8);
            const int r = static_cast<int>(uniform(static_cast<uint32_t>(__shfl(r0 + kUnits * j, u))));
            record(mi::same_open(w, bytes, u, kind, batch0 + b, r, row, b, &msg));
            if (kind == MI_SAME_EOM)
                record(mi::same_burst_end(w, bytes, 0, row, b, &msg));
            __syncthreads();  // mk is read before the next hit rewrites it
        }
        grid = (grid + 80u) % kUnits;
        if (lane < kTau && lane < mi::same_ahead(grid)) {  // the bit that waits for the next batch's first index
            const int j = static_cast<int>(words[lane * kWords + 3]) - 1;
            hist = hist << 1 | ((j < 64 ? w1 >> (j - 32) : w2 >> (j - 64)) & 1u);
        }
    }
    __syncthreads();
    if (lane < kTau)
        st->hist[lane] = hist;
    for (int i = lane; i < 3 * MI_SAME_RAW_BYTES / 8; i += 64)
        reinterpret_cast<uint2*>(st->bytes)[i] = reinterpret_cast<const uint2*>(bytes)[i];
    if (lane == 0) {
        st->batch = batch0 + nbatches;
        st->grid = grid;
        st->w = w;
        row_message_count[row] = n;
    }
}

// Launch 3.  mi::launch_row_scan (poststage.hip): exclusive scan of the rows' message counts, and the two counts.

// Launch 4.  One thread per (row, slot, 8 bytes of the record): a message the row closed goes to its place, unless that is at or
// beyond the capacity.
__global__ __launch_bounds__(256) void k_same_store(const mi_same_message* __restrict__ scratch, const uint32_t* __restrict__ row_message_count,
                                                    const uint32_t* __restrict__ row_first, const uint32_t rows, const uint32_t slots,
                                                    const uint32_t max_messages, mi_same_message* __restrict__ messages) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    const uint32_t rec = i / kMsgParts, part = i - rec * kMsgParts;
    const uint32_t row = rec / slots, j = rec - row * slots;
    if (row >= rows || j >= row_message_count[row])
        return;
    const uint32_t k = row_first[row] + j;
    if (k >= max_messages)
        return;
    reinterpret_cast<uint2*>(messages + k)[part] = reinterpret_cast<const uint2*>(scratch + rec)[part];  // 8-byte aligned, as the records are
}

// Launch 5.  mi::k_carry_tails (carry.hpp): the last 30 input samples of the call are an enabled row's new carried samples.

}  // namespace

extern "C" {

int mi_same_create(const mi_same_cfg* cfg, const uint8_t* row_enabled, int rows, int max_batches, size_t max_messages, int gpu, mi_same** out) {
    if (!row_enabled || !out)
        return fail(MI_ERR_INVALID, "NULL argument");
    mi::SamePlan plan;
    if (const int rc = mi::same_plan(cfg, &plan))
        return rc;
    if (const int rc = mi::batch_geometry_ok(kName, rows, max_batches))
        return rc;
    if (const int rc = mi::check_gpu(gpu, "no HIP device: the SAME stage runs on the GPU only"))
        return rc;
    mi_same* s = new mi_same();
    s->gpu = gpu;
    s->rows = rows;
    s->max_batches = max_batches;
    s->plan = plan;
    const size_t n = static_cast<size_t>(rows), blocks = n * static_cast<size_t>(max_batches);
    const size_t most = n * mi::same_max_messages(static_cast<uint64_t>(max_batches));
    s->max_messages = static_cast<uint32_t>(max_messages && max_messages < most ? max_messages : most);  // (no call has more messages than `most`)
    std::vector<float> T(4 * kUnits);
    mi::same_templates(T.data());
    if (hipSetDevice(gpu) != hipSuccess || dalloc_copy(s->d_enabled, as_flags(row_enabled, n)) != hipSuccess || dalloc_zero(s->d_state, n) != hipSuccess ||
        dalloc_copy(s->d_templates, T) != hipSuccess || dalloc(s->d_bits, blocks * kBlockWords) != hipSuccess || dalloc(s->d_q, blocks * kTau) != hipSuccess ||
        dalloc(s->d_scratch, most) != hipSuccess || dalloc(s->d_row_message_count, n) != hipSuccess ||
        hipHostMalloc(reinterpret_cast<void**>(s->h_count.put()), 2 * sizeof(uint32_t)) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
        delete s;
        return fail(MI_ERR_HIP, "SAME stage: device allocation failed");
    }
    *out = s;
    return MI_OK;
}

void mi_same_destroy(mi_same* s) {
    mi::destroy(s);
}

int mi_same_set_rows(mi_same* s, const uint8_t* row_enabled) {
    return mi::set_enabled(kName, s, row_enabled);
}

int mi_same_process_device(mi_same* s, const float* d_plane, size_t row_stride, int nbatches, uint32_t* d_bits, float* d_q, mi_same_message* d_messages,
                           uint32_t* d_row_first_message, uint32_t* d_count, void* hip_stream) {
    if (!s || !d_plane || !d_messages || !d_row_first_message || !d_count)
        return fail(MI_ERR_INVALID, "NULL argument");
    if (nbatches < 1 || nbatches > s->max_batches)
        return fail(MI_ERR_INVALID, "nbatches outside 1 .. max_batches");
    if (row_stride < static_cast<size_t>(nbatches) * mi::kWaveBatch)
        return fail(MI_ERR_INVALID, "a row stride is shorter than the call");
    if (row_stride % 4 != 0 || !aligned(d_plane, 16) || !aligned(d_bits, 4) || !aligned(d_q, 4) || !aligned(d_messages, 8) ||
        !aligned(d_row_first_message, 4) || !aligned(d_count, 4))
        return fail(MI_ERR_INVALID, "the plane must be 16-byte aligned with a row stride that is a multiple of 4 floats; message records 8-byte aligned");
    if (hipSetDevice(s->gpu) != hipSuccess)
        return fail(MI_ERR_HIP, "hipSetDevice failed");
    hipStream_t q = static_cast<hipStream_t>(hip_stream);
    const unsigned rows = static_cast<unsigned>(s->rows), nb = static_cast<unsigned>(nbatches);
    // the messages a row can close in this call: at most what create allocated, as nbatches <= max_batches
    const uint32_t slots = mi::same_max_messages(nb);
    uint32_t* const bits = d_bits ? d_bits : s->d_bits.get();
    float* const qs = d_q ? d_q : s->d_q.get();
    const WalkArgs a{s->plan.sync_errors, s->plan.max_bad, s->plan.gap_batches, s->plan.hold_timing, s->plan.min_quality};
    s->timing.stamp(0, q);
    hipLaunchKernelGGL(k_same_bits, dim3(rows * nb), dim3(256), 0, q, s->d_enabled.get(), s->d_state.get(), d_plane, row_stride, nb, s->d_templates.get(),
                       s->plan.space_gain, bits, qs);
    s->timing.stamp(1, q);
    hipLaunchKernelGGL(k_same_walk, dim3(rows), dim3(64), 0, q, s->d_enabled.get(), s->d_state.get(), bits, qs, nb, slots, a, s->d_scratch.get(),
                       s->d_row_message_count.get());
    s->timing.stamp(2, q);
    mi::launch_row_scan(q, s->d_row_message_count, s->rows, s->max_messages, d_row_first_message, d_count);
    s->timing.stamp(3, q);
    hipLaunchKernelGGL(k_same_store, dim3((rows * slots * kMsgParts + 255) / 256), dim3(256), 0, q, s->d_scratch.get(), s->d_row_message_count.get(),
                       d_row_first_message, rows, slots, s->max_messages, d_messages);
    s->timing.stamp(4, q);
    mi::launch_carry_tails<MI_SAME_HISTORY>(q, s->d_enabled.get(), d_plane, row_stride, rows, nbatches, s->d_state.get());
    s->timing.stamp(5, q);
    if (hipGetLastError() != hipSuccess)
        return fail(MI_ERR_HIP, "SAME stage kernel launch failed");
    s->called = true;
    s->last_messages = d_messages;
    s->last_row_first = d_row_first_message;
    s->last_count = d_count;
    return MI_OK;
}

int mi_same_download(mi_same* s, void* hip_stream, mi_same_message* messages, uint32_t* row_first_message, uint32_t* count) {
    if (!s || !count)
        return fail(MI_ERR_INVALID, "NULL argument");
    if (!s->last_count)
        return fail(MI_ERR_INVALID, "no mi_same_process_device call to download");
    hipStream_t q = static_cast<hipStream_t>(hip_stream);
    if (!mi::land_counts(s->gpu, q, s->h_count, s->last_count, count))
        return fail(MI_ERR_HIP, "SAME stage: reading the counts failed");
    const size_t k = count[1];
    bool ok = true;
    if (messages && k)
        ok = ok && hipMemcpyAsync(messages, s->last_messages, k * sizeof(mi_same_message), hipMemcpyDeviceToHost, q) == hipSuccess;
    if (row_first_message)
        ok = ok && hipMemcpyAsync(row_first_message, s->last_row_first, (static_cast<size_t>(s->rows) + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, q) ==
                       hipSuccess;
    if (!ok || hipStreamSynchronize(q) != hipSuccess)
        return fail(MI_ERR_HIP, "SAME stage: download failed");
    return MI_OK;
}

int mi_same_set_timing(mi_same* s, int on) {
    return mi::set_timing(s, on);
}

int mi_same_last_launch_ms(mi_same* s, float* ms) {
    return mi::last_launch_ms(s, ms, "mi_same_process_device");
}

size_t mi_same_state_size(const mi_same* s) {
    return mi::state_size(s, &mi_same::d_state);
}

int mi_same_get_state(mi_same* s, void* buf, size_t len) {
    return mi::get_state(kName, s, &mi_same::d_state, buf, len);
}

int mi_same_set_state(mi_same* s, const void* buf, size_t len) {
    if (!s)
        return fail(MI_ERR_INVALID, "SAME stage state: NULL argument or wrong length");
    const mi::SamePlan plan = s->plan;
    return mi::set_state(kName, s, &mi_same::d_state, buf, len, [plan](const mi::SameRowState* rows, size_t n) { return mi::same_state_ok(rows, n, plan); });
}

}  // extern "C"
