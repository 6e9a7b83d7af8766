// pocsag.hip -- the pager decoder stage: which pages a row's POCSAG transmissions carried.  Per (row, batch), a bank of bit sums under
// H timing hypotheses a twelfth-grid step apart and two slicers -- B bits and one quality sum per lane --; then, per row, a sequential
// walker over the slots: the sync compare on every lane while the row is idle, and the chosen lane's codewords, their BCH repair,
// the messages and the timing moves inside a transmission.  The reference leaves the transmissions in the recording.  The grid, the
// order of every sum, the sync's choice, the word's rule, the walker and the state blob are in include/mi_airband.h.  A post-stage in
// the ACARS stage's mould: five launches on the caller's stream, no atomics.  mi_pocsag_plan_host (poststage_host.cpp) is the host
// twin; the bit's sum, the sync compare and choice, the word's rule and the timing move are one text for both (pocsag_sum,
// pocsag_hit, pocsag_pick, pocsag_take / pocsag_word, pocsag_retime: poststage.hpp).  The handle's base and the bodies of the entry
// points every stage repeats are in poststage.hpp, the lead's load and the tails kernel in carry.hpp.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "../../include/mi_airband.h"
#include "carry.hpp"
#include "poststage.hpp"

constexpr char kName[] = "pager stage";

struct mi_pocsag : mi::RowStage {
    mi_pocsag() : RowStage(kName, 5) {}
    mi::PocsagPlan plan{};
    uint32_t max_messages = 0;
    mi::DevBuf<mi::PocsagRowState> d_state;     // [rows]: the checkpoint blob as it is
    mi::DevBuf<uint32_t> d_table;               // [1024]: the error pattern of every syndrome
    mi::DevBuf<uint32_t> d_bits;                // [rows][max_batches][2][H][W]: the bits of a call without d_bits
    mi::DevBuf<float> d_q;                      // [rows][max_batches][2][H]
    mi::DevBuf<mi_pocsag_message> d_scratch;    // [rows][most messages of a row in the call]: the walk's messages before they are placed
    mi::DevBuf<uint32_t> d_row_message_count;   // [rows]
    mi::PinnedBuf<uint32_t> h_count;            // [2], landing place of the counts in mi_pocsag_download
    // destinations of the last mi_pocsag_process_device (what mi_pocsag_download reads)
    const mi_pocsag_message* last_messages = nullptr;
    const uint32_t* last_row_first = nullptr;
    const uint32_t* last_count = nullptr;
};

namespace {

using mi::aligned;
using mi::as_flags;
using mi::fail;
constexpr int kBatch = mi::kWaveBatch;           // 2000 floats = 500 float4
constexpr int kLead = MI_POCSAG_HISTORY + 2;     // 36 floats staged in front of the block: two that are not used, then the 34 of the history
constexpr int kStage = kLead + kBatch;           // 2036
constexpr int kMaxLanes = MI_POCSAG_MAX_LANES;   // 30
constexpr int kMaxBlockWords = 200;              // 2 H W: 60, 100, 200
constexpr int kParts = sizeof(mi_pocsag_message) / 8;  // 46 uint2: six of fields, 40 of words
static_assert(kStage % 4 == 0 && kParts <= 64 && offsetof(mi::PocsagRowState, msg) % 8 == 0 && sizeof(mi::PocsagRowState) % 8 == 0,
              "whole float4 are staged; a wave moves a message 8 bytes a lane");

// Launch 1, the hot path.  One workgroup of four waves per (row, batch) block of an enabled row.  The block's 2000 samples behind the
// 36 in front of them -- out of the row's previous batch, or the carried samples at batch 0 -- go into LDS, 8144 bytes.  Wave 0 sums
// the block for mu in the header's order.  Wave w takes the hypotheses w, w + 4, ..; for each, passes of 64 slots, lane l on slot
// 64 p + l: the sum of the bit's 6 .. 32 samples out of LDS (pocsag_sum) serves both slicers; the two ballots are written as words by
// lane 0, and |v| is added to the lane's two running sums, which are the header's s_l; an xor butterfly stands for the halving tree
// (float addition commutes, so every lane holds the tree's element 0).  Where every sample of the block and the 34 in front of it
// is +-0 the sums are skipped: they would give bits 0 and Q = +0.0f everywhere.
__global__ __launch_bounds__(256) void k_pocsag_bits(const uint8_t* __restrict__ enabled, const mi::PocsagRowState* __restrict__ state,
                                                     const float* __restrict__ plane, const size_t row_stride, const uint32_t nbatches,
                                                     const mi::PocsagGeom g, uint32_t* __restrict__ bits, float* __restrict__ qout) {
    __shared__ __align__(16) float s[kStage];
    __shared__ float mu_s;
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
    const int block_words = 2 * g.H * g.W, lanes = 2 * g.H;
    uint32_t* const words = bits + static_cast<size_t>(blockIdx.x) * block_words;
    float* const Q = qout + static_cast<size_t>(blockIdx.x) * lanes;
    if (!__syncthreads_or(sound)) {  // (the whole workgroup) digital silence
        if (tid < block_words)
            words[tid] = 0u;
        if (tid < lanes)
            Q[tid] = 0.0f;
        return;
    }
    if (wave == 0) {
        float acc = s[kLead + lane];
        for (int n = lane + 64; n < kBatch; n += 64)
            acc = acc + s[kLead + n];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1)
            acc = acc + __shfl_xor(acc, d);
        if (lane == 0)
            mu_s = acc / 2000.0f;
    }
    __syncthreads();
    const float mu = mu_s;
    const int passes = (g.B + 63) / 64;
    for (int tau = wave; tau < g.H; tau += 4) {
        float acc0 = 0.0f, acc1 = 0.0f;
        for (int p = 0; p < passes; ++p) {
            const int j = 64 * p + lane;
            bool c0 = false, c1 = false;
            if (j < g.B) {
                int k;
                const float sum = mi::pocsag_sum(s, g, tau, j, &k);
                const float v1 = sum - static_cast<float>(k) * mu;
                c0 = sum < 0.0f;
                c1 = v1 < 0.0f;
                acc0 = p ? acc0 + fabsf(sum) : fabsf(sum);
                acc1 = p ? acc1 + fabsf(v1) : fabsf(v1);
            }
            const unsigned long long vote0 = __ballot(c0), vote1 = __ballot(c1);
            if (lane == 0) {
                uint32_t* const w0 = words + tau * g.W + 2 * p;
                uint32_t* const w1 = words + (g.H + tau) * g.W + 2 * p;
                w0[0] = static_cast<uint32_t>(vote0);
                w1[0] = static_cast<uint32_t>(vote1);
                if (2 * p + 1 < g.W) {
                    w0[1] = static_cast<uint32_t>(vote0 >> 32);
                    w1[1] = static_cast<uint32_t>(vote1 >> 32);
                }
            }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            acc0 = acc0 + __shfl_xor(acc0, d);
            acc1 = acc1 + __shfl_xor(acc1, d);
        }
        if (lane == 0) {
            Q[tau] = acc0;
            Q[g.H + tau] = acc1;
        }
    }
}

struct WalkArgs {
    mi::PocsagGeom g;
    uint32_t sync_errors, preamble_errors, correct, hold_timing;
};

__device__ __forceinline__ uint32_t uniform(const uint32_t v) {
    return static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(v)));
}

// Launch 2.  One wave, one workgroup, per row; lane l < 2 H holds bank lane l's last 64 bits.  The wave steps through the call's
// B * nbatches slots in order, a batch's words and Q in LDS beside the syndrome table and the open message.  Idle: every lane shifts
// its bit in and compares (pocsag_hit: three popcounts); a ballot says whether any lane hit, and only then the choice among them is
// made, in wave-uniform code over the lanes' counts in LDS (pocsag_pick).  Inside a transmission the chosen lane's bit is broadcast
// and the walker (pocsag_take) runs on wave-uniform values; a whole word is decoded where it ends, serially -- one syndrome, one table
// read --, and a closed message goes to the row's next slot of the scratch, 46 lanes storing 8 bytes each.  The walker's part of
// the state goes back at the end (the carried samples are the tails kernel's).
__global__ __launch_bounds__(64) void k_pocsag_walk(const uint8_t* __restrict__ enabled, mi::PocsagRowState* __restrict__ state,
                                                    const uint32_t* __restrict__ table_g, const uint32_t* __restrict__ bits, const float* __restrict__ qin,
                                                    const uint32_t nbatches, const uint32_t slots, const WalkArgs a, mi_pocsag_message* __restrict__ scratch,
                                                    uint32_t* __restrict__ row_message_count) {
    __shared__ __align__(8) mi_pocsag_message msg;
    __shared__ uint32_t table[1024];
    __shared__ uint32_t words[kMaxBlockWords];
    __shared__ float Q[kMaxLanes];
    __shared__ uint32_t mism[kMaxLanes];
    const int lane = threadIdx.x;
    const uint32_t row = blockIdx.x;
    if (!enabled[row]) {  // (the whole wave) the row sits out: no message, every byte of its state stays
        if (lane == 0)
            row_message_count[row] = 0;
        return;
    }
    const mi::PocsagGeom g = a.g;
    const int lanes = 2 * g.H, block_words = lanes * g.W;
    mi::PocsagRowState* const st = state + row;
    if (lane < kParts)
        reinterpret_cast<uint2*>(&msg)[lane] = reinterpret_cast<const uint2*>(&st->msg)[lane];
    for (int i = lane; i < 1024; i += 64)
        table[i] = table_g[i];
    uint64_t hist = lane < lanes ? st->hist[lane] : 0;
    const uint32_t batch0 = uniform(st->batch);
    mi::PocsagWalker w{uniform(st->phase), uniform(st->lane),      uniform(st->inverted),   uniform(st->pos),    uniform(st->cur),      uniform(st->nbits),
                       uniform(st->gbad),  uniform(st->lane_sync), uniform(st->mismatches), uniform(st->wbatch), uniform(st->wtwelfth), uniform(st->open)};
    uint32_t n = 0, b = 0;
    // the open message closes in batch b: its record, with the three fields the walker adds
    auto emit = [&]() {
        __syncthreads();  // the message's last word is in LDS
        if (n < slots && lane < kParts) {  // (n < slots always: slots is the most a row can close)
            uint2 v = reinterpret_cast<const uint2*>(&msg)[lane];
            if (lane == 0)
                v.x = row;
            else if (lane == 1)
                v.y = b;
            else if (lane == 3)
                v.y |= w.lane << 8;
            reinterpret_cast<uint2*>(scratch + static_cast<size_t>(row) * slots + n)[lane] = v;
        }
        ++n;
        __syncthreads();  // ... and is read before it is cleared
    };
    const auto take = [&](const uint32_t bit, const int t) {
        mi::pocsag_take(w, &msg, table, a.sync_errors, a.correct, bit, batch0 + b, t, emit);
        w.phase = uniform(w.phase), w.lane = uniform(w.lane), w.pos = uniform(w.pos), w.open = uniform(w.open);
    };
    for (b = 0; b < nbatches; ++b) {
        const size_t blk = static_cast<size_t>(row) * nbatches + b;
        __syncthreads();  // the batch before is done with words and Q
        for (int i = lane; i < block_words; i += 64)
            words[i] = bits[blk * block_words + i];
        if (lane < lanes)
            Q[lane] = qin[blk * lanes + lane];
        __syncthreads();
        bool skip = false;
        if (w.phase == MI_POCSAG_TRANSMISSION && !a.hold_timing) {
            const uint32_t move = uniform(static_cast<uint32_t>(mi::pocsag_retime(w, Q, g.H)));
            w.lane = uniform(w.lane);
            skip = move == mi::kPocsagSkip;
            if (move == mi::kPocsagReplay)  // hypothesis 0's last bit of the batch before
                take(uniform(static_cast<uint32_t>(__shfl(static_cast<int>(hist & 1u), static_cast<int>(w.lane)))) ^ w.inverted, -g.L);
        }
        for (int wi = 0; wi < g.W; ++wi) {
            const uint32_t word = lane < lanes ? words[lane * g.W + wi] : 0u;
            const int nbit = g.B - 32 * wi < 32 ? g.B - 32 * wi : 32;
            for (int t = 0; t < nbit; ++t) {
                const uint32_t c = word >> t & 1u;
                hist = hist << 1 | c;
                if (w.phase == MI_POCSAG_TRANSMISSION) {  // (wave-uniform)
                    if (skip)
                        skip = false;
                    else
                        take(uniform(static_cast<uint32_t>(__shfl(static_cast<int>(c), static_cast<int>(w.lane)))) ^ w.inverted,
                             mi::pocsag_slot_begin(g, static_cast<int>(w.lane) % g.H, 32 * wi + t));
                    continue;
                }
                uint32_t inv;
                const uint32_t m = mi::pocsag_hit(hist, a.sync_errors, a.preamble_errors, &inv);
                if (__ballot(lane < lanes && m != mi::kPocsagNoHit) == 0)
                    continue;
                if (lane < lanes)
                    mism[lane] = m;
                __syncthreads();
                const int u = static_cast<int>(uniform(static_cast<uint32_t>(mi::pocsag_pick(mism, Q, lanes))));
                mi::pocsag_open(w, u, uniform(static_cast<uint32_t>(__shfl(static_cast<int>(inv), u))), uniform(mism[u]));
                __syncthreads();  // mism is read before the next hit rewrites it
            }
        }
    }
    __syncthreads();
    if (lane < lanes)
        st->hist[lane] = hist;
    if (lane < kParts)
        reinterpret_cast<uint2*>(&st->msg)[lane] = reinterpret_cast<const uint2*>(&msg)[lane];
    if (lane == 0) {
        st->batch = batch0 + nbatches;
        st->phase = w.phase, st->lane = w.lane, st->inverted = w.inverted, st->pos = w.pos, st->cur = w.cur, st->nbits = w.nbits, st->gbad = w.gbad;
        st->lane_sync = w.lane_sync, st->mismatches = w.mismatches, st->wbatch = w.wbatch, st->wtwelfth = w.wtwelfth, st->open = w.open;
        row_message_count[row] = n;
    }
}

// Launch 3.  mi::launch_row_scan (poststage.hip): exclusive scan of the rows' message counts, and the two counts.

// Launch 4.  One thread per (row, slot, 8 bytes of the record): a message the row closed goes to its place, unless that is at or
// beyond the capacity.
__global__ __launch_bounds__(256) void k_pocsag_store(const mi_pocsag_message* __restrict__ scratch, const uint32_t* __restrict__ row_message_count,
                                                      const uint32_t* __restrict__ row_first, const uint32_t rows, const uint32_t slots,
                                                      const uint32_t max_messages, mi_pocsag_message* __restrict__ messages) {
    // (64 bits: rows * slots * 46 passes 2^32 from about 9.9e6 blocks of 2400 baud on, and create takes up to 2^24)
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
    const uint64_t rec = i / kParts, row = rec / slots;
    const uint32_t part = static_cast<uint32_t>(i - rec * kParts), j = static_cast<uint32_t>(rec - row * slots);
    if (row >= rows || j >= row_message_count[row])
        return;
    const uint32_t k = row_first[row] + j;
    if (k >= max_messages)
        return;
    reinterpret_cast<uint2*>(messages + k)[part] = reinterpret_cast<const uint2*>(scratch + rec)[part];  // 8-byte aligned, as the records are
}

// Launch 5.  mi::k_carry_tails (carry.hpp): the last 34 input samples of the call are an enabled row's new carried samples.

}  // namespace

extern "C" {

int mi_pocsag_create(const mi_pocsag_cfg* cfg, const uint8_t* row_enabled, int rows, int max_batches, size_t max_messages, int gpu, mi_pocsag** out) {
    if (!row_enabled || !out)
        return fail(MI_ERR_INVALID, "NULL argument");
    mi::PocsagPlan plan;
    if (const int rc = mi::pocsag_plan(cfg, &plan))
        return rc;
    if (const int rc = mi::batch_geometry_ok(kName, rows, max_batches))
        return rc;
    if (const int rc = mi::check_gpu(gpu, "no HIP device: the pager stage runs on the GPU only"))
        return rc;
    mi_pocsag* s = new mi_pocsag();
    s->gpu = gpu;
    s->rows = rows;
    s->max_batches = max_batches;
    s->plan = plan;
    const size_t n = static_cast<size_t>(rows), blocks = n * static_cast<size_t>(max_batches), lanes = 2 * static_cast<size_t>(plan.g.H);
    const size_t most = n * mi::pocsag_max_messages(plan.g, static_cast<uint64_t>(max_batches));
    s->max_messages = static_cast<uint32_t>(max_messages && max_messages < most ? max_messages : most);  // (no call has more messages than `most`)
    std::vector<uint32_t> table(1024);
    mi::pocsag_table(table.data());
    if (hipSetDevice(gpu) != hipSuccess || dalloc_copy(s->d_enabled, as_flags(row_enabled, n)) != hipSuccess || dalloc_zero(s->d_state, n) != hipSuccess ||
        dalloc_copy(s->d_table, table) != hipSuccess || dalloc(s->d_bits, blocks * lanes * plan.g.W) != hipSuccess || dalloc(s->d_q, blocks * lanes) != hipSuccess ||
        dalloc(s->d_scratch, most) != hipSuccess || dalloc(s->d_row_message_count, n) != hipSuccess ||
        hipHostMalloc(reinterpret_cast<void**>(s->h_count.put()), 2 * sizeof(uint32_t)) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
        delete s;
        return fail(MI_ERR_HIP, "pager stage: device allocation failed");
    }
    *out = s;
    return MI_OK;
}

void mi_pocsag_destroy(mi_pocsag* s) {
    mi::destroy(s);
}

int mi_pocsag_set_rows(mi_pocsag* s, const uint8_t* row_enabled) {
    return mi::set_enabled(kName, s, row_enabled);
}

int mi_pocsag_process_device(mi_pocsag* s, const float* d_plane, size_t row_stride, int nbatches, uint32_t* d_bits, float* d_q, mi_pocsag_message* d_messages,
                             uint32_t* d_row_first_message, uint32_t* d_count, void* hip_stream) {
    if (!s || !d_plane || !d_messages || !d_row_first_message || !d_count)
        return fail(MI_ERR_INVALID, "NULL argument");
    if (nbatches < 1 || nbatches > s->max_batches)
        return fail(MI_ERR_INVALID, "nbatches outside 1 .. max_batches");
    if (row_stride < static_cast<size_t>(nbatches) * mi::kWaveBatch)
        return fail(MI_ERR_INVALID, "a row stride is shorter than the call");
    if (row_stride % 4 != 0 || !aligned(d_plane, 16) || !aligned(d_bits, 4) || !aligned(d_q, 4) || !aligned(d_messages, 8) || !aligned(d_row_first_message, 4) ||
        !aligned(d_count, 4))
        return fail(MI_ERR_INVALID, "the plane must be 16-byte aligned with a row stride that is a multiple of 4 floats; message records 8-byte aligned");
    if (hipSetDevice(s->gpu) != hipSuccess)
        return fail(MI_ERR_HIP, "hipSetDevice failed");
    hipStream_t q = static_cast<hipStream_t>(hip_stream);
    const unsigned rows = static_cast<unsigned>(s->rows), nb = static_cast<unsigned>(nbatches);
    // the messages a row can close in this call: at most what create allocated, as nbatches <= max_batches
    const uint32_t slots = mi::pocsag_max_messages(s->plan.g, nb);
    uint32_t* const bits = d_bits ? d_bits : s->d_bits.get();
    float* const qs = d_q ? d_q : s->d_q.get();
    const WalkArgs a{s->plan.g, s->plan.sync_errors, s->plan.preamble_errors, s->plan.correct, s->plan.hold_timing};
    s->timing.stamp(0, q);
    hipLaunchKernelGGL(k_pocsag_bits, dim3(rows * nb), dim3(256), 0, q, s->d_enabled.get(), s->d_state.get(), d_plane, row_stride, nb, s->plan.g, bits, qs);
    s->timing.stamp(1, q);
    hipLaunchKernelGGL(k_pocsag_walk, dim3(rows), dim3(64), 0, q, s->d_enabled.get(), s->d_state.get(), s->d_table.get(), bits, qs, nb, slots, a,
                       s->d_scratch.get(), s->d_row_message_count.get());
    s->timing.stamp(2, q);
    mi::launch_row_scan(q, s->d_row_message_count, s->rows, s->max_messages, d_row_first_message, d_count);
    s->timing.stamp(3, q);
    // (at most 2^24 * 10 * 46 / 256 workgroups: inside the grid's 2^31)
    hipLaunchKernelGGL(k_pocsag_store, dim3(static_cast<unsigned>((static_cast<uint64_t>(rows) * slots * kParts + 255) / 256)), dim3(256), 0, q, s->d_scratch.get(), s->d_row_message_count.get(),
                       d_row_first_message, rows, slots, s->max_messages, d_messages);
    s->timing.stamp(4, q);
    mi::launch_carry_tails<MI_POCSAG_HISTORY>(q, s->d_enabled.get(), d_plane, row_stride, rows, nbatches, s->d_state.get());
    s->timing.stamp(5, q);
    if (hipGetLastError() != hipSuccess)
        return fail(MI_ERR_HIP, "pager stage kernel launch failed");
    s->called = true;
    s->last_messages = d_messages;
    s->last_row_first = d_row_first_message;
    s->last_count = d_count;
    return MI_OK;
}

int mi_pocsag_download(mi_pocsag* s, void* hip_stream, mi_pocsag_message* messages, uint32_t* row_first_message, uint32_t* count) {
    if (!s || !count)
        return fail(MI_ERR_INVALID, "NULL argument");
    if (!s->last_count)
        return fail(MI_ERR_INVALID, "no mi_pocsag_process_device call to download");
    hipStream_t q = static_cast<hipStream_t>(hip_stream);
    if (!mi::land_counts(s->gpu, q, s->h_count, s->last_count, count))
        return fail(MI_ERR_HIP, "pager stage: reading the counts failed");
    const size_t k = count[1];
    bool ok = true;
    if (messages && k)
        ok = ok && hipMemcpyAsync(messages, s->last_messages, k * sizeof(mi_pocsag_message), hipMemcpyDeviceToHost, q) == hipSuccess;
    if (row_first_message)
        ok = ok && hipMemcpyAsync(row_first_message, s->last_row_first, (static_cast<size_t>(s->rows) + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, q) ==
                       hipSuccess;
    if (!ok || hipStreamSynchronize(q) != hipSuccess)
        return fail(MI_ERR_HIP, "pager stage: download failed");
    return MI_OK;
}

int mi_pocsag_set_timing(mi_pocsag* s, int on) {
    return mi::set_timing(s, on);
}

int mi_pocsag_last_launch_ms(mi_pocsag* s, float* ms) {
    return mi::last_launch_ms(s, ms, "mi_pocsag_process_device");
}

size_t mi_pocsag_state_size(const mi_pocsag* s) {
    return mi::state_size(s, &mi_pocsag::d_state);
}

int mi_pocsag_get_state(mi_pocsag* s, void* buf, size_t len) {
    return mi::get_state(kName, s, &mi_pocsag::d_state, buf, len);
}

int mi_pocsag_set_state(mi_pocsag* s, const void* buf, size_t len) {
    if (!s)
        return fail(MI_ERR_INVALID, "pager stage state: NULL argument or wrong length");
    const mi::PocsagPlan plan = s->plan;
    return mi::set_state(kName, s, &mi_pocsag::d_state, buf, len,
                         [plan](const mi::PocsagRowState* rows, size_t n) { return mi::pocsag_state_ok(rows, n, plan); });
}

}  // extern "C"
