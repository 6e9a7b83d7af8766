// ax25.hip -- the packet decoder stage: which AX.25 frames a row's 1200 bit/s Bell 202 bursts carried.  Per (row, batch), a bank of
// tone detectors under 10 timing hypotheses four thirds of a sample apart -- 150 bits each, sliced three ways off one set of sums --;
// then, per row, 30 HDLC deframers side by side over the slots, one per lane of a wave, every lane at work in every slot: there is no
// sync to choose a hypothesis by, the frame check decides, and a rule on the frames' positions keeps one record per frame.  The
// reference leaves the bursts in the recording.  The grid, the order of every sum, the deframer, the ordering rule and the state blob
// are in include/mi_airband.h.  A post-stage in the ACARS stage's mould: five launches on the caller's stream, no atomics.
// mi_ax25_plan_host (poststage_host.cpp) is the host twin; the bit and the deframer's step are one text for both (ax25_bit, ax25_step:
// poststage.hpp).  The handle's base and the bodies of the entry points every stage repeats are in poststage.hpp, the lead's load and
// the tails kernel in carry.hpp.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "../../include/mi_airband.h"
#include "carry.hpp"
#include "poststage.hpp"

constexpr char kName[] = "packet stage";

struct mi_ax25 : mi::RowStage {
    mi_ax25() : RowStage(kName, 5) {}
    mi::Ax25Plan plan{};
    uint32_t max_frames = 0;
    mi::DevBuf<mi::Ax25RowState> d_state;    // [rows]: the checkpoint blob as it is
    mi::DevBuf<float> d_templates;           // [160]
    mi::DevBuf<uint32_t> d_bits;             // [rows][max_batches][30][5]: the tone bits of a call without d_bits
    mi::DevBuf<mi_ax25_frame> d_scratch;     // [rows][most frames of a row in the call]: the walk's frames before they are placed
    mi::DevBuf<uint32_t> d_row_frame_count;  // [rows]
    mi::PinnedBuf<uint32_t> h_count;         // [2], landing place of the counts in mi_ax25_download
    // destinations of the last mi_ax25_process_device (what mi_ax25_download reads)
    const mi_ax25_frame* last_frames = nullptr;
    const uint32_t* last_row_first = nullptr;
    const uint32_t* last_count = nullptr;
};

namespace {

using mi::aligned;
using mi::as_flags;
using mi::fail;
constexpr int kBatch = mi::kWaveBatch;          // 2000 floats = 500 float4
constexpr int kLead = MI_AX25_HISTORY + 2;      // 16 floats staged in front of the block: two that are not used, then the 14 of the history
constexpr int kStage = kLead + kBatch;          // 2016
constexpr int kTau = MI_AX25_HYPOTHESES;        // 10
constexpr int kBits = MI_AX25_BITS;             // 150
constexpr int kWords = MI_AX25_BIT_WORDS;       // 5
constexpr int kLanes = MI_AX25_LANES;           // 30
constexpr int kBlockWords = kLanes * kWords;    // 150
constexpr int kLaneWords = mi::kAx25LaneWords;  // 83
constexpr int kFrameWords = sizeof(mi_ax25_frame) / 4;  // 88: five of fields, 83 of bytes
constexpr uint32_t kLastWord = (1u << (kBits - 32 * (kWords - 1))) - 1u;
static_assert(kStage % 4 == 0 && kBits == 2 * 64 + 22 && kFrameWords == 5 + kLaneWords && kFrameWords <= 128 && kLanes <= 32,
              "whole float4 are staged; a hypothesis is three passes of a wave, the last of 22 lanes; a record is two passes of a wave");

// Launch 1, the hot path.  One workgroup of four waves per (row, batch) block of an enabled row.  The block's 2000 samples behind the
// 16 in front of them -- out of the row's previous batch, or the carried samples at batch 0 -- go into LDS, 8064 bytes, beside the
// four templates.  Wave w takes the hypotheses w, w + 4, w + 8; for each, three passes of 64 slots (the last of 22), lane l on slot
// 64 p + l: thirteen or fourteen samples against four templates out of LDS (ax25_bit), the three comparisons off the one set of
// sums, and a ballot per slicer written as two words by lane 0.  Neighbouring lanes begin 13 or 14 floats apart (40 / 3), so a
// 32-lane group reads addresses of stride 13 1/3 through 32 banks: DESIGN.md 5r counts the conflicts.  Where every sample of the
// block and the fourteen in front of it is +-0 the sums are skipped: they would give t = 1 everywhere.
__global__ __launch_bounds__(256) void k_ax25_bits(const uint8_t* __restrict__ enabled, const mi::Ax25RowState* __restrict__ state,
                                                   const float* __restrict__ plane, const size_t row_stride, const uint32_t nbatches,
                                                   const float* __restrict__ templates, const mi::Ax25Gains gain, uint32_t* __restrict__ bits) {
    __shared__ __align__(16) float s[kStage];
    __shared__ float T[160];
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
    if (tid < 160)
        T[tid] = templates[tid];
    uint32_t* const words = bits + static_cast<size_t>(blockIdx.x) * kBlockWords;
    if (!__syncthreads_or(sound)) {  // (the whole workgroup) digital silence
        if (tid < kBlockWords)
            words[tid] = tid % kWords == kWords - 1 ? kLastWord : 0xFFFFFFFFu;
        return;
    }
    for (int tau = wave; tau < kTau; tau += 4) {
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            const int j = 64 * p + lane;
            const uint32_t m = j < kBits ? mi::ax25_bit(s, T, gain, tau, j) : 0u;
#pragma unroll
            for (int g = 0; g < MI_AX25_SLICERS; ++g) {
                const unsigned long long vote = __ballot(m >> g & 1u);
                if (lane == 0) {
                    uint32_t* const w = words + (10 * g + tau) * kWords + 2 * p;
                    w[0] = static_cast<uint32_t>(vote);
                    if (p < 2)
                        w[1] = static_cast<uint32_t>(vote >> 32);
                }
            }
        }
    }
}

__device__ __forceinline__ uint32_t uniform(const uint32_t v) {
    return static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(v)));
}
__device__ __forceinline__ uint32_t from_lane(const uint32_t v, const int src) {
    return uniform(static_cast<uint32_t>(__shfl(static_cast<int>(v), src)));
}

// Launch 2.  One wave, one workgroup, per row; lane l < 30 is deframer l with its state in registers.  Per batch a lane loads its own
// five packed words (the next batch's while it works on this one) and shifts its bits out of a register, so the slot loop reads no
// memory for bits.  A frame's bytes go to LDS lane-interleaved -- word w of lane l at w * 32 + l, so the byte stores of a slot fall
// into 30 different banks -- and are never cleared: whoever reads a lane's bytes takes nbytes of them.  A slot in which some lane
// closes a candidate is rare; a ballot finds it, and only then the candidates are taken in ascending l in wave-uniform code: the
// ordering rule on values read from the lane, the address field by two ballots over the lane's first 70 bytes, and the record, 88
// words stored by 88 lanes-times-passes to the row's next slot of the scratch.  The deframers' part of the state goes back at the
// end, bytes behind nbytes as zeros (the carried samples are the tails kernel's).
__global__ __launch_bounds__(64) void k_ax25_walk(const uint8_t* __restrict__ enabled, mi::Ax25RowState* __restrict__ state,
                                                  const uint32_t* __restrict__ bits, const uint32_t nbatches, const uint32_t slots,
                                                  const uint32_t strict, mi_ax25_frame* __restrict__ scratch, uint32_t* __restrict__ row_frame_count) {
    __shared__ uint32_t fb[kLaneWords * 32];  // 10 624 bytes
    __shared__ uint32_t nby[32];
    const int lane = threadIdx.x;
    const uint32_t row = blockIdx.x;
    if (!enabled[row]) {  // (the whole wave) the row sits out: no frame, every byte of its state stays
        if (lane == 0)
            row_frame_count[row] = 0;
        return;
    }
    mi::Ax25RowState* const st = state + row;
    const bool work = lane < kLanes;
    const int me = work ? lane : 0;
    {
        const uint32_t* const src = reinterpret_cast<const uint32_t*>(&st->bytes[0][0]);
        for (int i = lane; i < kLanes * kLaneWords; i += 64)
            fb[(i % kLaneWords) * 32 + i / kLaneWords] = src[i];
    }
    mi::Ax25Lane L{};
    if (work)
        L = mi::Ax25Lane{st->prev[me], st->ones[me], st->phase[me], st->nbits[me], st->cur[me], st->nbytes[me], st->crc[me], st->start[me]};
    const uint64_t batch0 = st->batch;
    uint64_t last_end = st->last_end;  // (wave-uniform: every lane reads the same field)
    const int tau = me % kTau;
    uint8_t* const my_bytes = reinterpret_cast<uint8_t*>(fb + me);  // byte i of the lane's frame at my_bytes[(i >> 2) * 128 + (i & 3)]
    uint32_t n = 0;
    const uint32_t* my_words = bits + static_cast<size_t>(row) * nbatches * kBlockWords + me * kWords;
    uint32_t next[kWords];
#pragma unroll
    for (int wi = 0; wi < kWords; ++wi)
        next[wi] = my_words[wi];
    __syncthreads();  // the bytes are in LDS
    for (uint32_t b = 0; b < nbatches; ++b) {
        uint32_t cur[kWords];
#pragma unroll
        for (int wi = 0; wi < kWords; ++wi)
            cur[wi] = next[wi];
        if (b + 1 < nbatches) {
            my_words += kBlockWords;
#pragma unroll
            for (int wi = 0; wi < kWords; ++wi)
                next[wi] = my_words[wi];
        }
        // where the lane's slot j ends is lane_base + 40 j
        const uint64_t lane_base = 3ull * kBatch * (batch0 + b) + static_cast<uint64_t>(mi::ax25_slot_end(tau, 0));
#pragma unroll
        for (int wi = 0; wi < kWords; ++wi) {
            uint32_t word = cur[wi];
            const int nbit = wi < kWords - 1 ? 32 : kBits - 32 * (kWords - 1);
            for (int k = 0; k < nbit; ++k) {
                const uint32_t t = word & 1u;
                word >>= 1;
                uint32_t ev = 0;
                if (work)
                    ev = mi::ax25_step(L, t, [&](uint32_t i, uint32_t byte) { my_bytes[(i >> 2) * 128 + (i & 3)] = static_cast<uint8_t>(byte); });
                const uint64_t end = lane_base + 40u * static_cast<uint32_t>(32 * wi + k);
                unsigned long long cands = __ballot(ev & mi::kAx25Cand);
                if (cands) {          // (wave-uniform, rare)
                    __syncthreads();  // the candidates' last bytes are in LDS
                    do {
                        const int c = __builtin_ctzll(cands);
                        cands &= cands - 1;
                        const uint64_t c_start = static_cast<uint64_t>(from_lane(static_cast<uint32_t>(L.start >> 32), c)) << 32 |
                                                 from_lane(static_cast<uint32_t>(L.start), c);
                        if (c_start + 40 < last_end)
                            continue;
                        const uint32_t c_nbytes = from_lane(L.nbytes, c);
                        // the address field: lane i on byte i, then on byte 64 + i
                        const uint8_t* const c_bytes = reinterpret_cast<const uint8_t*>(fb + c);
                        const uint32_t i1 = 64u + static_cast<uint32_t>(lane);
                        const bool in0 = static_cast<uint32_t>(lane) + 3 < c_nbytes, in1 = i1 < 70 && i1 + 3 < c_nbytes;
                        const uint32_t b0 = in0 ? c_bytes[(lane >> 2) * 128 + (lane & 3)] : 0u, b1 = in1 ? c_bytes[(i1 >> 2) * 128 + (i1 & 3)] : 0u;
                        const unsigned long long ext0 = __ballot(b0 & 1u), ext1 = __ballot(b1 & 1u);
                        const uint32_t last = ext0 ? static_cast<uint32_t>(__builtin_ctzll(ext0)) : ext1 ? 64u + static_cast<uint32_t>(__builtin_ctzll(ext1)) : 70u;
                        uint32_t naddr = 0;
                        if (last < 70 && last % 7 == 6 && last >= 13) {
                            const bool bad0 = static_cast<uint32_t>(lane) < last && lane % 7 != 6 && !mi::ax25_call_char(b0);
                            const bool bad1 = i1 < last && i1 % 7 != 6 && !mi::ax25_call_char(b1);
                            if (__ballot(bad0 || bad1) == 0)
                                naddr = (last + 1) / 7;
                        }
                        if (strict && !naddr)
                            continue;
                        const uint64_t c_end = static_cast<uint64_t>(from_lane(static_cast<uint32_t>(end >> 32), c)) << 32 | from_lane(static_cast<uint32_t>(end), c);
                        if (n < slots) {  // (n < slots always: slots is the most a row can end)
                            uint32_t* const rec = reinterpret_cast<uint32_t*>(scratch + static_cast<size_t>(row) * slots + n);
                            for (uint32_t i = static_cast<uint32_t>(lane); i < static_cast<uint32_t>(kFrameWords); i += 64) {
                                uint32_t v;
                                if (i == 0)
                                    v = row;
                                else if (i == 1)
                                    v = static_cast<uint32_t>(c_start / (3u * kBatch));
                                else if (i == 2)
                                    v = static_cast<uint32_t>(c_start % (3u * kBatch));
                                else if (i == 3)
                                    v = b;
                                else if (i == 4)
                                    v = c_nbytes | static_cast<uint32_t>(c) << 16 | naddr << 24;
                                else {
                                    const uint32_t w = i - 5, have = c_nbytes > 4 * w ? c_nbytes - 4 * w : 0u;
                                    v = fb[w * 32 + c] & (have >= 4 ? 0xFFFFFFFFu : (1u << (8 * have)) - 1u);
                                }
                                rec[i] = v;
                            }
                        }
                        ++n;
                        last_end = c_end;
                    } while (cands);
                }
                if (ev & mi::kAx25Flag)
                    mi::ax25_open(L, end);
            }
        }
    }
    if (work)
        nby[lane] = L.nbytes;
    __syncthreads();
    {
        uint32_t* const dst = reinterpret_cast<uint32_t*>(&st->bytes[0][0]);
        for (int i = lane; i < kLanes * kLaneWords; i += 64) {
            const uint32_t l = i / kLaneWords, w = i % kLaneWords, have = nby[l] > 4 * w ? nby[l] - 4 * w : 0u;
            dst[i] = fb[w * 32 + l] & (have >= 4 ? 0xFFFFFFFFu : (1u << (8 * have)) - 1u);
        }
    }
    if (work) {
        st->prev[lane] = static_cast<uint8_t>(L.prev), st->ones[lane] = static_cast<uint8_t>(L.ones), st->phase[lane] = static_cast<uint8_t>(L.phase);
        st->nbits[lane] = static_cast<uint8_t>(L.nbits), st->cur[lane] = static_cast<uint8_t>(L.cur), st->nbytes[lane] = static_cast<uint16_t>(L.nbytes);
        st->crc[lane] = static_cast<uint16_t>(L.crc), st->start[lane] = L.start;
    }
    if (lane == 0) {
        st->batch = batch0 + nbatches;
        st->last_end = last_end;
        row_frame_count[row] = n;
    }
}

// Launch 3.  mi::launch_row_scan (poststage.hip): exclusive scan of the rows' frame counts, and the two counts.

// Launch 4.  One thread per (row, slot, 8 bytes of the record): a frame the row ended goes to its place, unless that is at or beyond
// the capacity.
constexpr int kFrameParts = sizeof(mi_ax25_frame) / 8;  // 44
__global__ __launch_bounds__(256) void k_ax25_store(const mi_ax25_frame* __restrict__ scratch, const uint32_t* __restrict__ row_frame_count,
                                                    const uint32_t* __restrict__ row_first, const uint32_t rows, const uint32_t slots,
                                                    const uint32_t max_frames, mi_ax25_frame* __restrict__ frames) {
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

// Launch 5.  mi::k_carry_tails (carry.hpp): the last 14 input samples of the call are an enabled row's new carried samples.

}  // namespace

extern "C" {

int mi_ax25_create(const mi_ax25_cfg* cfg, const uint8_t* row_enabled, int rows, int max_batches, size_t max_frames, int gpu, mi_ax25** out) {
    if (!row_enabled || !out)
        return fail(MI_ERR_INVALID, "NULL argument");
    mi::Ax25Plan plan;
    if (const int rc = mi::ax25_plan(cfg, &plan))
        return rc;
    if (const int rc = mi::batch_geometry_ok(kName, rows, max_batches))
        return rc;
    if (const int rc = mi::check_gpu(gpu, "no HIP device: the packet stage runs on the GPU only"))
        return rc;
    mi_ax25* s = new mi_ax25();
    s->gpu = gpu;
    s->rows = rows;
    s->max_batches = max_batches;
    s->plan = plan;
    const size_t n = static_cast<size_t>(rows), blocks = n * static_cast<size_t>(max_batches);
    const size_t most = n * mi::ax25_max_frames(static_cast<uint64_t>(max_batches));
    s->max_frames = static_cast<uint32_t>(max_frames && max_frames < most ? max_frames : most);  // (no call has more frames than `most`)
    std::vector<float> h(160);
    mi::ax25_templates(h.data());
    if (hipSetDevice(gpu) != hipSuccess || dalloc_copy(s->d_enabled, as_flags(row_enabled, n)) != hipSuccess || dalloc_zero(s->d_state, n) != hipSuccess ||
        dalloc_copy(s->d_templates, h) != hipSuccess || dalloc(s->d_bits, blocks * kBlockWords) != hipSuccess || dalloc(s->d_scratch, most) != hipSuccess ||
        dalloc(s->d_row_frame_count, n) != hipSuccess || hipHostMalloc(reinterpret_cast<void**>(s->h_count.put()), 2 * sizeof(uint32_t)) != hipSuccess ||
        hipDeviceSynchronize() != hipSuccess) {
        delete s;
        return fail(MI_ERR_HIP, "packet stage: device allocation failed");
    }
    *out = s;
    return MI_OK;
}

void mi_ax25_destroy(mi_ax25* s) {
    mi::destroy(s);
}

int mi_ax25_set_rows(mi_ax25* s, const uint8_t* row_enabled) {
    return mi::set_enabled(kName, s, row_enabled);
}

int mi_ax25_process_device(mi_ax25* s, const float* d_plane, size_t row_stride, int nbatches, uint32_t* d_bits, mi_ax25_frame* d_frames,
                           uint32_t* d_row_first_frame, uint32_t* d_count, void* hip_stream) {
    if (!s || !d_plane || !d_frames || !d_row_first_frame || !d_count)
        return fail(MI_ERR_INVALID, "NULL argument");
    if (nbatches < 1 || nbatches > s->max_batches)
        return fail(MI_ERR_INVALID, "nbatches outside 1 .. max_batches");
    if (row_stride < static_cast<size_t>(nbatches) * mi::kWaveBatch)
        return fail(MI_ERR_INVALID, "a row stride is shorter than the call");
    if (row_stride % 4 != 0 || !aligned(d_plane, 16) || !aligned(d_bits, 4) || !aligned(d_frames, 8) || !aligned(d_row_first_frame, 4) || !aligned(d_count, 4))
        return fail(MI_ERR_INVALID, "the plane must be 16-byte aligned with a row stride that is a multiple of 4 floats; frame records 8-byte aligned");
    if (hipSetDevice(s->gpu) != hipSuccess)
        return fail(MI_ERR_HIP, "hipSetDevice failed");
    hipStream_t q = static_cast<hipStream_t>(hip_stream);
    const unsigned rows = static_cast<unsigned>(s->rows), nb = static_cast<unsigned>(nbatches);
    // the frames a row can end in this call: at most what create allocated, as nbatches <= max_batches
    const uint32_t slots = mi::ax25_max_frames(nb);
    uint32_t* const bits = d_bits ? d_bits : s->d_bits.get();
    const mi::Ax25Gains gain{{s->plan.gain[0], s->plan.gain[1], s->plan.gain[2]}};
    s->timing.stamp(0, q);
    hipLaunchKernelGGL(k_ax25_bits, dim3(rows * nb), dim3(256), 0, q, s->d_enabled.get(), s->d_state.get(), d_plane, row_stride, nb, s->d_templates.get(),
                       gain, bits);
    s->timing.stamp(1, q);
    hipLaunchKernelGGL(k_ax25_walk, dim3(rows), dim3(64), 0, q, s->d_enabled.get(), s->d_state.get(), bits, nb, slots, s->plan.strict, s->d_scratch.get(),
                       s->d_row_frame_count.get());
    s->timing.stamp(2, q);
    mi::launch_row_scan(q, s->d_row_frame_count, s->rows, s->max_frames, d_row_first_frame, d_count);
    s->timing.stamp(3, q);
    hipLaunchKernelGGL(k_ax25_store, dim3((rows * slots * kFrameParts + 255) / 256), dim3(256), 0, q, s->d_scratch.get(), s->d_row_frame_count.get(),
                       d_row_first_frame, rows, slots, s->max_frames, d_frames);
    s->timing.stamp(4, q);
    mi::launch_carry_tails<MI_AX25_HISTORY>(q, s->d_enabled.get(), d_plane, row_stride, rows, nbatches, s->d_state.get());
    s->timing.stamp(5, q);
    if (hipGetLastError() != hipSuccess)
        return fail(MI_ERR_HIP, "packet stage kernel launch failed");
    s->called = true;
    s->last_frames = d_frames;
    s->last_row_first = d_row_first_frame;
    s->last_count = d_count;
    return MI_OK;
}

int mi_ax25_download(mi_ax25* s, void* hip_stream, mi_ax25_frame* frames, uint32_t* row_first_frame, uint32_t* count) {
    if (!s || !count)
        return fail(MI_ERR_INVALID, "NULL argument");
    if (!s->last_count)
        return fail(MI_ERR_INVALID, "no mi_ax25_process_device call to download");
    hipStream_t q = static_cast<hipStream_t>(hip_stream);
    if (!mi::land_counts(s->gpu, q, s->h_count, s->last_count, count))
        return fail(MI_ERR_HIP, "packet stage: reading the counts failed");
    const size_t k = count[1];
    bool ok = true;
    if (frames && k)
        ok = ok && hipMemcpyAsync(frames, s->last_frames, k * sizeof(mi_ax25_frame), hipMemcpyDeviceToHost, q) == hipSuccess;
    if (row_first_frame)
        ok = ok && hipMemcpyAsync(row_first_frame, s->last_row_first, (static_cast<size_t>(s->rows) + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, q) ==
                       hipSuccess;
    if (!ok || hipStreamSynchronize(q) != hipSuccess)
        return fail(MI_ERR_HIP, "packet stage: download failed");
    return MI_OK;
}

int mi_ax25_set_timing(mi_ax25* s, int on) {
    return mi::set_timing(s, on);
}

int mi_ax25_last_launch_ms(mi_ax25* s, float* ms) {
    return mi::last_launch_ms(s, ms, "mi_ax25_process_device");
}

size_t mi_ax25_state_size(const mi_ax25* s) {
    return mi::state_size(s, &mi_ax25::d_state);
}

int mi_ax25_get_state(mi_ax25* s, void* buf, size_t len) {
    return mi::get_state(kName, s, &mi_ax25::d_state, buf, len);
}

int mi_ax25_set_state(mi_ax25* s, const void* buf, size_t len) {
    return mi::set_state(kName, s, &mi_ax25::d_state, buf, len, [](const mi::Ax25RowState* rows, size_t n) { return mi::ax25_state_ok(rows, n); });
}

}  // extern "C"
