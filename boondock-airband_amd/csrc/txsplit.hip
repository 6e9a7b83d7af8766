// txsplit.hip -- one recording per transmission, decided in signal time on the device: which file each travelling block of the
// audio mi_demod_process_device wrote belongs to, when files close, and per file and call the peak and the energy of its blocks.
//   close_if_necessary   duration > 1.0 s and idle > 0.5 s, or duration > 3600 s          src/output.cpp:353-376
//   output_file_ready    a batch that is written opens a file when none is open            src/output.cpp:404-414, :454
//   file / rawfile       skip a silent batch once the batch before it was silent too       src/output.cpp:518-520, :560, :561
// restated on the jitter-free schedule (batch b of a row at t0 + b * WAVE_BATCH / WAVE_RATE), so every time is a count of batches:
// the rule, the thresholds, the record, the order of `energy` and the state blob are in include/mi_airband.h.  A post-stage of its
// own like the gate (outgate.hip), whose MI_GATE_OPEN_TRAIL rule lets the same blocks travel: four small launches on the caller's
// stream, no atomics.  mi_tx_plan_host (poststage_host.cpp) is the host twin.  The handle's base and the bodies of the entry points
// every stage repeats are in poststage.hpp.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "../../include/mi_airband.h"
#include "poststage.hpp"

constexpr char kName[] = "transmission splitter";

struct mi_txsplit : mi::RowStage {
    mi_txsplit() : RowStage(kName, 4) {}
    uint32_t max_records = 0;
    mi_tx_cfg cfg{};
    mi::DevBuf<mi::TxRowState> d_state;    // [rows]: the checkpoint blob as it is
    mi::DevBuf<int> d_rank;                // [rows][nbatches of the call]: place among the row's travelling blocks, -1 = does not travel
    mi::DevBuf<mi_tx_record> d_row_rec;    // [rows][nbatches + 1]: the walk's records, peak and energy still 0
    mi::DevBuf<uint32_t> d_row_rec_count;  // [rows]
    mi::DevBuf<double> d_block_sum;        // [rows][nbatches]: sum of x * x of the row's travelling block number `rank`
    mi::DevBuf<float> d_block_peak;        // the same for max |x|
    mi::PinnedBuf<uint32_t> h_count;       // [2], landing place of the counts in mi_txsplit_download
    // destinations of the last mi_txsplit_process_device (what mi_txsplit_download reads)
    const mi_tx_record* last_records = nullptr;
    const uint32_t* last_row_first = nullptr;
    const uint32_t* last_count = nullptr;
};

namespace {

using mi::aligned;
using mi::as_flags;
using mi::fail;
using mi::kRowsPerGroup;
constexpr uint32_t kNone = 0xFFFFFFFFu;

__device__ inline uint32_t uniform(uint32_t v) {
    return static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(v)));
}

__device__ inline uint64_t uniform64(uint64_t v) {
    return (static_cast<uint64_t>(uniform(static_cast<uint32_t>(v >> 32))) << 32) | uniform(static_cast<uint32_t>(v));
}

// Launch 1.  The row's wave loads 64 flags a trip, one per lane, and walks the state machine over the ballot mask in wave-uniform
// code; a stretch with no file open and nothing to write is skipped to the next flag that is set.  Lanes then take their batch's
// rank from the mask of the batches that travel; lane 0 stores a record whenever a file closes and, for the file still open, at
// the end of the call.
__global__ __launch_bounds__(256) void k_tx_walk(const uint8_t* __restrict__ enabled, mi::TxRowState* __restrict__ state, const char* __restrict__ axc,
                                                 const size_t axc_stride, const int rows, const int nbatches, const uint32_t min_b, const uint32_t idle_b,
                                                 const uint32_t max_b, int* __restrict__ rank, mi_tx_record* __restrict__ row_rec,
                                                 uint32_t* __restrict__ row_rec_count) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * kRowsPerGroup + (threadIdx.x >> 6);
    if (row >= rows)  // (the whole wave)
        return;
    if (!enabled[row]) {  // the row sits out: nothing travels, no record, every byte of its state stays
        for (int b = lane; b < nbatches; b += 64)
            rank[static_cast<size_t>(row) * nbatches + b] = -1;
        if (lane == 0)
            row_rec_count[row] = 0;
        return;
    }
    const mi::TxRowState st = state[row];  // (every lane the same address)
    uint64_t clock = uniform64(st.clock), opened = uniform64(st.opened), last_write = uniform64(st.last_write);
    uint32_t seq = uniform(st.seq);
    bool open = uniform(st.open) != 0, active = uniform(st.active) != 0;
    // the open file's part in this call
    bool have = false;
    uint32_t cur_seq = 0, cur_first_block = 0, cur_nblocks = 0, cur_first_batch = kNone, cur_flags = 0;
    uint32_t travelled = 0, nrec = 0;
    mi_tx_record* const rec = row_rec + static_cast<size_t>(row) * (static_cast<size_t>(nbatches) + 1);
    auto flush = [&](uint32_t close_batch) {
        if (lane == 0) {  // 40 bytes, 8-byte aligned: five 8-byte vector stores; peak and energy are the combine pass's
            uint2* p = reinterpret_cast<uint2*>(rec + nrec);
            p[0] = make_uint2(static_cast<uint32_t>(row), cur_seq);
            p[1] = make_uint2(cur_first_block, cur_nblocks);
            p[2] = make_uint2(cur_first_batch, close_batch);
            p[3] = make_uint2(cur_flags, 0u);
            p[4] = make_uint2(0u, 0u);
        }
        ++nrec;
        have = false;
    };
    auto begin = [&](uint32_t flags) {
        have = true;
        cur_seq = seq;
        cur_first_block = travelled;
        cur_nblocks = 0;
        cur_first_batch = kNone;
        cur_flags = flags;
    };
    for (int b0 = 0; b0 < nbatches; b0 += 64) {
        const int b = b0 + lane;
        const bool valid = b < nbatches;
        const bool sig = valid && axc[static_cast<size_t>(row) * axc_stride + b] != MI_NO_SIGNAL;
        const unsigned long long sigmask = __ballot(sig);  // lanes beyond nbatches contribute 0
        const int n = nbatches - b0 < 64 ? nbatches - b0 : 64;
        unsigned long long travel = 0;
        const uint32_t base = travelled;
        for (int l = 0; l < n;) {
            if (!open && !active) {  // nothing happens until the next signal
                const unsigned long long rest = sigmask >> l;
                const int skip = rest ? __builtin_ctzll(rest) : n - l;
                clock += static_cast<uint64_t>(skip);
                l += skip;
                if (l >= n)
                    break;
            }
            const bool signal = (sigmask >> l) & 1ull;
            if (open) {  // close_if_necessary, output.cpp:367-375
                const uint64_t d = clock - opened, i = clock - last_write;
                if (d > max_b || (d > min_b && i > idle_b)) {
                    open = false;
                    if (!have)
                        begin(1u);
                    flush(static_cast<uint32_t>(b0 + l));
                }
            }
            if (signal || active) {  // output.cpp:518-520
                if (!open) {         // output_file_ready, :404-414, :454
                    seq += 1;
                    open = true;
                    opened = clock;
                    begin(0u);
                } else if (!have) {
                    begin(1u);
                }
                if (cur_nblocks == 0)
                    cur_first_batch = static_cast<uint32_t>(b0 + l);
                cur_nblocks += 1;
                travelled += 1;
                travel |= 1ull << l;
                active = signal;     // :560
                last_write = clock;  // :561
            }
            clock += 1;
            ++l;
        }
        if (valid)
            rank[static_cast<size_t>(row) * nbatches + b] =
                ((travel >> lane) & 1ull) ? static_cast<int>(base + __popcll(travel & ((1ull << lane) - 1ull))) : -1;
    }
    if (have)
        flush(kNone);
    if (lane == 0) {
        row_rec_count[row] = nrec;
        uint4* p = reinterpret_cast<uint4*>(state + row);  // 32 bytes, 32-byte aligned
        p[0] = make_uint4(static_cast<uint32_t>(clock), static_cast<uint32_t>(clock >> 32), static_cast<uint32_t>(opened), static_cast<uint32_t>(opened >> 32));
        p[1] = make_uint4(static_cast<uint32_t>(last_write), static_cast<uint32_t>(last_write >> 32), seq, (open ? 1u : 0u) | (active ? 0x100u : 0u));
    }
}

// Launch 2.  mi::launch_row_scan (poststage.hip): exclusive scan of the rows' record counts, and the two counts.

// Launch 3.  One workgroup per (row, batch) on a 1-D grid; a block that does not travel returns at once.  Thread t squares float4
// number t and (t < 244) number 256 + t in double, which is exact, and adds the eight in sequence; the 256 sums are halved through
// LDS down to 64 and by __shfl_down in wave 0 from there: the order include/mi_airband.h defines.  Each sample is read once.
__global__ __launch_bounds__(256) void k_tx_block_stats(const int* __restrict__ rank, const float* __restrict__ wave, const size_t row_stride,
                                                        const int nbatches, double* __restrict__ block_sum, float* __restrict__ block_peak) {
    __shared__ double sh_sum[256];
    __shared__ float sh_peak[256];
    const int r = rank[blockIdx.x];
    if (r < 0)
        return;
    const uint32_t row = blockIdx.x / static_cast<uint32_t>(nbatches), b = blockIdx.x % static_cast<uint32_t>(nbatches);
    const int t = threadIdx.x;
    const float4* s = reinterpret_cast<const float4*>(wave + static_cast<size_t>(row) * row_stride + static_cast<size_t>(b) * mi::kWaveBatch);
    constexpr int kSecond = mi::kWaveBatch / 4 - 256;  // 244 threads have a second float4
    const float4 v0 = s[t];
    const float4 v1 = t < kSecond ? s[256 + t] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    double acc = static_cast<double>(v0.x) * static_cast<double>(v0.x);
    acc += static_cast<double>(v0.y) * static_cast<double>(v0.y);
    acc += static_cast<double>(v0.z) * static_cast<double>(v0.z);
    acc += static_cast<double>(v0.w) * static_cast<double>(v0.w);
    float peak = fmaxf(fmaxf(fabsf(v0.x), fabsf(v0.y)), fmaxf(fabsf(v0.z), fabsf(v0.w)));
    if (t < kSecond) {
        acc += static_cast<double>(v1.x) * static_cast<double>(v1.x);
        acc += static_cast<double>(v1.y) * static_cast<double>(v1.y);
        acc += static_cast<double>(v1.z) * static_cast<double>(v1.z);
        acc += static_cast<double>(v1.w) * static_cast<double>(v1.w);
        peak = fmaxf(peak, fmaxf(fmaxf(fabsf(v1.x), fabsf(v1.y)), fmaxf(fabsf(v1.z), fabsf(v1.w))));
    }
    sh_sum[t] = acc;
    sh_peak[t] = peak;
    __syncthreads();
    if (t < 128) {
        sh_sum[t] = acc + sh_sum[t + 128];
        sh_peak[t] = fmaxf(peak, sh_peak[t + 128]);
    }
    __syncthreads();
    if (t < 64) {  // wave 0
        acc = sh_sum[t] + sh_sum[t + 64];
        peak = fmaxf(sh_peak[t], sh_peak[t + 64]);
        for (int d = 32; d >= 1; d >>= 1) {  // lane t < d holds acc[t] + acc[t + d]; what the lanes above hold is not used
            acc += __shfl_down(acc, d);
            peak = fmaxf(peak, __shfl_down(peak, d));
        }
        if (t == 0) {
            const size_t k = static_cast<size_t>(row) * nbatches + static_cast<size_t>(r);
            block_sum[k] = acc;
            block_peak[k] = peak;
        }
    }
}

// Launch 4.  One lane per (row, record slot): it folds its record's block sums in block order and stores the record at the row's
// exclusive prefix plus the slot, unless that place is beyond the capacity.
__global__ __launch_bounds__(256) void k_tx_combine(const mi_tx_record* __restrict__ row_rec, const uint32_t* __restrict__ row_rec_count,
                                                    const uint32_t* __restrict__ row_first, const double* __restrict__ block_sum,
                                                    const float* __restrict__ block_peak, const int rows, const int nbatches, const int with_audio,
                                                    const uint32_t max_records, mi_tx_record* __restrict__ records) {
    const uint32_t slots = static_cast<uint32_t>(nbatches) + 1u;
    const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t row = idx / slots, j = idx % slots;
    if (row >= static_cast<uint32_t>(rows) || j >= row_rec_count[row])
        return;
    const uint32_t k = row_first[row] + j;
    if (k >= max_records)
        return;
    const uint2* src = reinterpret_cast<const uint2*>(row_rec + static_cast<size_t>(row) * slots + j);
    const uint2 a = src[0], bl = src[1], c = src[2], fl = src[3];
    double energy = 0.0;
    float peak = 0.0f;
    if (with_audio) {
        const size_t first = static_cast<size_t>(row) * nbatches + bl.x;
        for (uint32_t i = 0; i < bl.y; ++i) {
            energy += block_sum[first + i];
            peak = fmaxf(peak, block_peak[first + i]);
        }
    }
    uint2* dst = reinterpret_cast<uint2*>(records + k);
    dst[0] = a;
    dst[1] = bl;
    dst[2] = c;
    dst[3] = make_uint2(fl.x, __float_as_uint(peak));
    const unsigned long long e = static_cast<unsigned long long>(__double_as_longlong(energy));
    dst[4] = make_uint2(static_cast<uint32_t>(e), static_cast<uint32_t>(e >> 32));
}

}  // namespace

extern "C" {

int mi_txsplit_create(const mi_tx_cfg* cfg, const uint8_t* row_enabled, int rows, int max_batches, size_t max_records, int gpu, mi_txsplit** out) {
    if (!row_enabled || !out)
        return fail(MI_ERR_INVALID, "NULL argument");
    if (rows < 1 || rows >= (1 << 20) || max_batches < 1 ||
        static_cast<uint64_t>(rows) * (static_cast<uint64_t>(max_batches) + 1) >= (1ull << 24))
        return fail(MI_ERR_INVALID, "transmission splitter needs 1 <= rows < 2^20, max_batches >= 1 and rows * (max_batches + 1) < 2^24");
    if (const int rc = mi::check_gpu(gpu, "no HIP device: the transmission splitter runs on the GPU only"))
        return rc;
    mi_txsplit* t = new mi_txsplit();
    t->gpu = gpu;
    t->rows = rows;
    t->max_batches = max_batches;
    t->cfg = mi::tx_cfg_or_default(cfg);
    const size_t n = static_cast<size_t>(rows), all = n * static_cast<size_t>(max_batches), slots = n * (static_cast<size_t>(max_batches) + 1);
    t->max_records = static_cast<uint32_t>(max_records && max_records < slots ? max_records : slots);  // (no call has more records than `slots`)
    if (hipSetDevice(gpu) != hipSuccess || dalloc_copy(t->d_enabled, as_flags(row_enabled, static_cast<size_t>(rows))) != hipSuccess ||
        dalloc_zero(t->d_state, n) != hipSuccess || dalloc(t->d_rank, all) != hipSuccess || dalloc(t->d_row_rec, slots) != hipSuccess ||
        dalloc(t->d_row_rec_count, n) != hipSuccess || dalloc(t->d_block_sum, all) != hipSuccess || dalloc(t->d_block_peak, all) != hipSuccess ||
        hipHostMalloc(reinterpret_cast<void**>(t->h_count.put()), 2 * sizeof(uint32_t)) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
        delete t;
        return fail(MI_ERR_HIP, "transmission splitter: device allocation failed");
    }
    *out = t;
    return MI_OK;
}

void mi_txsplit_destroy(mi_txsplit* t) {
    mi::destroy(t);
}

int mi_txsplit_set_rows(mi_txsplit* t, const uint8_t* row_enabled) {
    return mi::set_enabled(kName, t, row_enabled);
}

int mi_txsplit_process_device(mi_txsplit* t, const float* d_waveout, size_t row_stride, const char* d_axc, size_t axc_stride, int nbatches,
                              mi_tx_record* d_records, uint32_t* d_row_first_record, uint32_t* d_count, void* hip_stream) {
    if (!t || !d_axc || !d_records || !d_row_first_record || !d_count)
        return fail(MI_ERR_INVALID, "NULL argument");
    if (nbatches < 1 || nbatches > t->max_batches)
        return fail(MI_ERR_INVALID, "nbatches outside 1 .. max_batches");
    if (axc_stride < static_cast<size_t>(nbatches) || (d_waveout && row_stride < static_cast<size_t>(nbatches) * mi::kWaveBatch))
        return fail(MI_ERR_INVALID, "a row stride is shorter than the call");
    if ((d_waveout && (row_stride % 4 != 0 || !aligned(d_waveout, 16))) || !aligned(d_records, 8) || !aligned(d_row_first_record, 4) ||
        !aligned(d_count, 4))
        return fail(MI_ERR_INVALID, "the audio buffer must be 16-byte aligned with a row stride that is a multiple of 4 floats; records 8-byte aligned");
    if (hipSetDevice(t->gpu) != hipSuccess)
        return fail(MI_ERR_HIP, "hipSetDevice failed");
    hipStream_t q = static_cast<hipStream_t>(hip_stream);
    const unsigned rows = static_cast<unsigned>(t->rows), nb = static_cast<unsigned>(nbatches);
    t->timing.stamp(0, q);
    hipLaunchKernelGGL(k_tx_walk, dim3((rows + kRowsPerGroup - 1) / kRowsPerGroup), dim3(256), 0, q, t->d_enabled.get(), t->d_state.get(), d_axc, axc_stride,
                       t->rows, nbatches, t->cfg.min_batches, t->cfg.idle_batches, t->cfg.max_batches, t->d_rank.get(), t->d_row_rec.get(),
                       t->d_row_rec_count.get());
    t->timing.stamp(1, q);
    mi::launch_row_scan(q, t->d_row_rec_count, t->rows, t->max_records, d_row_first_record, d_count);
    t->timing.stamp(2, q);
    if (d_waveout)
        hipLaunchKernelGGL(k_tx_block_stats, dim3(rows * nb), dim3(256), 0, q, t->d_rank.get(), d_waveout, row_stride, nbatches, t->d_block_sum.get(),
                           t->d_block_peak.get());
    t->timing.stamp(3, q);
    hipLaunchKernelGGL(k_tx_combine, dim3((rows * (nb + 1) + 255) / 256), dim3(256), 0, q, t->d_row_rec.get(), t->d_row_rec_count.get(), d_row_first_record,
                       t->d_block_sum.get(), t->d_block_peak.get(), t->rows, nbatches, d_waveout ? 1 : 0, t->max_records, d_records);
    t->timing.stamp(4, q);
    if (hipGetLastError() != hipSuccess)
        return fail(MI_ERR_HIP, "transmission splitter kernel launch failed");
    t->called = true;
    t->last_records = d_records;
    t->last_row_first = d_row_first_record;
    t->last_count = d_count;
    return MI_OK;
}

int mi_txsplit_download(mi_txsplit* t, void* hip_stream, mi_tx_record* records, uint32_t* row_first_record, uint32_t* count) {
    if (!t || !count)
        return fail(MI_ERR_INVALID, "NULL argument");
    if (!t->last_count)
        return fail(MI_ERR_INVALID, "no mi_txsplit_process_device call to download");
    hipStream_t q = static_cast<hipStream_t>(hip_stream);
    if (!mi::land_counts(t->gpu, q, t->h_count, t->last_count, count))
        return fail(MI_ERR_HIP, "transmission splitter: reading the counts failed");
    const size_t k = count[1];
    bool ok = true;
    if (records && k)
        ok = ok && hipMemcpyAsync(records, t->last_records, k * sizeof(mi_tx_record), hipMemcpyDeviceToHost, q) == hipSuccess;
    if (row_first_record)
        ok = ok && hipMemcpyAsync(row_first_record, t->last_row_first, (static_cast<size_t>(t->rows) + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, q) ==
                       hipSuccess;
    if (!ok || hipStreamSynchronize(q) != hipSuccess)
        return fail(MI_ERR_HIP, "transmission splitter: download failed");
    return MI_OK;
}

int mi_txsplit_set_timing(mi_txsplit* t, int on) {
    return mi::set_timing(t, on);
}

int mi_txsplit_last_launch_ms(mi_txsplit* t, float* ms) {
    return mi::last_launch_ms(t, ms, "mi_txsplit_process_device");
}

size_t mi_txsplit_state_size(const mi_txsplit* t) {
    return mi::state_size(t, &mi_txsplit::d_state);
}

int mi_txsplit_get_state(mi_txsplit* t, void* buf, size_t len) {
    return mi::get_state(kName, t, &mi_txsplit::d_state, buf, len);
}

int mi_txsplit_set_state(mi_txsplit* t, const void* buf, size_t len) {
    return mi::set_state(kName, t, &mi_txsplit::d_state, buf, len, [](const mi::TxRowState* rows, size_t n) -> const char* {
        for (size_t r = 0; r < n; ++r)
            if (rows[r].open > 1 || rows[r].active > 1 || rows[r].zero != 0)
                return "malformed blob";
        return nullptr;
    });
}

}  // extern "C"
