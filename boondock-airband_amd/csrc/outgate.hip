// outgate.hip -- the output gate on the device: which (row, batch) blocks of the audio mi_demod_process_device wrote the reference's
// outputs consume, and those blocks packed densely so that only they cross the link.
//   udp_stream / pulse  skip a batch whose axcindicate is NO_SIGNAL                        src/output.cpp:568-570, :581-582
//   file / rawfile      skip it once the batch before it was silent too                   src/output.cpp:518-520, active set at :560
//   continuous outputs  skip nothing                                                       the same lines, continuous == true
// A post-stage of its own like the mixer (mixer.hip): three small launches on the caller's stream, no atomics -- a block's place is
// its row's exclusive prefix plus its rank within the row, so the packed order is rows ascending, batches ascending, on every run.
// Everything moved is a copy: bandwidth-bound, one float4 per lane per access.  mi_gate_plan_host (poststage_host.cpp) is the host twin.
// The handle's base and the bodies of the entry points every stage repeats are in poststage.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/mi_airband.h"
#include "poststage.hpp"

constexpr char kName[] = "output gate";

struct mi_outgate : mi::BatchStage {
    mi_outgate() : BatchStage(kName, 3) {}
    uint32_t max_blocks = 0;
    bool any_iq = false;
    mi::DevBuf<uint8_t> d_rule, d_has_iq, d_carried;  // [rows]
    mi::DevBuf<int> d_rank;                           // [rows][nbatches of the call]: place within the row, -1 = does not travel
    mi::DevBuf<uint32_t> d_row_count;                 // [rows]
    mi::PinnedBuf<uint32_t> h_count;                  // [2], landing place of the counts in mi_outgate_download
    // destinations of the last mi_outgate_process_device (what mi_outgate_download reads)
    const float* last_blocks = nullptr;
    const float* last_iq_blocks = nullptr;
    const mi_gate_block* last_index = nullptr;
    const uint32_t* last_row_first = nullptr;
    const uint32_t* last_count = nullptr;
};

namespace {

using mi::aligned;
using mi::fail;
using mi::kRowsPerGroup;

// Launch 1.  Lane l of the row's wave takes batch b0 + l of a 64-batch chunk; the predecessor's flag comes from the lane below,
// lane 0 takes the carried flag (first chunk) or the last lane of the chunk before.
__global__ __launch_bounds__(256) void k_gate_rank(const uint8_t* __restrict__ rule, uint8_t* __restrict__ carried, const char* __restrict__ axc,
                                                   const size_t axc_stride, const int rows, const int nbatches, int* __restrict__ rank,
                                                   uint32_t* __restrict__ row_count) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * kRowsPerGroup + (threadIdx.x >> 6);
    if (row >= rows)  // (the whole wave)
        return;
    const int ru = rule[row];
    int carry = carried[row] != 0;
    uint32_t base = 0;
    for (int b0 = 0; b0 < nbatches; b0 += 64) {
        const int b = b0 + lane;
        const bool valid = b < nbatches;
        const int sig = valid && axc[static_cast<size_t>(row) * axc_stride + b] != MI_NO_SIGNAL;
        int prev = __shfl_up(sig, 1);
        if (lane == 0)
            prev = carry;
        const bool travel = valid && (ru == MI_GATE_ALL || (ru != MI_GATE_NONE && sig) || (ru == MI_GATE_OPEN_TRAIL && prev));
        const unsigned long long m = __ballot(travel);  // lanes beyond nbatches contribute 0
        if (valid)
            rank[static_cast<size_t>(row) * nbatches + b] = travel ? static_cast<int>(base + __popcll(m & ((1ull << lane) - 1ull))) : -1;
        base += __popcll(m);
        const int last = nbatches - 1 - b0;  // lane of the chunk's last batch
        carry = __shfl(sig, last < 63 ? last : 63);
    }
    if (lane == 0) {
        row_count[row] = base;
        if (ru != MI_GATE_NONE)
            carried[row] = static_cast<uint8_t>(carry);
    }
}

// Launch 2.  mi::launch_row_scan (poststage.hip): exclusive scan of the row counts into row_first, and the two counts.

// Launch 3.  One workgroup per (row, batch) on a 1-D grid; a block that does not travel, or whose place is beyond the capacity,
// returns at once.  500 float4 of audio, 1000 of raw I/Q where the row has them (k_move_blocks of gather.hip).
__global__ __launch_bounds__(256) void k_gate_copy(const int* __restrict__ rank, const uint32_t* __restrict__ row_first, const uint8_t* __restrict__ has_iq,
                                                   const float* __restrict__ wave, const size_t row_stride, const float* __restrict__ iq,
                                                   const size_t iq_row_stride, const int nbatches, const uint32_t max_blocks, float* __restrict__ blocks,
                                                   float* __restrict__ iq_blocks, mi_gate_block* __restrict__ index) {
    const uint32_t row = blockIdx.x / static_cast<uint32_t>(nbatches), b = blockIdx.x % static_cast<uint32_t>(nbatches);
    const int r = rank[blockIdx.x];
    if (r < 0)
        return;
    const uint32_t k = row_first[row] + static_cast<uint32_t>(r);
    if (k >= max_blocks)
        return;
    const float4* s = reinterpret_cast<const float4*>(wave + static_cast<size_t>(row) * row_stride + static_cast<size_t>(b) * mi::kWaveBatch);
    float4* d = reinterpret_cast<float4*>(blocks + static_cast<size_t>(k) * mi::kWaveBatch);
    for (int i = threadIdx.x; i < mi::kWaveBatch / 4; i += blockDim.x)
        d[i] = s[i];
    if (iq && has_iq[row]) {
        const float4* si = reinterpret_cast<const float4*>(iq + static_cast<size_t>(row) * iq_row_stride + static_cast<size_t>(b) * (2 * mi::kWaveBatch));
        float4* di = reinterpret_cast<float4*>(iq_blocks + static_cast<size_t>(k) * (2 * mi::kWaveBatch));
        for (int i = threadIdx.x; i < mi::kWaveBatch / 2; i += blockDim.x)
            di[i] = si[i];
    }
    if (threadIdx.x == 0)
        *reinterpret_cast<uint2*>(index + k) = make_uint2(row, b);
}

bool rules_valid(const uint8_t* row_rule, int rows) {
    for (int r = 0; r < rows; ++r)
        if (row_rule[r] > MI_GATE_ALL)
            return false;
    return true;
}

}  // namespace

extern "C" {

int mi_outgate_create(const uint8_t* row_rule, const uint8_t* row_has_iq, int rows, int max_batches, size_t max_blocks, int gpu, mi_outgate** out) {
    if (!row_rule || !out)
        return fail(MI_ERR_INVALID, "NULL argument");
    if (const int rc = mi::batch_geometry_ok(kName, rows, max_batches))
        return rc;
    const size_t all = static_cast<size_t>(rows) * static_cast<size_t>(max_batches);
    if (!rules_valid(row_rule, rows))
        return fail(MI_ERR_INVALID, "gate rule out of range 0..3");
    if (const int rc = mi::check_gpu(gpu, "no HIP device: the output gate runs on the GPU only"))
        return rc;
    const size_t n = static_cast<size_t>(rows);
    const std::vector<uint8_t> iq = row_has_iq ? mi::as_flags(row_has_iq, n) : std::vector<uint8_t>(n, 0);
    mi_outgate* g = new mi_outgate();
    g->gpu = gpu;
    g->rows = rows;
    g->max_batches = max_batches;
    g->max_blocks = static_cast<uint32_t>(max_blocks && max_blocks < all ? max_blocks : all);  // (no call has more blocks than `all`)
    g->any_iq = std::find(iq.begin(), iq.end(), 1) != iq.end();
    if (hipSetDevice(gpu) != hipSuccess || dalloc(g->d_rule, n) != hipSuccess || dalloc(g->d_has_iq, n) != hipSuccess ||
        dalloc(g->d_carried, n) != hipSuccess || dalloc(g->d_rank, all) != hipSuccess || dalloc(g->d_row_count, n) != hipSuccess ||
        hipHostMalloc(reinterpret_cast<void**>(g->h_count.put()), 2 * sizeof(uint32_t)) != hipSuccess ||
        hipMemcpy(g->d_rule, row_rule, n, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(g->d_has_iq, iq.data(), n, hipMemcpyHostToDevice) != hipSuccess || hipMemset(g->d_carried, 0, n) != hipSuccess ||
        hipDeviceSynchronize() != hipSuccess) {
        delete g;
        return fail(MI_ERR_HIP, "output gate: device allocation failed");
    }
    *out = g;
    return MI_OK;
}

void mi_outgate_destroy(mi_outgate* g) {
    mi::destroy(g);
}

int mi_outgate_set_rules(mi_outgate* g, const uint8_t* row_rule) {
    if (!g || !row_rule)
        return fail(MI_ERR_INVALID, "NULL argument");
    if (!rules_valid(row_rule, g->rows))
        return fail(MI_ERR_INVALID, "gate rule out of range 0..3");
    // (a call still queued reads the rules it was made with)
    if (!mi::sync_copy(g->gpu, g->d_rule, row_rule, static_cast<size_t>(g->rows), hipMemcpyHostToDevice))
        return fail(MI_ERR_HIP, "output gate: uploading the rules failed");
    return MI_OK;
}

int mi_outgate_process_device(mi_outgate* g, const float* d_waveout, size_t row_stride, const float* d_iq_out, size_t iq_row_stride, const char* d_axc,
                              size_t axc_stride, int nbatches, float* d_blocks, float* d_iq_blocks, mi_gate_block* d_index, uint32_t* d_row_first,
                              uint32_t* d_count, void* hip_stream) {
    if (!g || !d_waveout || !d_axc || !d_blocks || !d_index || !d_row_first || !d_count)
        return fail(MI_ERR_INVALID, "NULL argument");
    if (nbatches < 1 || nbatches > g->max_batches)
        return fail(MI_ERR_INVALID, "nbatches outside 1 .. max_batches");
    const size_t n = static_cast<size_t>(nbatches) * mi::kWaveBatch;
    if (row_stride < n || axc_stride < static_cast<size_t>(nbatches) || (d_iq_out && iq_row_stride < 2 * n))
        return fail(MI_ERR_INVALID, "a row stride is shorter than the call");
    if (d_iq_out && g->any_iq && !d_iq_blocks)
        return fail(MI_ERR_INVALID, "rows with raw I/Q need a d_iq_blocks buffer");
    if (row_stride % 4 != 0 || !aligned(d_waveout, 16) || !aligned(d_blocks, 16) ||
        (d_iq_out && (iq_row_stride % 4 != 0 || !aligned(d_iq_out, 16) || !aligned(d_iq_blocks, 16))) || !aligned(d_index, 8) ||
        !aligned(d_row_first, 4) || !aligned(d_count, 4))
        return fail(MI_ERR_INVALID, "audio and I/Q buffers must be 16-byte aligned with row strides that are multiples of 4 floats; index 8-byte aligned");
    if (hipSetDevice(g->gpu) != hipSuccess)
        return fail(MI_ERR_HIP, "hipSetDevice failed");
    hipStream_t q = static_cast<hipStream_t>(hip_stream);
    g->timing.stamp(0, q);
    const unsigned groups = static_cast<unsigned>((g->rows + kRowsPerGroup - 1) / kRowsPerGroup);
    hipLaunchKernelGGL(k_gate_rank, dim3(groups), dim3(256), 0, q, g->d_rule.get(), g->d_carried.get(), d_axc, axc_stride, g->rows, nbatches, g->d_rank.get(),
                       g->d_row_count.get());
    g->timing.stamp(1, q);
    mi::launch_row_scan(q, g->d_row_count, g->rows, g->max_blocks, d_row_first, d_count);
    g->timing.stamp(2, q);
    const float* iq = g->any_iq ? d_iq_out : nullptr;
    hipLaunchKernelGGL(k_gate_copy, dim3(static_cast<unsigned>(g->rows) * static_cast<unsigned>(nbatches)), dim3(256), 0, q, g->d_rank.get(), d_row_first,
                       g->d_has_iq.get(), d_waveout, row_stride, iq, iq_row_stride, nbatches, g->max_blocks, d_blocks, d_iq_blocks, d_index);
    g->timing.stamp(3, q);
    if (hipGetLastError() != hipSuccess)
        return fail(MI_ERR_HIP, "output gate kernel launch failed");
    g->called = true;
    g->last_blocks = d_blocks;
    g->last_iq_blocks = iq ? d_iq_blocks : nullptr;
    g->last_index = d_index;
    g->last_row_first = d_row_first;
    g->last_count = d_count;
    return MI_OK;
}

int mi_outgate_download(mi_outgate* g, void* hip_stream, float* blocks, float* iq_blocks, mi_gate_block* index, uint32_t* row_first, uint32_t* count) {
    if (!g || !count)
        return fail(MI_ERR_INVALID, "NULL argument");
    if (!g->last_count)
        return fail(MI_ERR_INVALID, "no mi_outgate_process_device call to download");
    if (iq_blocks && !g->last_iq_blocks)
        return fail(MI_ERR_INVALID, "the last call packed no raw I/Q");
    hipStream_t q = static_cast<hipStream_t>(hip_stream);
    if (!mi::land_counts(g->gpu, q, g->h_count, g->last_count, count))
        return fail(MI_ERR_HIP, "output gate: reading the counts failed");
    const size_t k = count[1];
    bool ok = true;
    if (blocks && k)
        ok = ok && hipMemcpyAsync(blocks, g->last_blocks, k * mi::kWaveBatch * sizeof(float), hipMemcpyDeviceToHost, q) == hipSuccess;
    if (iq_blocks && k)
        ok = ok && hipMemcpyAsync(iq_blocks, g->last_iq_blocks, k * 2 * mi::kWaveBatch * sizeof(float), hipMemcpyDeviceToHost, q) == hipSuccess;
    if (index && k)
        ok = ok && hipMemcpyAsync(index, g->last_index, k * sizeof(mi_gate_block), hipMemcpyDeviceToHost, q) == hipSuccess;
    if (row_first)
        ok = ok && hipMemcpyAsync(row_first, g->last_row_first, (static_cast<size_t>(g->rows) + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, q) == hipSuccess;
    if (!ok || hipStreamSynchronize(q) != hipSuccess)
        return fail(MI_ERR_HIP, "output gate: download failed");
    return MI_OK;
}

int mi_outgate_set_timing(mi_outgate* g, int on) {
    return mi::set_timing(g, on);
}

int mi_outgate_last_launch_ms(mi_outgate* g, float* ms) {
    return mi::last_launch_ms(g, ms, "mi_outgate_process_device");
}

size_t mi_outgate_state_size(const mi_outgate* g) {
    return mi::state_size(g, &mi_outgate::d_carried);
}

int mi_outgate_get_state(mi_outgate* g, void* buf, size_t len) {
    return mi::get_state(kName, g, &mi_outgate::d_carried, buf, len);
}

int mi_outgate_set_state(mi_outgate* g, const void* buf, size_t len) {  // (its own body: the blob is taken as truth values, not as it is)
    if (!g || !buf || len != static_cast<size_t>(g->rows))
        return fail(MI_ERR_INVALID, "output gate state: NULL argument or wrong length");
    if (!mi::sync_copy(g->gpu, g->d_carried, mi::as_flags(buf, len).data(), len, hipMemcpyHostToDevice))
        return fail(MI_ERR_HIP, "output gate: writing the state failed");
    return MI_OK;
}

}  // extern "C"
