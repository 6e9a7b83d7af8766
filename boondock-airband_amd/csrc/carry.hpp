// carry.hpp -- the device side of a stage that carries samples from call to call (pcm.hip, vband.hip, limit.hip, selcal.hip, acars.hip, same.hip, elt.hip, ax25.hip, pocsag.hip): a row's state is
// the last kHistory input samples of its last call, oldest first, and a block is staged behind a LEAD of kLead = kHistory + 2 floats --
// two that no output reaches, then the history -- so that the lead is whole float4 of the row's previous batch wherever there is one.
// (k_limit stages its lead with the text of load_lead4 written out: DESIGN.md section 6.)
#pragma once
#include <hip/hip_runtime.h>

#include "poststage.hpp"

namespace mi {

// float4 q of what is staged for the block at `blk`: the lead's out of the row's previous batch, or out of the carried samples at the
// call's first batch, the block's own behind them.  RowState: { float x[kLead - 2]; }.
template <int kLead, class RowState>
__device__ __forceinline__ float4 load_lead4(const float* blk, const RowState& carried, const int q, const bool first_batch) {
    static_assert(kLead % 4 == 0 && kLead <= kWaveBatch, "the lead is whole float4 inside the previous batch");
    static_assert(sizeof(RowState::x) == (kLead - 2) * sizeof(float) && alignof(RowState) % 4 == 0 && sizeof(RowState) % 8 == 0,
                  "the history is the lead less its first two floats, in whole float2");
    float4 v;
    if (q >= kLead / 4 || !first_batch) {
        v = reinterpret_cast<const float4*>(blk - kLead)[q];
    } else {  // floats 4q .. 4q + 3 of the lead are carried samples 4q - 2 .. 4q + 1
        const float* const c = carried.x + 4 * q;
        const float2 a = q ? *reinterpret_cast<const float2*>(c - 2) : make_float2(0.0f, 0.0f);
        const float2 b = *reinterpret_cast<const float2*>(c);
        v = make_float4(a.x, a.y, b.x, b.y);
    }
    return v;
}

// The launch behind a stage's main one in the stream, which read the old ones: the last kHistory input samples of the call are an
// enabled row's new carried samples.  One wave per row where the history fits one, else one workgroup per row.
template <int kHistory, class RowState>
__global__ __launch_bounds__(256) void k_carry_tails(const uint8_t* __restrict__ enabled, const float* __restrict__ wave, const size_t row_stride,
                                                     const uint32_t rows, const uint32_t nbatches, RowState* __restrict__ state) {
    static_assert(sizeof(RowState::x) == kHistory * sizeof(float) && kHistory <= kWaveBatch, "the blob begins with the history");
    if constexpr (kHistory <= 64) {
        const uint32_t row = blockIdx.x * kRowsPerGroup + (threadIdx.x >> 6), j = threadIdx.x & 63;
        if (row >= rows || j >= kHistory || !enabled[row])
            return;
        state[row].x[j] = wave[static_cast<size_t>(row) * row_stride + static_cast<size_t>(nbatches) * kWaveBatch - kHistory + j];
    } else {
        const uint32_t row = blockIdx.x;
        if (row >= rows || !enabled[row])
            return;
        const float* const tail = wave + static_cast<size_t>(row) * row_stride + static_cast<size_t>(nbatches) * kWaveBatch - kHistory;
        for (int j = threadIdx.x; j < kHistory; j += 256)
            state[row].x[j] = tail[j];
    }
}

template <int kHistory, class RowState>
void launch_carry_tails(hipStream_t q, const uint8_t* enabled, const float* wave, size_t row_stride, unsigned rows, int nbatches, RowState* state) {
    const unsigned grid = kHistory <= 64 ? (rows + kRowsPerGroup - 1) / kRowsPerGroup : rows;
    hipLaunchKernelGGL((k_carry_tails<kHistory, RowState>), dim3(grid), dim3(256), 0, q, enabled, wave, row_stride, rows, static_cast<uint32_t>(nbatches),
                       state);
}

}  // namespace mi
