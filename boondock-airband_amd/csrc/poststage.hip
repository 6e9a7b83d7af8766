// poststage.hip -- the row scan the output gate and the transmission splitter share: launch 2 of either.
#include "poststage.hpp"

namespace {

using mi::kScanTile;

// Exclusive scan of the row counts, one workgroup walking tiles of 256 rows, and the two counts.
__global__ __launch_bounds__(kScanTile) void k_row_scan(const uint32_t* __restrict__ row_count, const int rows, const uint32_t cap,
                                                        uint32_t* __restrict__ row_first, uint32_t* __restrict__ count) {
    __shared__ uint32_t wave_sum[kScanTile / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    uint32_t running = 0;
    for (int r0 = 0; r0 < rows; r0 += kScanTile) {
        const int r = r0 + t;
        const uint32_t c = r < rows ? row_count[r] : 0u;
        uint32_t incl = c;
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d);
            if (lane >= d)
                incl += up;
        }
        if (lane == 63)
            wave_sum[wave] = incl;
        __syncthreads();
        uint32_t before = 0, tile = 0;
        for (int w = 0; w < kScanTile / 64; ++w) {
            const uint32_t s = wave_sum[w];
            before += w < wave ? s : 0u;
            tile += s;
        }
        if (r < rows)
            row_first[r] = running + before + incl - c;
        running += tile;
        __syncthreads();  // wave_sum is rewritten by the next tile
    }
    if (t == 0) {
        row_first[rows] = running;
        count[0] = running;
        count[1] = running < cap ? running : cap;
    }
}

}  // namespace

void mi::launch_row_scan(hipStream_t stream, const uint32_t* row_count, int rows, uint32_t cap, uint32_t* row_first, uint32_t* count) {
    hipLaunchKernelGGL(k_row_scan, dim3(1), dim3(kScanTile), 0, stream, row_count, rows, cap, row_first, count);
}
