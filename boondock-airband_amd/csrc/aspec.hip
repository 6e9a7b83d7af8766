// aspec.hip -- the audio spectrum stage: a 2048-point power spectrum of every block the output gate lets travel, reduced to one
// record per block, and one mean spectrum per row.  What a channel's `notch` key (config.cpp:388-392, 519-567; filters.cpp:30-64)
// should hold is read off that mean by mi_aspec_notch_host.  The window, the FFT, the band and the order of every sum are in
// include/mi_airband.h.  A post-stage of its own like the PCM stage: one launch, or two, on the caller's stream, no atomics, no state.
// It reads the gate's index, row starts and counts where the gate left them, in device memory.  mi_aspec_plan_host
// (poststage_host.cpp) is the host twin.  The handle's base and the bodies of the entry points every stage repeats are in poststage.hpp.
//
// Compile with -ffp-contract=off (the FFT spec).
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/mi_airband.h"
#include "fft_radix8.hpp"
#include "poststage.hpp"

constexpr char kName[] = "audio spectrum stage";

struct mi_aspec : mi::BatchStage {
    mi_aspec() : BatchStage(kName, 2) {}
    uint32_t max_blocks = 0;
    mi::AspecBand band{};
    mi::DevBuf<float> d_window;       // [2000]
    mi::DevBuf<float> d_tw;           // [1024] x {re, im}
    mi::PinnedBuf<uint32_t> h_count;  // [2], landing place of the counts in mi_aspec_download
    // what the last mi_aspec_process_device was given (what mi_aspec_download reads)
    const mi_aspec_record* last_records = nullptr;
    const float* last_power = nullptr;
    const float* last_row_mean = nullptr;
    const uint32_t* last_row_blocks = nullptr;
    const uint32_t* last_count = nullptr;
};

namespace mi {
namespace {

constexpr int kL = MI_ASPEC_FFT_LOG;
using Gm = FftGeom<kL>;
constexpr int kThreads = Gm::TPF;         // 256: one FFT per workgroup
constexpr int kBatch = kWaveBatch;        // 2000 floats = 500 float4
constexpr int kBins = MI_ASPEC_BINS;
constexpr int kPerLane = kBins / kThreads;  // bins tau + 256 j, j = 0 .. 3
static_assert(Gm::BLOCK == kThreads && Gm::F == 1 && kBatch % 4 == 0 && kBatch / 4 <= 2 * kThreads && Gm::N / 4 == 2 * kThreads && kBins % kThreads == 0,
              "one FFT a workgroup; a lane loads two float4 of the padded block");

// The reductions' working set lies over the exchange slot, which is dead once every lane holds its bins.
struct Fold {
    double acc[kThreads];
    float pk[kThreads];
    uint32_t pb[kThreads];
};
static_assert(sizeof(Fold) <= sizeof(float2) * Gm::XN, "the reductions fit the exchange slot");

// Launch 1.  One workgroup per block k of the index (a workgroup strides on where the grid is shorter than the count).  The block's
// 500 float4 times the window's go into LDS as u[0 .. 2047] with the 48 zeros behind them; lane tau takes u at the bit-reversed places
// of 8 tau .. 8 tau + 7 as (u, 0.0f), runs pass 0 in registers and the three later passes through the exchange slot (the passes span
// the four waves: fft_sync<11> is the barrier).  Then the lane forms P of the bins tau + 256 j, stores them to the power row, one
// coalesced float per lane and j, and leaves them in LDS over u; the three reductions run in the order of the definition.
__global__ __launch_bounds__(kThreads) void k_aspec_block(const float* __restrict__ wave, const size_t row_stride, const uint32_t rows, const uint32_t nbatches,
                                                          const mi_gate_block* __restrict__ index, const uint32_t* __restrict__ count,
                                                          const uint32_t max_blocks, const float* __restrict__ window, const float* __restrict__ twf,
                                                          const uint32_t lo, const uint32_t hi, mi_aspec_record* __restrict__ records,
                                                          float* __restrict__ power) {
    __shared__ __align__(16) float2 xch[Gm::XN];
    __shared__ __align__(16) float u[Gm::N];  // the windowed block, then P[0 .. 1023]
    Fold& fold = *reinterpret_cast<Fold*>(xch);
    const int tau = threadIdx.x;

    // ---- per-lane constants: where the lane's 8 inputs lie, its window coefficients, its twiddles ----
    const int nrev = static_cast<int>(__brev(static_cast<unsigned>(tau)) >> (32 - (kL - 3)));
    int nidx[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int rev3 = ((r & 1) << 2) | (r & 2) | ((r >> 2) & 1);
        nidx[r] = rev3 * kThreads + nrev;  // natural sample index = bitrev_11(8 tau + r)
    }
    const float4 w0 = reinterpret_cast<const float4*>(window)[tau];
    const float4 w1 = tau + kThreads < kBatch / 4 ? reinterpret_cast<const float4*>(window)[tau + kThreads] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const float2* tw = reinterpret_cast<const float2*>(twf);
    const float2 w8 = tw[Gm::N / 8], w83 = tw[3 * Gm::N / 8];
    float2 twr[Gm::NPASS][7];
    load_all_tw<kL, 1>(tau, tw, twr);

    const uint32_t stored = count[1], limit = stored < max_blocks ? stored : max_blocks;
    for (uint32_t k = blockIdx.x; k < limit; k += gridDim.x) {  // (the same trips for the whole workgroup)
        const uint2 e = *reinterpret_cast<const uint2*>(index + k);
        const uint32_t row = e.x, batch = e.y;
        float* const prow = power ? power + static_cast<size_t>(k) * kBins : nullptr;
        if (row >= rows || batch >= nbatches) {  // (the whole workgroup) not an entry of this call: nothing read
            if (prow)
                reinterpret_cast<float4*>(prow)[tau] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (tau == 0)
                records[k] = mi_aspec_record{row, batch, 0xFFFFFFFFu, 0.0f, 0.0, 0.0};
            continue;
        }
        const float4* const blk = reinterpret_cast<const float4*>(wave + static_cast<size_t>(row) * row_stride + static_cast<size_t>(batch) * kBatch);
        {
            const float4 a = blk[tau];
            reinterpret_cast<float4*>(u)[tau] = make_float4(__fmul_rn(a.x, w0.x), __fmul_rn(a.y, w0.y), __fmul_rn(a.z, w0.z), __fmul_rn(a.w, w0.w));
            float4 b = make_float4(0.0f, 0.0f, 0.0f, 0.0f);  // float4 500 .. 511: u[2000 .. 2047]
            if (tau + kThreads < kBatch / 4) {
                const float4 v = blk[tau + kThreads];
                b = make_float4(__fmul_rn(v.x, w1.x), __fmul_rn(v.y, w1.y), __fmul_rn(v.z, w1.z), __fmul_rn(v.w, w1.w));
            }
            reinterpret_cast<float4*>(u)[tau + kThreads] = b;
        }
        __syncthreads();
        float2 x[8];
#pragma unroll
        for (int r = 0; r < 8; ++r)
            x[r] = make_float2(u[nidx[r]], 0.0f);
        pass0(x, w8, w83);
#pragma unroll
        for (int r = 0; r < 8; ++r)
            xch[xpad(tau * 8 + r)] = x[r];
        fft_sync<kL>();
        later_passes<kL, 1>(x, twr, xch, tau);
        // natural-order spectrum now sits in xch (behind the last pass's barrier); u is dead since the barrier behind pass 0
        float p[kPerLane];
#pragma unroll
        for (int j = 0; j < kPerLane; ++j) {
            const float2 v = xch[xpad(tau + j * kThreads)];
            p[j] = __fadd_rn(__fmul_rn(v.x, v.x), __fmul_rn(v.y, v.y));
            u[tau + j * kThreads] = p[j];
            if (prow)
                prow[tau + j * kThreads] = p[j];
        }
        __syncthreads();  // every lane has read its bins: the exchange slot becomes the reductions'
        {
            double acc = 0.0;
            float pk = -1.0f;  // below every P: a lane without a bin in the band loses against any lane that has one
            uint32_t pb = 0xFFFFFFFFu;
#pragma unroll
            for (int j = 0; j < kPerLane; ++j) {
                const uint32_t bin = static_cast<uint32_t>(tau + j * kThreads);
                if (bin >= lo && bin <= hi) {
                    acc += static_cast<double>(p[j]);
                    if (p[j] > pk) {  // bins ascending: the lowest bin of equal ones stays
                        pk = p[j];
                        pb = bin;
                    }
                }
            }
            fold.acc[tau] = acc;
            fold.pk[tau] = pk;
            fold.pb[tau] = pb;
        }
        __syncthreads();
        for (int d = kThreads / 2; d >= 1; d >>= 1) {
            if (tau < d) {
                fold.acc[tau] += fold.acc[tau + d];
                const float pk = fold.pk[tau + d];
                const uint32_t pb = fold.pb[tau + d];
                if (pk > fold.pk[tau] || (pk == fold.pk[tau] && pb < fold.pb[tau])) {
                    fold.pk[tau] = pk;
                    fold.pb[tau] = pb;
                }
            }
            __syncthreads();
        }
        if (tau == 0) {
            const uint32_t peak = fold.pb[0];  // lo <= peak <= hi: the band holds a bin, and P >= 0 > -1
            const uint32_t first = peak - lo < MI_ASPEC_LINE_HALF ? lo : peak - MI_ASPEC_LINE_HALF;
            const uint32_t last = hi - peak < MI_ASPEC_LINE_HALF ? hi : peak + MI_ASPEC_LINE_HALF;
            double line = 0.0;
            for (uint32_t bin = first; bin <= last; ++bin)
                line += static_cast<double>(u[bin]);
            records[k] = mi_aspec_record{row, batch, peak, fold.pk[0], fold.acc[0], line};
        }
        __syncthreads();  // (the next trip writes the LDS this one read)
    }
}

// Launch 2, only where a row mean is wanted: one thread per (row, bin) walks the row's stored power rows in order.
__global__ __launch_bounds__(kThreads) void k_aspec_rows(const float* __restrict__ power, const uint32_t* __restrict__ row_first,
                                                         const uint32_t* __restrict__ count, const uint32_t max_blocks, float* __restrict__ row_mean,
                                                         uint32_t* __restrict__ row_blocks) {
    const uint32_t row = blockIdx.x, bin = blockIdx.y * kThreads + threadIdx.x;
    const uint32_t stored = count[1] < max_blocks ? count[1] : max_blocks;
    const uint32_t a = row_first[row], b = row_first[row + 1];
    const uint32_t first = a < stored ? a : stored, last = b < stored ? b : stored;
    const uint32_t n = last > first ? last - first : 0;
    double s = 0.0;
    for (uint32_t k = first; k < first + n; ++k)
        s += static_cast<double>(power[static_cast<size_t>(k) * kBins + bin]);
    row_mean[static_cast<size_t>(row) * kBins + bin] = n ? static_cast<float>(s / static_cast<double>(n)) : 0.0f;
    if (bin == 0)
        row_blocks[row] = n;
}

}  // namespace
}  // namespace mi

using mi::aligned;
using mi::fail;

extern "C" {

int mi_aspec_create(const mi_aspec_cfg* cfg, int rows, int max_batches, size_t max_blocks, int gpu, mi_aspec** out) {
    if (!out)
        return fail(MI_ERR_INVALID, "NULL argument");
    *out = nullptr;
    mi::AspecBand band;
    if (const int rc = mi::aspec_band(cfg, &band))
        return rc;
    if (const int rc = mi::batch_geometry_ok(kName, rows, max_batches))
        return rc;
    std::vector<float> tw, window(mi::kWaveBatch);
    if (const int rc = mi::aspec_twiddles(tw))
        return rc;
    mi::aspec_window(window.data());
    if (const int rc = mi::check_gpu(gpu, "no HIP device: the audio spectrum stage runs on the GPU only"))
        return rc;
    mi_aspec* a = new mi_aspec();
    a->gpu = gpu;
    a->rows = rows;
    a->max_batches = max_batches;
    a->band = band;
    const size_t all = static_cast<size_t>(rows) * static_cast<size_t>(max_batches);
    a->max_blocks = static_cast<uint32_t>(max_blocks && max_blocks < all ? max_blocks : all);  // (the gate stores no more blocks than `all`)
    if (hipSetDevice(gpu) != hipSuccess || dalloc_copy(a->d_window, window) != hipSuccess || dalloc_copy(a->d_tw, tw) != hipSuccess ||
        hipHostMalloc(reinterpret_cast<void**>(a->h_count.put()), 2 * sizeof(uint32_t)) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
        delete a;
        return fail(MI_ERR_HIP, "audio spectrum stage: device allocation failed");
    }
    *out = a;
    return MI_OK;
}

void mi_aspec_destroy(mi_aspec* a) {
    mi::destroy(a);
}

int mi_aspec_process_device(mi_aspec* a, const float* d_waveout, size_t row_stride, int nbatches, const mi_gate_block* d_index, const uint32_t* d_row_first,
                            const uint32_t* d_count, mi_aspec_record* d_records, float* d_power, float* d_row_mean, uint32_t* d_row_blocks,
                            void* hip_stream) {
    if (!a || !d_waveout || !d_index || !d_count || !d_records)
        return fail(MI_ERR_INVALID, "NULL argument");
    if (nbatches < 1 || nbatches > a->max_batches)
        return fail(MI_ERR_INVALID, "nbatches outside 1 .. max_batches");
    if (row_stride < static_cast<size_t>(nbatches) * mi::kWaveBatch)
        return fail(MI_ERR_INVALID, "a row stride is shorter than the call");
    if ((d_row_mean != nullptr) != (d_row_blocks != nullptr) || (d_row_mean && (!d_power || !d_row_first)))
        return fail(MI_ERR_INVALID, "audio spectrum stage: a row mean needs the power rows, the row starts and the row counts");
    if (row_stride % 4 != 0 || !aligned(d_waveout, 16) || !aligned(d_index, 8) || !aligned(d_count, 4) || !aligned(d_row_first, 4) || !aligned(d_records, 8) ||
        !aligned(d_power, 16) || !aligned(d_row_mean, 16) || !aligned(d_row_blocks, 4))
        return fail(MI_ERR_INVALID,
                    "the audio buffer, the power rows and the row means must be 16-byte aligned with a row stride that is a multiple of 4 floats; the index "
                    "and the records 8-byte aligned");
    if (hipSetDevice(a->gpu) != hipSuccess)
        return fail(MI_ERR_HIP, "hipSetDevice failed");
    hipStream_t q = static_cast<hipStream_t>(hip_stream);
    const unsigned rows = static_cast<unsigned>(a->rows);
    const uint64_t call = static_cast<uint64_t>(rows) * static_cast<uint64_t>(nbatches);  // the most blocks a gate stores in this call
    const unsigned grid = static_cast<unsigned>(call < a->max_blocks ? call : a->max_blocks);
    a->timing.stamp(0, q);
    hipLaunchKernelGGL(mi::k_aspec_block, dim3(grid), dim3(mi::kThreads), 0, q, d_waveout, row_stride, rows, static_cast<uint32_t>(nbatches), d_index, d_count,
                       a->max_blocks, a->d_window.get(), a->d_tw.get(), a->band.lo, a->band.hi, d_records, d_power);
    a->timing.stamp(1, q);
    if (d_row_mean)
        hipLaunchKernelGGL(mi::k_aspec_rows, dim3(rows, mi::kBins / mi::kThreads), dim3(mi::kThreads), 0, q, d_power, d_row_first, d_count, a->max_blocks,
                           d_row_mean, d_row_blocks);
    a->timing.stamp(2, q);
    if (hipGetLastError() != hipSuccess)
        return fail(MI_ERR_HIP, "audio spectrum stage kernel launch failed");
    a->called = true;
    a->last_records = d_records;
    a->last_power = d_power;
    a->last_row_mean = d_row_mean;
    a->last_row_blocks = d_row_blocks;
    a->last_count = d_count;
    return MI_OK;
}

int mi_aspec_download(mi_aspec* a, void* hip_stream, mi_aspec_record* records, float* power, float* row_mean, uint32_t* row_blocks, uint32_t* count) {
    if (!a || !count)
        return fail(MI_ERR_INVALID, "NULL argument");
    if (!a->last_count)
        return fail(MI_ERR_INVALID, "no mi_aspec_process_device call to download");
    if ((power && !a->last_power) || ((row_mean || row_blocks) && !a->last_row_mean))
        return fail(MI_ERR_INVALID, "audio spectrum stage: the last call wrote no power rows or no row mean");
    hipStream_t q = static_cast<hipStream_t>(hip_stream);
    if (!mi::land_counts(a->gpu, q, a->h_count, a->last_count, count))
        return fail(MI_ERR_HIP, "audio spectrum stage: reading the counts failed");
    count[1] = count[1] < a->max_blocks ? count[1] : a->max_blocks;
    const size_t k = count[1], rows = static_cast<size_t>(a->rows);
    bool ok = true;
    if (records && k)
        ok = ok && hipMemcpyAsync(records, a->last_records, k * sizeof(mi_aspec_record), hipMemcpyDeviceToHost, q) == hipSuccess;
    if (power && k)
        ok = ok && hipMemcpyAsync(power, a->last_power, k * MI_ASPEC_BINS * sizeof(float), hipMemcpyDeviceToHost, q) == hipSuccess;
    if (row_mean)
        ok = ok && hipMemcpyAsync(row_mean, a->last_row_mean, rows * MI_ASPEC_BINS * sizeof(float), hipMemcpyDeviceToHost, q) == hipSuccess;
    if (row_blocks)
        ok = ok && hipMemcpyAsync(row_blocks, a->last_row_blocks, rows * sizeof(uint32_t), hipMemcpyDeviceToHost, q) == hipSuccess;
    if (!ok || hipStreamSynchronize(q) != hipSuccess)
        return fail(MI_ERR_HIP, "audio spectrum stage: download failed");
    return MI_OK;
}

int mi_aspec_set_timing(mi_aspec* a, int on) {
    return mi::set_timing(a, on);
}

int mi_aspec_last_launch_ms(mi_aspec* a, float* ms) {
    return mi::last_launch_ms(a, ms, "mi_aspec_process_device");
}

}  // extern "C"
