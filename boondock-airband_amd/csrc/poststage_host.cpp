// poststage_host.cpp -- the host twins of the output gate and the transmission splitter: what the device stages compute, from flags
// (and audio) the caller already has.  Plain C++, no device needed.  Each twin states its rule on its own: tests compare it with the
// device walk and with the Python model, which are the other two statements of the same rule.  The band survey's host half lives here
// too: mi_survey_bin_range, the plan's bin rule read backwards; the channel finder's twin, mi_occupancy_plan_host; and the channel probe's host half
// (target list, features, classification); the CTCSS tone finder's twin mi_tones_plan_host with its tone table and vote; the PCM
// stage's twin mi_pcm_plan_host with its taps and WAV headers; the audio spectrum stage's twin mi_aspec_plan_host with its window,
// band and the notch vote; the voice band stage's twin mi_vband_plan_host with its settings, taps and classes; the peak limiter
// stage's twin mi_limit_plan_host with its settings and the pregain helper; the noise reduction stage's twin mi_denoise_plan_host
// with its settings and window; and the SELCAL decoder stage's twin mi_selcal_plan_host with its tables, settings, window and code text.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

#include "poststage.hpp"

namespace mi {

// close_if_necessary's three constants (output.cpp:356-358) in batches: d * WAVE_BATCH > seconds * WAVE_RATE
constexpr uint32_t kTxMinBatches = 1 * kWaveRate / kWaveBatch;     // 8
constexpr uint32_t kTxIdleBatches = kWaveRate / 2 / kWaveBatch;    // 4
constexpr uint32_t kTxMaxBatches = 3600 * kWaveRate / kWaveBatch;  // 28800
static_assert(1 * kWaveRate % kWaveBatch == 0 && kWaveRate / 2 % kWaveBatch == 0, "the thresholds are whole batches");

mi_tx_cfg tx_cfg_or_default(const mi_tx_cfg* cfg) {
    mi_tx_cfg c = cfg ? *cfg : mi_tx_cfg{0, 0, 0};
    c.min_batches = c.min_batches ? c.min_batches : kTxMinBatches;
    c.idle_batches = c.idle_batches ? c.idle_batches : kTxIdleBatches;
    c.max_batches = c.max_batches ? c.max_batches : kTxMaxBatches;
    return c;
}

int device_plan(const mi_device_cfg& dev, Plan& p) {
    mi_channel_cfg ch{};
    ch.freq = dev.centerfreq;
    ch.modulation = MI_MOD_AM;
    ch.squelch_snr_db = -1.0f;
    ch.ampfactor = 1.0f;
    ch.tau = -1;
    const char* msg = "";
    const int rc = build_plan(dev, &ch, 1, p, &msg);
    return rc == MI_OK ? MI_OK : fail(rc, msg);
}

}  // namespace mi

using mi::fail;

// ---- output gate, host side (include/mi_airband.h "output gate"): the index mi_outgate_process_device computes.  One pass per row in
// batch order with the row's carried flag as output_t::active (output.cpp:518-520, 560, 568-570); outgate.hip holds the device twin.
extern "C" int mi_gate_plan_host(const uint8_t* row_rule, int rows, const char* axc, size_t axc_stride, int nbatches, uint8_t* carried_inout,
                                 mi_gate_block* index, uint32_t* row_first, uint32_t* count) {
    if (!row_rule || !axc || !carried_inout || !index || !row_first || !count)
        return fail(MI_ERR_INVALID, "NULL argument");
    if (rows < 1 || nbatches < 1 || axc_stride < static_cast<size_t>(nbatches))
        return fail(MI_ERR_INVALID, "gate plan needs rows >= 1 and 1 <= nbatches <= axc_stride");
    if (static_cast<uint64_t>(rows) * static_cast<uint64_t>(nbatches) > UINT32_MAX)
        return fail(MI_ERR_INVALID, "gate plan: rows * nbatches does not fit the 32-bit block index");
    for (int r = 0; r < rows; ++r)
        if (row_rule[r] > MI_GATE_ALL)
            return fail(MI_ERR_INVALID, "gate rule out of range 0..3");
    uint32_t k = 0;
    for (int r = 0; r < rows; ++r) {
        row_first[r] = k;
        const uint8_t rule = row_rule[r];
        if (rule == MI_GATE_NONE)
            continue;
        bool active = carried_inout[r] != 0;
        for (int b = 0; b < nbatches; ++b) {
            const bool signal = axc[static_cast<size_t>(r) * axc_stride + b] != MI_NO_SIGNAL;
            if (rule == MI_GATE_ALL || signal || (rule == MI_GATE_OPEN_TRAIL && active)) {
                index[k].row = static_cast<uint32_t>(r);
                index[k].batch = static_cast<uint32_t>(b);
                ++k;
            }
            active = signal;
        }
        carried_inout[r] = active ? 1 : 0;
    }
    row_first[rows] = k;
    count[0] = count[1] = k;
    return MI_OK;
}

// ---- band survey, host side (include/mi_airband.h "band survey"): the frequencies the plan's bin rule sends to one FFT bin.
// plan.cpp states the rule as the reference does (config.cpp:669-670), in double: with d = freq + sample_rate - centerfreq and the
// INTEGER quotient q = sample_rate / fft_size, B = ceil(d / q - 1.0) and bin = B % fft_size.  d / q misses an integer by at least 1 / q
// where it is not one, far more than a double's rounding, so B = ceil(d / q) - 1 in integers: B's frequencies are d = B q + 1 .. (B + 1) q.
extern "C" int mi_survey_bin_range(const mi_device_cfg* dev, int bin, int* lo_hz, int* hi_hz) {
    if (!dev || !lo_hz || !hi_hz)
        return fail(MI_ERR_INVALID, "NULL argument");
    if (dev->fft_size_log < 8 || dev->fft_size_log > 13)
        return fail(MI_ERR_INVALID, "fft_size must be a power of two in 2^8..2^13");
    if (dev->sample_rate <= mi::kWaveRate)
        return fail(MI_ERR_INVALID, "sample_rate must be greater than WAVE_RATE");
    const int64_t n = int64_t{1} << dev->fft_size_log, sr = dev->sample_rate, q = sr / n;
    if (bin < 0 || bin >= n)
        return fail(MI_ERR_INVALID, "bin outside 0 .. fft_size - 1");
    const int64_t d_first = sr - sr / 2, d_last = sr + (sr + 1) / 2 - 1;  // the band [centerfreq - sample_rate / 2, centerfreq + sample_rate / 2)
    int64_t best_lo = 0, best_len = 0;
    for (int64_t b = bin; b * q + 1 <= d_last; b += n) {  // the band holds fft_size + 1 values of B or a few more: at most two pieces
        const int64_t lo = std::max(b * q + 1, d_first), hi = std::min((b + 1) * q, d_last);
        if (hi - lo + 1 > best_len) {
            best_lo = lo;
            best_len = hi - lo + 1;
        }
    }
    if (best_len < 1)  // (every residue occurs among fft_size consecutive values of B, and the band is at least that wide)
        return fail(MI_ERR_INVALID, "no frequency of the band maps to this bin");
    *lo_hz = static_cast<int>(best_lo - sr + dev->centerfreq);
    *hi_hz = static_cast<int>(best_lo + best_len - 1 - sr + dev->centerfreq);
    return MI_OK;
}

// ---- transmission splitter, host side (include/mi_airband.h "transmission splitter"): close_if_necessary's rule in signal time,
// one row and one batch at a time, and a block's energy in the order the header defines; txsplit.hip holds the device twin.
namespace {

// sum of x * x over one block: 256 partial sums, each over float4 number t and (t < 244) number 256 + t, then the halving tree
double tx_block_energy(const float* x, float* peak) {
    double acc[256];
    float p = 0.0f;
    for (int t = 0; t < 256; ++t) {
        double a = 0.0;
        for (int f = t; f < mi::kWaveBatch / 4; f += 256)
            for (int e = 0; e < 4; ++e) {
                const float v = x[4 * f + e];
                a += static_cast<double>(v) * static_cast<double>(v);
                p = std::fabs(v) > p ? std::fabs(v) : p;
            }
        acc[t] = a;
    }
    for (int d = 128; d >= 1; d >>= 1)
        for (int t = 0; t < d; ++t)
            acc[t] += acc[t + d];
    *peak = p;
    return acc[0];
}

}  // namespace

extern "C" int mi_tx_plan_host(const mi_tx_cfg* cfg, const uint8_t* row_enabled, int rows, const char* axc, size_t axc_stride, int nbatches,
                               const float* waveout, size_t row_stride, void* state_inout, mi_tx_record* records, size_t max_records,
                               uint32_t* row_first_record, uint32_t* count) {
    if (!row_enabled || !axc || !state_inout || !records || !row_first_record || !count)
        return fail(MI_ERR_INVALID, "NULL argument");
    if (rows < 1 || nbatches < 1 || axc_stride < static_cast<size_t>(nbatches) || max_records < 1)
        return fail(MI_ERR_INVALID, "tx plan needs rows >= 1, 1 <= nbatches <= axc_stride and max_records >= 1");
    if (waveout && row_stride < static_cast<size_t>(nbatches) * mi::kWaveBatch)
        return fail(MI_ERR_INVALID, "a row stride is shorter than the call");
    if (static_cast<uint64_t>(rows) * (static_cast<uint64_t>(nbatches) + 1) > UINT32_MAX)
        return fail(MI_ERR_INVALID, "tx plan: rows * (nbatches + 1) does not fit the 32-bit record count");
    const mi_tx_cfg c = mi::tx_cfg_or_default(cfg);
    mi::TxRowState* state = static_cast<mi::TxRowState*>(state_inout);
    for (int r = 0; r < rows; ++r)
        if (state[r].open > 1 || state[r].active > 1 || state[r].zero != 0)
            return fail(MI_ERR_INVALID, "tx plan: malformed state blob");
    constexpr uint32_t kNone = 0xFFFFFFFFu;
    uint32_t k = 0;
    for (int r = 0; r < rows; ++r) {
        row_first_record[r] = k;
        if (!row_enabled[r])
            continue;
        mi::TxRowState s = state[r];
        mi_tx_record cur{};
        bool have = false;       // `cur` describes the open file's part in this call
        uint32_t travelled = 0;  // the row's travelling blocks so far
        auto begin = [&](uint32_t flags) {
            cur = mi_tx_record{static_cast<uint32_t>(r), s.seq, travelled, 0, kNone, kNone, flags, 0.0f, 0.0};
            have = true;
        };
        auto flush = [&] {
            if (k < max_records)
                records[k] = cur;
            ++k;
            have = false;
        };
        for (int b = 0; b < nbatches; ++b) {
            const bool signal = axc[static_cast<size_t>(r) * axc_stride + b] != MI_NO_SIGNAL;
            if (s.open) {  // close_if_necessary, output.cpp:367-375
                const uint64_t d = s.clock - s.opened, i = s.clock - s.last_write;
                if (d > c.max_batches || (d > c.min_batches && i > c.idle_batches)) {
                    s.open = 0;
                    if (!have)
                        begin(1);
                    cur.close_batch = static_cast<uint32_t>(b);
                    flush();
                }
            }
            if (signal || s.active) {  // output.cpp:518-520
                if (!s.open) {         // output_file_ready, :404-414, :454
                    s.seq += 1;
                    s.open = 1;
                    s.opened = s.last_write = s.clock;
                    begin(0);
                } else if (!have) {
                    begin(1);
                }
                if (cur.nblocks == 0)
                    cur.first_batch = static_cast<uint32_t>(b);
                cur.nblocks += 1;
                travelled += 1;
                if (waveout) {
                    float p;
                    cur.energy += tx_block_energy(waveout + static_cast<size_t>(r) * row_stride + static_cast<size_t>(b) * mi::kWaveBatch, &p);
                    cur.peak = p > cur.peak ? p : cur.peak;
                }
                s.active = signal ? 1 : 0;  // :560
                s.last_write = s.clock;     // :561
            }
            s.clock += 1;
        }
        if (have)
            flush();
        state[r] = s;
    }
    row_first_record[rows] = k;
    count[0] = k;
    count[1] = k < max_records ? k : static_cast<uint32_t>(max_records);
    return MI_OK;
}

// ---- channel finder, host side (include/mi_airband.h "channel finder"): the settings both halves share, and the twin of
// occupancy.hip -- the floor by std::nth_element on a copy of the column, everything else one pass in cell or position order.
namespace mi {

int occ_settings(const mi_device_cfg* dev, const mi_occ_cfg* cfg, mi_occ_cfg* out, int* log2n) {
    mi_occ_cfg c = cfg ? *cfg : mi_occ_cfg{0, 0.0f, 0};
    if (c.floor_permille > 1000)
        return fail(MI_ERR_INVALID, "channel finder: floor_permille must be at most 1000");
    if (!std::isfinite(c.ratio) || c.ratio < 0.0f)
        return fail(MI_ERR_INVALID, "channel finder: ratio must be finite and not negative (0 = the default 3.0)");
    c.floor_permille = c.floor_permille ? c.floor_permille : 250;
    c.ratio = c.ratio != 0.0f ? c.ratio : 3.0f;  // the amplitude ratio of 9.54 dB, the reference's default squelch SNR
    c.min_cells = c.min_cells ? c.min_cells : 1;
    Plan plan;
    if (const int rc = device_plan(*dev, plan))
        return rc;
    *out = c;
    *log2n = plan.log2n;
    return MI_OK;
}

}  // namespace mi

extern "C" int mi_occupancy_plan_host(const mi_device_cfg* dev, const mi_occ_cfg* cfg, const uint8_t* stream_enabled, int nstreams, const float* mean,
                                      const float* peak, int ncells, mi_occ_bin* bins, mi_occ_candidate* cands, size_t max_candidates,
                                      uint32_t* stream_first, uint32_t* count) {
    if (!dev || !mean || !peak || !bins || !cands || !stream_first || !count)
        return fail(MI_ERR_INVALID, "NULL argument");
    if (nstreams < 1 || nstreams > 65535 || ncells < 1 || ncells >= (1 << 24))
        return fail(MI_ERR_INVALID, "channel finder needs 1 <= nstreams < 2^16 and 1 <= ncells < 2^24");
    mi_occ_cfg c;
    int log2n = 0;
    if (const int rc = mi::occ_settings(dev, cfg, &c, &log2n))
        return rc;
    bool any = false;
    for (int s = 0; s < nstreams; ++s)
        any = any || !stream_enabled || stream_enabled[s];
    if (!any)
        return fail(MI_ERR_INVALID, "channel finder: no stream enabled");
    const size_t n = size_t{1} << log2n, cells = static_cast<size_t>(ncells);
    const size_t most = static_cast<size_t>(nstreams) * n / 2;
    const size_t cap = max_candidates && max_candidates < most ? max_candidates : most;
    const size_t kth = static_cast<size_t>(static_cast<uint64_t>(ncells - 1) * c.floor_permille / 1000);
    constexpr uint32_t kNone = 0xFFFFFFFFu;
    std::vector<float> col(cells);
    uint32_t k = 0;
    for (int s = 0; s < nstreams; ++s) {
        stream_first[s] = k;
        if (stream_enabled && !stream_enabled[s])
            continue;
        const float* m = mean + static_cast<size_t>(s) * cells * n;
        const float* pk = peak + static_cast<size_t>(s) * cells * n;
        mi_occ_bin* sb = bins + static_cast<size_t>(s) * n;
        for (size_t b = 0; b < n; ++b) {
            for (size_t cell = 0; cell < cells; ++cell)
                col[cell] = m[cell * n + b];
            std::nth_element(col.begin(), col.begin() + static_cast<std::ptrdiff_t>(kth), col.end());
            mi_occ_bin r{col[kth], 0.0f, 0, kNone, kNone, 0, 0.0f, 0.0f};
            r.threshold = r.floor * c.ratio;
            bool before = false;
            for (size_t cell = 0; cell < cells; ++cell) {
                const float v = m[cell * n + b];
                const bool active = v > r.threshold;
                if (active) {
                    r.active_cells += 1;
                    r.first_cell = r.first_cell == kNone ? static_cast<uint32_t>(cell) : r.first_cell;
                    r.last_cell = static_cast<uint32_t>(cell);
                    r.runs += before ? 0 : 1;
                    r.max_mean = v > r.max_mean ? v : r.max_mean;
                    r.max_peak = pk[cell * n + b] > r.max_peak ? pk[cell * n + b] : r.max_peak;
                }
                before = active;
            }
            sb[b] = r;
        }
        // candidates: maximal runs of occupied positions, position p = (bin + n / 2) % n
        mi_occ_candidate cur{};
        bool open = false;
        for (size_t p = 0; p <= n; ++p) {
            const size_t b = (p + n / 2) % n;
            const bool occupied = p < n && sb[b].active_cells >= c.min_cells;
            if (occupied && !open) {
                cur = mi_occ_candidate{static_cast<uint32_t>(s), static_cast<uint32_t>(b), static_cast<uint32_t>(b), 0, 0, 0, 0, 0, 0.0f, 0.0f};
                open = true;
            } else if (occupied && sb[b].max_mean > sb[cur.best_bin].max_mean) {
                cur.best_bin = static_cast<uint32_t>(b);
            }
            if (occupied) {
                cur.hi_bin = static_cast<uint32_t>(b);
                cur.nbins += 1;
            } else if (open) {
                const mi_occ_bin& best = sb[cur.best_bin];
                cur.active_cells = best.active_cells;
                cur.first_cell = best.first_cell;
                cur.last_cell = best.last_cell;
                cur.max_mean = best.max_mean;
                cur.max_peak = best.max_peak;
                if (k < cap)
                    cands[k] = cur;
                ++k;
                open = false;
            }
        }
    }
    stream_first[nstreams] = k;
    count[0] = k;
    count[1] = k < cap ? k : static_cast<uint32_t>(cap);
    return MI_OK;
}

// ---- channel probe, host side (include/mi_airband.h "channel probe"): the target list from the finder's candidates, and from the
// cells of one target to the features a channel plan asks for.  probe.hip makes the cells.
extern "C" int mi_probe_targets_from_candidates(const mi_occ_candidate* cands, size_t n, mi_probe_target* out) {
    if (!cands || !out)
        return fail(MI_ERR_INVALID, "NULL argument");
    for (size_t i = 0; i < n; ++i)
        out[i] = mi_probe_target{cands[i].stream, cands[i].best_bin};
    std::sort(out, out + n, [](const mi_probe_target& a, const mi_probe_target& b) { return a.stream != b.stream ? a.stream < b.stream : a.bin < b.bin; });
    return MI_OK;
}

extern "C" int mi_probe_features_host(const mi_device_cfg* dev, int bin, const mi_probe_cell* cells, int ncells, const uint8_t* cell_mask,
                                      mi_probe_features* out) {
    if (!dev || !cells || !out)
        return fail(MI_ERR_INVALID, "NULL argument");
    if (ncells < 1)
        return fail(MI_ERR_INVALID, "channel probe: ncells must be at least 1");
    mi::Plan plan;
    if (const int rc = mi::device_plan(*dev, plan))
        return rc;
    int lo = 0, hi = 0;
    if (const int rc = mi_survey_bin_range(dev, bin, &lo, &hi))
        return rc;
    mi_probe_features f{};
    for (int c = 0; c < ncells; ++c) {
        if (cell_mask && !cell_mask[c])
            continue;
        f.s1 += cells[c].s1;
        f.s2 += cells[c].s2;
        f.r_re += cells[c].r_re;
        f.r_im += cells[c].r_im;
        f.n += cells[c].windows;
        f.pairs += cells[c].pairs;
    }
    if (f.n == 0 || f.s1 == 0.0) {
        *out = mi_probe_features{};
        return MI_OK;
    }
    const double n = static_cast<double>(f.n);
    f.cv2 = n * f.s2 / (f.s1 * f.s1) - 1.0;
    f.coherence = std::hypot(f.r_re, f.r_im) / f.s2;
    f.dphi = std::atan2(f.r_im, f.r_re);
    const double two_pi = 6.283185307179586476925286766559;
    const double fw = static_cast<double>(dev->sample_rate) / static_cast<double>(plan.hop_samples());  // windows per second
    const double f0 = f.dphi / two_pi * fw;
    const double mid = (static_cast<double>(lo) + static_cast<double>(hi)) / 2.0;
    const double centre = static_cast<double>(dev->centerfreq);
    f.carrier_hz = centre + f0 + fw * std::nearbyint((mid - centre - f0) / fw);
    *out = f;
    return MI_OK;
}

namespace mi {
// The geometric middles between the nearest AM and NFM values measured over the synthetic captures of DESIGN.md section 5g.
constexpr double kProbeCoherenceMax = 0.9314, kProbeCv2Min = 0.1005;
}  // namespace mi

extern "C" int mi_probe_classify_host(const mi_probe_features* f, const mi_probe_rule* rule, int* modulation) {
    if (!f || !modulation)
        return fail(MI_ERR_INVALID, "NULL argument");
    if (f->n == 0)
        return fail(MI_ERR_INVALID, "channel probe: no window selected, nothing to classify");
    mi_probe_rule r = rule ? *rule : mi_probe_rule{0.0, 0.0};
    if (!(r.coherence_max >= 0.0) || !(r.cv2_min >= 0.0) || !std::isfinite(r.coherence_max) || !std::isfinite(r.cv2_min))
        return fail(MI_ERR_INVALID, "channel probe: the rule's thresholds must be finite and not negative (0 = the default)");
    r.coherence_max = r.coherence_max != 0.0 ? r.coherence_max : mi::kProbeCoherenceMax;
    r.cv2_min = r.cv2_min != 0.0 ? r.cv2_min : mi::kProbeCv2Min;
    *modulation = (f->coherence < r.coherence_max || f->cv2 < r.cv2_min) ? MI_MOD_NFM : MI_MOD_AM;
    return MI_OK;
}

// ---- CTCSS tone finder, host side (include/mi_airband.h "CTCSS tone finder"): the settings both halves share, the twin of tones.hip
// -- one row, one batch and one sample at a time, the 64 lanes in the inner loop --, the tone table and the vote.
namespace mi {

constexpr uint32_t kTonesDefaultWindow = static_cast<uint32_t>(kWaveRate * 0.4);  // Squelch::set_ctcss_freq's slow window, squelch.cpp:115

uint32_t tones_window(const mi_tones_cfg* cfg) {
    const uint32_t w = cfg && cfg->window_samples ? cfg->window_samples : kTonesDefaultWindow;
    if (w < 800 || w > 64000) {
        fail(MI_ERR_INVALID, "tone finder: window_samples outside 800 .. 64000 (0 = the default 6400)");
        return 0;
    }
    return w;
}

void tones_coeffs(uint32_t window, float* coeff) {
    for (int t = 0; t < MI_TONES_LANES; ++t)
        coeff[t] = t < kStandardTones ? tone_coeff(kStandardToneHz[t], static_cast<float>(kWaveRate), static_cast<int>(window)) : 0.0f;
}

bool tones_state_ok(const TonesRowState* state, size_t rows, uint32_t window) {
    for (size_t r = 0; r < rows; ++r) {
        if (state[r].count >= window)
            return false;
        for (int t = kStandardTones; t < MI_TONES_LANES; ++t) {
            uint32_t a, b;
            std::memcpy(&a, &state[r].q1[t], 4);
            std::memcpy(&b, &state[r].q2[t], 4);
            if (a | b)
                return false;
        }
    }
    return true;
}

}  // namespace mi
static_assert(mi::kTonesDefaultWindow == 6400 && mi::kStandardTones == MI_TONES_STANDARD, "the default window and the table's length are ABI");

extern "C" int mi_tones_plan_host(const mi_tones_cfg* cfg, const uint8_t* row_enabled, int rows, const char* axc, size_t axc_stride, int nbatches,
                                  const float* waveout, size_t row_stride, void* state_inout, mi_tone_record* records, float* powers,
                                  size_t max_records, uint32_t* row_first_record, uint32_t* count) {
    if (!row_enabled || !axc || !waveout || !state_inout || !records || !row_first_record || !count)
        return fail(MI_ERR_INVALID, "NULL argument");
    if (rows < 1 || nbatches < 1 || axc_stride < static_cast<size_t>(nbatches) || max_records < 1)
        return fail(MI_ERR_INVALID, "tone plan needs rows >= 1, 1 <= nbatches <= axc_stride and max_records >= 1");
    if (row_stride < static_cast<size_t>(nbatches) * mi::kWaveBatch)
        return fail(MI_ERR_INVALID, "a row stride is shorter than the call");
    const uint32_t window = mi::tones_window(cfg);
    if (!window)
        return MI_ERR_INVALID;
    if (static_cast<uint64_t>(rows) * mi::tones_max_windows(window, static_cast<uint64_t>(nbatches)) > UINT32_MAX)
        return fail(MI_ERR_INVALID, "tone plan: the windows of the call do not fit the 32-bit record count");
    mi::TonesRowState* state = static_cast<mi::TonesRowState*>(state_inout);
    if (!mi::tones_state_ok(state, static_cast<size_t>(rows), window))
        return fail(MI_ERR_INVALID, "tone plan: malformed state blob (count >= window or a padding lane not zero)");
    float coeff[MI_TONES_LANES];
    mi::tones_coeffs(window, coeff);
    uint32_t k = 0;
    for (int r = 0; r < rows; ++r) {
        row_first_record[r] = k;
        if (!row_enabled[r])
            continue;
        mi::TonesRowState s = state[r];
        for (int b = 0; b < nbatches; ++b) {
            if (axc[static_cast<size_t>(r) * axc_stride + b] == MI_NO_SIGNAL) {  // CTCSS::reset, ctcss.cpp:165-172
                s.count = 0;
                for (int t = 0; t < MI_TONES_LANES; ++t)
                    s.q1[t] = s.q2[t] = 0.0f;
                continue;
            }
            const float* x = waveout + static_cast<size_t>(r) * row_stride + static_cast<size_t>(b) * mi::kWaveBatch;
            for (int i = 0; i < mi::kWaveBatch; ++i) {
                const float v = x[i];
                for (int t = 0; t < mi::kStandardTones; ++t) {  // ToneDetector::process_sample, ctcss.cpp:44-49
                    const float q0 = coeff[t] * s.q1[t] - s.q2[t] + v;
                    s.q2[t] = s.q1[t];
                    s.q1[t] = q0;
                }
                if (++s.count < window)
                    continue;
                float p[MI_TONES_LANES] = {};
                for (int t = 0; t < mi::kStandardTones; ++t)  // ToneDetector::relative_power, ctcss.cpp:51-55
                    p[t] = s.q1[t] * s.q1[t] + s.q2[t] * s.q2[t] - s.q1[t] * s.q2[t] * coeff[t];
                float total = 0.0f, bp = p[0], sp = 0.0f;
                uint32_t best = 0, second = 0xFFFFFFFFu;
                for (int t = 0; t < mi::kStandardTones; ++t) {
                    total += p[t];
                    if (t == 0)
                        continue;
                    if (p[t] > bp) {
                        second = best;
                        sp = bp;
                        best = static_cast<uint32_t>(t);
                        bp = p[t];
                    } else if (second == 0xFFFFFFFFu || p[t] > sp) {
                        second = static_cast<uint32_t>(t);
                        sp = p[t];
                    }
                }
                if (k < max_records) {
                    records[k] = mi_tone_record{static_cast<uint32_t>(r), s.seq, static_cast<uint32_t>(b), static_cast<uint32_t>(i), best, second,
                                                bp, sp, total / 51.0f, 0};
                    if (powers)
                        std::memcpy(powers + static_cast<size_t>(k) * MI_TONES_LANES, p, sizeof(p));
                }
                ++k;
                s.count = 0;
                s.seq += 1;
                for (int t = 0; t < MI_TONES_LANES; ++t)
                    s.q1[t] = s.q2[t] = 0.0f;
            }
        }
        state[r] = s;
    }
    row_first_record[rows] = k;
    count[0] = k;
    count[1] = k < max_records ? k : static_cast<uint32_t>(max_records);
    return MI_OK;
}

extern "C" int mi_tones_table(uint32_t window, float* freq, float* coeff, uint32_t* alias_of) {
    const mi_tones_cfg cfg{window};
    const uint32_t w = mi::tones_window(&cfg);
    if (!w)
        return MI_ERR_INVALID;
    float c[MI_TONES_LANES];
    mi::tones_coeffs(w, c);
    for (int t = 0; t < mi::kStandardTones; ++t) {
        if (freq)
            freq[t] = mi::kStandardToneHz[t];
        if (coeff)
            coeff[t] = c[t];
        if (alias_of) {
            int first = t;
            for (int u = t - 1; u >= 0; --u)
                first = c[u] == c[t] ? u : first;
            alias_of[t] = static_cast<uint32_t>(first);
        }
    }
    return MI_OK;
}

extern "C" int mi_tones_vote_host(const mi_tone_record* records, size_t n, const mi_tones_rule* rule, mi_tones_vote* out) {
    if ((!records && n) || !out)
        return fail(MI_ERR_INVALID, "NULL argument");
    mi_tones_rule r = rule ? *rule : mi_tones_rule{0, 0};
    if (r.min_share_permille > 1000)
        return fail(MI_ERR_INVALID, "tone vote: min_share_permille must be at most 1000");
    if (n > UINT32_MAX)
        return fail(MI_ERR_INVALID, "tone vote: more than 2^32 - 1 records");
    r.min_windows = r.min_windows ? r.min_windows : 2;
    r.min_share_permille = r.min_share_permille ? r.min_share_permille : 500;
    uint32_t votes[MI_TONES_STANDARD] = {};
    for (size_t i = 0; i < n; ++i) {
        if (records[i].best >= MI_TONES_STANDARD)
            return fail(MI_ERR_INVALID, "tone vote: a record's best is not an index into the tone table");
        if (records[i].best_power > records[i].mean_power)  // ctcss.cpp:150
            votes[records[i].best] += 1;
    }
    uint32_t tone = 0;
    for (uint32_t t = 1; t < MI_TONES_STANDARD; ++t)
        tone = votes[t] > votes[tone] ? t : tone;
    mi_tones_vote v{static_cast<uint32_t>(n), votes[tone], 0, 0.0f, 0.0, 0, 0};
    if (v.votes) {
        v.tone = tone;
        v.freq_hz = mi::kStandardToneHz[tone];
        v.share = static_cast<double>(v.votes) / static_cast<double>(v.windows);
    }
    v.found = v.windows >= r.min_windows && static_cast<uint64_t>(v.votes) * 1000 >= static_cast<uint64_t>(r.min_share_permille) * v.windows ? 1 : 0;
    *out = v;
    return MI_OK;
}

// ---- PCM stage, host side (include/mi_airband.h "PCM stage"): the settings and taps both halves share, the twin of pcm.hip -- one
// block, one output sample and one tap at a time, all 63 taps in the sum --, and the WAV headers.
namespace mi {

const int kImaStepTable[kImaSteps] = {
    7,     8,     9,     10,    11,    12,    13,    14,    16,    17,    19,    21,    23,    25,    28,    31,    34,    37,
    41,    45,    50,    55,    60,    66,    73,    80,    88,    97,    107,   118,   130,   143,   157,   173,   190,   209,
    230,   253,   279,   307,   337,   371,   408,   449,   494,   544,   598,   658,   724,   796,   876,   963,   1060,  1166,
    1282,  1411,  1552,  1707,  1878,  2066,  2272,  2499,  2749,  3024,  3327,  3660,  4026,  4428,  4871,  5358,  5894,  6484,
    7132,  7845,  8630,  9493,  10442, 11487, 12635, 13899, 15289, 16818, 18500, 20350, 22385, 24623, 27086, 29794, 32767};

int pcm_geometry(const mi_pcm_cfg* cfg, PcmGeometry* out) {
    PcmGeometry g{cfg && cfg->rate ? cfg->rate : 8000u, cfg && cfg->format ? cfg->format : static_cast<uint32_t>(MI_PCM_S16), 0, 0};
    if (g.rate != 8000 && g.rate != static_cast<uint32_t>(kWaveRate))
        return fail(MI_ERR_INVALID, "PCM stage: rate must be 8000 or 16000 (0 = 8000)");
    if (g.format != MI_PCM_S16 && g.format != MI_PCM_IMA4)
        return fail(MI_ERR_INVALID, "PCM stage: format must be MI_PCM_S16 or MI_PCM_IMA4 (0 = MI_PCM_S16)");
    g.samples = g.rate == 8000 ? kWaveBatch / 2 : kWaveBatch;
    g.block_bytes = g.format == MI_PCM_S16 ? 2 * g.samples : MI_PCM_IMA_BYTES * g.samples / MI_PCM_IMA_SAMPLES;
    *out = g;
    return MI_OK;
}

// The design in float64.  The lower half and the centre come from the formula; the upper half is its mirror image, so that the
// symmetry holds bit for bit whatever cos() does with the two arguments.
void pcm_taps(float* h) {
    const double pi = 3.14159265358979323846;
    double g[MI_PCM_TAPS];
    for (int k = 0; k <= MI_PCM_HISTORY / 2; ++k) {
        const int c = k - MI_PCM_HISTORY / 2;
        if (c % 2 == 0 && c != 0) {
            g[k] = 0.0;
        } else {
            const double t = c / 2.0, sinc = c == 0 ? 1.0 : std::sin(pi * t) / (pi * t);
            g[k] = 0.5 * sinc * (0.42 - 0.5 * std::cos(2.0 * pi * k / MI_PCM_HISTORY) + 0.08 * std::cos(4.0 * pi * k / MI_PCM_HISTORY));
        }
        g[MI_PCM_HISTORY - k] = g[k];
    }
    double sum = 0.0;
    for (int k = 0; k < MI_PCM_TAPS; ++k)
        sum += g[k];
    for (int k = 0; k < MI_PCM_TAPS; ++k)
        h[k] = (k - MI_PCM_HISTORY / 2) % 2 == 0 && k != MI_PCM_HISTORY / 2 ? 0.0f : static_cast<float>(g[k] / sum);
}

PcmLiveTaps pcm_live_taps() {
    float h[MI_PCM_TAPS];
    pcm_taps(h);
    PcmLiveTaps live;
    int n = 0;
    for (int k = 0; k < MI_PCM_TAPS; ++k)
        if (k % 2 == 0 || k == MI_PCM_HISTORY / 2)
            live.h[n++] = h[k];
    return live;
}

namespace {

int16_t pcm_quantise(float y) {
    float v = y * 32767.0f;
    v = v < -32767.0f ? -32767.0f : v;
    v = v > 32767.0f ? 32767.0f : v;
    return static_cast<int16_t>(std::nearbyintf(v));  // (the default rounding mode: to nearest, ties to even)
}

void put16(uint8_t* p, uint32_t v) {
    p[0] = static_cast<uint8_t>(v);
    p[1] = static_cast<uint8_t>(v >> 8);
}

void put32(uint8_t* p, uint32_t v) {
    put16(p, v);
    put16(p + 2, v >> 16);
}

// one sub-block: 25 samples -> 16 bytes
void ima_subblock(const int16_t* s, uint8_t* out) {
    static const int kIndexStep[8] = {-1, -1, -1, -1, 2, 4, 6, 8};
    const int d = s[1] > s[0] ? s[1] - s[0] : s[0] - s[1];
    int index = kImaSteps - 1;
    for (int i = 0; i < kImaSteps; ++i)
        if (7 * kImaStepTable[i] >= 4 * d) {
            index = i;
            break;
        }
    put16(out, static_cast<uint16_t>(s[0]));
    out[2] = static_cast<uint8_t>(index);
    out[3] = 0;
    int p = s[0];
    for (int n = 1; n < MI_PCM_IMA_SAMPLES; ++n) {
        int step = kImaStepTable[index], diff = s[n] - p, code = 0;
        const int sign = diff < 0 ? 8 : 0;
        diff = diff < 0 ? -diff : diff;
        int vp = step >> 3;
        if (diff >= step) {
            code |= 4;
            diff -= step;
            vp += step;
        }
        step >>= 1;
        if (diff >= step) {
            code |= 2;
            diff -= step;
            vp += step;
        }
        step >>= 1;
        if (diff >= step) {
            code |= 1;
            vp += step;
        }
        p = sign ? p - vp : p + vp;
        p = p < -32768 ? -32768 : (p > 32767 ? 32767 : p);
        index += kIndexStep[code];
        index = index < 0 ? 0 : (index > kImaSteps - 1 ? kImaSteps - 1 : index);
        const uint8_t nibble = static_cast<uint8_t>(code | sign);
        uint8_t* byte = out + 4 + (n - 1) / 2;
        *byte = (n - 1) % 2 == 0 ? nibble : static_cast<uint8_t>(*byte | (nibble << 4));
    }
}

}  // namespace
}  // namespace mi

extern "C" size_t mi_pcm_block_bytes(const mi_pcm_cfg* cfg) {
    mi::PcmGeometry g;
    return mi::pcm_geometry(cfg, &g) == MI_OK ? g.block_bytes : 0;
}

extern "C" int mi_pcm_taps(float* out) {
    if (!out)
        return fail(MI_ERR_INVALID, "NULL argument");
    mi::pcm_taps(out);
    return MI_OK;
}

extern "C" int mi_pcm_plan_host(const mi_pcm_cfg* cfg, const uint8_t* row_enabled, int rows, int nbatches, const float* waveout, size_t row_stride,
                                const mi_gate_block* index, size_t nblocks, void* state_inout, void* out) {
    if (!row_enabled || !waveout || !state_inout || (nblocks && (!index || !out)))
        return fail(MI_ERR_INVALID, "NULL argument");
    mi::PcmGeometry g;
    if (const int rc = mi::pcm_geometry(cfg, &g))
        return rc;
    if (rows < 1 || nbatches < 1)
        return fail(MI_ERR_INVALID, "pcm plan needs rows >= 1 and nbatches >= 1");
    if (row_stride < static_cast<size_t>(nbatches) * mi::kWaveBatch)
        return fail(MI_ERR_INVALID, "a row stride is shorter than the call");
    mi::PcmRowState* state = static_cast<mi::PcmRowState*>(state_inout);
    float h[MI_PCM_TAPS];
    mi::pcm_taps(h);
    std::vector<float> x(MI_PCM_HISTORY + mi::kWaveBatch);
    std::vector<int16_t> s(mi::kWaveBatch);
    for (size_t k = 0; k < nblocks; ++k) {
        uint8_t* dst = static_cast<uint8_t*>(out) + k * g.block_bytes;
        const uint32_t row = index[k].row, batch = index[k].batch;
        if (row >= static_cast<uint32_t>(rows) || batch >= static_cast<uint32_t>(nbatches)) {
            std::memset(dst, 0, g.block_bytes);
            continue;
        }
        // x[62 + n] = sample n of the block, x[0 .. 61] = the 62 before it
        const float* blk = waveout + static_cast<size_t>(row) * row_stride + static_cast<size_t>(batch) * mi::kWaveBatch;
        std::memcpy(x.data(), batch ? blk - MI_PCM_HISTORY : state[row].x, MI_PCM_HISTORY * sizeof(float));
        std::memcpy(x.data() + MI_PCM_HISTORY, blk, mi::kWaveBatch * sizeof(float));
        for (uint32_t m = 0; m < g.samples; ++m) {
            float y = x[MI_PCM_HISTORY + m];
            if (g.rate == 8000) {
                y = 0.0f;
                for (int t = 0; t < MI_PCM_TAPS; ++t)
                    y = y + h[t] * x[MI_PCM_HISTORY + 2 * m - t];
            }
            s[m] = mi::pcm_quantise(y);
        }
        if (g.format == MI_PCM_S16) {
            for (uint32_t m = 0; m < g.samples; ++m)
                mi::put16(dst + 2 * m, static_cast<uint16_t>(s[m]));
        } else {
            for (uint32_t j = 0; j < g.samples / MI_PCM_IMA_SAMPLES; ++j)
                mi::ima_subblock(s.data() + j * MI_PCM_IMA_SAMPLES, dst + j * MI_PCM_IMA_BYTES);
        }
    }
    for (int r = 0; r < rows; ++r)  // (after every block: batch 0 of a row reads the samples the call found)
        if (row_enabled[r])
            std::memcpy(state[r].x, waveout + static_cast<size_t>(r) * row_stride + static_cast<size_t>(nbatches) * mi::kWaveBatch - MI_PCM_HISTORY,
                        MI_PCM_HISTORY * sizeof(float));
    return MI_OK;
}

extern "C" int mi_pcm_wav_header(const mi_pcm_cfg* cfg, uint64_t nblocks, void* buf, size_t cap, size_t* len) {
    if (!buf || !len)
        return fail(MI_ERR_INVALID, "NULL argument");
    mi::PcmGeometry g;
    if (const int rc = mi::pcm_geometry(cfg, &g))
        return rc;
    const bool ima = g.format == MI_PCM_IMA4;
    const size_t need = ima ? 60 : 44;
    if (cap < need)
        return fail(MI_ERR_INVALID, "PCM stage: the WAV header needs 44 bytes (S16) or 60 (IMA4)");
    if (nblocks > (UINT32_MAX - need) / g.block_bytes || nblocks > UINT32_MAX / g.samples)
        return fail(MI_ERR_INVALID, "PCM stage: a WAV file holds less than 2^32 bytes and samples");
    const uint32_t data = static_cast<uint32_t>(nblocks * g.block_bytes);
    uint8_t* b = static_cast<uint8_t*>(buf);
    std::memcpy(b, "RIFF", 4);
    mi::put32(b + 4, static_cast<uint32_t>(need) - 8 + data);
    std::memcpy(b + 8, "WAVEfmt ", 8);
    mi::put32(b + 16, ima ? 20 : 16);
    mi::put16(b + 20, ima ? 0x0011 : 0x0001);
    mi::put16(b + 22, 1);
    mi::put32(b + 24, g.rate);
    mi::put32(b + 28, ima ? g.rate * MI_PCM_IMA_BYTES / MI_PCM_IMA_SAMPLES : 2 * g.rate);
    mi::put16(b + 32, ima ? MI_PCM_IMA_BYTES : 2);
    mi::put16(b + 34, ima ? 4 : 16);
    uint8_t* d = b + 36;
    if (ima) {
        mi::put16(b + 36, 2);
        mi::put16(b + 38, MI_PCM_IMA_SAMPLES);
        std::memcpy(b + 40, "fact", 4);
        mi::put32(b + 44, 4);
        mi::put32(b + 48, static_cast<uint32_t>(nblocks * g.samples));
        d = b + 52;
    }
    std::memcpy(d, "data", 4);
    mi::put32(d + 4, data);
    *len = need;
    return MI_OK;
}

// ---- audio spectrum stage, host side (include/mi_airband.h "audio spectrum stage"): the band, the window and the twiddles both
// halves share, the twin of aspec.hip -- the FFT spec of DESIGN.md 2 stage by stage, one butterfly at a time --, and the vote that
// reads a notch frequency off a row's mean spectrum.
namespace mi {

int aspec_band(const mi_aspec_cfg* cfg, AspecBand* out) {
    const uint64_t lo_hz = cfg && cfg->lo_hz ? cfg->lo_hz : 60u, hi_hz = cfg && cfg->hi_hz ? cfg->hi_hz : 3800u;
    const uint64_t lo = (lo_hz * MI_ASPEC_FFT + (kWaveRate - 1)) / kWaveRate, hi = hi_hz * MI_ASPEC_FFT / kWaveRate;
    if (lo < 1 || lo > hi || hi > MI_ASPEC_BINS - 1)
        return fail(MI_ERR_INVALID, "audio spectrum stage: the band needs 1 <= lo_bin <= hi_bin <= 1023 (lo_hz 0 = 60, hi_hz 0 = 3800)");
    out->lo = static_cast<uint32_t>(lo);
    out->hi = static_cast<uint32_t>(hi);
    return MI_OK;
}

// The lower half comes from the formula; the upper half is its mirror image, so that the symmetry holds bit for bit whatever cos()
// does with the two arguments.
void aspec_window(float* w) {
    const double pi = 3.14159265358979323846;
    for (int i = 0; i < kWaveBatch / 2; ++i)
        w[i] = w[kWaveBatch - 1 - i] = static_cast<float>(0.5 - 0.5 * std::cos(2.0 * pi * i / (kWaveBatch - 1)));
}

// the plan's twiddle table at fft_size_log log2n, 2^(log2n - 1) x {re, im}
int spec_twiddles(int log2n, std::vector<float>& tw) {
    mi_device_cfg dev{};
    dev.sample_rate = 2560000;
    dev.centerfreq = 120000000;
    dev.fft_size_log = log2n;
    dev.sfmt = MI_SFMT_U8;
    dev.fullscale = 127.5f;
    dev.tau = -1;
    Plan p;
    if (const int rc = device_plan(dev, p))
        return rc;
    tw = p.tw;
    return MI_OK;
}

int aspec_twiddles(std::vector<float>& tw) {
    return spec_twiddles(MI_ASPEC_FFT_LOG, tw);
}

namespace {

// X = the FFT spec at N = 2^log2n, in place over z[N][2]: bit reversal, then stages s = 1 .. log2n of butterflies (a, b) -> (a + t, a - t)
// with t = w b, w = tw[j N / 2^s]; t = b for w = 1, (b.im, -b.re) for w = -j, else the two explicit fma.
void spec_fft(const float* tw, float* z, int log2n) {
    const uint32_t n = 1u << log2n;
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t r = 0;
        for (int b = 0; b < log2n; ++b)
            r |= ((i >> b) & 1u) << (log2n - 1 - b);
        if (r > i) {
            std::swap(z[2 * i], z[2 * r]);
            std::swap(z[2 * i + 1], z[2 * r + 1]);
        }
    }
    for (int s = 1; s <= log2n; ++s) {
        const uint32_t half = 1u << (s - 1), step = n >> s;
        for (uint32_t base = 0; base < n; base += 2 * half)
            for (uint32_t j = 0; j < half; ++j) {
                float* a = z + 2 * (base + j);
                float* b = z + 2 * (base + j + half);
                const uint32_t e = j * step;
                float tr, ti;
                if (e == 0) {
                    tr = b[0];
                    ti = b[1];
                } else if (e == n / 4) {
                    tr = b[1];
                    ti = -b[0];
                } else {
                    const float wr = tw[2 * e], wi = tw[2 * e + 1];
                    tr = std::fmaf(-b[1], wi, b[0] * wr);
                    ti = std::fmaf(b[1], wr, b[0] * wi);
                }
                const float ar = a[0], ai = a[1];
                a[0] = ar + tr;
                a[1] = ai + ti;
                b[0] = ar - tr;
                b[1] = ai - ti;
            }
    }
}

constexpr int kAspecThreads = 256;  // the lanes of aspec.hip's workgroup: the order of band_power is stated over them

// the record of one block from its P[0 .. 1023]
void aspec_reduce(const float* pw, const AspecBand& band, mi_aspec_record* rec) {
    double acc[kAspecThreads];
    for (uint32_t t = 0; t < kAspecThreads; ++t) {
        acc[t] = 0.0;
        for (uint32_t bin = t; bin < MI_ASPEC_BINS; bin += kAspecThreads)
            if (bin >= band.lo && bin <= band.hi)
                acc[t] += static_cast<double>(pw[bin]);
    }
    for (uint32_t d = kAspecThreads / 2; d >= 1; d /= 2)
        for (uint32_t t = 0; t < d; ++t)
            acc[t] += acc[t + d];
    uint32_t peak = band.lo;
    for (uint32_t bin = band.lo + 1; bin <= band.hi; ++bin)
        if (pw[bin] > pw[peak])
            peak = bin;
    const uint32_t first = peak - band.lo < MI_ASPEC_LINE_HALF ? band.lo : peak - MI_ASPEC_LINE_HALF;
    const uint32_t last = band.hi - peak < MI_ASPEC_LINE_HALF ? band.hi : peak + MI_ASPEC_LINE_HALF;
    double line = 0.0;
    for (uint32_t bin = first; bin <= last; ++bin)
        line += static_cast<double>(pw[bin]);
    rec->peak_bin = peak;
    rec->peak_power = pw[peak];
    rec->band_power = acc[0];
    rec->line_power = line;
}

}  // namespace
}  // namespace mi

extern "C" int mi_aspec_window(float* out) {
    if (!out)
        return fail(MI_ERR_INVALID, "NULL argument");
    mi::aspec_window(out);
    return MI_OK;
}

extern "C" int mi_aspec_band(const mi_aspec_cfg* cfg, uint32_t* lo_bin, uint32_t* hi_bin) {
    if (!lo_bin || !hi_bin)
        return fail(MI_ERR_INVALID, "NULL argument");
    mi::AspecBand band;
    if (const int rc = mi::aspec_band(cfg, &band))
        return rc;
    *lo_bin = band.lo;
    *hi_bin = band.hi;
    return MI_OK;
}

extern "C" int mi_aspec_plan_host(const mi_aspec_cfg* cfg, int rows, int nbatches, const float* waveout, size_t row_stride, const mi_gate_block* index,
                                  size_t nblocks, const uint32_t* row_first, mi_aspec_record* records, float* power, float* row_mean,
                                  uint32_t* row_blocks) {
    if (!waveout || (nblocks && (!index || !records)))
        return fail(MI_ERR_INVALID, "NULL argument");
    mi::AspecBand band;
    if (const int rc = mi::aspec_band(cfg, &band))
        return rc;
    if (rows < 1 || nbatches < 1)
        return fail(MI_ERR_INVALID, "audio spectrum plan needs rows >= 1 and nbatches >= 1");
    if (row_stride < static_cast<size_t>(nbatches) * mi::kWaveBatch)
        return fail(MI_ERR_INVALID, "a row stride is shorter than the call");
    if ((row_mean != nullptr) != (row_blocks != nullptr) || (row_mean && (!row_first || (nblocks && !power))))
        return fail(MI_ERR_INVALID, "audio spectrum stage: a row mean needs the power rows, the row starts and the row counts");
    std::vector<float> tw, w(mi::kWaveBatch), z(2 * MI_ASPEC_FFT), pw(MI_ASPEC_BINS);
    if (const int rc = mi::aspec_twiddles(tw))
        return rc;
    mi::aspec_window(w.data());
    for (size_t k = 0; k < nblocks; ++k) {
        const uint32_t row = index[k].row, batch = index[k].batch;
        mi_aspec_record rec{row, batch, 0xFFFFFFFFu, 0.0f, 0.0, 0.0};
        if (row >= static_cast<uint32_t>(rows) || batch >= static_cast<uint32_t>(nbatches)) {
            std::fill(pw.begin(), pw.end(), 0.0f);
        } else {
            const float* x = waveout + static_cast<size_t>(row) * row_stride + static_cast<size_t>(batch) * mi::kWaveBatch;
            std::fill(z.begin(), z.end(), 0.0f);
            for (int i = 0; i < mi::kWaveBatch; ++i)
                z[2 * static_cast<size_t>(i)] = x[i] * w[static_cast<size_t>(i)];
            mi::spec_fft(tw.data(), z.data(), MI_ASPEC_FFT_LOG);
            for (size_t j = 0; j < MI_ASPEC_BINS; ++j) {
                const float rr = z[2 * j] * z[2 * j], ii = z[2 * j + 1] * z[2 * j + 1];
                pw[j] = rr + ii;
            }
            mi::aspec_reduce(pw.data(), band, &rec);
        }
        records[k] = rec;
        if (power)
            std::memcpy(power + k * MI_ASPEC_BINS, pw.data(), MI_ASPEC_BINS * sizeof(float));
    }
    if (row_mean) {
        const uint64_t stored = nblocks;
        for (int r = 0; r < rows; ++r) {
            const uint64_t first = std::min<uint64_t>(row_first[r], stored), last = std::min<uint64_t>(row_first[r + 1], stored);
            const uint64_t n = last > first ? last - first : 0;
            row_blocks[r] = static_cast<uint32_t>(n);
            for (size_t j = 0; j < MI_ASPEC_BINS; ++j) {
                double s = 0.0;
                for (uint64_t k = first; k < first + n; ++k)
                    s += static_cast<double>(power[k * MI_ASPEC_BINS + j]);
                row_mean[static_cast<size_t>(r) * MI_ASPEC_BINS + j] = n ? static_cast<float>(s / static_cast<double>(n)) : 0.0f;
            }
        }
    }
    return MI_OK;
}

extern "C" int mi_aspec_notch_host(const float* row_mean, uint32_t row_blocks, const mi_aspec_record* records, size_t n, const mi_aspec_cfg* cfg,
                                   const mi_aspec_rule* rule, mi_aspec_notch* out) {
    if (!row_mean || !out || (n && !records))
        return fail(MI_ERR_INVALID, "NULL argument");
    mi::AspecBand band;
    if (const int rc = mi::aspec_band(cfg, &band))
        return rc;
    const uint32_t min_blocks = rule && rule->min_blocks ? rule->min_blocks : 8u;
    const float ratio = rule && rule->ratio != 0.0f ? rule->ratio : 16.0f;
    if (!(ratio >= 0.0f) || !std::isfinite(ratio))
        return fail(MI_ERR_INVALID, "audio spectrum stage: the ratio must be finite and not negative (0 = 16)");
    uint32_t p = band.lo;
    for (uint32_t j = band.lo + 1; j <= band.hi; ++j)
        if (row_mean[j] > row_mean[p])
            p = j;
    std::vector<float> around;
    for (uint32_t j = band.lo; j <= band.hi; ++j) {
        const uint32_t d = j > p ? j - p : p - j;
        if (d >= 3 && d <= 34)
            around.push_back(row_mean[j]);
    }
    std::sort(around.begin(), around.end());
    const float floor = around.empty() ? 0.0f : around[(around.size() - 1) / 2];
    const float threshold = ratio * floor;
    double num = 0.0, den = 0.0;
    for (uint32_t j = p - band.lo < 1 ? band.lo : p - 1; j <= (band.hi - p < 1 ? band.hi : p + 1); ++j) {
        num += static_cast<double>(j) * static_cast<double>(row_mean[j]);
        den += static_cast<double>(row_mean[j]);
    }
    uint32_t votes = 0;
    for (size_t i = 0; i < n; ++i) {
        const int64_t d = static_cast<int64_t>(records[i].peak_bin) - static_cast<int64_t>(p);
        votes += d >= -1 && d <= 1 ? 1u : 0u;
    }
    const double hz_per_bin = static_cast<double>(mi::kWaveRate) / MI_ASPEC_FFT;
    out->found = row_blocks >= min_blocks && row_mean[p] > 0.0f && row_mean[p] > threshold ? 1u : 0u;
    out->bin = p;
    out->freq_hz = hz_per_bin * (den > 0.0 ? num / den : static_cast<double>(p));
    out->peak = static_cast<double>(row_mean[p]);
    out->floor = static_cast<double>(floor);
    out->votes = votes;
    out->blocks = row_blocks;
    return MI_OK;
}

// ---- voice band stage, host side (include/mi_airband.h "voice band stage"): the settings' check, the taps and the classes both
// halves share, and the twin of vband.hip -- one block at a time, tap by tap over all of its outputs, all 511 taps in the sum.
namespace mi {

int vband_row_ok(const mi_vband_row& r) {
    if (r.hp_hz != 0 && (r.hp_hz < 50 || r.hp_hz > 4000))
        return fail(MI_ERR_INVALID, "voice band stage: hp_hz must be 0 or 50 .. 4000");
    if (r.lp_hz != 0 && (r.lp_hz < 500 || r.lp_hz > 7800))
        return fail(MI_ERR_INVALID, "voice band stage: lp_hz must be 0 or 500 .. 7800");
    if (r.lp_hz != 0 && r.lp_hz < r.hp_hz + 200)
        return fail(MI_ERR_INVALID, "voice band stage: lp_hz must be 0 or at least hp_hz + 200");
    return MI_OK;
}

// The design in float64.  The lower half and the centre come from the formula; the upper half is its mirror image, so that the
// symmetry holds bit for bit whatever cos() does with the two arguments.
void vband_taps(const mi_vband_row& r, float* h) {
    const double pi = 3.14159265358979323846;
    const int centre = MI_VBAND_HISTORY / 2;
    const double fl = r.hp_hz / static_cast<double>(kWaveRate), fh = r.lp_hz / static_cast<double>(kWaveRate);
    const auto sinc = [pi](double t) { return t == 0.0 ? 1.0 : std::sin(pi * t) / (pi * t); };
    for (int k = 0; k <= centre; ++k) {
        const int c = k - centre;
        const double upper = r.lp_hz ? 2.0 * fh * sinc(2.0 * fh * c) : (c == 0 ? 1.0 : 0.0);
        const double g = (upper - 2.0 * fl * sinc(2.0 * fl * c)) *
                         (0.42 - 0.5 * std::cos(2.0 * pi * k / MI_VBAND_HISTORY) + 0.08 * std::cos(4.0 * pi * k / MI_VBAND_HISTORY));
        h[k] = h[MI_VBAND_HISTORY - k] = static_cast<float>(g);
    }
}

int vband_classes(const mi_vband_row* row_cfg, size_t rows, std::vector<uint32_t>& class_of, std::vector<mi_vband_row>& classes) {
    class_of.assign(rows, 0);
    classes.clear();
    for (size_t r = 0; r < rows; ++r) {
        const mi_vband_row s = row_cfg ? row_cfg[r] : mi_vband_default_row();
        if (const int rc = vband_row_ok(s))
            return rc;
        size_t c = 0;
        while (c < classes.size() && (classes[c].hp_hz != s.hp_hz || classes[c].lp_hz != s.lp_hz))
            ++c;
        if (c == classes.size())
            classes.push_back(s);
        class_of[r] = static_cast<uint32_t>(c);
    }
    return MI_OK;
}

bool planes_overlap(const float* in, size_t in_stride, const float* out, size_t out_stride, size_t rows, size_t nbatches) {
    const size_t call = nbatches * static_cast<size_t>(kWaveBatch);
    const uintptr_t a = reinterpret_cast<uintptr_t>(in), b = reinterpret_cast<uintptr_t>(out);
    const uintptr_t a_end = a + ((rows - 1) * in_stride + call) * sizeof(float), b_end = b + ((rows - 1) * out_stride + call) * sizeof(float);
    return a < b_end && b < a_end;
}

}  // namespace mi

extern "C" mi_vband_row mi_vband_default_row(void) {
    return mi_vband_row{100, 2500};
}

extern "C" int mi_vband_taps(uint32_t hp_hz, uint32_t lp_hz, float* out) {
    if (!out)
        return fail(MI_ERR_INVALID, "NULL argument");
    const mi_vband_row r{hp_hz, lp_hz};
    if (const int rc = mi::vband_row_ok(r))
        return rc;
    mi::vband_taps(r, out);
    return MI_OK;
}

extern "C" int mi_vband_plan_host(const mi_vband_row* row_cfg, const uint8_t* row_enabled, int rows, int nbatches, const float* waveout,
                                  size_t row_stride, void* state_inout, float* out, size_t out_stride) {
    if (!row_enabled || !waveout || !state_inout || !out)
        return fail(MI_ERR_INVALID, "NULL argument");
    if (rows < 1 || nbatches < 1)
        return fail(MI_ERR_INVALID, "vband plan needs rows >= 1 and nbatches >= 1");
    std::vector<uint32_t> class_of;
    std::vector<mi_vband_row> classes;
    if (const int rc = mi::vband_classes(row_cfg, static_cast<size_t>(rows), class_of, classes))
        return rc;
    if (row_stride < static_cast<size_t>(nbatches) * mi::kWaveBatch || out_stride < static_cast<size_t>(nbatches) * mi::kWaveBatch)
        return fail(MI_ERR_INVALID, "a row stride is shorter than the call");
    if (mi::planes_overlap(waveout, row_stride, out, out_stride, static_cast<size_t>(rows), static_cast<size_t>(nbatches)))
        return fail(MI_ERR_INVALID, "the output overlaps the audio buffer");
    mi::VbandRowState* state = static_cast<mi::VbandRowState*>(state_inout);
    std::vector<float> taps(classes.size() * MI_VBAND_TAPS);
    for (size_t c = 0; c < classes.size(); ++c)
        mi::vband_taps(classes[c], taps.data() + c * MI_VBAND_TAPS);
    std::vector<float> x(MI_VBAND_HISTORY + mi::kWaveBatch), acc(mi::kWaveBatch);
    for (int r = 0; r < rows; ++r) {
        if (!row_enabled[r])
            continue;
        const float* const h = taps.data() + class_of[r] * MI_VBAND_TAPS;
        const float* const row = waveout + static_cast<size_t>(r) * row_stride;
        for (int b = 0; b < nbatches; ++b) {
            // x[510 + n] = sample n of the block, x[0 .. 509] = the 510 before it
            const float* const blk = row + static_cast<size_t>(b) * mi::kWaveBatch;
            std::memcpy(x.data(), b ? blk - MI_VBAND_HISTORY : state[r].x, MI_VBAND_HISTORY * sizeof(float));
            std::memcpy(x.data() + MI_VBAND_HISTORY, blk, mi::kWaveBatch * sizeof(float));
            std::fill(acc.begin(), acc.end(), 0.0f);
            for (int k = 0; k < MI_VBAND_TAPS; ++k) {  // (every output takes its taps in ascending order)
                const float hk = h[k];
                const float* const xk = x.data() + MI_VBAND_HISTORY - k;
                for (int n = 0; n < mi::kWaveBatch; ++n)
                    acc[n] = acc[n] + hk * xk[n];
            }
            float* const dst = out + static_cast<size_t>(r) * out_stride + static_cast<size_t>(b) * mi::kWaveBatch;
            for (int n = 0; n < mi::kWaveBatch; ++n)
                dst[n] = std::fmin(std::fmax(acc[n], -1.0f), 1.0f);
        }
        std::memcpy(state[r].x, row + static_cast<size_t>(nbatches) * mi::kWaveBatch - MI_VBAND_HISTORY, MI_VBAND_HISTORY * sizeof(float));
    }
    return MI_OK;
}

// ---- peak limiter stage, host side (include/mi_airband.h "peak limiter stage"): the settings' check, the twin of limit.hip -- a row's
// whole call at once, the window maximum by ten doublings, the 64 gains of an output added one array at a time -- and the pregain
// helper.
namespace mi {

int limit_row_ok(const mi_limit_row& r) {
    if (!std::isfinite(r.pregain) || r.pregain < 0.0009765625f || r.pregain > 1024.0f)
        return fail(MI_ERR_INVALID, "limiter stage: pregain must be finite and within 2^-10 .. 2^10");
    if (!std::isfinite(r.ceiling) || r.ceiling < 0.0625f || r.ceiling > 1.0f)
        return fail(MI_ERR_INVALID, "limiter stage: ceiling must be finite and within 0.0625 .. 1");
    return MI_OK;
}

int limit_rows(const mi_limit_row* row_cfg, size_t rows, std::vector<mi_limit_row>& out) {
    out.assign(rows, mi_limit_default_row());
    for (size_t r = 0; r < rows; ++r) {
        if (row_cfg)
            out[r] = row_cfg[r];
        if (const int rc = limit_row_ok(out[r]))
            return rc;
    }
    return MI_OK;
}

}  // namespace mi

extern "C" mi_limit_row mi_limit_default_row(void) {
    return mi_limit_row{1.0f, 0.89125094f};
}

extern "C" int mi_limit_plan_host(const mi_limit_row* row_cfg, const uint8_t* row_enabled, int rows, int nbatches, const float* in, size_t row_stride,
                                  void* state_inout, float* out, size_t out_stride) {
    if (!row_enabled || !in || !state_inout || !out)
        return fail(MI_ERR_INVALID, "NULL argument");
    if (rows < 1 || nbatches < 1)
        return fail(MI_ERR_INVALID, "limit plan needs rows >= 1 and nbatches >= 1");
    std::vector<mi_limit_row> cfg;
    if (const int rc = mi::limit_rows(row_cfg, static_cast<size_t>(rows), cfg))
        return rc;
    const size_t n = static_cast<size_t>(nbatches) * mi::kWaveBatch;
    if (row_stride < n || out_stride < n)
        return fail(MI_ERR_INVALID, "a row stride is shorter than the call");
    if (mi::planes_overlap(in, row_stride, out, out_stride, static_cast<size_t>(rows), static_cast<size_t>(nbatches)))
        return fail(MI_ERR_INVALID, "the output overlaps the input plane");
    mi::LimitRowState* state = static_cast<mi::LimitRowState*>(state_inout);
    const size_t hist = MI_LIMIT_HISTORY, look = MI_LIMIT_LOOKAHEAD;
    std::vector<float> u(hist + n), p(hist + n), s(n);
    for (int r = 0; r < rows; ++r) {
        if (!row_enabled[r])
            continue;
        const float pregain = cfg[r].pregain, ceiling = cfg[r].ceiling;
        const float* const row = in + static_cast<size_t>(r) * row_stride;
        // u[1086 + i] = sample i of the call times the pregain, u[0 .. 1085] = the carried samples times it
        for (size_t i = 0; i < hist; ++i)
            u[i] = state[r].x[i] * pregain;
        for (size_t i = 0; i < n; ++i)
            u[hist + i] = row[i] * pregain;
        // p[i] = max of |u| over the w values that end at i, w = 1, 2, 4, .. 1024 (fewer where the array begins: no output reads those)
        for (size_t i = 0; i < hist + n; ++i)
            p[i] = std::fabs(u[i]);
        for (size_t w = 1; w < MI_LIMIT_WINDOW; w *= 2)
            for (size_t i = hist + n - 1; i >= w; --i)  // (downwards: p[i - w] is still the narrower window's)
                p[i] = std::max(p[i], p[i - w]);
        // the gain of window maximum p[i], in p's place
        for (size_t i = 0; i < hist + n; ++i)
            p[i] = p[i] > ceiling ? ceiling / p[i] : 1.0f;
        // output i adds the gains of samples i - 63 .. i, which are p[1023 + i] .. p[1086 + i], in that order
        std::fill(s.begin(), s.end(), 0.0f);
        for (size_t k = 0; k <= look; ++k) {
            const float* const rk = p.data() + (hist - look) + k;
            for (size_t i = 0; i < n; ++i)
                s[i] = s[i] + rk[i];
        }
        float* const dst = out + static_cast<size_t>(r) * out_stride;
        for (size_t i = 0; i < n; ++i) {
            const float g = s[i] * 0.015625f;
            const float y = u[hist - look + i] * g;
            dst[i] = std::fmin(std::fmax(y, -ceiling), ceiling);
        }
        std::memcpy(state[r].x, row + n - hist, hist * sizeof(float));
    }
    return MI_OK;
}

extern "C" int mi_limit_pregain_host(const mi_tx_record* records, size_t n, uint32_t row, float ceiling, uint32_t percentile, float* pregain, uint32_t* used) {
    if (!pregain || !used || (!records && n))
        return fail(MI_ERR_INVALID, "NULL argument");
    if (!std::isfinite(ceiling) || ceiling < 0.0625f || ceiling > 1.0f)
        return fail(MI_ERR_INVALID, "limiter pregain: ceiling must be finite and within 0.0625 .. 1");
    if (percentile > 100)
        return fail(MI_ERR_INVALID, "limiter pregain: percentile must be 1 .. 100, or 0 for 90");
    if (percentile == 0)
        percentile = 90;
    std::vector<float> peaks;
    for (size_t i = 0; i < n; ++i)
        if (records[i].row == row && records[i].nblocks > 0 && records[i].peak > 0.0f)
            peaks.push_back(records[i].peak);
    *used = static_cast<uint32_t>(peaks.size());
    *pregain = 1.0f;
    if (peaks.empty())
        return MI_OK;
    std::sort(peaks.begin(), peaks.end());
    const float peak = peaks[static_cast<size_t>((static_cast<uint64_t>(peaks.size()) - 1) * percentile / 100)];
    *pregain = std::fmin(std::fmax(ceiling / peak, 0.0009765625f), 1024.0f);
    return MI_OK;
}

// ---- noise reduction stage, host side (include/mi_airband.h "noise reduction stage"): the settings' check, the window, and the twin
// of denoise.hip -- one block at a time as the device goes: its nine frames through spec_fft, M of the block, m over the eight rows
// that end with it, the gains, the conjugate transforms and the overlap-add.
namespace mi {

int denoise_rows(const mi_denoise_row* row_cfg, size_t rows, std::vector<DenoiseGains>& out) {
    out.resize(rows);
    for (size_t r = 0; r < rows; ++r) {
        const mi_denoise_row s = row_cfg ? row_cfg[r] : mi_denoise_default_row();
        if (!(s.reduction_db >= 0.0f && s.reduction_db <= 40.0f))
            return fail(MI_ERR_INVALID, "noise reduction stage: reduction_db must be within 0 .. 40");
        if (!(s.over >= 0.0f && s.over <= 64.0f))
            return fail(MI_ERR_INVALID, "noise reduction stage: over must be within 0 .. 64");
        out[r] = DenoiseGains{static_cast<float>(std::pow(10.0, -static_cast<double>(s.reduction_db) / 20.0)), s.over};
    }
    return MI_OK;
}

// The lower half comes from the formula; the upper half is its mirror image, so that the symmetry holds bit for bit whatever sin()
// does with the two arguments.
void denoise_window(float* w) {
    const double pi = 3.14159265358979323846;
    for (int i = 0; i < MI_DENOISE_HOP; ++i)
        w[i] = w[MI_DENOISE_FRAME - 1 - i] = static_cast<float>(std::sin(pi * (i + 0.5) / MI_DENOISE_FRAME));
}

void denoise_fresh(DenoiseRowState* state, size_t rows) {
    for (size_t r = 0; r < rows; ++r) {
        std::fill(state[r].x, state[r].x + MI_DENOISE_FRAME, 0.0f);
        std::fill(&state[r].m[0][0], &state[r].m[0][0] + (MI_DENOISE_DEPTH - 1) * MI_DENOISE_BINS, INFINITY);
    }
}

}  // namespace mi

extern "C" mi_denoise_row mi_denoise_default_row(void) {
    return mi_denoise_row{12.0f, 4.5f};
}

extern "C" int mi_denoise_window(float* out) {
    if (!out)
        return fail(MI_ERR_INVALID, "NULL argument");
    mi::denoise_window(out);
    return MI_OK;
}

extern "C" int mi_denoise_plan_host(const mi_denoise_row* row_cfg, const uint8_t* row_enabled, int rows, int nbatches, const float* in, size_t row_stride,
                                    void* state_inout, float* out, size_t out_stride) {
    if (!row_enabled || !in || !state_inout || !out)
        return fail(MI_ERR_INVALID, "NULL argument");
    if (rows < 1 || nbatches < 1)
        return fail(MI_ERR_INVALID, "denoise plan needs rows >= 1 and nbatches >= 1");
    std::vector<mi::DenoiseGains> cfg;
    if (const int rc = mi::denoise_rows(row_cfg, static_cast<size_t>(rows), cfg))
        return rc;
    if (row_stride < static_cast<size_t>(nbatches) * mi::kWaveBatch || out_stride < static_cast<size_t>(nbatches) * mi::kWaveBatch)
        return fail(MI_ERR_INVALID, "a row stride is shorter than the call");
    if (mi::planes_overlap(in, row_stride, out, out_stride, static_cast<size_t>(rows), static_cast<size_t>(nbatches)))
        return fail(MI_ERR_INVALID, "the output overlaps the input plane");
    constexpr int kHop = MI_DENOISE_HOP, kFrame = MI_DENOISE_FRAME, kN = MI_DENOISE_FFT, kBins = MI_DENOISE_BINS, kDepth = MI_DENOISE_DEPTH;
    constexpr int kFrames = mi::kWaveBatch / kHop + 1;  // 9 frames make a block
    std::vector<float> tw, w(kFrame);
    if (const int rc = mi::spec_twiddles(MI_DENOISE_FFT_LOG, tw))
        return rc;
    mi::denoise_window(w.data());
    std::vector<mi::DenoiseRowState> blob(static_cast<size_t>(rows));  // (the caller's bytes may not be aligned)
    std::memcpy(blob.data(), state_inout, blob.size() * sizeof(mi::DenoiseRowState));
    std::vector<float> x(kFrame + mi::kWaveBatch), X(static_cast<size_t>(kFrames) * 2 * kN), P(static_cast<size_t>(kFrames) * kBins),
        S(static_cast<size_t>(kFrames) * kBins), z(2 * kN), v(static_cast<size_t>(kFrames) * kFrame), noise(kBins);
    std::vector<float> floors;  // M of the seven batches before the call, then of the call's
    bool silent[kFrames];
    for (int r = 0; r < rows; ++r) {
        if (!row_enabled[r])
            continue;
        const float g_min = cfg[static_cast<size_t>(r)].g_min, over = cfg[static_cast<size_t>(r)].over;
        mi::DenoiseRowState& st = blob[static_cast<size_t>(r)];
        const float* const row = in + static_cast<size_t>(r) * row_stride;
        floors.assign(&st.m[0][0], &st.m[0][0] + (kDepth - 1) * kBins);
        floors.resize(static_cast<size_t>(kDepth - 1 + nbatches) * kBins);
        for (int b = 0; b < nbatches; ++b) {
            // x[500 + n] = sample n of the block, x[0 .. 499] = the 500 before it; frame j of the block begins at x[250 j]
            const float* const blk = row + static_cast<size_t>(b) * mi::kWaveBatch;
            std::memcpy(x.data(), b ? blk - kFrame : st.x, kFrame * sizeof(float));
            std::memcpy(x.data() + kFrame, blk, mi::kWaveBatch * sizeof(float));
            for (int j = 0; j < kFrames; ++j) {
                float* const Xj = X.data() + static_cast<size_t>(j) * 2 * kN;
                std::fill(Xj, Xj + 2 * kN, 0.0f);
                silent[j] = true;
                for (int i = 0; i < kFrame; ++i) {
                    const float s = x[static_cast<size_t>(kHop * j + i)];
                    silent[j] = silent[j] && s == 0.0f;
                    Xj[2 * i] = s * w[static_cast<size_t>(i)];
                }
                mi::spec_fft(tw.data(), Xj, MI_DENOISE_FFT_LOG);
                for (int k = 0; k < kBins; ++k) {
                    const float rr = Xj[2 * k] * Xj[2 * k], ii = Xj[2 * k + 1] * Xj[2 * k + 1];
                    P[static_cast<size_t>(j) * kBins + k] = rr + ii;
                }
            }
            float* const M = floors.data() + static_cast<size_t>(kDepth - 1 + b) * kBins;
            std::fill(M, M + kBins, INFINITY);
            for (int j = 1; j < kFrames; ++j) {
                const float* const p0 = P.data() + static_cast<size_t>(j - 1) * kBins;
                const float* const p1 = p0 + kBins;
                for (int k = 0; k < kBins; ++k) {
                    const int lo = k ? k - 1 : 1, hi = k < kBins - 1 ? k + 1 : kBins - 2;
                    const float t0 = (p0[lo] + p0[k]) + p0[hi], t1 = (p1[lo] + p1[k]) + p1[hi];
                    const float s = t0 + t1;
                    S[static_cast<size_t>(j) * kBins + k] = s;
                    if (!silent[j - 1] && !silent[j])
                        M[k] = std::fmin(M[k], s);
                }
            }
            std::memcpy(S.data(), S.data() + kBins, kBins * sizeof(float));  // the block's first frame takes S of the frame behind it
            for (int k = 0; k < kBins; ++k) {
                float m = INFINITY;
                for (int d = 0; d < kDepth; ++d)
                    m = std::fmin(m, floors[static_cast<size_t>(b + d) * kBins + k]);
                noise[static_cast<size_t>(k)] = std::isinf(m) ? 0.0f : over * m;
            }
            for (int j = 0; j < kFrames; ++j) {
                const float* const Xj = X.data() + static_cast<size_t>(j) * 2 * kN;
                for (int k = 0; k < kN; ++k) {
                    const int kk = k <= kN / 2 ? k : kN - k;
                    const float n = noise[static_cast<size_t>(kk)], s = S[static_cast<size_t>(j) * kBins + kk];
                    const float g = n >= s ? g_min : std::fmax(g_min, 1.0f - n / s);
                    z[2 * static_cast<size_t>(k)] = g * Xj[2 * k];
                    z[2 * static_cast<size_t>(k) + 1] = -(g * Xj[2 * k + 1]);
                }
                mi::spec_fft(tw.data(), z.data(), MI_DENOISE_FFT_LOG);
                for (int i = 0; i < kFrame; ++i)
                    v[static_cast<size_t>(j) * kFrame + i] = (z[2 * static_cast<size_t>(i)] * (1.0f / kN)) * w[static_cast<size_t>(i)];
            }
            float* const dst = out + static_cast<size_t>(r) * out_stride + static_cast<size_t>(b) * mi::kWaveBatch;
            for (int n = 0; n < mi::kWaveBatch; ++n) {
                const int q = n / kHop, i = n - q * kHop;  // the older frame q of the block, the newer one q + 1
                const float y = v[static_cast<size_t>(q) * kFrame + kHop + i] + v[static_cast<size_t>(q + 1) * kFrame + i];
                dst[n] = std::fmin(std::fmax(y, -1.0f), 1.0f);
            }
        }
        std::memcpy(st.x, row + static_cast<size_t>(nbatches) * mi::kWaveBatch - kFrame, kFrame * sizeof(float));
        std::memcpy(&st.m[0][0], floors.data() + static_cast<size_t>(nbatches) * kBins, (kDepth - 1) * kBins * sizeof(float));
    }
    std::memcpy(state_inout, blob.data(), blob.size() * sizeof(mi::DenoiseRowState));
    return MI_OK;
}

// ---- SELCAL decoder stage, host side (include/mi_airband.h "SELCAL decoder stage"): the tone tables, the settings' check, the window,
// the blob's check, and the twin of selcal.hip -- one row, one window and one tone at a time, then the decoder over the row's windows.
namespace mi {

namespace {

// ascending frequency; the classic sixteen are the even positions.  The odd ones (SELCAL 32) are written from memory: see the header.
constexpr float kSelcalHz[MI_SELCAL_MAX_TONES] = {312.6f,  329.2f,  346.7f,  365.2f,  384.6f,  405.0f,  426.6f,  449.3f,  473.2f,  498.3f,  524.8f,
                                                  552.7f,  582.1f,  613.1f,  645.7f,  680.0f,  716.1f,  754.2f,  794.3f,  836.6f,  881.0f,  927.9f,
                                                  977.2f,  1029.2f, 1083.9f, 1141.6f, 1202.3f, 1266.2f, 1333.5f, 1404.4f, 1479.1f, 1557.8f};
constexpr char kSelcalLetter[MI_SELCAL_MAX_TONES + 1] = "ATBUCVDWEXFYGZH1J2K3L4M5P6Q7R8S9";

bool in_range(float v, float lo, float hi) {
    return std::isfinite(v) && v >= lo && v <= hi;
}

}  // namespace

void selcal_window(float* w) {
    aspec_window(w);  // the same 2000-point Hann window, symmetric bit for bit
}

int selcal_plan(const mi_selcal_cfg* cfg, SelcalPlan* out) {
    mi_selcal_cfg c{};
    if (cfg)
        c = *cfg;
    SelcalPlan p{};
    if (c.mode == MI_SELCAL_16 || c.mode == MI_SELCAL_32) {
        const int step = c.mode == MI_SELCAL_16 ? 2 : 1;
        p.ntones = MI_SELCAL_MAX_TONES / step;
        for (uint32_t t = 0; t < p.ntones; ++t) {
            p.freq[t] = kSelcalHz[t * step];
            p.letter[t] = kSelcalLetter[t * step];
        }
        c.ntones = p.ntones;
        std::memcpy(c.freq, p.freq, sizeof(p.freq));
    } else if (c.mode == MI_SELCAL_CUSTOM) {
        if (c.ntones < 2 || c.ntones > MI_SELCAL_MAX_TONES)
            return fail(MI_ERR_INVALID, "SELCAL stage: a custom table needs 2 .. 32 tones");
        for (uint32_t t = 0; t < c.ntones; ++t) {
            if (!in_range(c.freq[t], 250.0f, 2000.0f))
                return fail(MI_ERR_INVALID, "SELCAL stage: a custom tone must lie within 250 .. 2000 Hz");
            if (t && !(c.freq[t] - c.freq[t - 1] >= 16.0f))
                return fail(MI_ERR_INVALID, "SELCAL stage: custom tones must ascend, at least 16 Hz apart");
            p.freq[t] = c.freq[t];
            p.letter[t] = '?';
        }
        for (uint32_t t = c.ntones; t < MI_SELCAL_MAX_TONES; ++t)
            c.freq[t] = 0.0f;
        p.ntones = c.ntones;
    } else {
        return fail(MI_ERR_INVALID, "SELCAL stage: mode must be MI_SELCAL_16, MI_SELCAL_32 or MI_SELCAL_CUSTOM");
    }
    const double pi = 3.14159265358979323846;
    for (uint32_t t = 0; t < p.ntones; ++t)
        p.coeff[t] = static_cast<float>(2.0 * std::cos(2.0 * pi * static_cast<double>(p.freq[t]) / kWaveRate));
    c.min_energy = c.min_energy == 0.0f ? 1e-3f : c.min_energy;
    c.min_tonality = c.min_tonality == 0.0f ? 0.5f : c.min_tonality;
    c.max_twist = c.max_twist == 0.0f ? 8.0f : c.max_twist;
    c.min_separation = c.min_separation == 0.0f ? 4.0f : c.min_separation;
    c.min_run = c.min_run ? c.min_run : 8;
    c.max_run = c.max_run ? c.max_run : (c.min_run > 22 ? c.min_run : 22);
    c.max_gap = c.max_gap ? c.max_gap : 8;
    if (!in_range(c.min_energy, 1e-12f, 1e6f))
        return fail(MI_ERR_INVALID, "SELCAL stage: min_energy must be finite and within 1e-12 .. 1e6 (0 = the default)");
    if (!in_range(c.min_tonality, 0.01f, 1.0f))
        return fail(MI_ERR_INVALID, "SELCAL stage: min_tonality must be within 0.01 .. 1 (0 = the default)");
    if (!in_range(c.max_twist, 1.0f, 1000.0f))
        return fail(MI_ERR_INVALID, "SELCAL stage: max_twist must be within 1 .. 1000 (0 = the default)");
    if (!in_range(c.min_separation, 1.0f, 1000.0f))
        return fail(MI_ERR_INVALID, "SELCAL stage: min_separation must be within 1 .. 1000 (0 = the default)");
    if (c.min_run < 2 || c.min_run > 64)
        return fail(MI_ERR_INVALID, "SELCAL stage: min_run must be within 2 .. 64 windows (0 = the default)");
    if (c.max_run < c.min_run || c.max_run > 1024)
        return fail(MI_ERR_INVALID, "SELCAL stage: max_run must be within min_run .. 1024 windows (0 = the default)");
    if (c.max_gap < 1 || c.max_gap > 64)
        return fail(MI_ERR_INVALID, "SELCAL stage: max_gap must be within 1 .. 64 windows (0 = the default)");
    if (c.zero)
        return fail(MI_ERR_INVALID, "SELCAL stage: the settings' zero field must be 0");
    float w[MI_SELCAL_WINDOW];
    selcal_window(w);
    double sw = 0.0, sw2 = 0.0;
    for (int j = 0; j < MI_SELCAL_WINDOW; ++j) {
        sw += static_cast<double>(w[j]);
        sw2 += static_cast<double>(w[j]) * static_cast<double>(w[j]);
    }
    p.c = static_cast<float>(sw * sw / (2.0 * sw2));
    p.min_energy = c.min_energy;
    p.tc = c.min_tonality * p.c;
    p.max_twist = c.max_twist;
    p.min_separation = c.min_separation;
    p.min_run = c.min_run;
    p.max_run = c.max_run;
    p.max_gap = c.max_gap;
    p.filled = c;
    *out = p;
    return MI_OK;
}

const char* selcal_state_ok(const SelcalRowState* state, size_t rows, const SelcalPlan& plan) {
    const auto pair_ok = [&](uint32_t p) { return p <= 0xFFFFu && (p & 0xFFu) < (p >> 8) && (p >> 8) < plan.ntones; };
    for (size_t r = 0; r < rows; ++r) {
        const SelcalRowState& s = state[r];
        if (s.zero)
            return "the zero field is not 0";
        bool ok = false;
        switch (s.phase) {
        case MI_SELCAL_IDLE:
            ok = s.pair1 == MI_SELCAL_NONE && s.pair2 == MI_SELCAL_NONE && !s.run1 && !s.run2 && !s.gap && !s.first_window;
            break;
        case MI_SELCAL_FIRST:
            ok = pair_ok(s.pair1) && s.pair2 == MI_SELCAL_NONE && s.run1 >= 1 && s.run1 <= plan.max_run && !s.run2 && !s.gap;
            break;
        case MI_SELCAL_OVER:
            ok = pair_ok(s.pair1) && s.pair2 == MI_SELCAL_NONE && s.run1 == plan.max_run + 1 && !s.run2 && !s.gap;
            break;
        case MI_SELCAL_GAP:
            ok = pair_ok(s.pair1) && s.pair2 == MI_SELCAL_NONE && s.run1 >= plan.min_run && s.run1 <= plan.max_run && !s.run2 && s.gap >= 1 &&
                 s.gap <= plan.max_gap;
            break;
        case MI_SELCAL_SECOND:
        case MI_SELCAL_DONE:
            ok = pair_ok(s.pair1) && pair_ok(s.pair2) && s.pair1 != s.pair2 && s.run1 >= plan.min_run && s.run1 <= plan.max_run && s.gap <= plan.max_gap &&
                 (s.phase == MI_SELCAL_DONE ? s.run2 == plan.min_run : s.run2 >= 1 && s.run2 < plan.min_run);
            break;
        default:
            return "an unknown decoder phase";
        }
        if (!ok)
            return "an impossible decoder state (pairs, runs or gap that the phase cannot have)";
    }
    return nullptr;
}

namespace {

// items 0 .. 4 of the header over the 2000 samples at x
mi_selcal_window_record selcal_window_record(const float* x, const float* w, const SelcalPlan& plan) {
    float y[MI_SELCAL_WINDOW], s[64], p[MI_SELCAL_MAX_TONES];
    for (int j = 0; j < MI_SELCAL_WINDOW; ++j)
        y[j] = x[j] * w[j];
    for (int l = 0; l < 64; ++l) {
        s[l] = y[l] * y[l];
        for (int j = l + 64; j < MI_SELCAL_WINDOW; j += 64)
            s[l] = s[l] + y[j] * y[j];
    }
    for (int h = 32; h >= 1; h /= 2)
        for (int l = 0; l < h; ++l)
            s[l] = s[l] + s[l + h];
    const float E = s[0];
    const int nt = static_cast<int>(plan.ntones);
    for (int t = 0; t < nt; ++t) {
        p[t] = 0.0f;
        if (E == 0.0f)  // a silent window: the powers are zero by definition
            continue;
        const float c = plan.coeff[t];
        float q1 = 0.0f, q2 = 0.0f;
        for (int j = 0; j < MI_SELCAL_WINDOW; ++j) {
            const float q0 = c * q1 - q2 + y[j];
            q2 = q1;
            q1 = q0;
        }
        p[t] = q1 * q1 + q2 * q2 - q1 * q2 * c;
    }
    int i0 = 0, i1 = -1, i2 = -1;
    for (int t = 1; t < nt; ++t) {
        if (p[t] > p[i0]) {
            i2 = i1;
            i1 = i0;
            i0 = t;
        } else if (i1 < 0 || p[t] > p[i1]) {
            i2 = i1;
            i1 = t;
        } else if (i2 < 0 || p[t] > p[i2]) {
            i2 = t;
        }
    }
    const float pb = p[i0], ps = p[i1], pt = i2 < 0 ? 0.0f : p[i2];
    const bool named = E >= plan.min_energy && pb + ps >= plan.tc * E && pb <= plan.max_twist * ps && ps >= plan.min_separation * pt;
    const uint32_t lo = static_cast<uint32_t>(i0 < i1 ? i0 : i1), hi = static_cast<uint32_t>(i0 < i1 ? i1 : i0);
    return mi_selcal_window_record{static_cast<uint8_t>(i0), static_cast<uint8_t>(i1), static_cast<uint8_t>(i2 < 0 ? MI_SELCAL_NONE8 : i2), 0, pb, ps, pt, E,
                                   named ? lo | hi << 8 : MI_SELCAL_NONE};
}

}  // namespace
}  // namespace mi

extern "C" int mi_selcal_table(const mi_selcal_cfg* cfg, uint32_t* ntones, float* freq, float* coeff, char* letter) {
    mi_selcal_cfg c{};
    if (cfg) {
        c.mode = cfg->mode;
        c.ntones = cfg->ntones;
        std::memcpy(c.freq, cfg->freq, sizeof(c.freq));
    }
    mi::SelcalPlan p;
    if (const int rc = mi::selcal_plan(&c, &p))
        return rc;
    if (ntones)
        *ntones = p.ntones;
    for (uint32_t t = 0; t < p.ntones; ++t) {
        if (freq)
            freq[t] = p.freq[t];
        if (coeff)
            coeff[t] = p.coeff[t];
        if (letter)
            letter[t] = p.letter[t];
    }
    return MI_OK;
}

extern "C" int mi_selcal_settings(const mi_selcal_cfg* cfg, mi_selcal_cfg* out, float* c) {
    if (!out)
        return fail(MI_ERR_INVALID, "NULL argument");
    mi::SelcalPlan p;
    if (const int rc = mi::selcal_plan(cfg, &p))
        return rc;
    *out = p.filled;
    if (c)
        *c = p.c;
    return MI_OK;
}

extern "C" int mi_selcal_window(float* out) {
    if (!out)
        return fail(MI_ERR_INVALID, "NULL argument");
    mi::selcal_window(out);
    return MI_OK;
}

extern "C" int mi_selcal_code_text(uint32_t mode, const uint8_t* tones, char* out) {
    if (!tones || !out)
        return fail(MI_ERR_INVALID, "NULL argument");
    if (mode != MI_SELCAL_16 && mode != MI_SELCAL_32 && mode != MI_SELCAL_CUSTOM)
        return fail(MI_ERR_INVALID, "SELCAL stage: mode must be MI_SELCAL_16, MI_SELCAL_32 or MI_SELCAL_CUSTOM");
    const uint32_t n = mode == MI_SELCAL_16 ? 16 : 32, step = mode == MI_SELCAL_16 ? 2 : 1;
    for (int i = 0; i < 4; ++i) {
        if (tones[i] >= n)
            return fail(MI_ERR_INVALID, "SELCAL stage: a tone index beyond the mode's table");
        out[i + (i >= 2)] = mode == MI_SELCAL_CUSTOM ? '?' : mi::kSelcalLetter[tones[i] * step];
    }
    out[2] = '-';
    out[5] = '\0';
    return MI_OK;
}

extern "C" int mi_selcal_plan_host(const mi_selcal_cfg* cfg, const uint8_t* row_enabled, int rows, int nbatches, const float* plane, size_t row_stride,
                                   void* state_inout, mi_selcal_window_record* windows, mi_selcal_code* codes, size_t max_codes, uint32_t* row_first_code,
                                   uint32_t* count) {
    if (!row_enabled || !plane || !state_inout || !codes || !row_first_code || !count)
        return fail(MI_ERR_INVALID, "NULL argument");
    if (rows < 1 || nbatches < 1 || max_codes < 1)
        return fail(MI_ERR_INVALID, "SELCAL plan needs rows >= 1, nbatches >= 1 and max_codes >= 1");
    if (row_stride < static_cast<size_t>(nbatches) * mi::kWaveBatch)
        return fail(MI_ERR_INVALID, "a row stride is shorter than the call");
    mi::SelcalPlan plan;
    if (const int rc = mi::selcal_plan(cfg, &plan))
        return rc;
    if (static_cast<uint64_t>(rows) * mi::selcal_max_codes(plan.min_run, static_cast<uint64_t>(nbatches)) > UINT32_MAX)
        return fail(MI_ERR_INVALID, "SELCAL plan: the codes of the call do not fit the 32-bit count");
    std::vector<mi::SelcalRowState> blob(static_cast<size_t>(rows));
    std::memcpy(blob.data(), state_inout, blob.size() * sizeof(mi::SelcalRowState));
    if (const char* const why = mi::selcal_state_ok(blob.data(), blob.size(), plan))
        return fail(MI_ERR_INVALID, std::string("SELCAL plan: malformed state blob: ") + why);
    std::vector<float> w(MI_SELCAL_WINDOW), x(MI_SELCAL_HOP + static_cast<size_t>(nbatches) * mi::kWaveBatch);
    mi::selcal_window(w.data());
    const uint32_t nwin = 2u * static_cast<uint32_t>(nbatches);
    uint32_t k = 0;
    for (int r = 0; r < rows; ++r) {
        row_first_code[r] = k;
        if (!row_enabled[r])
            continue;
        mi::SelcalRowState& st = blob[static_cast<size_t>(r)];
        const float* const row = plane + static_cast<size_t>(r) * row_stride;
        // x = the last 1000 carried samples, then the call's
        std::memcpy(x.data(), st.x + (MI_SELCAL_HISTORY - MI_SELCAL_HOP), MI_SELCAL_HOP * sizeof(float));
        std::memcpy(x.data() + MI_SELCAL_HOP, row, static_cast<size_t>(nbatches) * mi::kWaveBatch * sizeof(float));
        mi::SelcalDecoder d{st.phase, st.pair1, st.pair2, st.run1, st.run2, st.gap, st.first_window};
        for (uint32_t i = 0; i < nwin; ++i) {
            const mi_selcal_window_record rec = mi::selcal_window_record(x.data() + static_cast<size_t>(i) * MI_SELCAL_HOP, w.data(), plan);
            if (windows)
                windows[static_cast<size_t>(r) * nwin + i] = rec;
            const uint32_t n = st.window + i;
            if (mi::selcal_step(d, rec.pair, n, plan.min_run, plan.max_run, plan.max_gap)) {
                if (k < max_codes)
                    codes[k] = mi_selcal_code{static_cast<uint32_t>(r), st.seq, {static_cast<uint8_t>(d.pair1 & 0xFF), static_cast<uint8_t>(d.pair1 >> 8),
                                              static_cast<uint8_t>(d.pair2 & 0xFF), static_cast<uint8_t>(d.pair2 >> 8)},
                                              d.first_window, n, d.run1, d.gap, i / 2};
                ++k;
                st.seq += 1;
            }
        }
        st.window += nwin;
        st.phase = d.phase, st.pair1 = d.pair1, st.pair2 = d.pair2, st.run1 = d.run1, st.run2 = d.run2, st.gap = d.gap, st.first_window = d.first_window;
        std::memcpy(st.x, row + static_cast<size_t>(nbatches) * mi::kWaveBatch - MI_SELCAL_HISTORY, MI_SELCAL_HISTORY * sizeof(float));
    }
    row_first_code[rows] = k;
    count[0] = k;
    count[1] = k < max_codes ? k : static_cast<uint32_t>(max_codes);
    std::memcpy(state_inout, blob.data(), blob.size() * sizeof(mi::SelcalRowState));
    return MI_OK;
}

// ---- ACARS decoder stage, host side (include/mi_airband.h "ACARS decoder stage"): the settings' check, the templates, the blob's
// check, the record and its text, and the twin of acars.hip -- one row, one batch, one hypothesis and one slot at a time, then the
// walker over the batch's slots.  The bit, the walker's step, the sync's choice and the timing move are poststage.hpp's.
namespace mi {

int acars_plan(const mi_acars_cfg* cfg, AcarsPlan* out) {
    mi_acars_cfg c{};
    if (cfg)
        c = *cfg;
    if (c.sync_errors == 0)
        c.sync_errors = 2;
    if (c.sync_errors != MI_ACARS_SYNC_EXACT && c.sync_errors > 4)
        return fail(MI_ERR_INVALID, "ACARS stage: sync_errors must be within 1 .. 4 or MI_ACARS_SYNC_EXACT (0 = the default)");
    if (c.keep_bad > 1)
        return fail(MI_ERR_INVALID, "ACARS stage: keep_bad must be 0 or 1");
    if (!std::isfinite(c.min_quality) || c.min_quality < 0.0f)
        return fail(MI_ERR_INVALID, "ACARS stage: min_quality must be finite and not negative (0 = the default)");
    if (c.hold_timing > 1)
        return fail(MI_ERR_INVALID, "ACARS stage: hold_timing must be 0 or 1");
    c.min_quality = c.min_quality + 0.0f;  // (-0.0f is the default too)
    AcarsPlan p{};
    p.sync_errors = c.sync_errors == MI_ACARS_SYNC_EXACT ? 0u : c.sync_errors;
    p.keep_bad = c.keep_bad;
    p.hold_timing = c.hold_timing;
    p.min_quality = c.min_quality;
    p.filled = c;
    *out = p;
    return MI_OK;
}

void acars_templates(float* h1, float* h2) {
    const double pi = 3.14159265358979323846;
    for (int r = 0; r < 20; ++r) {
        h1[r] = static_cast<float>(std::sin(pi * r / 20.0));
        h2[r] = static_cast<float>(std::sin(2.0 * pi * r / 20.0));
    }
}

const char* acars_state_ok(const AcarsRowState* state, size_t rows) {
    for (size_t r = 0; r < rows; ++r) {
        const AcarsRowState& s = state[r];
        if (s.zero)
            return "the zero field is not 0";
        for (int t = 0; t < MI_ACARS_HYPOTHESES; ++t)
            if (s.hist[t] & ~kAcarsMask38)
                return "a hypothesis holds more than 38 change bits";
        if (s.phase > MI_ACARS_FRAME)
            return "an unknown walker phase";
        uint32_t used = 0;
        if (s.phase == MI_ACARS_IDLE) {
            if (s.u | s.prev | s.nbits | s.cur | s.nbytes | s.tail | s.crc | s.parity_errors | s.start_batch | s.start_third | s.tau_sync | s.mismatches | s.end)
                return "an impossible walker state (an idle row with a walker field set)";
        } else {
            bool ok = s.u < 20 && s.tau_sync < 20 && s.prev <= 1 && s.nbits <= 7 && s.cur < (1u << s.nbits) && s.tail <= 2 && s.mismatches <= 4 &&
                      s.start_third < 3u * kWaveBatch;
            if (ok && s.tail == 0)
                ok = s.nbytes < MI_ACARS_MAX_BYTES && s.end == 0;
            else if (ok)
                ok = s.nbytes > MI_ACARS_HEAD_BYTES && s.nbytes <= MI_ACARS_MAX_BYTES && (s.end == 0x03 || s.end == 0x17) &&
                     (s.bytes[s.nbytes - 1] & 0x7Fu) == s.end;
            if (!ok)
                return "an impossible walker state (counters, end or timing that a frame cannot have)";
            used = s.nbytes + (s.tail ? s.tail - 1 : 0);
            uint32_t crc = 0, bad = 0;
            for (uint32_t i = 0; i < used; ++i) {
                crc = acars_crc_byte(crc, s.bytes[i]);
                if (i >= s.nbytes)
                    continue;
                bad += (__builtin_popcount(s.bytes[i]) & 1) ^ 1;
                const uint32_t ch = s.bytes[i] & 0x7Fu;
                if (i >= MI_ACARS_HEAD_BYTES && i + 1 < s.nbytes + (s.tail ? 0u : 1u) && (ch == 0x03 || ch == 0x17))
                    return "an impossible walker state (a frame that goes on behind its ETX / ETB)";
            }
            if (crc != s.crc || bad != s.parity_errors)
                return "an impossible walker state (a crc or parity count that the bytes do not give)";
        }
        for (uint32_t i = used; i < MI_ACARS_RAW_BYTES; ++i)
            if (s.bytes[i])
                return "an impossible walker state (a byte set behind the ones taken)";
    }
    return nullptr;
}

namespace {

mi_acars_frame acars_frame(const AcarsWalker& w, const uint8_t* bytes, uint32_t row, uint32_t end_batch) {
    mi_acars_frame f{};
    f.row = row;
    f.batch = w.start_batch;
    f.third = w.start_third;
    f.tau_sync = static_cast<uint8_t>(w.tau_sync);
    f.tau_end = static_cast<uint8_t>(w.u);
    f.sync_errors = static_cast<uint8_t>(w.mismatches);
    f.crc_ok = w.crc == 0;
    f.nbytes = static_cast<uint16_t>(w.nbytes);
    f.parity_errors = static_cast<uint8_t>(w.parity_errors);
    f.end = static_cast<uint8_t>(w.end);
    f.end_batch = end_batch;
    std::memcpy(f.bytes, bytes, MI_ACARS_RAW_BYTES);
    return f;
}

}  // namespace
}  // namespace mi

extern "C" int mi_acars_settings(const mi_acars_cfg* cfg, mi_acars_cfg* out) {
    if (!out)
        return fail(MI_ERR_INVALID, "NULL argument");
    mi::AcarsPlan p;
    if (const int rc = mi::acars_plan(cfg, &p))
        return rc;
    *out = p.filled;
    return MI_OK;
}

extern "C" int mi_acars_templates(float* h1, float* h2) {
    if (!h1 || !h2)
        return fail(MI_ERR_INVALID, "NULL argument");
    mi::acars_templates(h1, h2);
    return MI_OK;
}

extern "C" uint32_t mi_acars_crc(const uint8_t* bytes, size_t n) {
    if (!bytes && n)
        return 0xFFFFFFFFu;
    uint32_t crc = 0;
    for (size_t i = 0; i < n; ++i)
        crc = mi::acars_crc_byte(crc, bytes[i]);
    return crc;
}

extern "C" int mi_acars_frame_text(const mi_acars_frame* f, mi_acars_text* out) {
    if (!f || !out)
        return fail(MI_ERR_INVALID, "NULL argument");
    if (f->nbytes <= MI_ACARS_HEAD_BYTES || f->nbytes > MI_ACARS_MAX_BYTES)
        return fail(MI_ERR_INVALID, "ACARS stage: a frame's nbytes must be within 13 .. 240");
    std::memset(out, 0, sizeof(*out));
    const auto put = [&](char* dst, int first, int n) {
        for (int i = 0; i < n; ++i) {
            const int ch = f->bytes[first + i] & 0x7F;
            dst[i] = ch >= 0x20 && ch <= 0x7E ? static_cast<char>(ch) : '.';
        }
    };
    put(out->mode, 0, 1);
    put(out->address, 1, 7);
    put(out->ack, 8, 1);
    put(out->label, 9, 2);
    put(out->block_id, 11, 1);
    put(out->text, MI_ACARS_HEAD_BYTES, f->nbytes - MI_ACARS_HEAD_BYTES - 1);
    return MI_OK;
}

extern "C" int mi_acars_plan_host(const mi_acars_cfg* cfg, const uint8_t* row_enabled, int rows, int nbatches, const float* plane, size_t row_stride,
                                  void* state_inout, uint32_t* bits, float* q, mi_acars_frame* frames, size_t max_frames, uint32_t* row_first_frame,
                                  uint32_t* count) {
    if (!row_enabled || !plane || !state_inout || !frames || !row_first_frame || !count)
        return fail(MI_ERR_INVALID, "NULL argument");
    if (rows < 1 || nbatches < 1 || max_frames < 1)
        return fail(MI_ERR_INVALID, "ACARS plan needs rows >= 1, nbatches >= 1 and max_frames >= 1");
    if (row_stride < static_cast<size_t>(nbatches) * mi::kWaveBatch)
        return fail(MI_ERR_INVALID, "a row stride is shorter than the call");
    mi::AcarsPlan plan;
    if (const int rc = mi::acars_plan(cfg, &plan))
        return rc;
    if (static_cast<uint64_t>(rows) * mi::acars_max_frames(static_cast<uint64_t>(nbatches)) > UINT32_MAX)
        return fail(MI_ERR_INVALID, "ACARS plan: the frames of the call do not fit the 32-bit count");
    std::vector<mi::AcarsRowState> blob(static_cast<size_t>(rows));
    std::memcpy(blob.data(), state_inout, blob.size() * sizeof(mi::AcarsRowState));
    if (const char* const why = mi::acars_state_ok(blob.data(), blob.size()))
        return fail(MI_ERR_INVALID, std::string("ACARS plan: malformed state blob: ") + why);
    constexpr int kLead = MI_ACARS_HISTORY + 2, kTau = MI_ACARS_HYPOTHESES, kBits = MI_ACARS_BITS, kWords = MI_ACARS_BIT_WORDS;
    float h1[20], h2[20];
    mi::acars_templates(h1, h2);
    std::vector<float> s(kLead + static_cast<size_t>(nbatches) * mi::kWaveBatch);
    uint32_t k = 0;
    for (int r = 0; r < rows; ++r) {
        row_first_frame[r] = k;
        if (!row_enabled[r])
            continue;
        mi::AcarsRowState& st = blob[static_cast<size_t>(r)];
        const float* const row = plane + static_cast<size_t>(r) * row_stride;
        s[0] = s[1] = 0.0f;
        std::memcpy(s.data() + 2, st.x, sizeof(st.x));
        std::memcpy(s.data() + kLead, row, static_cast<size_t>(nbatches) * mi::kWaveBatch * sizeof(float));
        mi::AcarsWalker w{st.phase, st.u, st.prev, st.nbits, st.cur, st.nbytes, st.tail, st.crc, st.parity_errors, st.start_batch, st.start_third,
                          st.tau_sync, st.mismatches, st.end};
        const auto event = [&](int ev, int b) {  // what a step's answer does
            if (ev == mi::kAcarsDone) {
                if (w.crc == 0 || plan.keep_bad) {
                    if (k < max_frames)
                        frames[k] = mi::acars_frame(w, st.bytes, static_cast<uint32_t>(r), static_cast<uint32_t>(b));
                    ++k;
                }
                mi::acars_idle(w, st.bytes);
            }
        };
        for (int b = 0; b < nbatches; ++b) {
            const float* const blk = s.data() + static_cast<size_t>(b) * mi::kWaveBatch;  // staged: blk[kLead + n] is the batch's sample n
            uint32_t word[kTau][kWords] = {};
            float Q[kTau], qs[kBits];
            for (int t = 0; t < kTau; ++t) {
                for (int j = 0; j < kBits; ++j)
                    word[t][j / 32] |= mi::acars_bit(blk, h1, h2, t, j, &qs[j]) << (j % 32);
                float lane[64];
                for (int l = 0; l < 64; ++l) {
                    lane[l] = qs[l];
                    for (int j = l + 64; j < kBits; j += 64)
                        lane[l] = lane[l] + qs[j];
                }
                for (int h = 32; h >= 1; h /= 2)
                    for (int l = 0; l < h; ++l)
                        lane[l] = lane[l] + lane[l + h];
                Q[t] = lane[0];
            }
            const size_t blk_i = static_cast<size_t>(r) * static_cast<size_t>(nbatches) + static_cast<size_t>(b);
            if (bits)
                std::memcpy(bits + blk_i * kTau * kWords, word, sizeof(word));
            if (q)
                std::memcpy(q + blk_i * kTau, Q, sizeof(Q));
            int skip = 0;
            if (w.phase == MI_ACARS_FRAME && !plan.hold_timing) {
                const int move = mi::acars_retime(w, Q);
                skip = move == mi::kAcarsSkip;
                if (move == mi::kAcarsReplay)
                    event(mi::acars_step(w, st.bytes, static_cast<uint32_t>(st.hist[0] & 1u)), b);
            }
            for (int j = 0; j < kBits; ++j) {
                uint32_t mism[kTau];
                for (int t = 0; t < kTau; ++t) {
                    const uint64_t h39 = st.hist[t] << 1 | (word[t][j / 32] >> (j % 32) & 1u);
                    mism[t] = static_cast<uint32_t>(__builtin_popcountll(h39 ^ mi::kAcarsSync));
                    st.hist[t] = h39 & mi::kAcarsMask38;
                }
                if (w.phase == MI_ACARS_FRAME) {
                    if (skip)
                        skip = 0;
                    else
                        event(mi::acars_step(w, st.bytes, word[w.u][j / 32] >> (j % 32) & 1u), b);
                } else if (const int u = mi::acars_pick(mism, Q, plan.sync_errors, plan.min_quality); u >= 0) {
                    mi::acars_open(w, u, mism[u], st.batch + static_cast<uint32_t>(b), j);
                }
            }
        }
        st.batch += static_cast<uint32_t>(nbatches);
        st.phase = w.phase, st.u = w.u, st.prev = w.prev, st.nbits = w.nbits, st.cur = w.cur, st.nbytes = w.nbytes, st.tail = w.tail, st.crc = w.crc;
        st.parity_errors = w.parity_errors, st.start_batch = w.start_batch, st.start_third = w.start_third, st.tau_sync = w.tau_sync;
        st.mismatches = w.mismatches, st.end = w.end;
        std::memcpy(st.x, row + static_cast<size_t>(nbatches) * mi::kWaveBatch - MI_ACARS_HISTORY, sizeof(st.x));
    }
    row_first_frame[rows] = k;
    count[0] = k;
    count[1] = k < max_frames ? k : static_cast<uint32_t>(max_frames);
    std::memcpy(state_inout, blob.data(), blob.size() * sizeof(mi::AcarsRowState));
    return MI_OK;
}

// ---- SAME decoder stage, host side (include/mi_airband.h "SAME decoder stage"): the settings' check, the templates, the blob's
// check, a header's text, and the twin of same.hip -- one row, one batch, one hypothesis and one bit at a time, then the walker over
// the batch's indices.  The bit, the walker's step, the sync's choice, the assembler and the timing move are poststage.hpp's.
namespace mi {

int same_plan(const mi_same_cfg* cfg, SamePlan* out) {
    mi_same_cfg c{};
    if (cfg)
        c = *cfg;
    if (c.sync_errors == 0)
        c.sync_errors = 4;
    if (c.sync_errors != MI_SAME_SYNC_EXACT && c.sync_errors > 4)
        return fail(MI_ERR_INVALID, "SAME stage: sync_errors must be within 1 .. 4 or MI_SAME_SYNC_EXACT (0 = the default)");
    if (c.max_bad == 0)
        c.max_bad = 4;
    if (c.max_bad > 16)
        return fail(MI_ERR_INVALID, "SAME stage: max_bad must be within 1 .. 16 (0 = the default)");
    if (c.gap_batches == 0)
        c.gap_batches = 20;
    if (c.gap_batches > 1000)
        return fail(MI_ERR_INVALID, "SAME stage: gap_batches must be within 1 .. 1000 (0 = the default)");
    if (!std::isfinite(c.min_quality) || c.min_quality < 0.0f)
        return fail(MI_ERR_INVALID, "SAME stage: min_quality must be finite and not negative (0 = the default)");
    if (!std::isfinite(c.space_gain) || c.space_gain < 0.0f)
        return fail(MI_ERR_INVALID, "SAME stage: space_gain must be finite and above 0 (0 = the default)");
    if (c.hold_timing > 1)
        return fail(MI_ERR_INVALID, "SAME stage: hold_timing must be 0 or 1");
    c.min_quality = c.min_quality + 0.0f;  // (-0.0f is the default too)
    if (c.space_gain == 0.0f)
        c.space_gain = 1.0f;
    SamePlan p{};
    p.sync_errors = c.sync_errors == MI_SAME_SYNC_EXACT ? 0u : c.sync_errors;
    p.max_bad = c.max_bad;
    p.gap_batches = c.gap_batches;
    p.hold_timing = c.hold_timing;
    p.min_quality = c.min_quality;
    p.space_gain = c.space_gain;
    p.filled = c;
    *out = p;
    return MI_OK;
}

void same_templates(float* T) {
    const double pi = 3.14159265358979323846;
    for (int r = 0; r < kSameTemplate; ++r) {
        T[r] = static_cast<float>(std::cos(2.0 * pi * 4.0 * r / 768.0));
        T[kSameTemplate + r] = static_cast<float>(std::sin(2.0 * pi * 4.0 * r / 768.0));
        T[2 * kSameTemplate + r] = static_cast<float>(std::cos(2.0 * pi * 3.0 * r / 768.0));
        T[3 * kSameTemplate + r] = static_cast<float>(std::sin(2.0 * pi * 3.0 * r / 768.0));
    }
}

const char* same_state_ok(const SameRowState* state, size_t rows, const SamePlan& plan) {
    for (size_t r = 0; r < rows; ++r) {
        const SameRowState& s = state[r];
        const SameWalker& w = s.w;
        if (s.zero)
            return "the zero field is not 0";
        if (s.grid >= MI_SAME_BIT_UNITS || s.grid % 16 != 0)
            return "a grid that is no multiple of 16 below 768";
        if (w.phase > MI_SAME_BURST)
            return "an unknown walker phase";
        if (w.phase == MI_SAME_IDLE) {
            if (w.u | w.kind | w.nbits | w.cur | w.nbytes | w.nbad | w.plus | w.dashes | w.start_batch | w.start_unit)
                return "an impossible walker state (an idle row with a burst field set)";
            if (w.deaf > MI_SAME_DEAF)
                return "an impossible walker state (deaf beyond 64)";
        } else {
            if (w.kind != MI_SAME_HEADER || w.u > 15 || w.nbits > 7 || w.cur >= (1u << w.nbits) || w.nbytes < 4 || w.nbytes >= MI_SAME_MAX_BYTES || w.deaf ||
                w.start_unit >= MI_SAME_BATCH_UNITS || std::memcmp(s.bytes[0], "ZCZC", 4) != 0 || (w.an && w.akind != MI_SAME_HEADER))
                return "an impossible walker state (counters, kind or timing that a burst cannot have)";
            SameWalker t{};
            t.nbytes = 4;
            uint8_t copy[MI_SAME_RAW_BYTES] = {'Z', 'C', 'Z', 'C'};
            uint32_t trunc = 0;
            for (uint32_t i = 4; i < w.nbytes; ++i)
                for (int bit = 0; bit < 8; ++bit)
                    if (same_step(t, copy, s.bytes[0][i] >> bit & 1u, plan.max_bad, &trunc))
                        return "an impossible walker state (bytes that would have ended the burst)";
            if (t.nbad != w.nbad || t.plus != w.plus || t.dashes != w.dashes)
                return "an impossible walker state (nbad, plus or dashes that the bytes do not give)";
        }
        if (w.an > 2 || w.akind > MI_SAME_EOM || w.atrunc0 > 1 || w.atrunc1 > 1 || w.astart_unit >= MI_SAME_BATCH_UNITS || w.aidle >= plan.gap_batches)
            return "an impossible assembler state (count, kind, flag, aidle or unit out of range)";
        const uint32_t len[3] = {w.phase == MI_SAME_BURST ? w.nbytes : 0u, w.an >= 1 ? w.alen0 : 0u, w.an >= 2 ? w.alen1 : 0u};
        if ((w.an < 1 && (w.alen0 | w.atrunc0 | w.akind | w.aidle | w.astart_batch | w.astart_unit)) || (w.an < 2 && (w.alen1 | w.atrunc1)))
            return "an impossible assembler state (a field set that its bursts do not use)";
        for (uint32_t i = 1; i <= w.an; ++i)
            if (len[i] < 4 || len[i] > MI_SAME_MAX_BYTES || (w.akind == MI_SAME_EOM && len[i] != 4))
                return "an impossible assembler state (a burst's length)";
        for (int k = 0; k < 3; ++k)
            for (uint32_t i = len[k]; i < MI_SAME_RAW_BYTES; ++i)
                if (s.bytes[k][i])
                    return "an impossible state (a byte set behind a burst's length)";
    }
    return nullptr;
}

}  // namespace mi

extern "C" int mi_same_settings(const mi_same_cfg* cfg, mi_same_cfg* out) {
    if (!out)
        return fail(MI_ERR_INVALID, "NULL argument");
    mi::SamePlan p;
    if (const int rc = mi::same_plan(cfg, &p))
        return rc;
    *out = p.filled;
    return MI_OK;
}

extern "C" int mi_same_templates(float* out) {
    if (!out)
        return fail(MI_ERR_INVALID, "NULL argument");
    mi::same_templates(out);
    return MI_OK;
}

extern "C" int mi_same_message_text(const mi_same_message* m, mi_same_text* out) {
    if (!m || !out)
        return fail(MI_ERR_INVALID, "NULL argument");
    if (m->kind != MI_SAME_HEADER || m->nbytes > MI_SAME_MAX_BYTES || !mi::same_fields_ok(m->bytes, m->nbytes, MI_SAME_HEADER))
        return fail(MI_ERR_INVALID, "SAME stage: not a header whose fields are in order");
    std::memset(out, 0, sizeof(*out));
    const uint8_t* const b = m->bytes;
    std::memcpy(out->originator, b + 5, 3);
    std::memcpy(out->event, b + 9, 3);
    const uint32_t nloc = (m->nbytes - 35u) / 7u;
    out->nlocations = nloc;
    for (uint32_t i = 0; i < nloc; ++i)
        std::memcpy(out->locations[i], b + 13 + 7 * i, 6);
    const uint8_t* const t = b + 12 + 7 * nloc;  // '+'
    std::memcpy(out->purge, t + 1, 4);
    std::memcpy(out->issue, t + 6, 7);
    std::memcpy(out->station, t + 14, 8);
    return MI_OK;
}

extern "C" int mi_same_plan_host(const mi_same_cfg* cfg, const uint8_t* row_enabled, int rows, int nbatches, const float* plane, size_t row_stride,
                                 void* state_inout, uint32_t* bits, float* q, mi_same_message* messages, size_t max_messages, uint32_t* row_first_message,
                                 uint32_t* count) {
    if (!row_enabled || !plane || !state_inout || !messages || !row_first_message || !count)
        return fail(MI_ERR_INVALID, "NULL argument");
    if (rows < 1 || nbatches < 1 || max_messages < 1)
        return fail(MI_ERR_INVALID, "SAME plan needs rows >= 1, nbatches >= 1 and max_messages >= 1");
    if (row_stride < static_cast<size_t>(nbatches) * mi::kWaveBatch)
        return fail(MI_ERR_INVALID, "a row stride is shorter than the call");
    mi::SamePlan plan;
    if (const int rc = mi::same_plan(cfg, &plan))
        return rc;
    if (static_cast<uint64_t>(rows) * (2 * (2 + 66 * static_cast<uint64_t>(nbatches) / 65) + 1) > UINT32_MAX)
        return fail(MI_ERR_INVALID, "SAME plan: the messages of the call do not fit the 32-bit count");
    std::vector<mi::SameRowState> blob(static_cast<size_t>(rows));
    std::memcpy(blob.data(), state_inout, blob.size() * sizeof(mi::SameRowState));
    if (const char* const why = mi::same_state_ok(blob.data(), blob.size(), plan))
        return fail(MI_ERR_INVALID, std::string("SAME plan: malformed state blob: ") + why);
    constexpr int kLead = MI_SAME_HISTORY + 2, kTau = MI_SAME_HYPOTHESES, kWords = MI_SAME_BIT_WORDS;
    std::vector<float> T(4 * mi::kSameTemplate);
    mi::same_templates(T.data());
    std::vector<float> s(kLead + static_cast<size_t>(nbatches) * mi::kWaveBatch);
    uint32_t k = 0;
    mi_same_message m;
    for (int r = 0; r < rows; ++r) {
        row_first_message[r] = k;
        if (!row_enabled[r])
            continue;
        mi::SameRowState& st = blob[static_cast<size_t>(r)];
        const float* const row = plane + static_cast<size_t>(r) * row_stride;
        s[0] = s[1] = 0.0f;
        std::memcpy(s.data() + 2, st.x, sizeof(st.x));
        std::memcpy(s.data() + kLead, row, static_cast<size_t>(nbatches) * mi::kWaveBatch * sizeof(float));
        mi::SameWalker& w = st.w;
        uint8_t* const bytes = st.bytes[0];
        const auto record = [&](bool closed) {
            if (!closed)
                return;
            if (k < max_messages)
                messages[k] = m;
            ++k;
        };
        const auto step = [&](uint32_t c, int b) {  // one bit of the chosen hypothesis inside a burst
            uint32_t trunc = 0;
            if (mi::same_step(w, bytes, c, plan.max_bad, &trunc))
                record(mi::same_burst_end(w, bytes, trunc, static_cast<uint32_t>(r), static_cast<uint32_t>(b), &m));
        };
        for (int b = 0; b < nbatches; ++b) {
            const float* const blk = s.data() + static_cast<size_t>(b) * mi::kWaveBatch;  // staged: blk[kLead + n] is the batch's sample n
            uint32_t word[kTau][kWords] = {};
            int r0[kTau], cnt[kTau];
            float Q[kTau], qs[MI_SAME_MAX_BITS];
            for (int t = 0; t < kTau; ++t) {
                r0[t] = mi::same_first(st.grid, t);
                cnt[t] = mi::same_count(r0[t]);
                for (int j = 0; j < cnt[t]; ++j)
                    word[t][j / 32] |= mi::same_bit(blk, T.data(), r0[t] + MI_SAME_BIT_UNITS * j, plan.space_gain, &qs[j]) << (j % 32);
                word[t][3] = static_cast<uint32_t>(cnt[t]);
                float lane[64];
                for (int l = 0; l < 64; ++l)
                    lane[l] = l + 64 < cnt[t] ? qs[l] + qs[l + 64] : qs[l];
                for (int h = 32; h >= 1; h /= 2)
                    for (int l = 0; l < h; ++l)
                        lane[l] = lane[l] + lane[l + h];
                Q[t] = lane[0];
            }
            const size_t blk_i = static_cast<size_t>(r) * static_cast<size_t>(nbatches) + static_cast<size_t>(b);
            if (bits)
                std::memcpy(bits + blk_i * kTau * kWords, word, sizeof(word));
            if (q)
                std::memcpy(q + blk_i * kTau, Q, sizeof(Q));
            const int ahead = mi::same_ahead(st.grid);
            record(mi::same_gap(w, bytes, plan.gap_batches, static_cast<uint32_t>(r), static_cast<uint32_t>(b), &m));
            int skip = 0;
            if (w.phase == MI_SAME_BURST && !plan.hold_timing) {
                const int move = mi::same_retime(w, Q);
                skip = move == mi::kSameSkip;
                if (move == mi::kSameReplay)
                    step(static_cast<uint32_t>(st.hist[15] & 1u), b);
            }
            for (int i = 0; i < cnt[15]; ++i) {
                uint32_t mk[kTau], c[kTau];
                for (int t = 0; t < kTau; ++t) {
                    const int j = i - (t < ahead);
                    if (j >= 0) {
                        c[t] = word[t][j / 32] >> (j % 32) & 1u;
                        st.hist[t] = st.hist[t] << 1 | c[t];
                    } else {
                        c[t] = static_cast<uint32_t>(st.hist[t] & 1u);
                    }
                    mk[t] = mi::same_mismatch(st.hist[t]);
                }
                if (w.phase == MI_SAME_BURST) {
                    if (skip)
                        skip = 0;
                    else
                        step(c[w.u], b);
                } else if (w.deaf) {
                    --w.deaf;
                } else if (const int u = mi::same_pick(mk, Q, plan.sync_errors, plan.min_quality); u >= 0) {
                    const uint32_t kind = mk[u] >> 8;
                    record(mi::same_open(w, bytes, u, kind, st.batch + static_cast<uint32_t>(b), r0[u] + MI_SAME_BIT_UNITS * (i - (u < ahead)),
                                         static_cast<uint32_t>(r), static_cast<uint32_t>(b), &m));
                    if (kind == MI_SAME_EOM)
                        record(mi::same_burst_end(w, bytes, 0, static_cast<uint32_t>(r), static_cast<uint32_t>(b), &m));
                }
            }
            const uint32_t next = (st.grid + 80u) % MI_SAME_BIT_UNITS;
            for (int t = 0; t < mi::same_ahead(next); ++t) {  // the bit that waits for the next batch's first index
                const int j = cnt[t] - 1;
                st.hist[t] = st.hist[t] << 1 | (word[t][j / 32] >> (j % 32) & 1u);
            }
            st.grid = next;
        }
        st.batch += static_cast<uint32_t>(nbatches);
        std::memcpy(st.x, row + static_cast<size_t>(nbatches) * mi::kWaveBatch - MI_SAME_HISTORY, sizeof(st.x));
    }
    row_first_message[rows] = k;
    count[0] = k;
    count[1] = k < max_messages ? k : static_cast<uint32_t>(max_messages);
    std::memcpy(state_inout, blob.data(), blob.size() * sizeof(mi::SameRowState));
    return MI_OK;
}

// ---- ELT detector stage, host side (include/mi_airband.h "ELT detector stage"): the settings' check, the window, the coefficients,
// the blob's check, an event's text, and the twin of elt.hip -- one row and one frame at a time, the 32 recurrences side by side, then
// the walker over the row's frames.  The walker's step is poststage.hpp's.
namespace mi {

void elt_window(float* w) {
    const double pi = 3.14159265358979323846;
    for (int j = 0; j < MI_ELT_FRAME / 2; ++j)
        w[j] = w[MI_ELT_FRAME - 1 - j] = static_cast<float>(0.5 - 0.5 * std::cos(2.0 * pi * j / (MI_ELT_FRAME - 1)));
}

int elt_plan(const mi_elt_cfg* cfg, EltPlan* out) {
    mi_elt_cfg c{};
    if (cfg)
        c = *cfg;
    c.min_energy = c.min_energy == 0.0f ? 1e-4f : c.min_energy;
    c.min_tonality = c.min_tonality == 0.0f ? 0.5f : c.min_tonality;
    c.band_lo = c.band_lo ? c.band_lo : 4;
    c.band_hi = c.band_hi ? c.band_hi : (c.band_lo > 26 ? c.band_lo : 26);
    c.min_span = c.min_span ? c.min_span : 10;
    c.min_len = c.min_len ? c.min_len : 40;
    c.max_len = c.max_len ? c.max_len : (c.min_len > 120 ? c.min_len : 120);
    c.max_step = c.max_step ? c.max_step : 3;
    c.max_drop = c.max_drop ? c.max_drop : 2;
    c.max_gap = c.max_gap ? c.max_gap : 10;
    c.min_sweeps = c.min_sweeps ? c.min_sweeps : 6;
    const uint32_t top = MI_ELT_BIN0 + MI_ELT_BINS - 1;
    if (!in_range(c.min_energy, 1e-12f, 1e6f))
        return fail(MI_ERR_INVALID, "ELT stage: min_energy must be finite and within 1e-12 .. 1e6 (0 = the default)");
    if (!in_range(c.min_tonality, 0.01f, 1.5f))
        return fail(MI_ERR_INVALID, "ELT stage: min_tonality must be within 0.01 .. 1.5 (0 = the default)");
    if (c.band_lo < MI_ELT_BIN0 || c.band_lo > top)
        return fail(MI_ERR_INVALID, "ELT stage: band_lo must be within 2 .. 33 bins (0 = the default)");
    if (c.band_hi < c.band_lo || c.band_hi > top)
        return fail(MI_ERR_INVALID, "ELT stage: band_hi must be within band_lo .. 33 bins (0 = the default)");
    if (c.min_span < 1 || c.min_span > MI_ELT_BINS - 1)
        return fail(MI_ERR_INVALID, "ELT stage: min_span must be within 1 .. 31 bins (0 = the default)");
    if (c.min_len < 2 || c.min_len > 4096)
        return fail(MI_ERR_INVALID, "ELT stage: min_len must be within 2 .. 4096 frames (0 = the default)");
    if (c.max_len < c.min_len || c.max_len > 65536)
        return fail(MI_ERR_INVALID, "ELT stage: max_len must be within min_len .. 65536 frames (0 = the default)");
    if (c.max_step < 1 || c.max_step > MI_ELT_BINS - 1)
        return fail(MI_ERR_INVALID, "ELT stage: max_step must be within 1 .. 31 bins (0 = the default)");
    if (c.max_drop < 1 || c.max_drop > 64)
        return fail(MI_ERR_INVALID, "ELT stage: max_drop must be within 1 .. 64 frames (0 = the default)");
    if (c.max_gap < 1 || c.max_gap > 1024)
        return fail(MI_ERR_INVALID, "ELT stage: max_gap must be within 1 .. 1024 frames (0 = the default)");
    if (c.min_sweeps < 1 || c.min_sweeps > 1024)
        return fail(MI_ERR_INVALID, "ELT stage: min_sweeps must be within 1 .. 1024 sweeps (0 = the default)");
    if (c.zero)
        return fail(MI_ERR_INVALID, "ELT stage: the settings' zero field must be 0");
    EltPlan p{};
    float w[MI_ELT_FRAME];
    elt_window(w);
    double sw = 0.0, sw2 = 0.0;
    for (int j = 0; j < MI_ELT_FRAME; ++j) {
        sw += static_cast<double>(w[j]);
        sw2 += static_cast<double>(w[j]) * static_cast<double>(w[j]);
    }
    p.c = static_cast<float>(sw * sw / (2.0 * sw2));
    const double pi = 3.14159265358979323846;
    for (int t = 0; t < MI_ELT_BINS; ++t)
        p.coeff[t] = static_cast<float>(2.0 * std::cos(2.0 * pi * (t + MI_ELT_BIN0) / MI_ELT_FRAME));
    p.min_energy = c.min_energy;
    p.tc = c.min_tonality * p.c;
    p.band_lo = c.band_lo, p.band_hi = c.band_hi, p.min_span = c.min_span, p.min_len = c.min_len, p.max_len = c.max_len;
    p.max_step = c.max_step, p.max_drop = c.max_drop, p.max_gap = c.max_gap, p.min_sweeps = c.min_sweeps;
    p.filled = c;
    *out = p;
    return MI_OK;
}

const char* elt_state_ok(const EltRowState* state, size_t rows, const EltPlan& plan) {
    const auto bin_ok = [](uint32_t b) { return b >= MI_ELT_BIN0 && b < MI_ELT_BIN0 + MI_ELT_BINS; };
    const auto dir_of = [](uint32_t from, uint32_t to) { return to > from ? MI_ELT_UP : to < from ? MI_ELT_DOWN : 0; };
    for (size_t r = 0; r < rows; ++r) {
        const EltRowState& s = state[r];
        const uint32_t f = s.frame - 1u;  // the last frame the walker saw
        if (s.open > 1u || s.alarmed > 1u)
            return "open or alarmed beyond 1";
        if (!s.open) {
            if (s.start || s.first_bin || s.last_bin || s.last_frame || s.dir || s.drops)
                return "a closed segment with a field set";
        } else {
            if (!bin_ok(s.first_bin) || !bin_ok(s.last_bin))
                return "a segment's bin outside 2 .. 33";
            if (s.dir > MI_ELT_DOWN || s.dir != static_cast<uint32_t>(dir_of(s.first_bin, s.last_bin)))
                return "a segment's dir that its bins contradict";
            if (s.drops > plan.max_drop || f - s.last_frame != s.drops)
                return "drops over max_drop, or not the frames since last_frame";
            if (s.last_frame - s.start >= 0x80000000u)
                return "a segment of 2^31 frames or more";
        }
        if (!s.count) {
            if (s.chain_dir || s.chain_first || s.last_end || s.alarmed || s.bin_from || s.bin_to)
                return "a cleared chain with a field set";
        } else {
            if (!bin_ok(s.bin_from) || !bin_ok(s.bin_to))
                return "a chain's bin outside 2 .. 33";
            if (s.chain_dir < MI_ELT_UP || s.chain_dir > MI_ELT_DOWN || s.chain_dir != static_cast<uint32_t>(dir_of(s.bin_from, s.bin_to)))
                return "a chain's chain_dir that its bins contradict";
            if ((s.bin_from > s.bin_to ? s.bin_from - s.bin_to : s.bin_to - s.bin_from) < plan.min_span)
                return "a chain whose last sweep spans less than min_span";
            if (s.alarmed != (s.count >= plan.min_sweeps ? 1u : 0u))
                return "alarmed is not (count >= min_sweeps)";
            if (s.last_end - s.chain_first >= 0x80000000u || f - s.last_end >= 0x80000000u || (s.open && s.start - s.last_end - 1u >= 0x7FFFFFFFu))
                return "a chain whose frames are out of order";
            const bool alive = f - s.last_end <= plan.max_gap || (s.open && s.start - s.last_end <= plan.max_gap && f - s.start + 1u <= plan.max_len);
            if (!alive)
                return "a chain that would have expired";
        }
    }
    return nullptr;
}

namespace {

// items 0 .. 4 of the header over the 256 samples at x
mi_elt_frame_record elt_frame_record(const float* x, const float* w, const EltPlan& plan) {
    float y[MI_ELT_FRAME], s[64], p[MI_ELT_BINS], q1[MI_ELT_BINS], q2[MI_ELT_BINS];
    for (int j = 0; j < MI_ELT_FRAME; ++j)
        y[j] = x[j] * w[j];
    for (int l = 0; l < 64; ++l) {
        s[l] = y[l] * y[l];
        for (int j = l + 64; j < MI_ELT_FRAME; j += 64)
            s[l] = s[l] + y[j] * y[j];
    }
    for (int h = 32; h >= 1; h /= 2)
        for (int l = 0; l < h; ++l)
            s[l] = s[l] + s[l + h];
    const float E = s[0];
    for (int t = 0; t < MI_ELT_BINS; ++t)
        p[t] = q1[t] = q2[t] = 0.0f;
    if (E != 0.0f) {  // (a silent frame: the powers are zero by definition)
        for (int j = 0; j < MI_ELT_FRAME; ++j)
            for (int t = 0; t < MI_ELT_BINS; ++t) {
                const float q0 = plan.coeff[t] * q1[t] - q2[t] + y[j];
                q2[t] = q1[t];
                q1[t] = q0;
            }
        for (int t = 0; t < MI_ELT_BINS; ++t)
            p[t] = q1[t] * q1[t] + q2[t] * q2[t] - q1[t] * q2[t] * plan.coeff[t];
    }
    int best = 0;
    for (int t = 1; t < MI_ELT_BINS; ++t)
        if (p[t] > p[best])
            best = t;
    const float below = best > 0 ? p[best - 1] : 0.0f, above = best < MI_ELT_BINS - 1 ? p[best + 1] : 0.0f;
    const float p3 = below + p[best] + above;
    const uint32_t bin = static_cast<uint32_t>(best) + MI_ELT_BIN0;
    const bool tonal = E >= plan.min_energy && p3 >= plan.tc * E && bin >= plan.band_lo && bin <= plan.band_hi;
    return mi_elt_frame_record{static_cast<uint8_t>(bin), static_cast<uint8_t>(tonal ? bin : MI_ELT_NONE8), 0, E, p[best], p3};
}

}  // namespace
}  // namespace mi

extern "C" int mi_elt_settings(const mi_elt_cfg* cfg, mi_elt_cfg* out, float* c) {
    if (!out)
        return fail(MI_ERR_INVALID, "NULL argument");
    mi::EltPlan p;
    if (const int rc = mi::elt_plan(cfg, &p))
        return rc;
    *out = p.filled;
    if (c)
        *c = p.c;
    return MI_OK;
}

extern "C" int mi_elt_window(float* out) {
    if (!out)
        return fail(MI_ERR_INVALID, "NULL argument");
    mi::elt_window(out);
    return MI_OK;
}

extern "C" int mi_elt_coeffs(float* out) {
    if (!out)
        return fail(MI_ERR_INVALID, "NULL argument");
    mi::EltPlan p;
    if (const int rc = mi::elt_plan(nullptr, &p))
        return rc;
    std::memcpy(out, p.coeff, sizeof(p.coeff));
    return MI_OK;
}

extern "C" int mi_elt_event_text(const mi_elt_event* e, char* out) {
    if (!e || !out)
        return fail(MI_ERR_INVALID, "NULL argument");
    const auto bin_ok = [](uint32_t b) { return b >= MI_ELT_BIN0 && b < MI_ELT_BIN0 + MI_ELT_BINS; };
    if ((e->kind != MI_ELT_ONSET && e->kind != MI_ELT_END) || (e->dir != MI_ELT_UP && e->dir != MI_ELT_DOWN) || !bin_ok(e->bin_from) || !bin_ok(e->bin_to))
        return fail(MI_ERR_INVALID, "ELT stage: not an event record the stage writes (kind, dir or a bin out of range)");
    std::snprintf(out, 96, "%s %s %.1f -> %.1f Hz, %u sweeps, %.3f s", e->kind == MI_ELT_ONSET ? "ONSET" : "END", e->dir == MI_ELT_UP ? "up" : "down",
                  62.5 * e->bin_from, 62.5 * e->bin_to, e->sweeps, 0.005 * static_cast<double>(e->frame - e->first_frame));
    return MI_OK;
}

extern "C" int mi_elt_plan_host(const mi_elt_cfg* cfg, const uint8_t* row_enabled, int rows, int nbatches, const float* plane, size_t row_stride,
                                void* state_inout, mi_elt_frame_record* frames, mi_elt_event* events, size_t max_events, uint32_t* row_first_event,
                                uint32_t* count) {
    if (!row_enabled || !plane || !state_inout || !events || !row_first_event || !count)
        return fail(MI_ERR_INVALID, "NULL argument");
    if (rows < 1 || nbatches < 1 || max_events < 1)
        return fail(MI_ERR_INVALID, "ELT plan needs rows >= 1, nbatches >= 1 and max_events >= 1");
    if (row_stride < static_cast<size_t>(nbatches) * mi::kWaveBatch)
        return fail(MI_ERR_INVALID, "a row stride is shorter than the call");
    mi::EltPlan plan;
    if (const int rc = mi::elt_plan(cfg, &plan))
        return rc;
    if (static_cast<uint64_t>(rows) * mi::elt_max_events(plan.min_sweeps, plan.min_len, static_cast<uint64_t>(nbatches)) > UINT32_MAX)
        return fail(MI_ERR_INVALID, "ELT plan: the events of the call do not fit the 32-bit count");
    std::vector<mi::EltRowState> blob(static_cast<size_t>(rows));
    std::memcpy(blob.data(), state_inout, blob.size() * sizeof(mi::EltRowState));
    if (const char* const why = mi::elt_state_ok(blob.data(), blob.size(), plan))
        return fail(MI_ERR_INVALID, std::string("ELT plan: malformed state blob: ") + why);
    constexpr int kBack = MI_ELT_FRAME - MI_ELT_HOP;  // 176: the samples of a batch's first frame that lie before the batch
    std::vector<float> x(kBack + static_cast<size_t>(nbatches) * mi::kWaveBatch);
    float w[MI_ELT_FRAME];
    mi::elt_window(w);
    const mi::EltRules rules = mi::elt_rules(plan);
    const uint32_t nframes = MI_ELT_FRAMES * static_cast<uint32_t>(nbatches);
    uint32_t k = 0;
    for (int r = 0; r < rows; ++r) {
        row_first_event[r] = k;
        if (!row_enabled[r])
            continue;
        mi::EltRowState& st = blob[static_cast<size_t>(r)];
        const float* const row = plane + static_cast<size_t>(r) * row_stride;
        // x = the last 176 carried samples, then the call's
        std::memcpy(x.data(), st.x + (MI_ELT_HISTORY - kBack), kBack * sizeof(float));
        std::memcpy(x.data() + kBack, row, static_cast<size_t>(nbatches) * mi::kWaveBatch * sizeof(float));
        mi::EltWalker wk{st.open, st.start, st.first_bin, st.last_bin, st.last_frame, st.dir, st.drops, st.count, st.chain_dir, st.chain_first, st.last_end,
                         st.alarmed, st.bin_from, st.bin_to};
        for (uint32_t i = 0; i < nframes; ++i) {
            const mi_elt_frame_record rec = mi::elt_frame_record(x.data() + static_cast<size_t>(i) * MI_ELT_HOP, w, plan);
            if (frames)
                frames[static_cast<size_t>(r) * nframes + i] = rec;
            const uint32_t f = st.frame + i;
            mi::elt_step(wk, rules, rec.bin, f, [&](uint32_t kind) {
                if (k < max_events)
                    events[k] = mi_elt_event{static_cast<uint32_t>(r), st.seq, static_cast<uint8_t>(kind), static_cast<uint8_t>(wk.chain_dir),
                                             static_cast<uint8_t>(wk.bin_from), static_cast<uint8_t>(wk.bin_to), f, wk.chain_first, wk.last_end, wk.count,
                                             i / MI_ELT_FRAMES};
                ++k;
                st.seq += 1;
            });
        }
        st.frame += nframes;
        st.open = wk.open, st.start = wk.start, st.first_bin = wk.first_bin, st.last_bin = wk.last_bin, st.last_frame = wk.last_frame, st.dir = wk.dir;
        st.drops = wk.drops, st.count = wk.count, st.chain_dir = wk.chain_dir, st.chain_first = wk.chain_first, st.last_end = wk.last_end;
        st.alarmed = wk.alarmed, st.bin_from = wk.bin_from, st.bin_to = wk.bin_to;
        std::memcpy(st.x, row + static_cast<size_t>(nbatches) * mi::kWaveBatch - MI_ELT_HISTORY, MI_ELT_HISTORY * sizeof(float));
    }
    row_first_event[rows] = k;
    count[0] = k;
    count[1] = k < max_events ? k : static_cast<uint32_t>(max_events);
    std::memcpy(state_inout, blob.data(), blob.size() * sizeof(mi::EltRowState));
    return MI_OK;
}

// ---- packet decoder stage, host side (include/mi_airband.h "packet decoder stage"): the settings' check, the templates, the blob's
// check, the frame check, a record's TNC2 line, and the twin of ax25.hip -- one row, one batch, one hypothesis and one slot at a time,
// then the 30 deframers over the batch's slots.  The bit, the deframer's step and the address field's check are poststage.hpp's.
namespace mi {

int ax25_plan(const mi_ax25_cfg* cfg, Ax25Plan* out) {
    mi_ax25_cfg c{};
    if (cfg)
        c = *cfg;
    const float def[MI_AX25_SLICERS] = {MI_AX25_GAIN0, MI_AX25_GAIN1, MI_AX25_GAIN2};
    Ax25Plan p{};
    for (int g = 0; g < MI_AX25_SLICERS; ++g) {
        if (!std::isfinite(c.gain[g]) || c.gain[g] < 0.0f)
            return fail(MI_ERR_INVALID, "packet stage: every gain must be finite and positive (0 = the default)");
        if (c.gain[g] == 0.0f)
            c.gain[g] = def[g];
        p.gain[g] = c.gain[g];
    }
    if (c.strict > 1 && c.strict != MI_AX25_STRICT_OFF)
        return fail(MI_ERR_INVALID, "packet stage: strict must be 0, 1 or MI_AX25_STRICT_OFF");
    if (c.strict == 0)
        c.strict = 1;
    p.strict = c.strict == 1;
    p.filled = c;
    *out = p;
    return MI_OK;
}

void ax25_templates(float* t) {
    const double pi = 3.14159265358979323846;
    for (int r = 0; r < 40; ++r) {
        t[r] = static_cast<float>(std::cos(2.0 * pi * 1200.0 * r / 48000.0));
        t[40 + r] = static_cast<float>(std::sin(2.0 * pi * 1200.0 * r / 48000.0));
        t[80 + r] = static_cast<float>(std::cos(2.0 * pi * 2200.0 * r / 48000.0));
        t[120 + r] = static_cast<float>(std::sin(2.0 * pi * 2200.0 * r / 48000.0));
    }
}

const char* ax25_state_ok(const Ax25RowState* state, size_t rows) {
    for (size_t r = 0; r < rows; ++r) {
        const Ax25RowState& s = state[r];
        if (s.zero[0] | s.zero[1])
            return "the zero field is not 0";
        if (s.batch >= (1ull << 40))
            return "a batch count at or beyond 2^40";
        const uint64_t now = 3ull * kWaveBatch * s.batch;
        if (s.last_end > now)
            return "an impossible position (the last record ends behind the row's last batch)";
        for (int l = 0; l < MI_AX25_LANES; ++l) {
            if (s.prev[l] > 1 || s.ones[l] > 7 || s.nbits[l] > 7 || s.cur[l] >> s.nbits[l] || s.nbytes[l] > MI_AX25_MAX_BYTES)
                return "an impossible lane state (a counter beyond its range)";
            if (s.phase[l] > MI_AX25_FRAME)
                return "an unknown lane phase";
            uint32_t used = 0;
            if (s.phase[l] == MI_AX25_WAIT) {
                if (s.start[l] | s.nbytes[l] | s.crc[l] | s.nbits[l] | s.cur[l])
                    return "an impossible lane state (a waiting lane with a frame field set)";
            } else {
                // the lane's last slot ended at lane_now, and every collected bit took a slot of 40 thirds behind start
                const int64_t lane_now = static_cast<int64_t>(now) + ax25_slot_end(l % MI_AX25_HYPOTHESES, -1);
                if (s.start[l] > now || static_cast<int64_t>(s.start[l]) + 40 * (8 * static_cast<int64_t>(s.nbytes[l]) + s.nbits[l]) > lane_now)
                    return "an impossible position (a frame begins behind the row's last batch or later than its collected bits allow)";
                used = s.nbytes[l];
                uint32_t crc = 0xFFFFu;
                for (uint32_t i = 0; i < used; ++i)
                    for (int k = 0; k < 8; ++k)
                        crc = ax25_crc_bit(crc, s.bytes[l][i] >> k & 1u);
                for (uint32_t k = 0; k < s.nbits[l]; ++k)
                    crc = ax25_crc_bit(crc, s.cur[l] >> k & 1u);
                if (crc != s.crc[l])
                    return "an impossible lane state (a crc that the bytes do not give)";
            }
            for (uint32_t i = used; i < MI_AX25_RAW_BYTES; ++i)
                if (s.bytes[l][i])
                    return "an impossible lane state (a byte set behind the ones taken)";
        }
    }
    return nullptr;
}

}  // namespace mi

extern "C" int mi_ax25_settings(const mi_ax25_cfg* cfg, mi_ax25_cfg* out) {
    if (!out)
        return fail(MI_ERR_INVALID, "NULL argument");
    mi::Ax25Plan p;
    if (const int rc = mi::ax25_plan(cfg, &p))
        return rc;
    *out = p.filled;
    return MI_OK;
}

extern "C" int mi_ax25_templates(float* t) {
    if (!t)
        return fail(MI_ERR_INVALID, "NULL argument");
    mi::ax25_templates(t);
    return MI_OK;
}

extern "C" uint32_t mi_ax25_crc(const uint8_t* bytes, size_t n) {
    if (!bytes && n)
        return 0xFFFFFFFFu;
    uint32_t crc = 0xFFFFu;
    for (size_t i = 0; i < n; ++i)
        for (int k = 0; k < 8; ++k)
            crc = mi::ax25_crc_bit(crc, bytes[i] >> k & 1u);
    return crc ^ 0xFFFFu;
}

extern "C" int mi_ax25_frame_text(const mi_ax25_frame* f, char* text, size_t cap) {
    if (!f || !text)
        return fail(MI_ERR_INVALID, "NULL argument");
    if (f->nbytes < MI_AX25_MIN_BYTES || f->nbytes > MI_AX25_MAX_BYTES)
        return fail(MI_ERR_INVALID, "packet stage: a frame's nbytes must be within 17 .. 330");
    const uint32_t naddr = mi::ax25_naddr(f->bytes, f->nbytes);
    if (!naddr)
        return fail(MI_ERR_INVALID, "packet stage: the frame's address field is not well formed");
    std::string line;
    const auto call = [&](uint32_t a) {
        const uint8_t* const b = f->bytes + 7 * a;
        int len = 6;
        while (len > 0 && b[len - 1] >> 1 == ' ')
            --len;
        for (int i = 0; i < len; ++i)
            line += static_cast<char>(b[i] >> 1);
        if (const uint32_t ssid = b[6] >> 1 & 15u)
            line += "-" + std::to_string(ssid);
    };
    call(1);
    line += '>';
    call(0);
    uint32_t last_h = 0;  // the address behind which the '*' goes
    for (uint32_t a = 2; a < naddr; ++a)
        if (f->bytes[7 * a + 6] & 0x80u)
            last_h = a;
    for (uint32_t a = 2; a < naddr; ++a) {
        line += ',';
        call(a);
        if (a == last_h)
            line += '*';
    }
    line += ':';
    const uint32_t control = f->bytes[7 * naddr];
    uint32_t at = 7 * naddr + ((control | 0x10u) == 0x13u ? 2u : 1u);
    for (; at + 2 < f->nbytes; ++at)
        line += f->bytes[at] >= 0x20 && f->bytes[at] <= 0x7E ? static_cast<char>(f->bytes[at]) : '.';
    if (line.size() + 1 > cap)
        return fail(MI_ERR_INVALID, "packet stage: the text buffer is shorter than the line");
    std::memcpy(text, line.c_str(), line.size() + 1);
    return MI_OK;
}

extern "C" int mi_ax25_plan_host(const mi_ax25_cfg* cfg, const uint8_t* row_enabled, int rows, int nbatches, const float* plane, size_t row_stride,
                                 void* state_inout, uint32_t* bits, mi_ax25_frame* frames, size_t max_frames, uint32_t* row_first_frame,
                                 uint32_t* count) {
    if (!row_enabled || !plane || !state_inout || !frames || !row_first_frame || !count)
        return fail(MI_ERR_INVALID, "NULL argument");
    if (rows < 1 || nbatches < 1 || max_frames < 1)
        return fail(MI_ERR_INVALID, "packet plan needs rows >= 1, nbatches >= 1 and max_frames >= 1");
    if (row_stride < static_cast<size_t>(nbatches) * mi::kWaveBatch)
        return fail(MI_ERR_INVALID, "a row stride is shorter than the call");
    mi::Ax25Plan plan;
    if (const int rc = mi::ax25_plan(cfg, &plan))
        return rc;
    if (static_cast<uint64_t>(rows) * mi::ax25_max_frames(static_cast<uint64_t>(nbatches)) > UINT32_MAX)
        return fail(MI_ERR_INVALID, "packet plan: the frames of the call do not fit the 32-bit count");
    std::vector<mi::Ax25RowState> blob(static_cast<size_t>(rows));
    std::memcpy(blob.data(), state_inout, blob.size() * sizeof(mi::Ax25RowState));
    if (const char* const why = mi::ax25_state_ok(blob.data(), blob.size()))
        return fail(MI_ERR_INVALID, std::string("packet plan: malformed state blob: ") + why);
    constexpr int kLead = MI_AX25_HISTORY + 2, kTau = MI_AX25_HYPOTHESES, kBits = MI_AX25_BITS, kWords = MI_AX25_BIT_WORDS, kLanes = MI_AX25_LANES;
    float T[160];
    mi::ax25_templates(T);
    const mi::Ax25Gains gain{{plan.gain[0], plan.gain[1], plan.gain[2]}};
    std::vector<float> s(kLead + static_cast<size_t>(nbatches) * mi::kWaveBatch);
    uint32_t k = 0;
    for (int r = 0; r < rows; ++r) {
        row_first_frame[r] = k;
        if (!row_enabled[r])
            continue;
        mi::Ax25RowState& st = blob[static_cast<size_t>(r)];
        const float* const row = plane + static_cast<size_t>(r) * row_stride;
        s[0] = s[1] = 0.0f;
        std::memcpy(s.data() + 2, st.x, sizeof(st.x));
        std::memcpy(s.data() + kLead, row, static_cast<size_t>(nbatches) * mi::kWaveBatch * sizeof(float));
        mi::Ax25Lane lane[kLanes];
        for (int l = 0; l < kLanes; ++l)
            lane[l] = mi::Ax25Lane{st.prev[l], st.ones[l], st.phase[l], st.nbits[l], st.cur[l], st.nbytes[l], st.crc[l], st.start[l]};
        for (int b = 0; b < nbatches; ++b) {
            const float* const blk = s.data() + static_cast<size_t>(b) * mi::kWaveBatch;  // staged: blk[kLead + n] is the batch's sample n
            uint32_t word[kLanes][kWords] = {};
            for (int t = 0; t < kTau; ++t)
                for (int j = 0; j < kBits; ++j) {
                    const uint32_t m = mi::ax25_bit(blk, T, gain, t, j);
                    for (int g = 0; g < MI_AX25_SLICERS; ++g)
                        word[10 * g + t][j / 32] |= (m >> g & 1u) << (j % 32);
                }
            if (bits)
                std::memcpy(bits + (static_cast<size_t>(r) * static_cast<size_t>(nbatches) + static_cast<size_t>(b)) * kLanes * kWords, word, sizeof(word));
            const uint64_t base = 3ull * mi::kWaveBatch * (st.batch + static_cast<uint64_t>(b));
            for (int j = 0; j < kBits; ++j)
                for (int l = 0; l < kLanes; ++l) {
                    mi::Ax25Lane& L = lane[l];
                    const uint32_t ev = mi::ax25_step(L, word[l][j / 32] >> (j % 32) & 1u, [&](uint32_t i, uint32_t byte) { st.bytes[l][i] = static_cast<uint8_t>(byte); });
                    if (!ev)
                        continue;
                    const uint64_t end = base + static_cast<uint64_t>(mi::ax25_slot_end(l % kTau, j));
                    if ((ev & mi::kAx25Cand) && L.start + 40 >= st.last_end) {
                        const uint32_t naddr = mi::ax25_naddr(st.bytes[l], L.nbytes);
                        if (naddr || !plan.strict) {
                            if (k < max_frames) {
                                mi_ax25_frame f{};
                                f.row = static_cast<uint32_t>(r);
                                f.batch = static_cast<uint32_t>(L.start / (3u * mi::kWaveBatch));
                                f.third = static_cast<uint32_t>(L.start % (3u * mi::kWaveBatch));
                                f.end_batch = static_cast<uint32_t>(b);
                                f.nbytes = static_cast<uint16_t>(L.nbytes);
                                f.lane = static_cast<uint8_t>(l);
                                f.naddr = static_cast<uint8_t>(naddr);
                                std::memcpy(f.bytes, st.bytes[l], L.nbytes);
                                frames[k] = f;
                            }
                            ++k;
                            st.last_end = end;
                        }
                    }
                    mi::ax25_open(L, end);
                }
        }
        st.batch += static_cast<uint64_t>(nbatches);
        for (int l = 0; l < kLanes; ++l) {
            const mi::Ax25Lane& L = lane[l];
            st.prev[l] = static_cast<uint8_t>(L.prev), st.ones[l] = static_cast<uint8_t>(L.ones), st.phase[l] = static_cast<uint8_t>(L.phase);
            st.nbits[l] = static_cast<uint8_t>(L.nbits), st.cur[l] = static_cast<uint8_t>(L.cur), st.nbytes[l] = static_cast<uint16_t>(L.nbytes);
            st.crc[l] = static_cast<uint16_t>(L.crc), st.start[l] = L.start;
            std::memset(st.bytes[l] + L.nbytes, 0, MI_AX25_RAW_BYTES - L.nbytes);  // (what an earlier frame left behind the ones taken)
        }
        std::memcpy(st.x, row + static_cast<size_t>(nbatches) * mi::kWaveBatch - MI_AX25_HISTORY, sizeof(st.x));
    }
    row_first_frame[rows] = k;
    count[0] = k;
    count[1] = k < max_frames ? k : static_cast<uint32_t>(max_frames);
    std::memcpy(state_inout, blob.data(), blob.size() * sizeof(mi::Ax25RowState));
    return MI_OK;
}

// ---- pager decoder stage, host side (include/mi_airband.h "pager decoder stage"): the settings' check, the syndrome table, the
// blob's check, the codeword helpers, a message's text, and the twin of pocsag.hip -- one row, one batch, one hypothesis and one
// slot at a time, then the walker over the batch's slots.  The bit's sum, the sync compare and choice, the word's rule and the timing
// move are poststage.hpp's.
namespace mi {

int pocsag_plan(const mi_pocsag_cfg* cfg, PocsagPlan* out) {
    mi_pocsag_cfg c{};
    if (cfg)
        c = *cfg;
    if (c.baud == 0)
        c.baud = 1200;
    if (c.baud != 512 && c.baud != 1200 && c.baud != 2400)
        return fail(MI_ERR_INVALID, "pager stage: baud must be 512, 1200 or 2400 (0 = the default, 1200)");
    if (c.sync_errors == 0)
        c.sync_errors = 2;
    if (c.sync_errors != MI_POCSAG_SYNC_EXACT && c.sync_errors > 4)
        return fail(MI_ERR_INVALID, "pager stage: sync_errors must be within 1 .. 4 or MI_POCSAG_SYNC_EXACT (0 = the default)");
    if (c.preamble_errors == 0)
        c.preamble_errors = 4;
    if (c.preamble_errors != MI_POCSAG_PREAMBLE_EXACT && c.preamble_errors != MI_POCSAG_PREAMBLE_OFF && c.preamble_errors > 8)
        return fail(MI_ERR_INVALID, "pager stage: preamble_errors must be within 1 .. 8, MI_POCSAG_PREAMBLE_EXACT or MI_POCSAG_PREAMBLE_OFF (0 = the default)");
    if (c.correct == 0)
        c.correct = 1;
    if (c.correct != MI_POCSAG_CORRECT_NONE && c.correct > 2)
        return fail(MI_ERR_INVALID, "pager stage: correct must be 1, 2 or MI_POCSAG_CORRECT_NONE (0 = the default)");
    if (c.hold_timing > 1)
        return fail(MI_ERR_INVALID, "pager stage: hold_timing must be 0 or 1");
    PocsagPlan p{};
    p.g = pocsag_geom(c.baud);
    p.sync_errors = c.sync_errors == MI_POCSAG_SYNC_EXACT ? 0u : c.sync_errors;
    p.preamble_errors = c.preamble_errors == MI_POCSAG_PREAMBLE_EXACT ? 0u : c.preamble_errors == MI_POCSAG_PREAMBLE_OFF ? 32u : c.preamble_errors;
    p.correct = c.correct == MI_POCSAG_CORRECT_NONE ? 0u : c.correct;
    p.hold_timing = c.hold_timing;
    p.filled = c;
    *out = p;
    return MI_OK;
}

void pocsag_table(uint32_t* t) {
    for (int i = 0; i < 1024; ++i)
        t[i] = kPocsagNoPattern;
    t[0] = 0;
    for (int a = 1; a < 32; ++a) {
        t[pocsag_syndrome(1u << a)] = 1u << a;
        for (int b = a + 1; b < 32; ++b)
            t[pocsag_syndrome(1u << a | 1u << b)] = 1u << a | 1u << b;
    }
}

const char* pocsag_state_ok(const PocsagRowState* state, size_t rows, const PocsagPlan& plan) {
    const uint32_t H = static_cast<uint32_t>(plan.g.H), lanes = 2 * H;
    for (size_t r = 0; r < rows; ++r) {
        const PocsagRowState& s = state[r];
        const mi_pocsag_message& m = s.msg;
        if (s.zero)
            return "the zero field is not 0";
        if (s.phase > MI_POCSAG_TRANSMISSION)
            return "an unknown walker phase";
        for (uint32_t l = lanes; l < MI_POCSAG_MAX_LANES; ++l)
            if (s.hist[l])
                return "history bits in a lane the baud does not have";
        bool any = false;  // a byte of the message set
        for (size_t i = 0; i < sizeof(m); ++i)
            any = any || reinterpret_cast<const uint8_t*>(&m)[i];
        if (s.phase == MI_POCSAG_IDLE) {
            if (s.lane | s.inverted | s.pos | s.cur | s.nbits | s.gbad | s.lane_sync | s.mismatches | s.wbatch | s.wtwelfth | s.open || any)
                return "an impossible walker state (an idle row with a walker field or a byte of the message set)";
            continue;
        }
        if (s.lane >= lanes || s.lane_sync >= lanes || s.lane / H != s.lane_sync / H)
            return "an impossible walker state (a lane the baud does not have, or two slicers in one transmission)";
        if (s.inverted > 1 || s.open > 1 || s.pos > 16 || s.nbits > 31 || s.cur >> s.nbits || s.gbad > s.pos || s.gbad > 15 || s.mismatches > 4 ||
            s.wtwelfth >= static_cast<uint32_t>(kPocsagTwelfths))
            return "an impossible walker state (counters, a running word or timing that a transmission cannot have)";
        if (!s.open) {
            if (any)
                return "an impossible walker state (a message set though none is open)";
            continue;
        }
        if (m.row | m.end_batch | m.lane_end | m.zero | m.zero2 || m.address >> 21 || m.function > 3 || m.nwords > MI_POCSAG_MAX_WORDS || m.truncated > 1 ||
            (m.truncated && m.nwords < MI_POCSAG_MAX_WORDS) || m.twelfth >= static_cast<uint32_t>(kPocsagTwelfths) || m.inverted != s.inverted ||
            m.lane_sync != s.lane_sync || m.sync_errors != s.mismatches)
            return "an impossible open message (a field that no message of the transmission has)";
        uint32_t nbad = 0;
        for (uint32_t i = 0; i < 96; ++i) {
            const uint32_t bad = m.bad[i / 32] >> (i % 32) & 1u;
            if (i >= m.nwords && (bad || (i < MI_POCSAG_MAX_WORDS && m.words[i])))
                return "an impossible open message (a bad bit or a word behind nwords)";
            nbad += bad;
        }
        if (nbad != m.nbad || m.corrected > 2u * (m.nwords - nbad + 1u))
            return "an impossible open message (an nbad that the mask does not give, or more repairs than its words can have)";
    }
    return nullptr;
}

namespace {

const uint32_t* pocsag_table_once() {
    static const std::vector<uint32_t> t = [] {
        std::vector<uint32_t> v(1024);
        pocsag_table(v.data());
        return v;
    }();
    return t.data();
}

}  // namespace
}  // namespace mi

extern "C" int mi_pocsag_settings(const mi_pocsag_cfg* cfg, mi_pocsag_cfg* out) {
    if (!out)
        return fail(MI_ERR_INVALID, "NULL argument");
    mi::PocsagPlan p;
    if (const int rc = mi::pocsag_plan(cfg, &p))
        return rc;
    *out = p.filled;
    return MI_OK;
}

extern "C" int mi_pocsag_geometry(uint32_t baud, int* hypotheses, int* bits, int* words) {
    mi_pocsag_cfg c{};
    c.baud = baud;
    mi::PocsagPlan p;
    if (const int rc = mi::pocsag_plan(&c, &p))
        return rc;
    if (hypotheses)
        *hypotheses = p.g.H;
    if (bits)
        *bits = p.g.B;
    if (words)
        *words = p.g.W;
    return MI_OK;
}

extern "C" uint32_t mi_pocsag_max_messages(uint32_t baud, uint64_t nbatches) {
    mi_pocsag_cfg c{};
    c.baud = baud;
    mi::PocsagPlan p;
    if (mi::pocsag_plan(&c, &p))
        return 0;
    return mi::pocsag_max_messages(p.g, nbatches);
}

extern "C" uint32_t mi_pocsag_encode(uint32_t data21) {
    const uint32_t cw = (data21 & 0x1FFFFFu) << 11;
    const uint32_t word = cw | mi::pocsag_syndrome(cw) << 1;  // (the remainder of the data times x^10, the check bits still 0)
    return word | static_cast<uint32_t>(__builtin_popcount(word) & 1);
}

extern "C" int mi_pocsag_decode(uint32_t word, uint32_t correct, uint32_t* fixed, uint32_t* errors) {
    mi_pocsag_cfg c{};
    c.correct = correct;
    mi::PocsagPlan p;
    if (const int rc = mi::pocsag_plan(&c, &p))
        return rc;
    uint32_t f;
    const uint32_t e = mi::pocsag_repair(mi::pocsag_table_once(), word, &f);
    const bool good = e <= p.correct;
    if (fixed)
        *fixed = good ? f : word;
    if (errors)
        *errors = e;
    return good ? 1 : 0;
}

extern "C" int mi_pocsag_message_text(const mi_pocsag_message* m, int mode, char* text, size_t cap) {
    if (!m || !text)
        return fail(MI_ERR_INVALID, "NULL argument");
    if (m->nwords > MI_POCSAG_MAX_WORDS)
        return fail(MI_ERR_INVALID, "pager stage: a message's nwords must be within 0 .. 80");
    if (mode != MI_POCSAG_TEXT_AUTO && mode != MI_POCSAG_TEXT_NUMERIC && mode != MI_POCSAG_TEXT_ALPHA)
        return fail(MI_ERR_INVALID, "pager stage: the text mode must be MI_POCSAG_TEXT_AUTO, _NUMERIC or _ALPHA");
    if (mode == MI_POCSAG_TEXT_AUTO)
        mode = m->function == 0 ? MI_POCSAG_TEXT_NUMERIC : MI_POCSAG_TEXT_ALPHA;
    const int width = mode == MI_POCSAG_TEXT_NUMERIC ? 4 : 7;
    const uint32_t nbits = 20u * m->nwords;
    // payload bit i of the message: bit 30 - i % 20 of word i / 20
    const auto bit = [&](uint32_t i) { return m->words[i / 20] >> (30 - i % 20) & 1u; };
    const auto bad = [&](uint32_t i) { return m->bad[i / 20 / 32] >> (i / 20 % 32) & 1u; };
    std::string s;
    for (uint32_t i = 0; i + width <= nbits; i += width) {
        uint32_t v = 0, b = 0;
        for (int k = 0; k < width; ++k) {
            v |= bit(i + k) << k;
            b |= bad(i + k);
        }
        s += b ? '?' : width == 4 ? "0123456789*U -)("[v] : v >= 0x20 && v <= 0x7E ? static_cast<char>(v) : '.';
    }
    if (width == 7) {  // the fill behind the text: NUL, ETX, EOT
        while (!s.empty()) {
            uint32_t v = 0;
            for (int k = 0; k < 7; ++k)
                v |= bit(7 * (static_cast<uint32_t>(s.size()) - 1) + k) << k;
            if (s.back() == '?' || (v != 0x00 && v != 0x03 && v != 0x04))
                break;
            s.pop_back();
        }
    }
    if (s.size() + 1 > cap)
        return fail(MI_ERR_INVALID, "pager stage: the text does not fit the buffer");
    std::memcpy(text, s.c_str(), s.size() + 1);
    return MI_OK;
}

extern "C" int mi_pocsag_plan_host(const mi_pocsag_cfg* cfg, const uint8_t* row_enabled, int rows, int nbatches, const float* plane, size_t row_stride,
                                   void* state_inout, uint32_t* bits, float* q, mi_pocsag_message* messages, size_t max_messages,
                                   uint32_t* row_first_message, uint32_t* count) {
    if (!row_enabled || !plane || !state_inout || !messages || !row_first_message || !count)
        return fail(MI_ERR_INVALID, "NULL argument");
    if (rows < 1 || nbatches < 1 || max_messages < 1)
        return fail(MI_ERR_INVALID, "pager plan needs rows >= 1, nbatches >= 1 and max_messages >= 1");
    if (row_stride < static_cast<size_t>(nbatches) * mi::kWaveBatch)
        return fail(MI_ERR_INVALID, "a row stride is shorter than the call");
    mi::PocsagPlan plan;
    if (const int rc = mi::pocsag_plan(cfg, &plan))
        return rc;
    const mi::PocsagGeom g = plan.g;
    if (static_cast<uint64_t>(rows) * mi::pocsag_max_messages(g, static_cast<uint64_t>(nbatches)) > UINT32_MAX)
        return fail(MI_ERR_INVALID, "pager plan: the messages of the call do not fit the 32-bit count");
    std::vector<mi::PocsagRowState> blob(static_cast<size_t>(rows));
    std::memcpy(blob.data(), state_inout, blob.size() * sizeof(mi::PocsagRowState));
    if (const char* const why = mi::pocsag_state_ok(blob.data(), blob.size(), plan))
        return fail(MI_ERR_INVALID, std::string("pager plan: malformed state blob: ") + why);
    constexpr int kLead = MI_POCSAG_HISTORY + 2;
    const int lanes = 2 * g.H;
    const uint32_t* const table = mi::pocsag_table_once();
    std::vector<float> s(kLead + static_cast<size_t>(nbatches) * mi::kWaveBatch);
    std::vector<uint32_t> word(static_cast<size_t>(lanes) * g.W);
    std::vector<float> v0(g.B), v1(g.B);
    uint32_t k = 0;
    // a[0 .. n - 1] summed in the order of the header: 64 running sums, then the halving tree
    const auto tree = [](const float* a, int n) {
        float lane[64];
        for (int l = 0; l < 64; ++l) {
            lane[l] = a[l];
            for (int j = l + 64; j < n; j += 64)
                lane[l] = lane[l] + a[j];
        }
        for (int h = 32; h >= 1; h /= 2)
            for (int l = 0; l < h; ++l)
                lane[l] = lane[l] + lane[l + h];
        return lane[0];
    };
    for (int r = 0; r < rows; ++r) {
        row_first_message[r] = k;
        if (!row_enabled[r])
            continue;
        mi::PocsagRowState& st = blob[static_cast<size_t>(r)];
        const float* const row = plane + static_cast<size_t>(r) * row_stride;
        s[0] = s[1] = 0.0f;
        std::memcpy(s.data() + 2, st.x, sizeof(st.x));
        std::memcpy(s.data() + kLead, row, static_cast<size_t>(nbatches) * mi::kWaveBatch * sizeof(float));
        mi::PocsagWalker w{st.phase, st.lane, st.inverted, st.pos, st.cur, st.nbits, st.gbad, st.lane_sync, st.mismatches, st.wbatch, st.wtwelfth, st.open};
        int b = 0;
        const auto emit = [&]() {
            if (k < max_messages) {
                mi_pocsag_message m = st.msg;
                m.row = static_cast<uint32_t>(r);
                m.end_batch = static_cast<uint32_t>(b);
                m.lane_end = static_cast<uint8_t>(w.lane);
                messages[k] = m;
            }
            ++k;
        };
        for (b = 0; b < nbatches; ++b) {
            const float* const blk = s.data() + static_cast<size_t>(b) * mi::kWaveBatch;  // staged: blk[kLead + n] is the batch's sample n
            const float mu = tree(blk + kLead, mi::kWaveBatch) / 2000.0f;
            std::vector<float> Q(static_cast<size_t>(lanes));
            std::fill(word.begin(), word.end(), 0u);
            for (int t = 0; t < g.H; ++t) {
                for (int j = 0; j < g.B; ++j) {
                    int n;
                    const float sum = mi::pocsag_sum(blk, g, t, j, &n);
                    const float a = sum, c = sum - static_cast<float>(n) * mu;
                    word[static_cast<size_t>(t) * g.W + j / 32] |= (a < 0.0f ? 1u : 0u) << (j % 32);
                    word[static_cast<size_t>(g.H + t) * g.W + j / 32] |= (c < 0.0f ? 1u : 0u) << (j % 32);
                    v0[j] = std::fabs(a);
                    v1[j] = std::fabs(c);
                }
                Q[t] = tree(v0.data(), g.B);
                Q[g.H + t] = tree(v1.data(), g.B);
            }
            const size_t blk_i = static_cast<size_t>(r) * static_cast<size_t>(nbatches) + static_cast<size_t>(b);
            if (bits)
                std::memcpy(bits + blk_i * word.size(), word.data(), word.size() * sizeof(uint32_t));
            if (q)
                std::memcpy(q + blk_i * lanes, Q.data(), Q.size() * sizeof(float));
            const uint32_t batch = st.batch + static_cast<uint32_t>(b);
            int skip = 0;
            if (w.phase == MI_POCSAG_TRANSMISSION && !plan.hold_timing) {
                const int move = mi::pocsag_retime(w, Q.data(), g.H);
                skip = move == mi::kPocsagSkip;
                if (move == mi::kPocsagReplay)  // hypothesis 0's last bit of the batch before
                    mi::pocsag_take(w, &st.msg, table, plan.sync_errors, plan.correct, static_cast<uint32_t>(st.hist[w.lane] & 1u) ^ w.inverted, batch, -g.L, emit);
            }
            for (int j = 0; j < g.B; ++j) {
                uint32_t mism[MI_POCSAG_MAX_LANES], inv[MI_POCSAG_MAX_LANES];
                for (int l = 0; l < lanes; ++l) {
                    st.hist[l] = st.hist[l] << 1 | (word[static_cast<size_t>(l) * g.W + j / 32] >> (j % 32) & 1u);
                    mism[l] = mi::pocsag_hit(st.hist[l], plan.sync_errors, plan.preamble_errors, &inv[l]);
                }
                if (w.phase == MI_POCSAG_TRANSMISSION) {
                    if (skip)
                        skip = 0;
                    else
                        mi::pocsag_take(w, &st.msg, table, plan.sync_errors, plan.correct, static_cast<uint32_t>(st.hist[w.lane] & 1u) ^ w.inverted, batch,
                                        mi::pocsag_slot_begin(g, static_cast<int>(w.lane) % g.H, j), emit);
                } else if (const int u = mi::pocsag_pick(mism, Q.data(), lanes); u >= 0) {
                    mi::pocsag_open(w, u, inv[u], mism[u]);
                }
            }
        }
        st.batch += static_cast<uint32_t>(nbatches);
        st.phase = w.phase, st.lane = w.lane, st.inverted = w.inverted, st.pos = w.pos, st.cur = w.cur, st.nbits = w.nbits, st.gbad = w.gbad;
        st.lane_sync = w.lane_sync, st.mismatches = w.mismatches, st.wbatch = w.wbatch, st.wtwelfth = w.wtwelfth, st.open = w.open;
        std::memcpy(st.x, row + static_cast<size_t>(nbatches) * mi::kWaveBatch - MI_POCSAG_HISTORY, sizeof(st.x));
    }
    row_first_message[rows] = k;
    count[0] = k;
    count[1] = k < max_messages ? k : static_cast<uint32_t>(max_messages);
    std::memcpy(state_inout, blob.data(), blob.size() * sizeof(mi::PocsagRowState));
    return MI_OK;
}
