// mi_airband.cpp -- the C ABI of include/mi_airband.h over the HIP kernels.
// No CPU fallback exists: without a HIP device every compute entry point fails with MI_ERR_NO_DEVICE.
#include "../../include/mi_airband.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "hip_own.hpp"
#include "kernels.hpp"
#include "plan.hpp"
#include "poststage.hpp"
#include "tuning.hpp"

namespace {

thread_local std::string g_err;

}  // namespace

namespace mi {
std::string& last_error_ref() {  // declared in poststage.hpp
    return g_err;
}
}  // namespace mi

namespace {

using mi::fail;

int hip_fail(hipError_t e, const char* where) {
    g_err = std::string(where) + ": " + hipGetErrorString(e);
    return (e == hipErrorNoDevice || e == hipErrorInvalidDevice) ? MI_ERR_NO_DEVICE : (e == hipErrorOutOfMemory ? MI_ERR_NOMEM : MI_ERR_HIP);
}

#define HIP_TRY(expr)                      \
    do {                                   \
        hipError_t e__ = (expr);           \
        if (e__ != hipSuccess)             \
            return hip_fail(e__, #expr);   \
    } while (0)
const char kFailedMsg[] = "an earlier call on this handle failed after its state had advanced: destroy it, or restore a checkpoint (mi_demod_set_state)";
// ... after the DSP state of the handle has advanced (enqueue() succeeded): the results of this call are lost and the state cannot be
// rolled back, so the handle is marked and refuses further calls (mi_demod_set_state with a checkpoint revives it)
#define HIP_TRY_F(expr)                                                              \
    do {                                                                             \
        hipError_t e__ = (expr);                                                     \
        if (e__ != hipSuccess) {                                                     \
            h->failed = true;                                                        \
            return hip_fail(e__, #expr);                                             \
        }                                                                            \
    } while (0)

}  // namespace

struct mi_plan {
    mi::Plan plan;
};

// The timing events of a call.  The numbers are public (mi_demod_event_ms takes those of ChunkEv) and stay as they are.
enum CallEv {  // per call (CallSet::ev)
    kEvBegin = 0,
    kEvStage1Done = 1,
    kEvDone = 2,
    kEvSerialBegin = 3,  // serial k_demod begins (pipelined serial calls, mixed plans)
    kEvSerialEnd = 4,    // ... ends (mixed plans)
    kEvPerCall
};
enum ChunkEv {  // per chunk of a time-parallel call (CallSet::chunk_ev)
    kEvStage1Begin = 0,  // front stream: stage 1
    kEvStage1End = 1,
    kEvFullBegin = 11,  // ... k_tp_full
    kEvFullEnd = 2,
    kEvCoreBegin = 3,  // aux stream: the core chain
    kEvCoreEnd = 4,
    kEvSegBegin = 5,  // segment stream: the segment pass
    kEvSegEnd = 12,
    kEvSegLaunched = 6,  // ... all segment launches of the chunk done
    kEvScanBegin = 10,   // caller's stream: scan#0
    kEvScanEnd = 7,
    kEvFixEnd = 8,     // ... fix#0 + redo#0
    kEvFinishEnd = 9,  // ... finish
    kEvPerChunk = 13
};
static_assert(kEvPerCall == 5 && kEvStage1Begin == 0 && kEvStage1End == 1 && kEvFullEnd == 2 && kEvCoreBegin == 3 && kEvCoreEnd == 4 &&
                  kEvSegBegin == 5 && kEvSegLaunched == 6 && kEvScanEnd == 7 && kEvFixEnd == 8 && kEvFinishEnd == 9 && kEvScanBegin == 10 &&
                  kEvFullBegin == 11 && kEvSegEnd == 12 && kEvPerChunk == 13,
              "callers of mi_demod_event_ms pass these numbers");
// The stage-2 path of a call.  mi_demod_last_path returns kPathSerial / kPathTimeParallel; a CallSet also tells a pipelined serial
// call apart; kPathAfc is a schedule of enqueue() only (an AFC call is recorded, and timed, as a serial one).
enum Path { kPathSerial = 0, kPathTimeParallel = 1, kPathSerialPipelined = 2, kPathAfc = 3 };
static_assert(kPathSerial == 0 && kPathTimeParallel == 1 && kPathSerialPipelined == 2, "mi_demod_last_path returns the first two");

struct mi_demod {
    mi::Plan plan;
    int gpu = 0;
    int nstreams = 0, nch = 0, rows = 0, max_batches = 0;
    bool first_call = true;  // waveend starts at 0: the first batch needs AGC_EXTRA more windows (config.cpp:808)
    size_t plane_stride = 0;
    mi::Stream own_stream;
    // The time-parallel path keeps kSets sets of its per-call scratch (magnitude planes, block aggregates, core snapshots,
    // segment records, timing events) and cycles through them: stage 1, the aggregates, the core chain and the segment
    // passes of a call never touch what the tails of the two calls before it still read, so calls overlap (see enqueue_time_parallel()).
    // `cur` is the set of the last call; the serial path stays on it.
    int cur = 0;
    // a call writes the set of the call six back: the host may then keep four or five calls queued behind the one whose timings it
    // reads (mi_demod_kernel_time_prev, age 4 or 5).  The tail of a call ends 2.8 ms after its core chain starts and stage 1 + the
    // aggregates of a call need 0.85 ms before its own, so with the host reading at age 3 (four sets, rounds 2-3) the period could
    // not fall below (2.8 + 0.85) / 3 = 1.2 ms -- which is what the step took once the chain itself was down to 1.03
    static constexpr int kSets = 6;
    static_assert(kSets % 2 == 0, "a call's scratch set picks its complex plane set by parity: the two must stay in step when the sets wrap");
    static constexpr int kMaxChunks = 64, kSegStreams = 1;
    struct CallSet {  // scratch set q: what one call in flight owns of the device, and what later calls have to know of it
        mi::DevBuf<float> mag;    // magnitude planes (d_mag is a view of the last call's)
        mi::DevBuf<float> carry;  // audio lookahead: a time-parallel call writes its own set's (the next call's segment pass may run
                                  // before this call's tail has applied its fades and the next call has emitted the lookahead)
        mi::DevBuf<unsigned> xmax;  // per row: the largest magnitude stage 1 wrote
        mi::DevBuf<float> blk_fe, blk_fm, blk_x0, blk_xm;  // block aggregates
        mi::DevBuf<mi::TpCore> core;                       // core snapshots
        mi::DevBuf<int> rec;  // segment records: the segment passes of the next call write theirs while this call's tail reads its own
        mi::Event ev[kEvPerCall];          // indexed by CallEv
        std::vector<mi::Event> chunk_ev;   // kEvPerChunk per chunk, indexed by ChunkEv
        hipEvent_t chunk(int i, ChunkEv k) const { return chunk_ev[static_cast<size_t>(i) * kEvPerChunk + k]; }
        uint64_t seq = 0;          // call number that last used this set (0 = never)
        Path path = kPathSerial;   // ... and its path (an AFC call: kPathSerial)
        bool mixed = false;  // ... with the serial kernel beside the chain (a mixed plan)
        int chunks = 0;      // ... the number of its chunks
        uint32_t nseg = 0;   // ... and of its segments
        const float *out_lo = nullptr, *out_hi = nullptr;  // audio buffer of the time-parallel call that used this set last
    } set[kSets];
    mi::Stream aux_stream;    // carries the serial core chain of the time-parallel path
    mi::Stream front_stream;  // stage 1 + aggregates of the time-parallel path
    mi::Event ev_entry;       // recorded on the caller's stream when a call starts
    mi::Event ev_head;        // ... and after the audio head of the call has been written
    mi::DevBuf<float2> d_cplx_set[2];  // pipelined serial calls alternate two plane sets (set[0 / 1].mag, d_cplx_set[0 / 1])
    int pset = 0;                  // ... the one holding the carried head
    bool serial_pipe = false;      // the last call was a pipelined serial call
    float* d_mag_last = nullptr;   // ... and these are the planes it worked on (mi_demod_read_planes): views
    float2* d_cplx_last = nullptr;
    uint32_t head_off = 0;     // plane index where the AGC_EXTRA carried samples of every row live (0 after a serial call)
    mi::Tuning opt;  // the tuning switches of this handle (tuning.hpp)
    bool chain_live = false;   // d_core_carry holds the chain state at the end of the previous call (it was time-parallel)
    mi::Stream seg_stream[kSegStreams];  // the speculative segment passes (need core(i) only)
    // MI_OPT_RESERVE_CUS: twins of the front and segment streams whose kernels keep off the last `reserve_cus` CUs (see enqueue_time_parallel)
    mi::Stream front_stream_m;
    mi::Stream seg_stream_m[kSegStreams];
    // MI_OPT_SPLIT_CUS: pipelined serial calls: stage 1 keeps off the last n CUs, k_demod runs on them alone (see enqueue_serial_pipelined)
    int split_state = 0;  // 0 undecided, 1 the two CU-masked streams exist, 2 none
    mi::Stream ps_front_m, ps_demod_m;
    mi::Event ev_ps_entry, ev_ps_done;
    int last_masked = -1;      // which side the previous time-parallel call used
    int masked_state = 0;      // 0 undecided, 1 the masked twins carry the time-parallel passes of this handle, 2 the plain streams do
    mi::DevBuf<mi::TpCore> d_core_carry;
    mi::DevBuf<float> d_full0;
    mi::DevBuf<float> d_fullbound;
    mi::DevBuf<float> d_afc_spec;  // [nstreams][fft_size] squared spectrum of the last window of a batch (AFC handles only)
    uint64_t call_seq = 0;
    // device memory
    mi::DevBuf<float> d_window;
    mi::DevBuf<float> d_tw;
    mi::DevBuf<float> d_prune_t1;  // stage-1 pruning tables (plan.prune)
    mi::DevBuf<float> d_prune_t2;
    mi::DevBuf<int> d_prune_rank;
    mi::DevBuf<L64Chan> d_l64_chan;       // per-channel tables of the lane-resident stage 1 (plan.l64): the plan's own instance,
    mi::DevBuf<L64Chan> d_l64_chan_full;  // the full-graph instance
    mi::DevBuf<unsigned> d_l64_tickets;   // run counters of its launches (kernels.hpp, kL64Tickets)
    unsigned l64_ticket_seq = 0;
    const mi::L64Jit* l64_jit = nullptr; // the kernel compiled for this plan's masks (owned by the process-wide cache), or null
    bool l64_jit_tried = false;
    const mi::L64Jit* l64_jit_masked = nullptr;  // ... its twin that takes a stream list, asked for when a mask first sets a stream aside
    bool l64_jit_masked_tried = false;
    bool l64_why_said = false;           // MI_AIRBAND_DEBUG: why this plan does not get the lane-resident kernel, said once
    int last_stage1 = 0;  // MI_STAGE1_* of the last call
    mi::DevBuf<float> d_levels;
    mi::DevBuf<float> d_sin;
    mi::DevBuf<float> d_cos;
    mi::DevBuf<mi::ChanParams> d_cp;
    mi::DevBuf<mi::ChanState> d_state;
    float* d_mag = nullptr;    // view: the planes of the last call, one of set[.].mag
    float2* d_cplx = nullptr;  // view: one of d_cplx_set[.]
    float* d_carry = nullptr;  // view: the audio lookahead the last call left, one of set[.].carry
    mi::DevBuf<float> d_ring;
    mi::DevBuf<float> d_ctcss_coeff;
    mi::DevBuf<float> d_ctcss_q;
    mi::DevBuf<mi_channel_stats> d_stats;
    mi::DevBuf<unsigned> d_pre_timeouts;  // waits of a channel wave for its pre-filter wave that ran out (k_demod_pw): expected 0
    // staging for the host-buffer entries: three slots, so that one call can be uploaded and one downloaded while a third
    // computes (mi_demod_submit / mi_demod_wait; mi_demod_process uses slot 0 alone).  A time-parallel call has ~2.5 ms of
    // latency whatever its length (segment pass -> scan -> fix -> ...), so with two slots a 16-s call could not be fed faster
    // than one per (upload + latency) / 2.
    static constexpr int kSlots = 3;
    struct Slot {
        mi::DevBuf<unsigned char> d_iq;   // [nstreams][iq_stride]
        mi::DevBuf<float> d_wout;         // [rows][max steps + AGC_EXTRA]: emitted audio + lookahead, the host layout
        mi::DevBuf<float2> d_iqout;       // [rows][max steps]
        mi::DevBuf<char> d_axc;           // [rows][max batches]
        mi::DevBuf<mi_channel_stats> d_stats;  // [rows] snapshot of the statistics after this call
        mi::PinnedBuf<unsigned char> h_in;   // upload staging for sources that are not pinned themselves
        mi::PinnedBuf<unsigned char> h_out;  // audio / raw I/Q / flags / statistics on their way back
        mi::Event up_done, done;
        bool busy = false;
        // where the results of the call in flight go
        int nbatches = 0;
        float* waveout = nullptr;
        float* iq_out = nullptr;
        char* axc = nullptr;
        mi_channel_stats* stats = nullptr;
        bool wave_direct = false;  // waveout is page-locked: the audio is downloaded straight into it
        bool masked = false;       // a call of some streams only: the regions of the others in the caller's arrays stay as they are
    } slot[kSlots];
    size_t iq_stride = 0, h_out_bytes = 0;
    bool slots_ready[kSlots] = {};
    int slot_next = 0, slot_oldest = 0, in_flight = 0;
    bool failed = false;  // a call advanced the DSP state and then could not deliver its results: every further call is refused
    mi::Stream copy_stream;  // uploads of submitted calls
    mi::Stream down_stream;  // their downloads
    // time-parallel stage 2 (tp.hip): the plain AM channels of the plan.  A mixed plan (cls.tp_mixed) sends those rows down that path and
    // the others through the serial kernel in the same call (MI_OPT_MIXED_PLAN), on a stream of its own beside the chain.
    mi::RowClasses cls;                  // rows of either kind (cls.tp_rows + cls.ser_rows == rows)
    mi::DevBuf<int> d_srows;             // the serial kernel's rows of a mixed plan (d_rows: the time-parallel path's)
    mi::Stream ser_stream;               // ... and its stream
    mi::Event ev_cplx_free[2];           // the serial kernel of a mixed call has read complex plane set p
    bool cplx_busy[2] = {};
    bool ser_head_next = false;          // the serial kernel of the last (mixed) call left its rows' carried samples in the next plane set
    Path last_path = kPathSerial;  // kPathSerial (any serial kernel) or kPathTimeParallel
    mi::DevBuf<int> d_rows;
    const float* prev_out_lo = nullptr;  // view: the caller's audio buffer of the previous call (its tail may still be writing it)
    const float* prev_out_hi = nullptr;
    // mi_demod_process_planes (test entry): stage 1 is replaced by a copy of caller-supplied planes, [row][inject_count]: views
    const float* inject_mag = nullptr;
    const float2* inject_cplx = nullptr;
    size_t inject_count = 0;
    mi::DevBuf<int> d_tstart;
    mi::DevBuf<int> d_need;
    mi::DevBuf<int> d_redo;  // [1 + rows*max_seg]: count, then the (row, segment) indices k_tp_fix leaves for k_tp_redo
    mi::DevBuf<mi::TpFinal> d_fin;
    mi::DevBuf<int> d_diag;
    size_t tp_max_blk = 0, tp_max_seg = 0;
    uint32_t tp_L = 512;  // steps per segment (kernels.hpp, TP_L_MIN .. TP_L_MAX), fixed when the handle is created
    // mi_demod_set_active_streams: the streams that take part in the calls made from now on.  A masked call (not every stream
    // active) runs stage 1 and the serial stage 2 over the lists below and nothing else: what the other streams carry between
    // calls (ChanState rows, lookahead, plane heads, squelch ring, CTCSS table, AFC bin) is in arrays indexed by handle row or
    // stream, which the kernels of such a call address through the lists alone.
    std::vector<uint8_t> active;   // [nstreams] 0 / 1
    int nactive = 0;
    bool masked = false;           // nactive < nstreams
    mi::DevBuf<int> d_act_streams; // [nactive] the active streams, ascending (uploaded when the mask is set, not per call)
    mi::DevBuf<int> d_act_rows;    // [nactive * nch] their handle rows
};

namespace {

int n_fft_for(const mi_demod* h, int nbatches) {
    return nbatches * mi::kWaveBatch + (h->first_call ? mi::kAgcExtra : 0);
}

constexpr int kTpMinBatches = 8;  // below this the segments are too few to pay for the extra passes
// Above this many rows the serial kernel is the faster path by itself: its time is the latency of one row (≈ 20-30 ns per step since
// round 3) whatever the number of rows, while the wide passes of the time-parallel path grow with them -- 8 / 16 / 32 / 64 streams x 8
// AM channels, 8-s calls: 1.35 / 1.67 / 2.60 / 4.69 ms time-parallel against 2.4 / 2.5 / 2.5 / 3.9 ms for k_demod, which also leaves
// stage 1 of the next call more of every SIMD.  MI_OPT_TIME_PARALLEL = 1 still forces the time-parallel path.
constexpr int kTpAutoMaxRows = 256;
// A mixed plan's call is as long as the longer of its two halves, and the time-parallel half has a fixed latency of a millisecond and
// more whatever the call's length (segment pass, scan, fix ...), while the serial kernel takes 0.3 ms per second of signal for every
// row: the split pays from about six seconds per call on (8 streams x 32 mixed channels, 2 / 4 / 8 s per call: 1.36 / 1.83 / 2.24 ms
// split against 0.70 / 1.41 / 2.58 whole; 1 stream x 32 at fft 2048, 8 s: 1.85 against 2.51).
constexpr int kMixedMinBatches = 64;

int slot_prepare(mi_demod* h, int k);  // (defined with the host-buffer entries below)

// The plan's own instance of the lane-resident stage 1 (hipRTC, or the code object an earlier start left on disk): 0.3-0.6 s
// when it has to be compiled, so it is asked for when the handle is created -- before any input thread fills a ring.
// `masked`: the instance that takes a stream list (calls of some streams only; never with AFC): compiled, or loaded from the
// cache, when mi_demod_set_active_streams first sets a stream aside -- a host that cannot afford the compilation between two
// batches sets such a mask once before its input threads start
void stage1_compile(mi_demod* h, bool masked) {
    bool& tried = masked ? h->l64_jit_masked_tried : h->l64_jit_tried;
    if (tried || !h->opt.l64_jit || !h->opt.l64 || !h->plan.l64.enabled || !h->d_l64_chan || (masked && h->plan.any_afc))
        return;
    tried = true;
    (masked ? h->l64_jit_masked : h->l64_jit) = mi::l64_jit_get(h->gpu, h->plan.log2n, h->plan.hop_samples(), h->plan.l64.need, nullptr, masked);
}

// MI_AIRBAND_DEBUG=1: once per handle, why its plan does not get the lane-resident stage 1
void stage1_explain(mi_demod* h) {
    if (h->l64_why_said)
        return;
    h->l64_why_said = true;  // (decided on the handle's first call, whatever the outcome)
    if (!mi::debug_enabled())
        return;
    const char* why = nullptr;
    if (!h->plan.l64.enabled)
        why = h->plan.l64.why ? h->plan.l64.why : "the plan does not allow it";
    else if (h->opt.l64 && h->opt.l64_jit && h->l64_jit_tried && !h->l64_jit)
        why = "hipRTC could not provide the plan's own instance";
    if (!why)
        return;
    std::fprintf(stderr, "mi_airband: no lane-resident stage 1 for this plan (%s); the exchange kernel runs\n", why);
}

int lanes_per_wave_for(const mi_demod* h, int rows) {
    // up to opt.uni_rows waves keep one channel each (the uniform instantiation of k_demod); beyond that pack lanes
    int lpw = (rows + h->opt.uni_rows - 1) / h->opt.uni_rows;
    return std::min(64, std::max(1, lpw));
}

// the second plane set of the pipelined serial path, allocated the first time it is wanted
bool serial_sets_ready(mi_demod* h) {
    if (h->set[1].mag && (h->d_cplx_set[1] || !h->d_cplx_set[0]))
        return true;
    mi::DevBuf<float> m;
    mi::DevBuf<float2> z;
    if ((!h->set[1].mag && dalloc_zero(m, static_cast<size_t>(h->rows) * h->plane_stride) != hipSuccess) ||
        (h->d_cplx_set[0] && !h->d_cplx_set[1] && dalloc_zero(z, static_cast<size_t>(h->nstreams) * h->plan.n_iq_rows * h->plane_stride) != hipSuccess)) {
        (void)hipGetLastError();
        return false;
    }
    if (m)
        h->set[1].mag = std::move(m);
    if (z)
        h->d_cplx_set[1] = std::move(z);
    return true;
}

// One call on its way to the GPU: what every path reads of it
struct Call {
    // the arguments of enqueue()
    const unsigned char* d_iq;
    size_t stream_stride, valid_bytes;
    int nbatches;
    float* d_wmain;
    size_t wmain_stride;
    float2* d_iq_out;
    size_t iq_out_stride;
    char* d_axc;
    hipStream_t s;
    hipEvent_t iq_ready;
    bool early_input;  // the IQ is valid when the streams that read it have waited for iq_ready (if any) and for nothing else
    bool partial;      // a masked call: some streams sit it out
    int act_streams, act_rows;
    mi::ChannelizeArgs ca;   // stage 1 of the whole call on the planes of the last call (the paths point it elsewhere)
    mi::DemodArgs da;        // ... and the serial stage 2
    const mi::Event* evc;    // the per-call events (CallEv) of the scratch set this call records on
};

void make_channelize_args(mi_demod* h, Call& call) {
    const bool partial = call.partial;
    mi::ChannelizeArgs& ca = call.ca;
    ca.iq = call.d_iq;
    ca.stream_stride = call.stream_stride;
    ca.valid_bytes = call.valid_bytes;
    ca.hop_bytes = static_cast<uint32_t>(h->plan.hop_bytes);
    ca.nfft = static_cast<uint32_t>(n_fft_for(h, call.nbatches));
    ca.mag = h->d_mag;
    ca.cplx = h->d_cplx;
    ca.plane_stride = h->plane_stride;
    ca.plane_off = h->first_call ? 0 : mi::kAgcExtra;
    ca.window = h->d_window;
    ca.tw = h->d_tw;
    ca.prune = h->plan.prune;
    ca.prune.enabled = (ca.prune.enabled && h->opt.prune) ? 1 : 0;
    ca.prune_t1 = h->d_prune_t1;
    ca.prune_t2 = h->d_prune_t2;
    ca.prune_rank = h->d_prune_rank;
    ca.l64 = h->plan.l64;
    ca.l64.enabled = (ca.l64.enabled && h->opt.l64 && h->d_l64_chan) ? 1 : 0;
    ca.l64.linear_tiles = 0;
    ca.l64.wg_per_cu = h->opt.l64_wgs;  // (MI_AIRBAND_L64_WGS: workgroups per CU of the persistent stage-1 launch, 0 = default)
    ca.l64_chan = h->d_l64_chan;
    ca.l64_tickets = h->d_l64_tickets;
    ca.l64_ticket_seq = &h->l64_ticket_seq;
    ca.l64_chan_full = h->d_l64_chan_full;
    if (ca.l64.enabled) {  // (normally done by mi_demod_create / _set_active_streams; here only if the option was switched on afterwards)
        stage1_compile(h, false);
        if (partial)
            stage1_compile(h, true);
    }
    ca.l64_jit = h->opt.l64_jit ? (partial ? h->l64_jit_masked : h->l64_jit) : nullptr;
    // The prebuilt full-graph instance keeps all 64 points of a lane live and is slower than the exchange kernels: it runs
    // only when asked for (MI_OPT_LANE_FFT_JIT = 0, tests); without hipRTC the pruned / full exchange kernels take over.
    if (ca.l64.enabled && h->opt.l64_jit && !ca.l64_jit)
        ca.l64.enabled = 0;
    stage1_explain(h);
    ca.levels = h->d_levels;
    {
        const bool pruned = ca.prune.enabled && h->plan.log2n == 9 && !h->plan.any_afc;
        const int cc = h->opt.conv;
        ca.conv_arith = (h->plan.conv_arith && (cc < 0 ? !pruned : cc == 1)) ? 1 : 0;
    }
    ca.conv_scale = h->plan.conv_scale;
    ca.cp = h->d_cp;
    ca.nch = h->nch;
    ca.n_iq_rows = h->plan.n_iq_rows;
    ca.streams = partial ? h->d_act_streams.get() : nullptr;
    ca.nactive = call.act_streams;
    h->last_stage1 = (ca.l64.enabled && !h->plan.any_afc) ? (ca.l64_jit ? MI_STAGE1_LANE_PLAN : MI_STAGE1_LANE_FULL)
                     : ((ca.prune.enabled && h->plan.log2n == 9 && !h->plan.any_afc) ? MI_STAGE1_EXCHANGE_PRUNED : MI_STAGE1_EXCHANGE_FULL);
    ca.xmax = nullptr;  // (the time-parallel path points it at its scratch set)
}

void make_demod_args(const mi_demod* h, Call& call) {
    const bool partial = call.partial;
    const int nbatches = call.nbatches, act_rows = call.act_rows;
    mi::DemodArgs& da = call.da;
    da.nstreams = h->nstreams;
    da.nch = h->nch;
    da.rows = partial ? h->d_act_rows.get() : nullptr;
    da.nrows = act_rows;
    da.carry_in = nullptr;
    da.n_iq_rows = h->plan.n_iq_rows;
    da.n_ctcss_rows = h->plan.n_ctcss_rows;
    da.nsteps = static_cast<uint32_t>(nbatches) * mi::kWaveBatch;
    da.nbatches = static_cast<uint32_t>(nbatches);
    da.mag = h->d_mag;
    da.cplx = h->d_cplx;
    da.mag_head = h->d_mag;
    da.cplx_head = h->d_cplx;
    da.plane_stride = h->plane_stride;
    da.wmain = call.d_wmain;
    da.wmain_stride = call.wmain_stride;
    da.carry = h->d_carry;
    da.iq_out = call.d_iq_out;
    da.iq_out_stride = call.iq_out_stride;
    da.axc = call.d_axc;
    da.axc_stride = static_cast<uint32_t>(nbatches);
    da.cp = h->d_cp;
    da.st = h->d_state;
    da.sin_lut = h->d_sin;
    da.cos_lut = h->d_cos;
    da.sq_ring = h->d_ring;
    da.ctcss_coeff = h->d_ctcss_coeff;
    da.ctcss_q = h->d_ctcss_q;
    da.stats = h->d_stats;
    da.fm_quadri = h->plan.dev.fm_quadri;
    da.lanes_per_wave = lanes_per_wave_for(h, act_rows);
    da.steady_blocks = h->opt.steady_blocks ? 1 : 0;
    // the pre-filter wave pays where a call is bound by the latency of its rows (4 / 8 / 16 streams x 32 mixed channels: +44 / +37 /
    // +12 %); with a thousand rows and more the machine is full and a second wave per row only takes LDS and issue slots from
    // stage 1 (32 streams: +-0, 64 streams: -27 %)
    // (round 3: four waves per channel, each with a SIMD's register file to itself: one channel per CU, so up to 256 rows)
    // ... and two waves per channel (the channel with its audio, the pre-filter wave) up to 1 024 rows: 2 = k_demod_pw2
    da.pre_wave = h->opt.pre_wave < 0 ? (act_rows <= 256 ? 1 : (act_rows <= 1024 ? 2 : 0)) : std::min(2, h->opt.pre_wave);
    da.audio_wave = h->opt.audio_wave ? 1 : 0;
    da.pre_timeouts = h->d_pre_timeouts;
}

// The path of a call.  The conditions are evaluated left to right and no further than they decide: serial_sets_ready() allocates the
// second plane set, which a handle gets only when a call of its own is about to use it.
Path choose_path(mi_demod* h, const Call& call) {
    const int env = h->opt.tp;
    if (!call.partial && h->cls.tp_eligible && env != 0 && (!h->cls.tp_mixed || (h->opt.mixed && serial_sets_ready(h))) &&
        (env == 1 || (call.nbatches >= (h->cls.tp_mixed ? kMixedMinBatches : kTpMinBatches) && h->cls.tp_rows <= kTpAutoMaxRows)))
        return kPathTimeParallel;
    if (h->plan.any_afc)
        return kPathAfc;
    // (a handle whose plan the time-parallel path could take as well -- many rows, or MI_OPT_TIME_PARALLEL = 0 -- pipelines its serial
    //  calls like any other as long as its planes are where that path keeps them: never after a time-parallel call)
    if (!call.partial && call.early_input && !h->first_call &&
        (!h->cls.tp_eligible || (h->head_off == 0 && (h->d_mag == h->set[0].mag || h->d_mag == h->set[1].mag))) && serial_sets_ready(h))
        return kPathSerialPipelined;
    return kPathSerial;
}

// the serial kernels expect the carried AGC_EXTRA samples of every row at the front of the planes they work on
int head_in_place(mi_demod* h, const Call& call) {
    if (h->head_off != 0) {
        HIP_TRY(mi::launch_move_head(h->d_mag, h->d_mag + h->head_off, h->plane_stride, h->rows, call.s));
        h->head_off = 0;
    }
    return MI_OK;
}

// stage 1 of the windows [f0, f0 + cc.nfft) of this call -- or, for mi_demod_process_planes, the caller's planes in their place
hipError_t stage1_launch(const mi_demod* h, const mi::ChannelizeArgs& cc, uint32_t f0, hipStream_t st) {
    if (!h->inject_mag)
        return mi::launch_channelize(cc, h->plan.log2n, h->plan.dev.sfmt, h->nstreams, st);
    hipError_t e = hipMemcpy2DAsync(cc.mag + cc.plane_off, cc.plane_stride * 4, h->inject_mag + f0, h->inject_count * 4, static_cast<size_t>(cc.nfft) * 4,
                                    static_cast<size_t>(h->rows), hipMemcpyDeviceToDevice, st);
    const size_t zrows = static_cast<size_t>(h->nstreams) * h->plan.n_iq_rows;
    if (e == hipSuccess && zrows && h->inject_cplx)
        e = hipMemcpy2DAsync(cc.cplx + cc.plane_off, cc.plane_stride * 8, h->inject_cplx + f0, h->inject_count * 8, static_cast<size_t>(cc.nfft) * 8, zrows,
                             hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess && cc.xmax)
        e = mi::launch_row_max(cc.mag + cc.plane_off, cc.plane_stride, cc.nfft, h->rows, cc.xmax, st);
    return e;
}

// CU mask of a stream (hipExtStreamCreateWithCUMask) over the CUs [lo, hi) of ncu
std::vector<uint32_t> cu_mask(int ncu, int lo, int hi) {
    std::vector<uint32_t> mask(static_cast<size_t>((ncu + 31) / 32), 0u);
    for (int i = lo; i < hi; ++i)
        mask[static_cast<size_t>(i) / 32] |= 1u << (i % 32);
    return mask;
}

hipError_t cu_stream_create(mi::Stream& st, const std::vector<uint32_t>& mask) {
    return hipExtStreamCreateWithCUMask(st.put(), static_cast<uint32_t>(mask.size()), mask.data());
}

// A non-blocking stream at the highest or the lowest priority: a queue class of its own either way.  HIP multiplexes its streams onto
// a few hardware queues and two streams that share one run their kernels one after the other (so the wide passes share few streams).
hipError_t priority_stream(mi::Stream& st, bool highest) {
    int lo_prio = 0, hi_prio = 0;
    const hipError_t e = hipDeviceGetStreamPriorityRange(&lo_prio, &hi_prio);
    return e != hipSuccess ? e : hipStreamCreateWithPriority(st.put(), hipStreamNonBlocking, highest ? hi_prio : lo_prio);
}

// Scratch set q of a handle the time-parallel path can serve (set 0 has its planes and lookahead already: every handle needs them)
int alloc_call_set(mi_demod* h, int q) {
    mi_demod::CallSet& cs = h->set[q];
    const size_t rows = static_cast<size_t>(h->rows);
    if (q >= 1) {
        HIP_TRY(dalloc_zero(cs.mag, rows * h->plane_stride));
        HIP_TRY(dalloc(cs.carry, rows * mi::kAgcExtra));
    }
    HIP_TRY(dalloc(cs.xmax, rows));
    for (mi::DevBuf<float>* agg : {&cs.blk_fe, &cs.blk_fm, &cs.blk_x0, &cs.blk_xm})
        HIP_TRY(dalloc(*agg, rows * h->tp_max_blk));
    HIP_TRY(dalloc(cs.core, rows * (h->tp_max_seg + 1)));
    HIP_TRY(dalloc(cs.rec, static_cast<size_t>(mi::TP_NREC) * rows * h->tp_max_seg));
    return MI_OK;
}

// Chunk i of a time-parallel call covers units [bound[i], bound[i+1]): `want` chunks (at most one per unit), each `ratio` times the
// one before it
std::vector<uint32_t> tp_chunk_bounds(uint32_t units, int want, double ratio) {
    std::vector<uint32_t> bound{0};
    if (units > 0) {
        want = std::min<int>(want, static_cast<int>(units));
        double total = 0.0, w = 1.0;
        for (int i = 0; i < want; ++i, w *= ratio)
            total += w;
        double acc = 0.0;
        w = 1.0;
        for (int i = 0; i < want; ++i, w *= ratio) {
            acc += w;
            uint32_t bd = (i == want - 1) ? units : static_cast<uint32_t>(acc / total * units + 0.5);
            bd = std::max(bd, bound.back() + 1);
            bd = std::min(bd, units - static_cast<uint32_t>(want - 1 - i));
            bound.push_back(bd);
        }
    } else {
        bound.push_back(0);
    }
    return bound;
}

// what every chunk of a time-parallel call on scratch set q shares (the chunks add their own ranges)
mi::TpArgs make_tp_args(const mi_demod* h, const Call& call, int q, bool overlap, bool spec_head) {
    const uint32_t n = call.da.nsteps, L = h->tp_L;
    mi::TpArgs ta{};
    ta.rows = h->d_rows;
    ta.nrows = h->cls.tp_rows;
    ta.nch = h->nch;
    ta.nsteps = n;
    ta.nbatches = call.da.nbatches;
    ta.nblk = n / 16;
    ta.L = L;
    ta.nseg = (n + L - 1) / L;
    ta.mag = h->set[q].mag;
    ta.plane_stride = h->plane_stride;
    ta.wmain = call.d_wmain;
    ta.wmain_stride = call.wmain_stride;
    ta.carry = h->set[q].carry;
    ta.carry_prev = h->d_carry;
    ta.axc = call.d_axc;
    ta.cp = h->d_cp;
    ta.st = h->d_state;
    ta.stats = h->d_stats;
    ta.xmax = h->set[q].xmax;
    ta.blk_fe = h->set[q].blk_fe;
    ta.blk_fm = h->set[q].blk_fm;
    ta.blk_x0 = h->set[q].blk_x0;
    ta.blk_xm = h->set[q].blk_xm;
    ta.core = h->set[q].core;
    ta.core_carry = h->d_core_carry;
    ta.full0 = h->d_full0;
    ta.fullbound = h->d_fullbound;
    ta.prev_mag = overlap ? h->d_mag : nullptr;  // (still the previous call's planes here)
    ta.prev_n = h->head_off;
    ta.xmax_prev = h->set[h->cur].xmax;
    ta.rec = h->set[q].rec;
    ta.rec_stride = static_cast<size_t>(h->rows) * h->tp_max_seg;
    ta.tstart = h->d_tstart;
    ta.need = h->d_need;
    ta.redo = h->d_redo;
    ta.fin = h->d_fin;
    ta.diag = h->d_diag;
    ta.seg_lpw = h->opt.tp_lpw;
    ta.core_split = (h->opt.core_split && h->cls.core_split_ok) ? 1 : 0;
    ta.core_lead = h->opt.core_lead;
    ta.core_guess = h->opt.core_guess;
    ta.core_decay = h->opt.core_decay;
    ta.core_lean = h->opt.core_lean;
    ta.agc_hint = h->opt.agc_hint;
    ta.eager_samples = h->opt.tp_eager;
    ta.spec_head = spec_head ? 1 : 0;
    ta.prev_blk_fe = h->set[h->cur].blk_fe, ta.prev_blk_fm = h->set[h->cur].blk_fm;
    ta.prev_blk_x0 = h->set[h->cur].blk_x0, ta.prev_blk_xm = h->set[h->cur].blk_xm;
    ta.prev_core = h->set[h->cur].core;
    ta.prev_nblk = h->head_off / 16;
    ta.prev_nseg = h->set[h->cur].nseg;
    return ta;
}

// ---- time-parallel stage 2, pipelined over chunks of the call and across calls ----
// The exact core chain (k_tp_core) is serial per channel and latency bound on 8 waves; everything else is wide.
//   front stream : head carry, then per chunk stage 1 + k_tp_full           (needs the IQ; chunk 0's k_tp_full needs
//                                                                             the chain state at the call start)
//   aux stream   : k_tp_core(i) as soon as chunk i's aggregates exist         (one chain across chunks AND calls)
//   seg streams  : k_tp_seg(i) as soon as core(i) is done and the previous call has left its final state
//   caller's     : audio head, then scan / fix / redo / finish of chunk i after seg(i) and the chain of chunk i-1
// With MI_OPT_EARLY_INPUT the front and aux streams do not wait for the caller's stream, i.e. for the segment
// and fix passes of the previous call: consecutive calls overlap and the core chain runs back to back.
int enqueue_time_parallel(mi_demod* h, Call& call) {
    const hipStream_t s = call.s;
    mi::ChannelizeArgs& ca = call.ca;
    const int q = (h->cur + 1) % mi_demod::kSets;  // the scratch set of this call
    mi_demod::CallSet& cs = h->set[q];
    float* const planes = cs.mag;
    const bool overlap = call.early_input && h->chain_live && !h->first_call;
    const float* out_lo = call.d_wmain;
    const float* out_hi = call.d_wmain + static_cast<size_t>(h->rows - 1) * call.wmain_stride + call.da.nsteps;
    // segment passes may run under the previous call's tail only if they write a different audio buffer
    const bool seg_early = overlap && (out_hi <= h->prev_out_lo || out_lo >= h->prev_out_hi);
    const uint32_t n = call.da.nsteps;
    const uint32_t L = h->tp_L;
    const uint32_t chunk_unit = mi::tp_chunk_unit(L);
    const uint32_t units = n / chunk_unit;
    // Chunk sizes grow geometrically: a short first chunk gets the serial core chain going early (its stage 1 +
    // aggregates are all that precedes it), later chunks are long because every wide pass has a fixed latency per
    // launch.  MI_AIRBAND_TP_CHUNKS / MI_AIRBAND_TP_RATIO override the measured defaults.
    // An isolated call: 3 chunks growing by 1.5x (round 1; see below).  When calls overlap the chain is already running and stage 1 of this
    // call hides under the previous call: one chunk then -- every chunk boundary costs the chain a launch gap and the
    // tail passes on the caller's stream (scan / fix / redo / settle / finish) their fixed latencies once more, and with
    // two chunks those passes took as long per call as the chain itself (1 / 2 / 3 / 4 chunks over 20 steps: 2.21 / 2.40 /
    // 2.9 / 3.5 ms per step; over 5 steps, where the last call's drain weighs more, 1 and 2 are level).
    // (that is the few-rows case, where the per-channel chain is the critical path; with hundreds of rows the wide passes
    // are, and two chunks let stage 1 of the second run under the segment / fix passes of the first: 64 streams x 8
    // channels 168 vs 147 GS/s)
    // (isolated calls, round 2: with the chain on three waves an isolated call is a sum of fixed latencies -- stage 1, aggregates,
    // chain, segment pass, scan, fix, finish -- and every chunk adds the last four once more: 2 chunks, the second twice the
    // first, 3.7 instead of 4.1 ms per 64-s call and 2.6 instead of 3.3 per 16-s call; with many rows 2, 3 and 4 are level)
    int want = overlap ? (h->cls.tp_rows <= 64 ? 1 : 2) : (h->cls.tp_rows <= 64 ? 2 : 3);
    double ratio = overlap ? 1.0 : (h->cls.tp_rows <= 64 ? 2.0 : 1.5);
    if (h->opt.tp_chunks > 0)
        want = h->opt.tp_chunks;
    if (h->opt.tp_ratio > 0)
        ratio = h->opt.tp_ratio;
    const std::vector<uint32_t> bound = tp_chunk_bounds(units, want, ratio);
    const int C = static_cast<int>(bound.size()) - 1;
    if (C > mi_demod::kMaxChunks)
        return fail(MI_ERR_INVALID, "too many chunks");
    while (static_cast<int>(cs.chunk_ev.size()) < C * kEvPerChunk) {
        mi::Event e;
        HIP_TRY(hipEventCreate(e.put()));
        cs.chunk_ev.push_back(std::move(e));
    }
    call.evc = cs.ev;
    const mi::Event* const evc = call.evc;
    // Speculative head: when this call's segment pass may run under the previous call's tail at all (seg_early) and that call
    // left what the warm-up needs (aggregates, core states at boundaries of the same segment length, TP_W steps of them),
    // no lane starts from the carried ChanState and no launch of the pass waits for the previous call.
    const bool spec_head = seg_early && h->opt.spec_head && h->head_off >= mi::TP_W && h->set[h->cur].seq &&
                           h->set[h->cur].path == kPathTimeParallel;
    const mi::TpArgs ta = make_tp_args(h, call, q, overlap, spec_head);
    cs.nseg = ta.nseg;
    auto chunk = [&](int i) {
        mi::TpArgs c = ta;
        c.step0 = bound[static_cast<size_t>(i)] * chunk_unit;
        c.step1 = (i == C - 1) ? n : bound[static_cast<size_t>(i) + 1] * chunk_unit;
        c.seg0 = c.step0 / L;
        c.seg1 = (c.step1 + L - 1) / L;
        c.blk0 = c.step0 / 16;
        c.blk1 = c.step1 / 16;
        c.bat0 = c.step0 / mi::kWaveBatch;
        c.bat1 = c.step1 / mi::kWaveBatch;
        c.first_chunk = i == 0;
        c.last_chunk = i == C - 1;
        return c;
    };
    const bool first_call = h->first_call;
    // A mixed plan: stage 1 leaves the raw bins of this call in complex plane set p, the serial kernel reads them there and leaves
    // its carried head in the other set for the next call (as the pipelined serial calls do).
    const int zp = (h->d_cplx && h->d_cplx == h->d_cplx_set[1]) ? 1 : 0, znp = zp ^ 1;
    if (h->cls.tp_mixed) {
        ca.cplx = h->d_cplx_set[zp];
    }
    // The wide passes of a call (stage 1, aggregates, segment pass: thousands of waves that hold most of a SIMD's registers for a
    // millisecond) run beside the latency-bound kernels of its neighbours: the core chains, and the tail (scan / fix / redo /
    // settle / finish: a handful of lanes, 280-430 VGPRs a wave), which then wait for a wide wave to retire before they can
    // start at all -- 1.5 ms per call for 0.65 ms of work.  So on plans of few rows the wide passes keep off a few CUs
    // (hipExtStreamCreateWithCUMask), where the others always find room.  Such a stream is a blocking one (it synchronises
    // with the NULL stream): the twins are created at the handle's first time-parallel call and used by every call whose stream
    // is not the NULL stream.
    if (h->masked_state == 0) {
        const int want = h->opt.reserve_cus >= 0 ? h->opt.reserve_cus : (h->cls.tp_rows <= 64 ? 32 : 0);
        h->masked_state = 2;
        hipDeviceProp_t prop{};
        if (want > 0 && hipGetDeviceProperties(&prop, h->gpu) == hipSuccess && prop.multiProcessorCount >= want + 32) {
            const int ncu = prop.multiProcessorCount, keep = ncu - want;
            const std::vector<uint32_t> mask = cu_mask(ncu, 0, keep);
            hipError_t me = cu_stream_create(h->front_stream_m, mask);
            for (mi::Stream& ssm : h->seg_stream_m)
                if (me == hipSuccess)
                    me = cu_stream_create(ssm, mask);
            if (me == hipSuccess)
                h->masked_state = 1;
            else
                (void)hipGetLastError();  // (no such streams here: the plain ones serve)
        }
    }
    // (a call on the NULL stream takes the plain streams whatever the handle decided; changing sides between calls is rare and
    //  costs a host wait: the passes of consecutive calls are ordered by their stream, not by events)
    const bool masked = h->masked_state == 1 && s != nullptr;
    if (h->last_masked >= 0 && h->last_masked != (masked ? 1 : 0)) {
        HIP_TRY(hipStreamSynchronize(h->last_masked ? h->front_stream_m : h->front_stream));
        for (int i = 0; i < mi_demod::kSegStreams; ++i)
            HIP_TRY(hipStreamSynchronize(h->last_masked ? h->seg_stream_m[i] : h->seg_stream[i]));
    }
    h->last_masked = masked ? 1 : 0;
    hipStream_t fs = masked ? h->front_stream_m : h->front_stream;
    auto stage1 = [&](const mi::TpArgs& c) -> hipError_t {  // the windows whose magnitudes are the chunk's squelch samples
        mi::ChannelizeArgs cc = ca;
        const uint32_t f0 = first_call ? (c.first_chunk ? 0u : c.step0 + mi::kAgcExtra) : c.step0;
        const uint32_t f1 = first_call ? c.step1 + mi::kAgcExtra : c.step1;
        cc.iq = ca.iq + static_cast<size_t>(f0) * ca.hop_bytes;
        cc.valid_bytes = ca.valid_bytes - static_cast<size_t>(f0) * ca.hop_bytes;
        cc.nfft = f1 - f0;
        cc.plane_off = ca.plane_off + f0;
        cc.mag = planes;
        cc.xmax = cs.xmax;
        return stage1_launch(h, cc, f0, fs);
    };
    HIP_TRY(hipEventRecord(h->ev_entry, s));
    HIP_TRY(hipEventRecord(evc[kEvBegin], s));
    HIP_TRY(hipEventRecord(evc[kEvStage1Done], s));
    HIP_TRY(mi::launch_tp_audio_head(ta, s));
    HIP_TRY(hipEventRecord(h->ev_head, s));  // the previous call is complete and its lookahead has been taken over
    if (call.iq_ready)
        HIP_TRY(hipStreamWaitEvent(fs, call.iq_ready, 0));
    if (!overlap)
        HIP_TRY(hipStreamWaitEvent(fs, h->ev_entry, 0));  // stage 1 honours the caller's stream order
    else if (cs.seq)
        HIP_TRY(hipStreamWaitEvent(fs, cs.ev[kEvDone], 0));  // the call that used this scratch set last (kSets back) has left it
    {
        // ... and the call after that one has read what its speculative head needed from that set (planes, aggregates, core
        // states): its segment pass is done (always long before; the wait costs nothing)
        const mi_demod::CallSet& next = h->set[(q + 1) % mi_demod::kSets];
        if (next.seq && next.path == kPathTimeParallel && next.chunks > 0)
            HIP_TRY(hipStreamWaitEvent(fs, next.chunk(next.chunks - 1, kEvSegLaunched), 0));
    }
    if (h->cls.tp_mixed && h->cplx_busy[zp])  // (the serial kernel of the call before the previous one read this complex plane set)
        HIP_TRY(hipStreamWaitEvent(fs, h->ev_cplx_free[zp], 0));
    // the carried samples of the previous call (wherever they are) become the head of this call's planes -- of a mixed plan the
    // time-parallel rows' only where the serial kernel of the previous call has put its own rows' there itself
    if (h->cls.tp_mixed && h->ser_head_next && planes == h->set[(h->cur + 1) % mi_demod::kSets].mag)
        HIP_TRY(mi::launch_move_head(planes, h->d_mag + h->head_off, h->plane_stride, h->cls.tp_rows, fs, h->d_rows));
    else
        HIP_TRY(mi::launch_move_head(planes, h->d_mag + h->head_off, h->plane_stride, h->rows, fs));
    HIP_TRY(hipMemsetAsync(cs.xmax, 0, static_cast<size_t>(h->rows) * sizeof(unsigned), fs));
    // Stage 1 + aggregates of every chunk first: nothing else feeds them (when calls overlap, k_tp_full warms its first
    // lanes up on the previous call's planes, so not even the chain state of that call).
    for (int i = 0; i < C; ++i) {
        const mi::TpArgs c = chunk(i);
        HIP_TRY(hipEventRecord(cs.chunk(i, kEvStage1Begin), fs));
        HIP_TRY(stage1(c));
        HIP_TRY(hipEventRecord(cs.chunk(i, kEvStage1End), fs));
        HIP_TRY(hipEventRecord(cs.chunk(i, kEvFullBegin), fs));
        HIP_TRY(mi::launch_tp_front(c, fs, /*seed_chain=*/!overlap));
        HIP_TRY(hipEventRecord(cs.chunk(i, kEvFullEnd), fs));
    }
    for (int i = 0; i < C; ++i) {
        const mi::TpArgs c = chunk(i);
        HIP_TRY(hipStreamWaitEvent(h->aux_stream, cs.chunk(i, kEvFullEnd), 0));
        HIP_TRY(hipEventRecord(cs.chunk(i, kEvCoreBegin), h->aux_stream));
        HIP_TRY(mi::launch_tp_core(c, h->aux_stream));
        HIP_TRY(hipEventRecord(cs.chunk(i, kEvCoreEnd), h->aux_stream));
        hipStream_t ss = masked ? h->seg_stream_m[i % mi_demod::kSegStreams] : h->seg_stream[i % mi_demod::kSegStreams];
        // A segment pass needs core(i).  It also has to wait for the previous call (ev_head) where it touches what
        // that call's tail still owns: the carried ChanState (the lanes of the first TP_W / L + 1 segments start
        // from it), the audio lookahead (written by the last segments) and the caller's audio buffer if it is the
        // one the previous call wrote.
        HIP_TRY(hipStreamWaitEvent(ss, cs.chunk(i, kEvCoreEnd), 0));
        if (seg_early) {
            // The pass writes the caller's audio buffer: the last call that wrote the same memory has to be complete (its fades
            // rewrite audio).  Not the previous call (seg_early); with two buffers alternating the one before it, with three the
            // one before that -- then the pass has two tail periods of slack instead of one and the tails run back to back.
            for (int back = 1; back < mi_demod::kSets - 1; ++back) {
                const mi_demod::CallSet& past = h->set[(h->cur + mi_demod::kSets - back) % mi_demod::kSets];
                if (!past.seq)
                    break;
                if (past.path != kPathTimeParallel || !(out_hi <= past.out_lo || out_lo >= past.out_hi)) {
                    HIP_TRY(hipStreamWaitEvent(ss, past.ev[kEvDone], 0));
                    break;
                }
            }
        }
        // (events kEvSegBegin -> kEvSegEnd time the pass itself: they sit inside every wait of the segment stream; of a split first
        // chunk the body is timed, its few head segments are not)
        // With a speculative head nothing of the pass waits for the previous call; otherwise the whole pass does where it may not
        // run early at all or is the call's last chunk, and of a first chunk only the few head segments, launched after the body.
        const uint32_t head_end = std::min<uint32_t>(c.seg1, mi::TP_W / L + 1);
        const bool wait_first = !spec_head && (!seg_early || c.last_chunk);
        const bool split_head = !spec_head && !wait_first && c.first_chunk && c.seg0 < head_end;
        mi::TpArgs body = c, head = c;
        if (split_head)
            body.seg0 = head.seg1 = head_end;
        if (wait_first)
            HIP_TRY(hipStreamWaitEvent(ss, h->ev_head, 0));
        HIP_TRY(hipEventRecord(cs.chunk(i, kEvSegBegin), ss));
        if (!split_head || body.seg0 < body.seg1)
            HIP_TRY(mi::launch_tp_seg(body, ss));
        HIP_TRY(hipEventRecord(cs.chunk(i, kEvSegEnd), ss));
        if (split_head) {
            HIP_TRY(hipStreamWaitEvent(ss, h->ev_head, 0));
            HIP_TRY(mi::launch_tp_seg(head, ss));
        }
        HIP_TRY(hipEventRecord(cs.chunk(i, kEvSegLaunched), ss));
        HIP_TRY(hipStreamWaitEvent(s, cs.chunk(i, kEvSegLaunched), 0));
        HIP_TRY(hipEventRecord(cs.chunk(i, kEvScanBegin), s));
        hipEvent_t marks[mi::TP_REST_MARKS] = {cs.chunk(i, kEvScanEnd), cs.chunk(i, kEvFixEnd), cs.chunk(i, kEvFinishEnd)};
        HIP_TRY(mi::launch_tp_rest(c, s, marks));
    }
    cs.mixed = false;
    h->ser_head_next = false;
    if (h->cls.tp_mixed && h->cls.ser_rows > 0) {
        // ---- the rows the time-parallel path does not take: k_demod on its own stream, beside the chain ----
        // It needs stage 1 of the whole call (the last chunk's end on the front stream), the serial kernel of the previous call
        // (same stream) and, where calls do not overlap, the caller's stream order.
        hipStream_t zs = h->ser_stream;
        HIP_TRY(hipStreamWaitEvent(zs, cs.chunk(C - 1, kEvStage1End), 0));
        if (!overlap)
            HIP_TRY(hipStreamWaitEvent(zs, h->ev_entry, 0));
        if (!seg_early)
            HIP_TRY(hipStreamWaitEvent(zs, h->ev_head, 0));  // (it writes the audio buffer the previous call wrote)
        mi::DemodArgs dm = call.da;
        dm.rows = h->d_srows;
        dm.nrows = h->cls.ser_rows;
        dm.mag = planes;
        dm.cplx = h->d_cplx_set[zp];
        dm.mag_head = h->set[(q + 1) % mi_demod::kSets].mag;  // (free: the call that used it last is four calls back)
        dm.cplx_head = h->d_cplx_set[znp];
        dm.carry = cs.carry;
        dm.carry_in = h->d_carry;
        dm.lanes_per_wave = lanes_per_wave_for(h, h->cls.ser_rows);
        dm.pre_wave = (h->opt.pre_wave < 0 ? h->cls.ser_rows <= 256 : h->opt.pre_wave != 0) ? 1 : 0;
        HIP_TRY(hipEventRecord(evc[kEvSerialBegin], zs));
        HIP_TRY(mi::launch_demod(dm, zs));
        HIP_TRY(hipEventRecord(evc[kEvSerialEnd], zs));
        HIP_TRY(hipEventRecord(h->ev_cplx_free[zp], zs));
        h->cplx_busy[zp] = true;
        HIP_TRY(hipStreamWaitEvent(s, evc[kEvSerialEnd], 0));
        h->d_cplx = h->d_cplx_set[znp];
        h->d_cplx_last = h->d_cplx_set[zp];
        h->pset = znp;
        cs.mixed = true;
        h->ser_head_next = true;
    }
    cs.chunks = C;
    h->cur = q;
    h->d_carry = cs.carry;
    h->d_mag = planes;
    h->head_off = n;  // (first call: the planes hold AGC_EXTRA + n samples, the last AGC_EXTRA start at n as well)
    h->chain_live = true;
    h->prev_out_lo = out_lo;
    h->prev_out_hi = out_hi;
    cs.out_lo = out_lo;
    cs.out_hi = out_hi;
    return MI_OK;
}

// AFC (rtl_airband.cpp:180-251): the bins stage 1 picks in batch b+1 depend on the squelch outcome of batch b, so
// the batches are enqueued one at a time -- stage 1, channel loop, AFC::finalize -- with the bin table and the
// previous indicator resident in ChanState: no host round trip inside the call.
int enqueue_afc(mi_demod* h, const Call& call) {
    const hipStream_t s = call.s;
    const mi::ChannelizeArgs& ca = call.ca;
    if (call.iq_ready)
        HIP_TRY(hipStreamWaitEvent(s, call.iq_ready, 0));
    HIP_TRY(hipEventRecord(call.evc[kEvBegin], s));
    size_t f0 = 0;  // first window of the batch, relative to the call
    for (int b = 0; b < call.nbatches; ++b) {
        const bool first = h->first_call && b == 0;
        const uint32_t nf = mi::kWaveBatch + (first ? mi::kAgcExtra : 0);
        mi::ChannelizeArgs cb = ca;
        cb.iq = ca.iq + f0 * ca.hop_bytes;
        cb.valid_bytes = ca.valid_bytes - f0 * ca.hop_bytes;
        cb.nfft = nf;
        cb.plane_off = first ? 0 : mi::kAgcExtra;
        cb.st = h->d_state;
        cb.afc_spec = h->d_afc_spec;
        HIP_TRY(mi::launch_channelize(cb, h->plan.log2n, h->plan.dev.sfmt, h->nstreams, s));
        if (b == 0)
            HIP_TRY(hipEventRecord(call.evc[kEvStage1Done], s));
        mi::DemodArgs db = call.da;
        db.nsteps = mi::kWaveBatch;
        db.nbatches = 1;
        db.wmain = call.d_wmain + static_cast<size_t>(b) * mi::kWaveBatch;
        db.iq_out = call.d_iq_out ? call.d_iq_out + static_cast<size_t>(b) * mi::kWaveBatch : nullptr;
        db.axc = call.d_axc + b;
        HIP_TRY(mi::launch_demod(db, s));
        mi::AfcArgs aa{};
        aa.nstreams = call.act_streams;
        aa.streams = ca.streams;
        aa.nch = h->nch;
        aa.fft_size = h->plan.fft_size;
        aa.cp = h->d_cp;
        aa.st = h->d_state;
        aa.spec = h->d_afc_spec;
        aa.axc = call.d_axc + b;
        aa.axc_stride = static_cast<uint32_t>(call.nbatches);
        HIP_TRY(mi::launch_afc(aa, s));
        f0 += nf;
    }
    return MI_OK;
}

// ---- serial stage 2 with consecutive calls overlapping (MI_OPT_EARLY_INPUT) ----
// Two plane sets alternate.  Stage 1 of this call fills the body of set p on the front stream while the previous
// call's k_demod, which reads the other set, still runs on the caller's stream (all that k_demod writes into set p
// is the carried head, entries [0, AGC_EXTRA), which stage 1 does not touch).  k_demod of this call waits for its
// stage 1 and leaves the head in the other set for the next call.
int enqueue_serial_pipelined(mi_demod* h, Call& call) {
    const hipStream_t s = call.s;
    mi::ChannelizeArgs& ca = call.ca;
    mi::DemodArgs& da = call.da;
    if (h->cls.tp_eligible)
        h->pset = h->d_mag == h->set[1].mag ? 1 : 0;
    const int q = (h->cur + 1) % mi_demod::kSets;  // event / timing set of this call
    const int before_prev = (h->cur + mi_demod::kSets - 1) % mi_demod::kSets;
    const int p = h->pset, np = p ^ 1;
    call.evc = h->set[q].ev;
    const mi::Event* const evc = call.evc;
    if (h->split_state == 0) {
        h->split_state = 2;
        hipDeviceProp_t prop{};
        // Two waves per row (k_demod_pw2) of 449 .. 512 rows fill 128 CUs two to a SIMD -- the kernel's pace alone -- and stage 1 of
        // that many streams takes as long on the other 128 as the kernel does: side by side on disjoint CUs 3.47 ms per 8-s call of
        // 64 x 8 AM channels, sharing every SIMD 3.8 (stage 1 3.4-3.5 ms beside the kernel's waves against 1.9 alone).  With fewer
        // rows the call is the kernel's latency either way and the split only takes CUs from stage 1 (tools/split_rows.sh); with
        // more the kernel needs more than 128 CUs (112 for 512 rows: 3.7 ms).
        const int want = h->opt.split_cus >= 0 ? h->opt.split_cus : ((da.pre_wave == 2 && h->rows > 448 && h->rows <= 512) ? 128 : 0);
        if (want > 0 && hipGetDeviceProperties(&prop, h->gpu) == hipSuccess && prop.multiProcessorCount >= want + 32) {
            const int ncu = prop.multiProcessorCount, keep = ncu - want;
            hipError_t me = cu_stream_create(h->ps_front_m, cu_mask(ncu, 0, keep));
            if (me == hipSuccess)
                me = cu_stream_create(h->ps_demod_m, cu_mask(ncu, keep, ncu));
            if (me == hipSuccess)
                me = hipEventCreateWithFlags(h->ev_ps_entry.put(), hipEventDisableTiming);
            if (me == hipSuccess)
                me = hipEventCreateWithFlags(h->ev_ps_done.put(), hipEventDisableTiming);
            if (me == hipSuccess)
                h->split_state = 1;
            else
                (void)hipGetLastError();
        }
    }
    const bool split = h->split_state == 1 && s != nullptr;
    hipStream_t fs = split ? h->ps_front_m : h->front_stream;
    if (call.iq_ready)
        HIP_TRY(hipStreamWaitEvent(fs, call.iq_ready, 0));
    if (h->serial_pipe && h->set[before_prev].seq)  // the call before the previous one read the body of set p
        HIP_TRY(hipStreamWaitEvent(fs, h->set[before_prev].ev[kEvDone], 0));
    else
        HIP_TRY(hipStreamWaitEvent(fs, h->set[h->cur].ev[kEvDone], 0));  // (first pipelined call: everything before it)
    ca.mag = h->set[p].mag;
    ca.cplx = h->d_cplx_set[p];
    HIP_TRY(hipEventRecord(evc[kEvBegin], fs));
    HIP_TRY(stage1_launch(h, ca, 0, fs));
    HIP_TRY(hipEventRecord(evc[kEvStage1Done], fs));
    da.mag = h->set[p].mag;
    da.cplx = h->d_cplx_set[p];
    da.mag_head = h->set[np].mag;
    da.cplx_head = h->d_cplx_set[np];
    if (split) {  // k_demod on the CUs stage 1 keeps off, in the caller's stream order all the same
        hipStream_t ds = h->ps_demod_m;
        HIP_TRY(hipEventRecord(h->ev_ps_entry, s));
        HIP_TRY(hipStreamWaitEvent(ds, h->ev_ps_entry, 0));
        HIP_TRY(hipStreamWaitEvent(ds, evc[kEvStage1Done], 0));
        HIP_TRY(hipEventRecord(evc[kEvSerialBegin], ds));
        HIP_TRY(mi::launch_demod(da, ds));
        HIP_TRY(hipEventRecord(h->ev_ps_done, ds));
        HIP_TRY(hipStreamWaitEvent(s, h->ev_ps_done, 0));
    } else {
        HIP_TRY(hipStreamWaitEvent(s, evc[kEvStage1Done], 0));
        HIP_TRY(hipEventRecord(evc[kEvSerialBegin], s));
        HIP_TRY(mi::launch_demod(da, s));
    }
    h->chain_live = false;
    h->cur = q;
    h->pset = np;
    h->d_mag = h->set[np].mag;
    h->d_cplx = h->d_cplx_set[np];
    h->d_mag_last = h->set[p].mag;
    h->d_cplx_last = h->d_cplx_set[p];
    h->serial_pipe = true;
    return MI_OK;
}

int enqueue_serial(mi_demod* h, const Call& call) {
    const hipStream_t s = call.s;
    if (call.iq_ready)
        HIP_TRY(hipStreamWaitEvent(s, call.iq_ready, 0));
    int rc = head_in_place(h, call);
    if (rc != MI_OK)
        return rc;
    h->chain_live = false;  // k_demod does not maintain the time-parallel chain state
    h->serial_pipe = false;
    HIP_TRY(hipEventRecord(call.evc[kEvBegin], s));
    HIP_TRY(stage1_launch(h, call.ca, 0, s));
    HIP_TRY(hipEventRecord(call.evc[kEvStage1Done], s));
    HIP_TRY(mi::launch_demod(call.da, s));
    return MI_OK;
}

// shared by both entry points; everything is enqueued on `s`
int enqueue(mi_demod* h, const unsigned char* d_iq, size_t stream_stride, size_t valid_bytes, int nbatches, float* d_wmain, size_t wmain_stride,
            float2* d_iq_out, size_t iq_out_stride, char* d_axc, hipStream_t s, hipEvent_t iq_ready = nullptr) {
    // iq_ready (host-buffer entry, calls in flight): the IQ becomes valid when this event fires -- the streams that read it wait
    // for it and for nothing else, exactly as if the caller had vouched for the bytes (MI_OPT_EARLY_INPUT)
    const bool early_input = h->opt.early_input || iq_ready != nullptr;
    // A masked call (mi_demod_set_active_streams): one stage-1 launch and the serial stage 2 over the active streams, enqueued as a
    // call without a predecessor (heads in place first, no overlap).  It leaves chain_live and serial_pipe clear, so the full
    // call after it takes nothing from the previous call's arrays (prev_mag, prev_blk_*, prev_core, spec_head, xmax_prev: they
    // would not hold every row) and seeds its chain from the ChanState rows.
    const bool partial = h->masked;
    if (partial && h->first_call)
        return fail(MI_ERR_INVALID, "the handle's first call needs every stream active");
    const int act_streams = partial ? h->nactive : h->nstreams;
    Call call{d_iq, stream_stride, valid_bytes, nbatches, d_wmain, wmain_stride, d_iq_out, iq_out_stride, d_axc, s, iq_ready,
              early_input, partial, act_streams, act_streams * h->nch, /*ca=*/{}, /*da=*/{},
              /*evc=*/h->set[h->cur].ev};  // (the time-parallel and the pipelined serial path switch to the next set)
    make_channelize_args(h, call);
    make_demod_args(h, call);
    const Path path = choose_path(h, call);
    int rc = MI_OK;
    switch (path) {
        case kPathTimeParallel:
            rc = enqueue_time_parallel(h, call);
            break;
        case kPathAfc:
            rc = enqueue_afc(h, call);
            break;
        case kPathSerialPipelined:
            rc = enqueue_serial_pipelined(h, call);
            break;
        case kPathSerial:
            rc = enqueue_serial(h, call);
            break;
    }
    if (rc != MI_OK)
        return rc;
    h->last_path = path == kPathTimeParallel ? kPathTimeParallel : kPathSerial;
    if (path != kPathTimeParallel)
        h->ser_head_next = false;
    HIP_TRY(hipEventRecord(call.evc[kEvDone], s));
    h->set[h->cur].seq = ++h->call_seq;
    h->set[h->cur].path = path == kPathSerialPipelined ? kPathSerialPipelined : h->last_path;  // (an AFC call is timed as a serial one)
    h->first_call = false;
    return MI_OK;
}

}  // namespace

extern "C" {

const char* mi_last_error(void) {
    return g_err.c_str();
}

int mi_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess)
        return 0;
    return n;
}

void mi_demod_destroy(mi_demod* h) {
    if (!h)
        return;
    (void)hipSetDevice(h->gpu);
    (void)hipDeviceSynchronize();  // calls may still be in flight on the handle's own streams
    delete h;
}

int mi_demod_create(const mi_device_cfg* dev, const mi_channel_cfg* chans, int nch, int nstreams, int max_batches, int gpu, mi_demod** out) {
    if (!out)
        return fail(MI_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!dev || !chans)
        return fail(MI_ERR_INVALID, "dev/chans is NULL");
    if (nstreams < 1 || max_batches < 1)
        return fail(MI_ERR_INVALID, "nstreams and max_batches must be >= 1");
    mi_demod* h = new (std::nothrow) mi_demod();
    if (!h)
        return fail(MI_ERR_NOMEM, "host allocation failed");
    mi::tuning_from_env(h->opt);
    const char* msg = "";
    int rc = mi::build_plan(*dev, chans, nch, h->plan, &msg);
    if (rc != MI_OK) {
        delete h;
        return fail(rc, msg);
    }
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev < 1) {
        delete h;
        return fail(MI_ERR_NO_DEVICE, "no HIP device: the MI355X path has no CPU fallback");
    }
    if (gpu < 0 || gpu >= ndev) {
        delete h;
        return fail(MI_ERR_INVALID, "gpu index out of range");
    }
    h->gpu = gpu;
    h->nstreams = nstreams;
    h->nch = nch;
    h->rows = nstreams * nch;
    h->max_batches = max_batches;
    h->active.assign(static_cast<size_t>(nstreams), 1);
    h->nactive = nstreams;
    const mi::Plan& p = h->plan;
    const size_t max_steps = static_cast<size_t>(max_batches) * mi::kWaveBatch;
    h->plane_stride = (max_steps + 2 * mi::kAgcExtra + 3) & ~static_cast<size_t>(3);

    auto bail = [&](int code) {
        std::string keep = g_err;
        mi_demod_destroy(h);
        g_err = keep;
        return code;
    };
#define TRY_OR_BAIL(expr)                          \
    do {                                           \
        hipError_t e__ = (expr);                   \
        if (e__ != hipSuccess)                     \
            return bail(hip_fail(e__, #expr));     \
    } while (0)

    TRY_OR_BAIL(hipSetDevice(gpu));
    TRY_OR_BAIL(hipStreamCreateWithFlags(h->own_stream.put(), hipStreamNonBlocking));
    for (mi_demod::CallSet& cs : h->set)
        for (mi::Event& ev : cs.ev)
            TRY_OR_BAIL(hipEventCreate(ev.put()));
    TRY_OR_BAIL(hipEventCreate(h->ev_entry.put()));
    TRY_OR_BAIL(hipEventCreate(h->ev_head.put()));
    TRY_OR_BAIL(priority_stream(h->aux_stream, /*highest=*/true));  // the core chain must never queue behind a wide pass
    TRY_OR_BAIL(hipStreamCreateWithFlags(h->front_stream.put(), hipStreamNonBlocking));
    for (mi::Stream& ss : h->seg_stream)
        TRY_OR_BAIL(hipStreamCreateWithFlags(ss.put(), hipStreamNonBlocking));
    // the plan's tables
    TRY_OR_BAIL(dalloc_copy(h->d_window, p.window));
    TRY_OR_BAIL(dalloc_copy(h->d_tw, p.tw));
    TRY_OR_BAIL(dalloc_copy(h->d_levels, p.levels));
    TRY_OR_BAIL(dalloc_copy(h->d_sin, p.sin_lut));
    TRY_OR_BAIL(dalloc_copy(h->d_cos, p.cos_lut));
    TRY_OR_BAIL(dalloc_copy(h->d_cp, p.cp));
    TRY_OR_BAIL(dalloc_copy(h->d_ctcss_coeff, p.ctcss_coeff));
    if (p.prune.enabled) {
        TRY_OR_BAIL(dalloc_copy(h->d_prune_t1, p.prune_t1));
        TRY_OR_BAIL(dalloc_copy(h->d_prune_t2, p.prune_t2));
        TRY_OR_BAIL(dalloc_copy(h->d_prune_rank, p.prune_chan_rank));
    }
    if (p.l64.enabled) {
        TRY_OR_BAIL(dalloc_copy(h->d_l64_chan, p.l64_chan));
        TRY_OR_BAIL(dalloc_copy(h->d_l64_chan_full, p.l64_chan_full));
        TRY_OR_BAIL(dalloc_zero(h->d_l64_tickets, mi::kL64Tickets));
    }
    // what the channels carry from call to call (zeroed here, or filled by launch_init_state below), and the first set's planes
    const size_t rows = static_cast<size_t>(h->rows);
    TRY_OR_BAIL(dalloc(h->d_state, rows));
    TRY_OR_BAIL(dalloc_zero(h->set[0].mag, rows * h->plane_stride));
    h->d_mag = h->set[0].mag;
    TRY_OR_BAIL(dalloc_zero(h->d_cplx_set[0], static_cast<size_t>(nstreams) * p.n_iq_rows * h->plane_stride));
    h->d_cplx = h->d_cplx_set[0];
    TRY_OR_BAIL(dalloc(h->set[0].carry, rows * mi::kAgcExtra));
    h->d_carry = h->set[0].carry;
    TRY_OR_BAIL(dalloc(h->d_ring, rows * mi::kSquelchRing));
    TRY_OR_BAIL(dalloc(h->d_ctcss_q, static_cast<size_t>(nstreams) * p.n_ctcss_rows * 4 * mi::kMaxTones));
    TRY_OR_BAIL(dalloc_zero(h->d_stats, rows));
    TRY_OR_BAIL(dalloc_zero(h->d_pre_timeouts, 1));
    TRY_OR_BAIL(dalloc(h->d_afc_spec, p.any_afc ? static_cast<size_t>(nstreams) * p.fft_size : 0));
    h->cls = mi::classify_rows(p, nstreams, nch);
    if (h->cls.tp_eligible) {
        h->tp_max_blk = max_steps / 16;
        // segment length of the time-parallel path: short segments where rows are few (the parallelism has to come from time),
        // long ones where they are many (each lane pays TP_W steps of warm-up whatever its segment's length)
        // (by row count: 2048 beyond 128 rows until the segment pass ran full waves: DESIGN 6)
        h->tp_L = h->opt.tp_L ? static_cast<uint32_t>(h->opt.tp_L) : (h->cls.tp_rows <= 32 ? 512u : 1024u);
        h->tp_max_seg = (max_steps + h->tp_L - 1) / h->tp_L;
        TRY_OR_BAIL(dalloc_copy(h->d_rows, h->cls.tp_list, rows));
        if (!h->cls.ser_list.empty()) {
            TRY_OR_BAIL(dalloc_copy(h->d_srows, h->cls.ser_list));
            // (on a stream of the default class the serial kernel, a millisecond and more, took turns with stage 1 of the next call)
            TRY_OR_BAIL(priority_stream(h->ser_stream, /*highest=*/false));
            for (mi::Event& e : h->ev_cplx_free)
                TRY_OR_BAIL(hipEventCreateWithFlags(e.put(), hipEventDisableTiming));
        }
        for (int q = 0; q < mi_demod::kSets; ++q)
            if (const int rc_set = alloc_call_set(h, q); rc_set != MI_OK)
                return bail(rc_set);
        TRY_OR_BAIL(dalloc(h->d_tstart, rows * h->tp_max_seg * 8));
        TRY_OR_BAIL(dalloc(h->d_need, rows * h->tp_max_seg));
        TRY_OR_BAIL(dalloc(h->d_redo, rows * h->tp_max_seg + 1));
        TRY_OR_BAIL(dalloc_zero(h->d_fin, rows));
        TRY_OR_BAIL(dalloc(h->d_core_carry, rows));
        TRY_OR_BAIL(dalloc(h->d_full0, rows));
        TRY_OR_BAIL(dalloc_zero(h->d_fullbound, rows));
        TRY_OR_BAIL(dalloc_zero(h->d_diag, rows * 8));
    }
    TRY_OR_BAIL(mi::launch_init_state(h->d_state, h->d_carry, h->d_ring, h->d_ctcss_q, h->d_cp, nstreams, nch, p.n_ctcss_rows, h->own_stream));
    TRY_OR_BAIL(hipStreamSynchronize(h->own_stream));
#undef TRY_OR_BAIL
    if (!p.any_afc)
        stage1_compile(h, false);  // (a failure leaves the exchange kernels: never an error)
    *out = h;
    return MI_OK;
}

int mi_demod_prepare(mi_demod* h, int host_slots) {
    if (!h)
        return fail(MI_ERR_INVALID, "NULL handle");
    if (host_slots < 0 || host_slots > mi_demod::kSlots)
        return fail(MI_ERR_INVALID, "host_slots out of range (0 .. 3)");
    HIP_TRY(hipSetDevice(h->gpu));
    stage1_compile(h, false);
    for (int k = 0; k < host_slots; ++k) {
        const int rc = slot_prepare(h, k);
        if (rc != MI_OK)
            return rc;
    }
    // The runtime gives a stream its hardware queue (and a copy engine its first transfer) when the stream is first used: a few
    // milliseconds each.  One small operation on every stream of the handle now, so that the first batch does not pay for them.
    mi::DevBuf<unsigned char> d_warm;
    HIP_TRY(dalloc(d_warm, 256));
    std::vector<hipStream_t> streams = {h->own_stream, h->aux_stream, h->front_stream, h->copy_stream, h->down_stream};
    for (hipStream_t ss : h->seg_stream)
        streams.push_back(ss);
    hipError_t e = hipSuccess;
    for (hipStream_t st : streams)
        if (st && e == hipSuccess)
            e = hipMemsetAsync(d_warm, 0, 256, st);
    if (e == hipSuccess && host_slots > 0 && h->copy_stream && h->down_stream) {
        e = hipMemcpyAsync(d_warm, h->slot[0].h_in, 64, hipMemcpyHostToDevice, h->copy_stream);
        if (e == hipSuccess)
            e = hipStreamSynchronize(h->copy_stream);
        if (e == hipSuccess)
            e = hipMemcpyAsync(h->slot[0].h_out, d_warm, 64, hipMemcpyDeviceToHost, h->down_stream);
    }
    for (hipStream_t st : streams)
        if (st && e == hipSuccess)
            e = hipStreamSynchronize(st);
    HIP_TRY(e);
    // ... and one rehearsal of the call itself (the first dispatch of a kernel on a queue sets up its scratch and kernel-argument
    // memory: 7 ms on the first batch otherwise).  The handle's state is saved before and restored after: a prepared handle is
    // bit for bit the handle mi_demod_create returned.
    std::vector<unsigned char> saved(mi_demod_state_size(h));
    int rc = mi_demod_get_state(h, saved.data(), saved.size());
    if (rc != MI_OK)
        return rc;
    struct AllActive {  // the rehearsals take every stream (a handle's first call must), whatever mask the caller has set
        mi_demod* h;
        bool masked;
        explicit AllActive(mi_demod* hh) : h(hh), masked(hh->masked) { h->masked = false; }
        ~AllActive() { h->masked = masked; }
    } all_active(h);
    std::vector<int> rehearsals = {1};
    if (h->cls.tp_eligible && h->opt.tp != 0 && h->max_batches >= kTpMinBatches)
        rehearsals.push_back(kTpMinBatches);
    for (const int nb : rehearsals) {
        const size_t need = mi_demod_bytes_needed(h, nb);
        const size_t stride = (need + 255) & ~static_cast<size_t>(255);
        const size_t nsteps = static_cast<size_t>(nb) * mi::kWaveBatch, rows = static_cast<size_t>(h->rows);
        mi::DevBuf<unsigned char> d_iq;
        mi::DevBuf<float> d_wo, d_iqo;
        mi::DevBuf<char> d_axc;
        e = dalloc(d_iq, stride * h->nstreams);
        if (e == hipSuccess)
            e = hipMemset(d_iq, 0x80, stride * h->nstreams);
        if (e == hipSuccess)
            e = dalloc(d_wo, rows * nsteps);
        if (e == hipSuccess)
            e = dalloc(d_iqo, rows * nsteps * 2);
        if (e == hipSuccess)
            e = dalloc(d_axc, rows * static_cast<size_t>(nb));
        if (e == hipSuccess) {
            rc = mi_demod_process_device(h, d_iq, stride, nb, d_wo, d_iqo, d_axc, h->own_stream);
            if (rc == MI_OK)
                e = hipDeviceSynchronize();
        }
        if (rc == MI_OK && e == hipSuccess)
            rc = mi_demod_set_state(h, saved.data(), saved.size());
        else if (rc == MI_OK)
            rc = fail(MI_ERR_HIP, hipGetErrorString(e));
        if (rc != MI_OK)
            return rc;
    }
    return MI_OK;
}

int mi_set_cache_dir(const char* dir) {
    mi::l64_jit_set_cache_dir(dir);
    return MI_OK;
}

int mi_jit_counts(int* compiled, int* from_cache) {
    mi::l64_jit_counts(compiled, from_cache);
    return MI_OK;
}

size_t mi_demod_hop_bytes(const mi_demod* h) {
    return h ? h->plan.hop_bytes : 0;
}

size_t mi_demod_bytes_needed(const mi_demod* h, int nbatches) {
    if (!h || nbatches < 1)
        return 0;
    const size_t nfft = static_cast<size_t>(n_fft_for(h, nbatches));
    return (nfft - 1) * h->plan.hop_bytes + 2 * static_cast<size_t>(h->plan.bytes_per_sample) * h->plan.fft_size;
}

size_t mi_demod_bytes_consumed(const mi_demod* h, int nbatches) {
    if (!h || nbatches < 1)
        return 0;
    return static_cast<size_t>(n_fft_for(h, nbatches)) * h->plan.hop_bytes;
}

int mi_demod_process_device(mi_demod* h, const void* d_iq, size_t stream_stride_bytes, int nbatches, float* d_waveout, float* d_iq_out,
                            char* d_axc, void* hip_stream) {
    if (!h || !d_iq || !d_waveout || !d_axc)
        return fail(MI_ERR_INVALID, "NULL argument");
    if (h->failed)
        return fail(MI_ERR_HIP, kFailedMsg);
    if (nbatches < 1 || nbatches > h->max_batches)
        return fail(MI_ERR_INVALID, "nbatches out of range for this handle");
    const size_t align = 2 * static_cast<size_t>(h->plan.bytes_per_sample);
    if (reinterpret_cast<uintptr_t>(d_iq) % align != 0 || stream_stride_bytes % align != 0)
        return fail(MI_ERR_INVALID, "IQ pointer and stride must be aligned to one complex sample");
    if (reinterpret_cast<uintptr_t>(d_waveout) % 16 != 0 || (d_iq_out && reinterpret_cast<uintptr_t>(d_iq_out) % 16 != 0))
        return fail(MI_ERR_INVALID, "d_waveout / d_iq_out must be 16-byte aligned (the kernels store four samples at a time)");
    const size_t need = mi_demod_bytes_needed(h, nbatches);
    if (h->nstreams > 1 && stream_stride_bytes < need)
        return fail(MI_ERR_INVALID, "stream stride shorter than the bytes one call reads");
    HIP_TRY(hipSetDevice(h->gpu));
    const size_t nsteps = static_cast<size_t>(nbatches) * mi::kWaveBatch;
    return enqueue(h, static_cast<const unsigned char*>(d_iq), stream_stride_bytes, need, nbatches, d_waveout, nsteps,
                   reinterpret_cast<float2*>(d_iq_out), nsteps, d_axc, static_cast<hipStream_t>(hip_stream));
}

namespace {

// Staging of slot k, allocated on first use and only committed when every piece exists (a failure leaves the slot unallocated
// and the handle usable: the next call tries again).
int slot_prepare(mi_demod* h, int k) {
    if (h->slots_ready[k])
        return MI_OK;
    mi_demod::Slot tmp;
    const size_t rows = static_cast<size_t>(h->rows);
    const size_t max_steps = static_cast<size_t>(h->max_batches) * mi::kWaveBatch;
    const size_t max_fft = max_steps + mi::kAgcExtra;
    const size_t stride = ((max_fft - 1) * h->plan.hop_bytes + 2 * static_cast<size_t>(h->plan.bytes_per_sample) * h->plan.fft_size + 255) & ~static_cast<size_t>(255);
    const size_t out_bytes = rows * (max_steps + mi::kAgcExtra) * 4 + rows * max_steps * 8 + rows * static_cast<size_t>(h->max_batches) + rows * sizeof(mi_channel_stats) + 64;
    hipError_t e = dalloc(tmp.d_iq, stride * h->nstreams);
    if (e == hipSuccess)
        e = dalloc(tmp.d_wout, rows * (max_steps + mi::kAgcExtra));
    if (e == hipSuccess)
        e = dalloc(tmp.d_iqout, rows * max_steps);
    if (e == hipSuccess)
        e = dalloc(tmp.d_axc, rows * static_cast<size_t>(h->max_batches));
    if (e == hipSuccess)
        e = dalloc(tmp.d_stats, rows);
    if (e == hipSuccess)
        e = hipHostMalloc(reinterpret_cast<void**>(tmp.h_in.put()), stride * h->nstreams, hipHostMallocDefault);
    if (e == hipSuccess)
        e = hipHostMalloc(reinterpret_cast<void**>(tmp.h_out.put()), out_bytes, hipHostMallocDefault);
    if (e == hipSuccess)
        e = hipEventCreateWithFlags(tmp.up_done.put(), hipEventDisableTiming);
    if (e == hipSuccess)
        e = hipEventCreateWithFlags(tmp.done.put(), hipEventDisableTiming);
    if (e == hipSuccess && !h->copy_stream)
        e = hipStreamCreateWithFlags(h->copy_stream.put(), hipStreamNonBlocking);
    if (e == hipSuccess && !h->down_stream)
        e = hipStreamCreateWithFlags(h->down_stream.put(), hipStreamNonBlocking);
    if (e != hipSuccess)
        return hip_fail(e, "staging for the host-buffer entry");  // (tmp releases what it got)
    h->iq_stride = stride;
    h->h_out_bytes = out_bytes;
    h->slot[k] = std::move(tmp);
    h->slots_ready[k] = true;
    return MI_OK;
}

// Is `p` host memory the GPU can read directly (hipHostMalloc / hipHostRegister / mi_host_alloc)?  Then the upload needs no
// staging copy: the copy engine reads the caller's ring itself.
bool is_pinned(const void* p) {
    hipPointerAttribute_t at{};
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return at.type == hipMemoryTypeHost;
}

// offsets of the pieces of a call's results inside a slot's pinned return buffer
struct OutLayout {
    size_t wave, iq, axc, stats;
};
OutLayout out_layout(const mi_demod* h, int nbatches) {
    const size_t rows = static_cast<size_t>(h->rows), n = static_cast<size_t>(nbatches) * mi::kWaveBatch;
    OutLayout o;
    o.wave = 0;
    o.iq = o.wave + rows * (n + mi::kAgcExtra) * 4;
    o.axc = o.iq + rows * n * 8;
    o.stats = (o.axc + rows * static_cast<size_t>(nbatches) + 15) & ~static_cast<size_t>(15);
    return o;
}

// upload + both stages + download of one call, all asynchronous; `pipelined`: upload and download on their own streams so
// that they overlap the compute of the neighbouring calls
int slot_launch(mi_demod* h, int k, const uint8_t* const* iq, int nbatches, bool want_iq, bool want_stats, bool pipelined) {
    mi_demod::Slot& sl = h->slot[k];
    const size_t rows = static_cast<size_t>(h->rows);
    const size_t nsteps = static_cast<size_t>(nbatches) * mi::kWaveBatch;
    const size_t need = mi_demod_bytes_needed(h, nbatches);
    hipStream_t s = h->own_stream;
    hipStream_t up = pipelined ? h->copy_stream : s;
    if (h->masked && h->first_call)  // (before anything is staged)
        return fail(MI_ERR_INVALID, "the handle's first call needs every stream active");
    sl.masked = h->masked;
    for (int i = 0; i < h->nstreams; ++i) {
        if (sl.masked && !h->active[static_cast<size_t>(i)])
            continue;  // a stream that sits this call out: its pointer is not looked at, nothing is staged or uploaded
        if (!iq[i])
            return fail(MI_ERR_INVALID, "NULL stream pointer");
        const unsigned char* src = iq[i];
        if (!is_pinned(src)) {
            std::memcpy(sl.h_in + static_cast<size_t>(i) * h->iq_stride, src, need);
            src = sl.h_in + static_cast<size_t>(i) * h->iq_stride;
        }
        HIP_TRY(hipMemcpyAsync(sl.d_iq + static_cast<size_t>(i) * h->iq_stride, src, need, hipMemcpyHostToDevice, up));
    }
    hipEvent_t ready = nullptr;
    if (pipelined) {
        HIP_TRY(hipEventRecord(sl.up_done, up));
        ready = sl.up_done;
    }
    // mi_demod_process: the staging copy is ordered by the stream, MI_OPT_EARLY_INPUT (valid when the call is made) does not hold.
    // mi_demod_submit: the upload has its own stream and event, which is all the front of the call waits for -- so consecutive
    // submitted calls overlap on the device like device-resident calls with the option set (their audio goes to the two
    // slots' buffers in turn, which is what lets the segment passes of one run under the tail of the other).
    const bool early = h->opt.early_input;
    h->opt.early_input = pipelined;
    const size_t wstride = nsteps + mi::kAgcExtra;  // the host layout: emitted audio followed by the lookahead (channel_t.waveout)
    int rc = enqueue(h, sl.d_iq, h->iq_stride, need, nbatches, sl.d_wout, wstride, want_iq ? sl.d_iqout : nullptr, nsteps, sl.d_axc, s, ready);
    h->opt.early_input = early;
    if (rc != MI_OK)
        return rc;
    // the lookahead and the statistics belong to the handle and move on with the next call: snapshot them behind this one
    HIP_TRY_F(hipMemcpy2DAsync(sl.d_wout + nsteps, wstride * sizeof(float), h->d_carry, mi::kAgcExtra * sizeof(float), mi::kAgcExtra * sizeof(float), rows,
                             hipMemcpyDeviceToDevice, s));
    if (want_stats)
        HIP_TRY_F(hipMemcpyAsync(sl.d_stats, h->d_stats, rows * sizeof(mi_channel_stats), hipMemcpyDeviceToDevice, s));
    hipStream_t down = s;
    if (pipelined) {
        HIP_TRY_F(hipEventRecord(sl.done, s));
        HIP_TRY_F(hipStreamWaitEvent(h->down_stream, sl.done, 0));
        down = h->down_stream;
    }
    const OutLayout o = out_layout(h, nbatches);
    sl.wave_direct = !sl.masked && is_pinned(sl.waveout);  // (a masked call hands over the active streams' regions only: slot_collect)
    HIP_TRY_F(hipMemcpyAsync(sl.wave_direct ? reinterpret_cast<unsigned char*>(sl.waveout) : sl.h_out + o.wave, sl.d_wout, rows * wstride * sizeof(float),
                           hipMemcpyDeviceToHost, down));
    if (want_iq) {
        for (size_t r = 0; r < rows; ++r) {
            if (!h->plan.cp[r % h->nch].has_iq_outputs || (sl.masked && !h->active[r / static_cast<size_t>(h->nch)]))
                continue;
            HIP_TRY_F(hipMemcpyAsync(sl.h_out + o.iq + r * nsteps * 8, sl.d_iqout + r * nsteps, nsteps * sizeof(float2), hipMemcpyDeviceToHost, down));
        }
    }
    HIP_TRY_F(hipMemcpyAsync(sl.h_out + o.axc, sl.d_axc, rows * static_cast<size_t>(nbatches), hipMemcpyDeviceToHost, down));
    if (want_stats)
        HIP_TRY_F(hipMemcpyAsync(sl.h_out + o.stats, sl.d_stats, rows * sizeof(mi_channel_stats), hipMemcpyDeviceToHost, down));
    HIP_TRY_F(hipEventRecord(sl.done, down));
    return MI_OK;
}

// wait for slot k's call and hand its results to the caller's arrays
int slot_collect(mi_demod* h, int k) {
    mi_demod::Slot& sl = h->slot[k];
    HIP_TRY(hipEventSynchronize(sl.done));
    const size_t nsteps = static_cast<size_t>(sl.nbatches) * mi::kWaveBatch;
    const OutLayout o = out_layout(h, sl.nbatches);
    const size_t nch = static_cast<size_t>(h->nch), wlen = nsteps + mi::kAgcExtra, nb = static_cast<size_t>(sl.nbatches);
    // the regions of streams [s0, s0 + n) of the caller's arrays
    auto hand_over = [&](size_t s0, size_t n) {
        const size_t r0 = s0 * nch, nr = n * nch;
        if (!sl.wave_direct)
            std::memcpy(sl.waveout + r0 * wlen, sl.h_out + o.wave + r0 * wlen * sizeof(float), nr * wlen * sizeof(float));
        for (size_t r = r0; sl.iq_out && r < r0 + nr; ++r)
            if (h->plan.cp[r % nch].has_iq_outputs)  // rows of channels without iq outputs are untouched
                std::memcpy(sl.iq_out + r * nsteps * 2, sl.h_out + o.iq + r * nsteps * 8, nsteps * 8);
        std::memcpy(sl.axc + r0 * nb, sl.h_out + o.axc + r0 * nb, nr * nb);
        if (sl.stats)
            std::memcpy(sl.stats + r0, sl.h_out + o.stats + r0 * sizeof(mi_channel_stats), nr * sizeof(mi_channel_stats));
    };
    if (!sl.masked) {
        hand_over(0, static_cast<size_t>(h->nstreams));
    } else {  // (the mask cannot have changed since the call was made: setting one completes what is in flight)
        for (size_t st = 0; st < static_cast<size_t>(h->nstreams); ++st)
            if (h->active[st])
                hand_over(st, 1);
    }
    sl.busy = false;
    return MI_OK;
}

int check_host_call(mi_demod* h, const uint8_t* const* iq, int nbatches, float* waveout, char* axc) {
    if (!h || !iq || !waveout || !axc)
        return fail(MI_ERR_INVALID, "NULL argument");
    if (h->failed)
        return fail(MI_ERR_HIP, kFailedMsg);
    if (nbatches < 1 || nbatches > h->max_batches)
        return fail(MI_ERR_INVALID, "nbatches out of range for this handle");
    return MI_OK;
}

}  // namespace

void* mi_host_alloc(size_t bytes) {
    void* p = nullptr;
    if (bytes == 0 || hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    return p;
}

void mi_host_free(void* p) {
    if (p)
        (void)hipHostFree(p);
}

int mi_demod_wait(mi_demod* h) {
    if (!h)
        return fail(MI_ERR_INVALID, "NULL handle");
    if (h->in_flight == 0)
        return fail(MI_ERR_INVALID, "no submitted call is in flight");
    HIP_TRY(hipSetDevice(h->gpu));
    const int k = h->slot_oldest;
    int rc = slot_collect(h, k);
    h->slot_oldest = (h->slot_oldest + 1) % mi_demod::kSlots;
    h->in_flight--;
    return rc;
}

int mi_demod_submit(mi_demod* h, const uint8_t* const* iq, int nbatches, float* waveout, float* iq_out, char* axc, mi_channel_stats* stats) {
    int rc = check_host_call(h, iq, nbatches, waveout, axc);
    if (rc != MI_OK)
        return rc;
    HIP_TRY(hipSetDevice(h->gpu));
    if (h->in_flight == mi_demod::kSlots) {  // every slot taken: the oldest call completes first (its outputs become valid here)
        rc = mi_demod_wait(h);
        if (rc != MI_OK)
            return rc;
    }
    const int k = h->slot_next;
    rc = slot_prepare(h, k);
    if (rc != MI_OK)
        return rc;
    mi_demod::Slot& sl = h->slot[k];
    sl.nbatches = nbatches;
    sl.waveout = waveout, sl.iq_out = iq_out, sl.axc = axc, sl.stats = stats;
    rc = slot_launch(h, k, iq, nbatches, iq_out != nullptr, stats != nullptr, /*pipelined=*/true);
    if (rc != MI_OK)
        return rc;
    sl.busy = true;
    if (h->in_flight == 0)
        h->slot_oldest = k;
    h->slot_next = (k + 1) % mi_demod::kSlots;
    h->in_flight++;
    return MI_OK;
}

int mi_demod_process(mi_demod* h, const uint8_t* const* iq, int nbatches, float* waveout, float* iq_out, char* axc, mi_channel_stats* stats) {
    int rc = check_host_call(h, iq, nbatches, waveout, axc);
    if (rc != MI_OK)
        return rc;
    HIP_TRY(hipSetDevice(h->gpu));
    while (h->in_flight > 0) {  // calls complete in order
        rc = mi_demod_wait(h);
        if (rc != MI_OK)
            return rc;
    }
    rc = slot_prepare(h, 0);
    if (rc != MI_OK)
        return rc;
    mi_demod::Slot& sl = h->slot[0];
    sl.nbatches = nbatches;
    sl.waveout = waveout, sl.iq_out = iq_out, sl.axc = axc, sl.stats = stats;
    // one call at a time: everything in order on the handle's own stream (the shortest path for the reference's cadence of one
    // WAVE_BATCH per call)
    rc = slot_launch(h, 0, iq, nbatches, iq_out != nullptr, stats != nullptr, /*pipelined=*/false);
    if (rc != MI_OK)
        return rc;
    return slot_collect(h, 0);
}

int mi_demod_process_planes(mi_demod* h, const float* mag, const float* cplx, int nbatches, float* waveout, float* iq_out, char* axc, mi_channel_stats* stats) {
    if (!h || !mag || !waveout || !axc)
        return fail(MI_ERR_INVALID, "NULL argument");
    if (nbatches < 1 || nbatches > h->max_batches)
        return fail(MI_ERR_INVALID, "nbatches out of range for this handle");
    if (h->plan.any_afc)
        return fail(MI_ERR_UNSUPPORTED, "AFC channels read the spectrum of stage 1: no plane entry for them");
    if (h->in_flight)
        return fail(MI_ERR_INVALID, "submitted calls are in flight");
    if (h->masked)
        return fail(MI_ERR_UNSUPPORTED, "the plane entry takes every stream: not while mi_demod_set_active_streams has set some aside");
    const size_t zrows = static_cast<size_t>(h->nstreams) * h->plan.n_iq_rows;
    if (zrows && !cplx)
        return fail(MI_ERR_INVALID, "this plan has raw-I/Q rows: cplx planes are needed");
    HIP_TRY(hipSetDevice(h->gpu));
    const size_t rows = static_cast<size_t>(h->rows), count = static_cast<size_t>(n_fft_for(h, nbatches));
    const size_t nsteps = static_cast<size_t>(nbatches) * mi::kWaveBatch, wlen = nsteps + mi::kAgcExtra;
    mi::DevBuf<float> d_m, d_wo;
    mi::DevBuf<float2> d_z, d_io;
    mi::DevBuf<char> d_ax;
    hipError_t e = dalloc(d_m, rows * count);
    if (e == hipSuccess && zrows)
        e = dalloc(d_z, zrows * count);
    if (e == hipSuccess)
        e = dalloc(d_wo, rows * wlen);
    if (e == hipSuccess && iq_out)
        e = dalloc(d_io, rows * nsteps);
    if (e == hipSuccess)
        e = dalloc(d_ax, rows * static_cast<size_t>(nbatches));
    if (e == hipSuccess)
        e = hipMemcpy(d_m, mag, rows * count * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess && zrows)
        e = hipMemcpy(d_z, cplx, zrows * count * 8, hipMemcpyHostToDevice);
    int rc = MI_OK;
    if (e == hipSuccess) {
        h->inject_mag = d_m, h->inject_cplx = d_z, h->inject_count = count;
        // (the IQ pointer is never read: stage 1 is the copy above; the audio goes to [row][wlen] like the host entry's)
        rc = enqueue(h, reinterpret_cast<const unsigned char*>(d_m.get()), 0, 0, nbatches, d_wo, wlen, d_io, nsteps, d_ax, h->own_stream);
        h->inject_mag = nullptr, h->inject_cplx = nullptr, h->inject_count = 0;
        if (rc == MI_OK)
            e = hipDeviceSynchronize();
    }
    if (rc == MI_OK && e == hipSuccess)
        e = hipMemcpy2D(waveout, wlen * 4, d_wo, wlen * 4, nsteps * 4, rows, hipMemcpyDeviceToHost);
    if (rc == MI_OK && e == hipSuccess)  // the lookahead: what the handle carries to the next call
        e = hipMemcpy2D(waveout + nsteps, wlen * 4, h->d_carry, mi::kAgcExtra * 4, mi::kAgcExtra * 4, rows, hipMemcpyDeviceToHost);
    if (rc == MI_OK && e == hipSuccess && iq_out)
        e = hipMemcpy(iq_out, d_io, rows * nsteps * 8, hipMemcpyDeviceToHost);
    if (rc == MI_OK && e == hipSuccess)
        e = hipMemcpy(axc, d_ax, rows * static_cast<size_t>(nbatches), hipMemcpyDeviceToHost);
    if (rc == MI_OK && e == hipSuccess && stats)
        e = hipMemcpy(stats, h->d_stats, rows * sizeof(mi_channel_stats), hipMemcpyDeviceToHost);
    if (rc != MI_OK)
        return rc;
    HIP_TRY(e);
    return MI_OK;
}

int mi_demod_get_stats(mi_demod* h, mi_channel_stats* stats) {
    if (!h || !stats)
        return fail(MI_ERR_INVALID, "NULL argument");
    HIP_TRY(hipSetDevice(h->gpu));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(stats, h->d_stats, static_cast<size_t>(h->rows) * sizeof(mi_channel_stats), hipMemcpyDeviceToHost));
    return MI_OK;
}

// ---- checkpoint: [header][ChanState rows][carry][ring][ctcss_q][mag head][cplx head] ----
namespace {
struct StateHeader {
    uint32_t magic, rows, nch, n_iq_rows, n_ctcss_rows, first_call, fft_log, pad;
};
size_t state_bytes(const mi_demod* h) {
    const size_t rows = static_cast<size_t>(h->rows);
    return sizeof(StateHeader) + rows * sizeof(mi::ChanState) + rows * mi::kAgcExtra * 4 + rows * mi::kSquelchRing * 4 +
           static_cast<size_t>(h->nstreams) * h->plan.n_ctcss_rows * 4 * mi::kMaxTones * 4 + rows * mi::kAgcExtra * 4 +
           static_cast<size_t>(h->nstreams) * h->plan.n_iq_rows * mi::kAgcExtra * 8;
}
}  // namespace

size_t mi_demod_state_size(const mi_demod* h) {
    return h ? state_bytes(h) : 0;
}

int mi_demod_get_state(mi_demod* h, void* buf, size_t len) {
    if (!h || !buf || len < state_bytes(h))
        return fail(MI_ERR_INVALID, "state buffer too small");
    HIP_TRY(hipSetDevice(h->gpu));
    HIP_TRY(hipDeviceSynchronize());
    auto* o = static_cast<unsigned char*>(buf);
    StateHeader hd{0x4d494142u, static_cast<uint32_t>(h->rows), static_cast<uint32_t>(h->nch), static_cast<uint32_t>(h->plan.n_iq_rows),
                   static_cast<uint32_t>(h->plan.n_ctcss_rows), h->first_call ? 1u : 0u, static_cast<uint32_t>(h->plan.log2n), 0};
    std::memcpy(o, &hd, sizeof(hd));
    o += sizeof(hd);
    const size_t rows = static_cast<size_t>(h->rows);
    auto pull = [&](const void* d, size_t bytes) -> hipError_t {
        if (bytes == 0)
            return hipSuccess;
        hipError_t e = hipMemcpy(o, d, bytes, hipMemcpyDeviceToHost);
        o += bytes;
        return e;
    };
    HIP_TRY(pull(h->d_state, rows * sizeof(mi::ChanState)));
    HIP_TRY(pull(h->d_carry, rows * mi::kAgcExtra * 4));
    HIP_TRY(pull(h->d_ring, rows * mi::kSquelchRing * 4));
    HIP_TRY(pull(h->d_ctcss_q, static_cast<size_t>(h->nstreams) * h->plan.n_ctcss_rows * 4 * mi::kMaxTones * 4));
    HIP_TRY(hipMemcpy2D(o, mi::kAgcExtra * 4, h->d_mag + h->head_off, h->plane_stride * 4, mi::kAgcExtra * 4, rows, hipMemcpyDeviceToHost));
    o += rows * mi::kAgcExtra * 4;
    const size_t zrows = static_cast<size_t>(h->nstreams) * h->plan.n_iq_rows;
    if (zrows)
        HIP_TRY(hipMemcpy2D(o, mi::kAgcExtra * 8, h->d_cplx, h->plane_stride * 8, mi::kAgcExtra * 8, zrows, hipMemcpyDeviceToHost));
    return MI_OK;
}

int mi_demod_set_state(mi_demod* h, const void* buf, size_t len) {
    if (!h || !buf || len < state_bytes(h))
        return fail(MI_ERR_INVALID, "state buffer too small");
    const auto* o = static_cast<const unsigned char*>(buf);
    StateHeader hd;
    std::memcpy(&hd, o, sizeof(hd));
    if (hd.magic != 0x4d494142u || hd.rows != static_cast<uint32_t>(h->rows) || hd.nch != static_cast<uint32_t>(h->nch) ||
        hd.n_iq_rows != static_cast<uint32_t>(h->plan.n_iq_rows) || hd.n_ctcss_rows != static_cast<uint32_t>(h->plan.n_ctcss_rows) ||
        hd.fft_log != static_cast<uint32_t>(h->plan.log2n))
        return fail(MI_ERR_INVALID, "state blob does not match this handle's configuration");
    o += sizeof(hd);
    HIP_TRY(hipSetDevice(h->gpu));
    HIP_TRY(hipDeviceSynchronize());
    const size_t rows = static_cast<size_t>(h->rows);
    auto push = [&](void* d, size_t bytes) -> hipError_t {
        if (bytes == 0)
            return hipSuccess;
        hipError_t e = hipMemcpy(d, o, bytes, hipMemcpyHostToDevice);
        o += bytes;
        return e;
    };
    HIP_TRY(push(h->d_state, rows * sizeof(mi::ChanState)));
    HIP_TRY(push(h->d_carry, rows * mi::kAgcExtra * 4));
    HIP_TRY(push(h->d_ring, rows * mi::kSquelchRing * 4));
    HIP_TRY(push(h->d_ctcss_q, static_cast<size_t>(h->nstreams) * h->plan.n_ctcss_rows * 4 * mi::kMaxTones * 4));
    HIP_TRY(hipMemcpy2D(h->d_mag, h->plane_stride * 4, o, mi::kAgcExtra * 4, mi::kAgcExtra * 4, rows, hipMemcpyHostToDevice));
    h->head_off = 0;
    h->ser_head_next = false;
    h->chain_live = false;  // the chain state of the time-parallel path is re-seeded from the restored ChanState
    o += rows * mi::kAgcExtra * 4;
    const size_t zrows = static_cast<size_t>(h->nstreams) * h->plan.n_iq_rows;
    if (zrows)
        HIP_TRY(hipMemcpy2D(h->d_cplx, h->plane_stride * 8, o, mi::kAgcExtra * 8, mi::kAgcExtra * 8, zrows, hipMemcpyHostToDevice));
    h->first_call = hd.first_call != 0;
    h->failed = false;
    return MI_OK;
}

int mi_demod_set_active_streams(mi_demod* h, const uint8_t* active) {
    if (!h)
        return fail(MI_ERR_INVALID, "NULL handle");
    const size_t ns = static_cast<size_t>(h->nstreams), nch = static_cast<size_t>(h->nch);
    std::vector<uint8_t> want(ns, 1);
    std::vector<int> streams, rows;
    for (size_t s = 0; s < ns; ++s) {
        want[s] = (!active || active[s]) ? 1 : 0;
        if (!want[s])
            continue;
        streams.push_back(static_cast<int>(s));
        for (size_t c = 0; c < nch; ++c)
            rows.push_back(static_cast<int>(s * nch + c));
    }
    if (streams.empty())
        return fail(MI_ERR_INVALID, "no active stream");
    HIP_TRY(hipSetDevice(h->gpu));
    while (h->in_flight > 0) {  // submitted calls were made under the mask they saw
        const int rc = mi_demod_wait(h);
        if (rc != MI_OK)
            return rc;
    }
    if (want == h->active)
        return MI_OK;
    if (streams.size() < ns) {
        // (the lists of the previous mask may still be read by a device-entry call on the caller's stream)
        HIP_TRY(hipDeviceSynchronize());
        if (!h->d_act_streams) {
            mi::DevBuf<int> ds, dr;
            HIP_TRY(dalloc(ds, ns));
            HIP_TRY(dalloc(dr, ns * nch));
            h->d_act_streams = std::move(ds);
            h->d_act_rows = std::move(dr);
        }
        HIP_TRY(hipMemcpy(h->d_act_streams, streams.data(), streams.size() * sizeof(int), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(h->d_act_rows, rows.data(), rows.size() * sizeof(int), hipMemcpyHostToDevice));
        stage1_compile(h, true);  // (a failure leaves the exchange kernels: never an error)
    }
    h->active = want;
    h->nactive = static_cast<int>(streams.size());
    h->masked = streams.size() < ns;
    return MI_OK;
}

int mi_demod_get_active_streams(const mi_demod* h, uint8_t* active) {
    if (!h || !active)
        return fail(MI_ERR_INVALID, "NULL argument");
    std::memcpy(active, h->active.data(), h->active.size());
    return MI_OK;
}

int mi_demod_last_path(mi_demod* h, int* time_parallel, int* unverified_rows) {
    if (!h)
        return fail(MI_ERR_INVALID, "NULL argument");
    HIP_TRY(hipSetDevice(h->gpu));
    HIP_TRY(hipDeviceSynchronize());
    if (time_parallel)
        *time_parallel = h->last_path;
    if (unverified_rows) {
        *unverified_rows = 0;
        if (h->last_path == kPathTimeParallel) {
            std::vector<mi::TpFinal> f(static_cast<size_t>(h->cls.tp_rows));
            HIP_TRY(hipMemcpy(f.data(), h->d_fin, f.size() * sizeof(mi::TpFinal), hipMemcpyDeviceToHost));
            for (const mi::TpFinal& x : f)
                *unverified_rows += x.all_ok ? 0 : 1;
        }
    }
    return MI_OK;
}

int mi_demod_pre_wave_timeouts(mi_demod* h, unsigned* count) {
    if (!h || !count)
        return fail(MI_ERR_INVALID, "NULL argument");
    HIP_TRY(hipSetDevice(h->gpu));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(count, h->d_pre_timeouts, sizeof(unsigned), hipMemcpyDeviceToHost));
    return MI_OK;
}

int mi_demod_last_stage1(mi_demod* h, int* kind) {
    if (!h || !kind)
        return fail(MI_ERR_INVALID, "NULL argument");
    *kind = h->last_stage1;
    return MI_OK;
}

int mi_demod_tp_debug(mi_demod* h, int row, float* core4, int max_entries, int* diag4, int* nseg) {
    if (!h || row < 0 || row >= h->cls.tp_rows || !h->cls.tp_eligible || h->last_path != kPathTimeParallel)
        return fail(MI_ERR_INVALID, "the last call did not take the time-parallel path");
    HIP_TRY(hipSetDevice(h->gpu));
    HIP_TRY(hipDeviceSynchronize());
    if (nseg)
        *nseg = static_cast<int>(h->set[h->cur].nseg);
    if (core4) {
        const size_t n = std::min<size_t>(static_cast<size_t>(max_entries), h->set[h->cur].nseg + 1);
        HIP_TRY(hipMemcpy(core4, h->set[h->cur].core + static_cast<size_t>(row) * (h->set[h->cur].nseg + 1), n * sizeof(mi::TpCore), hipMemcpyDeviceToHost));
    }
    if (diag4) {  // [0..3] scan rounds, [4..7] core-chain blocks: in accepted runs, single O(1), stepped, failed hypotheses
        HIP_TRY(hipMemcpy(diag4, h->d_diag + static_cast<size_t>(row) * 4, 4 * sizeof(int), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(diag4 + 4, h->d_diag + static_cast<size_t>(h->cls.tp_rows) * 4 + static_cast<size_t>(row) * 4, 4 * sizeof(int), hipMemcpyDeviceToHost));
    }
    return MI_OK;
}

int mi_demod_read_planes(mi_demod* h, int stream, int ch, int first, int count, float* mag, float* iq) {
    if (!h || !mag || stream < 0 || stream >= h->nstreams || ch < 0 || ch >= h->nch || first < 0 || count < 0 ||
        static_cast<size_t>(first) + count > h->plane_stride)
        return fail(MI_ERR_INVALID, "bad plane range");
    HIP_TRY(hipSetDevice(h->gpu));
    HIP_TRY(hipDeviceSynchronize());
    const size_t row = static_cast<size_t>(stream) * h->nch + ch;
    const float* pm = h->serial_pipe ? h->d_mag_last : h->d_mag;  // (a pipelined serial call leaves d_mag on the set with the next head)
    const float2* pz = h->serial_pipe ? h->d_cplx_last : h->d_cplx;
    HIP_TRY(hipMemcpy(mag, pm + row * h->plane_stride + first, static_cast<size_t>(count) * 4, hipMemcpyDeviceToHost));
    const int iq_row = h->plan.cp[ch].iq_row;
    if (iq && iq_row >= 0) {
        const size_t zrow = static_cast<size_t>(stream) * h->plan.n_iq_rows + iq_row;
        HIP_TRY(hipMemcpy(iq, pz + zrow * h->plane_stride + first, static_cast<size_t>(count) * 8, hipMemcpyDeviceToHost));
    }
    return MI_OK;
}

// timing of the last call (age 0) or of the call before it (age 1, only while its event set has not been reused)
static int kernel_time_of(mi_demod* h, int age, int index, const char** name, float* ms_total, int* launches) {
    if (!h || index < 0 || age < 0 || age >= mi_demod::kSets)
        return fail(MI_ERR_INVALID, "bad argument");
    const int q = (h->cur + mi_demod::kSets - age) % mi_demod::kSets;
    if (!h->set[q].seq || h->set[q].seq + static_cast<uint64_t>(age) != h->set[h->cur].seq)
        return fail(MI_ERR_INVALID, "that call has not been timed (or its events were reused)");
    HIP_TRY(hipSetDevice(h->gpu));
    const mi::Event* evq = h->set[q].ev;
    HIP_TRY(hipEventSynchronize(evq[kEvDone]));
    float t = 0.f;
    int n = 1;
    const char* nm = nullptr;
    if (h->set[q].path != kPathTimeParallel) {
        if (index > 1)
            return fail(MI_ERR_INVALID, "kernel index out of range");
        nm = index == 0 ? "k_channelize" : "k_demod";
        if (index == 0)
            HIP_TRY(hipEventElapsedTime(&t, evq[kEvBegin], evq[kEvStage1Done]));
        else  // (a pipelined serial call: k_demod starts at its own event on the caller's stream)
            HIP_TRY(hipEventElapsedTime(&t, evq[h->set[q].path == kPathSerialPipelined ? kEvSerialBegin : kEvStage1Done], evq[kEvDone]));
    } else {
        static const struct {
            const char* name;
            ChunkEv from, to;
        } timed[] = {{"k_channelize", kEvStage1Begin, kEvStage1End}, {"k_tp_full", kEvFullBegin, kEvFullEnd},  {"k_tp_core", kEvCoreBegin, kEvCoreEnd},
                     {"k_tp_seg", kEvSegBegin, kEvSegEnd},           {"k_tp_scan#0", kEvScanBegin, kEvScanEnd}, {"k_tp_fix#0", kEvScanEnd, kEvFixEnd},
                     {"k_tp_rest", kEvFixEnd, kEvFinishEnd}};
        if (index == 7 && h->set[q].mixed) {  // a mixed plan: the serial kernel of the other rows, on its own stream
            HIP_TRY(hipEventElapsedTime(&t, evq[kEvSerialBegin], evq[kEvSerialEnd]));
            if (name)
                *name = "k_demod";
            if (ms_total)
                *ms_total = t;
            if (launches)
                *launches = 1;
            return MI_OK;
        }
        if (index > 6)
            return fail(MI_ERR_INVALID, "kernel index out of range");
        nm = timed[index].name;
        n = h->set[q].chunks;
        for (int i = 0; i < n; ++i) {
            float d = 0.f;
            HIP_TRY(hipEventElapsedTime(&d, h->set[q].chunk(i, timed[index].from), h->set[q].chunk(i, timed[index].to)));
            t += d;
        }
    }
    if (name)
        *name = nm;
    if (ms_total)
        *ms_total = t;
    if (launches)
        *launches = n;
    return MI_OK;
}

int mi_demod_kernel_time(mi_demod* h, int index, const char** name, float* ms_total, int* launches) {
    return kernel_time_of(h, 0, index, name, ms_total, launches);
}

int mi_demod_kernel_time_prev(mi_demod* h, int age, int index, const char** name, float* ms_total, int* launches) {
    return kernel_time_of(h, age, index, name, ms_total, launches);
}

int mi_demod_event_ms(mi_demod* h, int ref_age, int age, int chunk, int event, float* ms) {
    if (!h || !ms || age < 0 || ref_age < age || ref_age >= mi_demod::kSets || event < 0 || event >= kEvPerChunk || chunk < 0)
        return fail(MI_ERR_INVALID, "bad argument");
    const int q = (h->cur + mi_demod::kSets - age) % mi_demod::kSets, qr = (h->cur + mi_demod::kSets - ref_age) % mi_demod::kSets;
    for (const int s : {q, qr})
        if (!h->set[s].seq || h->set[s].path != kPathTimeParallel)
            return fail(MI_ERR_INVALID, "that call was not a time-parallel one (or its events were reused)");
    if (h->set[q].seq + static_cast<uint64_t>(age) != h->set[h->cur].seq || h->set[qr].seq + static_cast<uint64_t>(ref_age) != h->set[h->cur].seq ||
        chunk >= h->set[q].chunks)
        return fail(MI_ERR_INVALID, "no such call or chunk");
    HIP_TRY(hipSetDevice(h->gpu));
    HIP_TRY(hipEventSynchronize(h->set[q].ev[kEvDone]));
    HIP_TRY(hipEventElapsedTime(ms, h->set[qr].chunk(0, kEvCoreBegin), h->set[q].chunk(chunk, static_cast<ChunkEv>(event))));
    return MI_OK;
}

int mi_demod_last_kernel_ms(mi_demod* h, float* channelize_ms, float* demod_ms) {
    if (!h || !h->set[h->cur].seq)
        return fail(MI_ERR_INVALID, "no call has been timed yet");
    HIP_TRY(hipSetDevice(h->gpu));
    const mi::Event* evq = h->set[h->cur].ev;
    HIP_TRY(hipEventSynchronize(evq[kEvDone]));
    float a = 0.f, b = 0.f;
    if (h->last_path == kPathSerial) {
        HIP_TRY(hipEventElapsedTime(&a, evq[kEvBegin], evq[kEvStage1Done]));
        HIP_TRY(hipEventElapsedTime(&b, evq[h->serial_pipe ? kEvSerialBegin : kEvStage1Done], evq[kEvDone]));
    } else {  // pipelined: stage 1 summed over the chunks, stage 2 = the rest of the call's wall time on the stream
        float total = 0.f;
        HIP_TRY(hipEventElapsedTime(&total, evq[kEvBegin], evq[kEvDone]));
        int rc = mi_demod_kernel_time(h, 0, nullptr, &a, nullptr);
        if (rc != MI_OK)
            return rc;
        b = total - a;
    }
    if (channelize_ms)
        *channelize_ms = a;
    if (demod_ms)
        *demod_ms = b;
    return MI_OK;
}

int mi_demod_set_option(mi_demod* h, int option, int value) {
    if (!h)
        return fail(MI_ERR_INVALID, "NULL handle");
    if (option == MI_OPT_RESERVE_CUS && h->masked_state != 0)
        return fail(MI_ERR_INVALID, "MI_OPT_RESERVE_CUS is decided at the handle's first time-parallel call: set it before");
    if (option == MI_OPT_SPLIT_CUS && h->split_state != 0)
        return fail(MI_ERR_INVALID, "MI_OPT_SPLIT_CUS is decided at the handle's first overlapped serial call: set it before");
    const char* why = "";
    const int rc = mi::tuning_set(h->opt, option, value, &why);
    return rc == MI_OK ? MI_OK : fail(rc, why);
}

// ---------------- host-only plan views ----------------

int mi_plan_create(const mi_device_cfg* dev, const mi_channel_cfg* chans, int nch, mi_plan** out) {
    if (!out || !dev)
        return fail(MI_ERR_INVALID, "NULL argument");
    *out = nullptr;
    mi_plan* p = new (std::nothrow) mi_plan();
    if (!p)
        return fail(MI_ERR_NOMEM, "host allocation failed");
    const char* msg = "";
    int rc = mi::build_plan(*dev, chans, nch, p->plan, &msg);
    if (rc != MI_OK) {
        delete p;
        return fail(rc, msg);
    }
    *out = p;
    return MI_OK;
}

void mi_plan_destroy(mi_plan* p) {
    delete p;
}

int mi_plan_fft_size(const mi_plan* p) {
    return p ? p->plan.fft_size : 0;
}

int mi_plan_window(const mi_plan* p, float* out) {
    if (!p || !out)
        return fail(MI_ERR_INVALID, "NULL argument");
    std::memcpy(out, p->plan.window.data(), p->plan.window.size() * 4);
    return MI_OK;
}

int mi_plan_twiddles(const mi_plan* p, float* out) {
    if (!p || !out)
        return fail(MI_ERR_INVALID, "NULL argument");
    std::memcpy(out, p->plan.tw.data(), p->plan.tw.size() * 4);
    return MI_OK;
}

int mi_plan_levels(const mi_plan* p, float* out) {
    if (!p || !out)
        return fail(MI_ERR_INVALID, "NULL argument");
    std::memcpy(out, p->plan.levels.data(), 256 * 4);
    return MI_OK;
}

int mi_plan_sincos_lut(const mi_plan* p, float* sin_out, float* cos_out) {
    if (!p || !sin_out || !cos_out)
        return fail(MI_ERR_INVALID, "NULL argument");
    std::memcpy(sin_out, p->plan.sin_lut, 257 * 4);
    std::memcpy(cos_out, p->plan.cos_lut, 257 * 4);
    return MI_OK;
}

int mi_plan_channel(const mi_plan* p, int ch, mi_channel_derived* out) {
    if (!p || !out || ch < 0 || ch >= p->plan.nch)
        return fail(MI_ERR_INVALID, "bad channel index");
    const mi::ChanParams& c = p->plan.cp[ch];
    out->bin = c.bin;
    out->dm_dphi = c.dm_dphi;
    out->needs_raw_iq = c.needs_raw_iq;
    out->has_iq_outputs = c.has_iq_outputs;
    out->modulation = c.modulation;
    out->using_manual_level = c.using_manual_level;
    out->manual_signal_level = c.manual_signal_level;
    out->normal_signal_ratio = c.normal_signal_ratio;
    out->flappy_signal_ratio = c.flappy_signal_ratio;
    out->ampfactor = c.ampfactor;
    out->alpha = c.alpha;
    out->notch_enabled = c.notch_enabled;
    out->notch_d[0] = c.notch_d0;
    out->notch_d[1] = c.notch_d1;
    out->notch_d[2] = c.notch_d2;
    out->lowpass_enabled = c.lowpass_enabled;
    out->lowpass_gain = c.lowpass_gain;
    out->lowpass_ycoeffs[0] = c.lowpass_yc0;
    out->lowpass_ycoeffs[1] = c.lowpass_yc1;
    out->ctcss_enabled = c.ctcss_enabled;
    out->ctcss_fast_window = c.ctcss_fast_window;
    out->ctcss_slow_window = c.ctcss_slow_window;
    out->ctcss_fast_ndet = c.ctcss_fast_ndet;
    out->ctcss_slow_ndet = c.ctcss_slow_ndet;
    return MI_OK;
}

int mi_plan_lane_fft(const mi_plan* p, int* enabled, uint64_t need[6], int* lanes_per_window, int* slots, float* stage_tw) {
    if (!p)
        return fail(MI_ERR_INVALID, "NULL argument");
    const mi::Plan& pl = p->plan;
    const bool on = pl.l64.enabled != 0;
    const int nst = pl.log2n > 6 ? pl.log2n - 6 : 0;
    if (enabled)
        *enabled = on ? 1 : 0;
    if (lanes_per_window)
        *lanes_per_window = on ? pl.fft_size / 64 : 0;
    for (int s = 0; need && s < 6; ++s)
        need[s] = on ? pl.l64.need[s] : 0;
    for (int i = 0; i < pl.nch; ++i) {
        if (slots)
            slots[i] = on ? pl.l64_chan[static_cast<size_t>(i)].slot : 0;
        for (int k = 0; stage_tw && k < 2 * nst; ++k)
            stage_tw[static_cast<size_t>(i) * 2 * nst + k] = (on && k < 10) ? pl.l64_chan[static_cast<size_t>(i)].w[k] : 0.0f;
    }
    return MI_OK;
}

int mi_plan_ctcss_coeffs(const mi_plan* p, int ch, int slow, float* out) {
    if (!p || !out || ch < 0 || ch >= p->plan.nch)
        return fail(MI_ERR_INVALID, "bad channel index");
    const mi::ChanParams& c = p->plan.cp[ch];
    if (!c.ctcss_enabled)
        return fail(MI_ERR_INVALID, "channel has no ctcss");
    const float* base = p->plan.ctcss_coeff.data() + (static_cast<size_t>(c.ctcss_row) * 2 + (slow ? 1 : 0)) * mi::kMaxTones;
    std::memcpy(out, base, static_cast<size_t>(slow ? c.ctcss_slow_ndet : c.ctcss_fast_ndet) * 4);
    return MI_OK;
}

// ---------------- synthetic IQ ----------------

int mi_iqgen_host(const mi_iqgen_cfg* cfg, uint32_t stream_id, uint64_t first, uint64_t count, uint8_t* out) {
    if (!cfg || !out || cfg->ncarriers < 0 || cfg->ncarriers > 64 || cfg->sample_rate <= 0)
        return fail(MI_ERR_INVALID, "bad iqgen configuration");
    mi::IqGenDerived g;
    mi::iqgen_derive(*cfg, g);
    const int16_t* tab = mi::iqgen_sine_table();
    for (uint64_t i = 0; i < count; ++i)
        mi::iq_sample(g, tab, stream_id, first + i, out + 2 * i);
    return MI_OK;
}

int mi_iqgen_device(const mi_iqgen_cfg* cfg, uint32_t first_stream_id, uint32_t nstreams, size_t stream_stride_bytes, uint64_t first,
                    uint64_t count, void* d_out, void* hip_stream) {
    if (!cfg || !d_out || cfg->ncarriers < 0 || cfg->ncarriers > 64 || cfg->sample_rate <= 0)
        return fail(MI_ERR_INVALID, "bad iqgen configuration");
    if (reinterpret_cast<uintptr_t>(d_out) % 16 != 0 || stream_stride_bytes % 16 != 0)
        return fail(MI_ERR_INVALID, "iqgen output must be 16-byte aligned");
    mi::IqGenDerived g;
    mi::iqgen_derive(*cfg, g);
    mi::DevBuf<mi::IqGenDerived> d_cfg;
    mi::DevBuf<int16_t> d_tab;
    HIP_TRY(dalloc(d_cfg, 1));
    HIP_TRY(dalloc(d_tab, 1024));
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    int rc = MI_OK;
    hipError_t e;
    if ((e = hipMemcpy(d_cfg, &g, sizeof(g), hipMemcpyHostToDevice)) != hipSuccess ||
        (e = hipMemcpy(d_tab, mi::iqgen_sine_table(), 1024 * sizeof(int16_t), hipMemcpyHostToDevice)) != hipSuccess ||
        (e = mi::launch_iqgen(d_cfg, d_tab, first_stream_id, nstreams, stream_stride_bytes, first, count, static_cast<unsigned char*>(d_out), s)) !=
            hipSuccess ||
        (e = hipStreamSynchronize(s)) != hipSuccess)
        rc = hip_fail(e, "mi_iqgen_device");
    return rc;
}

}  // extern "C"

namespace mi {

void iqgen_derive(const mi_iqgen_cfg& cfg, IqGenDerived& out) {
    std::memset(&out, 0, sizeof(out));
    out.seed = cfg.seed;
    out.gate_samples = cfg.gate_samples;
    out.noise_q8_mul = cfg.noise_q8_mul;
    out.ncarriers = cfg.ncarriers;
    const double turn = 4294967296.0;
    for (int k = 0; k < cfg.ncarriers; ++k) {
        const mi_iqgen_carrier& c = cfg.carriers[k];
        const long long d = std::llround(static_cast<double>(c.offset_hz) / cfg.sample_rate * turn);
        out.c[k].dphi = static_cast<uint32_t>(static_cast<uint64_t>(d));
        out.c[k].dpsi_1k = static_cast<uint32_t>(std::llround(1000.0 / cfg.sample_rate * turn));
        out.c[k].dpsi_100 = static_cast<uint32_t>(std::llround(100.0 / cfg.sample_rate * turn));
        out.c[k].kind = c.kind;
        out.c[k].amp_q8 = c.amp_q8;
        out.c[k].gate_phase = c.gate_phase;
    }
}

const int16_t* iqgen_sine_table() {
    static int16_t tab[1024];
    static bool init = false;
    if (!init) {
        for (int i = 0; i < 1024; ++i)
            tab[i] = static_cast<int16_t>(std::lround(32767.0 * std::sin(2.0 * M_PI * i / 1024.0)));
        init = true;
    }
    return tab;
}

}  // namespace mi
