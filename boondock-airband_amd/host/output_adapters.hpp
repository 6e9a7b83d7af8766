// output_adapters.hpp -- the byte formats the reference's output thread derives from the demod contract (SURVEY 8f
// rank 4).  Only the payloads are rebuilt, so that a replayed capture yields the same bytes; file naming / rotation,
// sockets, LAME and icecast stay with the reference.
//   rawfile     src/output.cpp:513-561   cf32: one batch = 2 * sizeof(float) * WAVE_BATCH bytes of channel->iq_out
//   file split  src/output.cpp:353-376, :404-462   split_on_transmission's one file per transmission, in signal time (txfile_put)
//   udp_stream  src/udp_stream.cpp:86-102, output.cpp:565-576   float32 PCM, mono or L/R interleaved, one datagram per batch
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>

#include "airband_host.hpp"

// O_RAWFILE state that matters for the payload stream: file_data::continuous and output_t::active
struct rawfile_out_t {
    FILE* f = nullptr;
    bool continuous = false;  // file_data::continuous (config key `continuous`)
    bool active = false;      // output_t::active: the previous batch had a signal (output.cpp:560)
    size_t batches_written = 0;
};

// One batch of the output thread's O_RAWFILE branch.  A non-continuous output skips a NO_SIGNAL batch only once the
// previous one was NO_SIGNAL too (output.cpp:516-519), i.e. every transmission is followed by one trailing batch.
// Returns 1 if the batch was written, 0 if skipped, -1 on a short write (the reference disables the output).
int rawfile_put(rawfile_out_t* out, const float* iq_out, char axcindicate);

// O_FILE / O_RAWFILE with split_on_transmission: one file per transmission, closed by close_if_necessary (output.cpp:353-376)
// -- in signal time: the reference asks gettimeofday(), a replay has no meaningful wall clock, so batch b is handled at
// t0 + b * WAVE_BATCH / WAVE_RATE and durations are counts of batches (include/mi_airband.h "transmission splitter": the same rule
// the device applies).  The per-batch twin of mi_tx_plan_host, for a host that writes the files itself.
struct txfile_out_t {
    std::string dir;  // files are <dir>/row_<row>_tx_<seq>, seq counting from 1
    unsigned row = 0;
    uint32_t min_batches = 8, idle_batches = 4, max_batches = 28800;  // 1.0 s, 0.5 s, 3600 s (output.cpp:356-358)
    FILE* f = nullptr;                                                // fdata->f
    bool active = false;                                              // output_t::active
    uint32_t seq = 0;
    uint64_t clock = 0, opened = 0, last_write = 0;  // batches: this row's clock, fdata->open_time, fdata->last_write_time
    size_t files_opened = 0, files_closed = 0, batches_written = 0;
};
enum { TXFILE_WRITTEN = 1, TXFILE_OPENED = 2, TXFILE_CLOSED = 4 };

// One batch of the output thread's file branch (output.cpp:515-561) under split_on_transmission: `payload` is what the output
// writes for a batch (the rawfile's cf32 block, an encoder's bytes), `bytes` its length.  Returns a mask of TXFILE_* -- a batch
// can close one file and open the next -- or -1 when a file cannot be opened or a write falls short (the reference disables
// the output).
int txfile_put(txfile_out_t* out, const void* payload, size_t bytes, char axcindicate);
// Closes the file still open at the end of a replay (the reference's files end with the process).
void txfile_finish(txfile_out_t* out);
// The reference's file name suffix "_%Y%m%d_%H%M%S" in UTC, "_<freq>" appended when include_freq (output.cpp:426, :446-448),
// for the batch's own time: epoch_us_of_batch_0 microseconds since the epoch plus batch * WAVE_BATCH / WAVE_RATE seconds.
// `buf` holds at least 48 bytes; returns the length.
size_t tx_file_suffix(int64_t epoch_us_of_batch_0, uint64_t batch, bool include_freq, int freq, char* buf);

// O_UDP_STREAM: is a datagram sent for this batch (output.cpp:568-570)?
bool udp_stream_sends(bool continuous, char axcindicate);
// Datagram payloads.  `out` must hold udp_payload_bytes(stereo) bytes; returns the payload length.
size_t udp_payload_bytes(bool stereo);
size_t udp_payload_mono(const float* waveout, unsigned char* out);                             // udp_stream.cpp:86-91
size_t udp_payload_stereo(const float* waveout, const float* waveout_r, unsigned char* out);  // udp_stream.cpp:93-102
