#include "output_adapters.hpp"

#include <cstring>
#include <ctime>

int rawfile_put(rawfile_out_t* out, const float* iq_out, char axcindicate) {
    if (!out->continuous && axcindicate == NO_SIGNAL && !out->active)
        return 0;  // output.cpp:516-519 (the file would be closed here if a transmission just ended)
    const size_t buflen = 2 * sizeof(float) * WAVE_BATCH;  // output.cpp:548-551
    const size_t written = fwrite(iq_out, 1, buflen, out->f);
    out->active = (axcindicate != NO_SIGNAL);  // output.cpp:560
    if (written < buflen)
        return -1;
    out->batches_written++;
    return 1;
}

static int txfile_close_if_necessary(txfile_out_t* out) {  // output.cpp:367-375 with batches for seconds
    if (!out->f)
        return 0;
    const uint64_t duration = out->clock - out->opened, idle = out->clock - out->last_write;
    if (!(duration > out->max_batches || (duration > out->min_batches && idle > out->idle_batches)))
        return 0;
    fclose(out->f);
    out->f = nullptr;
    out->files_closed++;
    return TXFILE_CLOSED;
}

int txfile_put(txfile_out_t* out, const void* payload, size_t bytes, char axcindicate) {
    int what = txfile_close_if_necessary(out);  // on either side of the skip below (output.cpp:519, :410)
    if (axcindicate == NO_SIGNAL && !out->active) {
        out->clock++;
        return what;  // output.cpp:518-520
    }
    if (!out->f) {  // output_file_ready, output.cpp:404-414, :454
        out->seq++;
        const std::string path = out->dir + "/row_" + std::to_string(out->row) + "_tx_" + std::to_string(out->seq);
        out->f = fopen(path.c_str(), "wb");
        if (!out->f)
            return -1;
        out->opened = out->last_write = out->clock;
        out->files_opened++;
        what |= TXFILE_OPENED;
    }
    const size_t written = fwrite(payload, 1, bytes, out->f);
    out->active = (axcindicate != NO_SIGNAL);  // output.cpp:560
    out->last_write = out->clock;              // output.cpp:561
    out->clock++;
    if (written < bytes)
        return -1;
    out->batches_written++;
    return what | TXFILE_WRITTEN;
}

void txfile_finish(txfile_out_t* out) {
    if (out->f) {
        fclose(out->f);
        out->f = nullptr;
        out->files_closed++;
    }
}

size_t tx_file_suffix(int64_t epoch_us_of_batch_0, uint64_t batch, bool include_freq, int freq, char* buf) {
    const int64_t us = epoch_us_of_batch_0 + (int64_t)batch * WAVE_BATCH * 1000000 / WAVE_RATE;
    time_t sec = (time_t)(us / 1000000 - (us % 1000000 < 0 ? 1 : 0));  // floor, before 1970 too
    struct tm utc;
    gmtime_r(&sec, &utc);
    size_t n = strftime(buf, 32, "_%Y%m%d_%H%M%S", &utc);
    if (include_freq)
        n += (size_t)snprintf(buf + n, 16, "_%d", freq);
    return n;
}

bool udp_stream_sends(bool continuous, char axcindicate) {
    return continuous || axcindicate != NO_SIGNAL;
}

size_t udp_payload_bytes(bool stereo) {
    return (size_t)WAVE_BATCH * sizeof(float) * (stereo ? 2 : 1);
}

size_t udp_payload_mono(const float* waveout, unsigned char* out) {
    memcpy(out, waveout, (size_t)WAVE_BATCH * sizeof(float));
    return (size_t)WAVE_BATCH * sizeof(float);
}

size_t udp_payload_stereo(const float* waveout, const float* waveout_r, unsigned char* out) {
    // The reference interleaves into stereo_buffer and sends `len * 2` bytes with len = WAVE_BATCH * sizeof(float):
    // 2 * WAVE_BATCH floats = WAVE_BATCH frames of (left, right).
    float* o = reinterpret_cast<float*>(out);
    for (size_t i = 0; i < (size_t)WAVE_BATCH; ++i) {
        o[2 * i] = waveout[i];
        o[2 * i + 1] = waveout_r[i];
    }
    return (size_t)WAVE_BATCH * sizeof(float) * 2;
}
