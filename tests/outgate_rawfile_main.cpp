// Stand-alone driver for tests/test_outgate_host.py: feeds rawfile_put (host/output_adapters.cpp) one batch at a time, one
// non-continuous rawfile_out_t per row, and leaves each row's byte stream in <outdir>/row_<r>.cf32.
//   usage: outgate_rawfile <rows> <nbatches> <axc file: rows x nbatches bytes> <iq file: rows x nbatches x 2*WAVE_BATCH floats> <outdir>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "output_adapters.hpp"

int main(int argc, char** argv) {
    if (argc != 6)
        return 2;
    const size_t rows = strtoul(argv[1], nullptr, 10), nb = strtoul(argv[2], nullptr, 10);
    std::vector<char> axc(rows * nb);
    std::vector<float> iq(rows * nb * 2 * WAVE_BATCH);
    FILE* f = fopen(argv[3], "rb");
    if (!f || fread(axc.data(), 1, axc.size(), f) != axc.size())
        return 3;
    fclose(f);
    f = fopen(argv[4], "rb");
    if (!f || fread(iq.data(), sizeof(float), iq.size(), f) != iq.size())
        return 3;
    fclose(f);
    for (size_t r = 0; r < rows; ++r) {
        rawfile_out_t out;
        out.f = fopen((std::string(argv[5]) + "/row_" + std::to_string(r) + ".cf32").c_str(), "wb");
        if (!out.f)
            return 4;
        for (size_t b = 0; b < nb; ++b)
            if (rawfile_put(&out, iq.data() + (r * nb + b) * 2 * WAVE_BATCH, axc[r * nb + b]) < 0)
                return 5;
        fclose(out.f);
    }
    return 0;
}
