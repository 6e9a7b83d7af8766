// Stand-alone driver for tests/test_txsplit_files.py: feeds txfile_put (host/output_adapters.cpp) one batch at a time, one
// txfile_out_t per row, which leaves <outdir>/row_<r>_tx_<seq>; prints "event <row> <batch> <mask>" for every batch whose mask is
// not 0 and "row <row> <opened> <closed> <written> <open at the end>" per row.
//   usage: txsplit_files run <rows> <nbatches> <min> <idle> <max> <payload bytes a batch> <axc file> <payload file> <outdir>
//          txsplit_files suffix <epoch us of batch 0> <batch> <include_freq> <freq>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "output_adapters.hpp"

int main(int argc, char** argv) {
    if (argc == 6 && !strcmp(argv[1], "suffix")) {
        char buf[48];
        const size_t n = tx_file_suffix(strtoll(argv[2], nullptr, 10), strtoull(argv[3], nullptr, 10), atoi(argv[4]) != 0, atoi(argv[5]), buf);
        printf("%s %zu\n", buf, n);
        return 0;
    }
    if (argc != 11 || strcmp(argv[1], "run"))
        return 2;
    const size_t rows = strtoul(argv[2], nullptr, 10), nb = strtoul(argv[3], nullptr, 10), bytes = strtoul(argv[7], nullptr, 10);
    std::vector<char> axc(rows * nb);
    std::vector<unsigned char> payload(rows * nb * bytes);
    FILE* f = fopen(argv[8], "rb");
    if (!f || fread(axc.data(), 1, axc.size(), f) != axc.size())
        return 3;
    fclose(f);
    f = fopen(argv[9], "rb");
    if (!f || fread(payload.data(), 1, payload.size(), f) != payload.size())
        return 3;
    fclose(f);
    for (size_t r = 0; r < rows; ++r) {
        txfile_out_t out;
        out.dir = argv[10];
        out.row = static_cast<unsigned>(r);
        out.min_batches = static_cast<uint32_t>(strtoul(argv[4], nullptr, 10));
        out.idle_batches = static_cast<uint32_t>(strtoul(argv[5], nullptr, 10));
        out.max_batches = static_cast<uint32_t>(strtoul(argv[6], nullptr, 10));
        for (size_t b = 0; b < nb; ++b) {
            const int mask = txfile_put(&out, payload.data() + (r * nb + b) * bytes, bytes, axc[r * nb + b]);
            if (mask < 0)
                return 5;
            if (mask)
                printf("event %zu %zu %d\n", r, b, mask);
        }
        const bool open_at_end = out.f != nullptr;
        txfile_finish(&out);
        printf("row %zu %zu %zu %zu %d\n", r, out.files_opened, out.files_closed, out.batches_written, open_at_end ? 1 : 0);
    }
    return 0;
}
