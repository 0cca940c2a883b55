// lines_host_check.cpp — the command line's no-device line code (fcx_cli_host.h: host_lines,
// host_find_numbered, parse_lines, parse_delim) and the host decoder (fcx_decode.cpp) as a stand-alone host
// program, for a sanitizer build:
//
//   hipcc -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -Iinclude \
//         -Imy_compress_amd/csrc tools/lines_host_check.cpp my_compress_amd/csrc/fcx_decode.cpp -o lines_host_check
//   ./lines_host_check FILE.fcx HH count          the totals for the delimiter HH (two hex digits)
//   ./lines_host_check FILE.fcx HH lines A:N OUT  lines A .. A+N-1 (A from 1, "A:" to the end) to OUT
//   ./lines_host_check FILE.fcx HH find HEX       the hits of the pattern's bytes with their lines
//
// Exit status 0 when the file decodes, 1 when the decoder rejects it (a damaged record), 2 for arguments the
// parsers refuse: all are clean runs; a sanitizer report is not.
#include <cstdio>
#include <cstring>

#include "fcx.h"
#include "fcx_cli_host.h"

int main(int argc, char **argv) {
    if (argc < 4) {
        fprintf(stderr, "usage: lines_host_check FILE.fcx HH count | lines A:N OUT | find HEX\n");
        return 2;
    }
    uint8_t delim = 0;
    if (!fcx_cli::parse_delim(argv[2], &delim)) {
        fprintf(stderr, "bad delimiter %s\n", argv[2]);
        return 2;
    }
    const bool count = strcmp(argv[3], "count") == 0 && argc == 4, lines = strcmp(argv[3], "lines") == 0 && argc == 6,
               find = strcmp(argv[3], "find") == 0 && argc == 5;
    uint64_t first = 0, n = 0;
    std::vector<uint8_t> pat;
    if (!(count || lines || find) || (lines && !fcx_cli::parse_lines(argv[4], &first, &n)) || (find && !fcx_cli::parse_hex(argv[4], &pat))) {
        fprintf(stderr, "bad arguments\n");
        return 2;
    }
    FILE *fin = fopen(argv[1], "rb");
    if (!fin) return 2;
    uint8_t hdr[FCX_HEADER_BYTES];   // "FCX7", u32 total, u16 blocks
    uint16_t nblocks = 0;
    if (fread(hdr, 1, sizeof(hdr), fin) == sizeof(hdr)) memcpy(&nblocks, hdr + 8, 2);
    else memset(hdr, 0, sizeof(hdr));
    if (memcmp(hdr, "FCX7", 4) != 0) {
        fprintf(stderr, "not an FCX7 file\n");
        fclose(fin);
        return 2;
    }
    int r;
    if (find) {
        r = fcx_cli::host_find_numbered(fin, nblocks, pat.data(), (uint32_t)pat.size(), delim, nullptr);
    } else {
        FILE *fout = lines ? fopen(argv[5], "wb") : nullptr;
        if (lines && !fout) {
            fclose(fin);
            return 2;
        }
        uint64_t stats[4] = {};
        r = fcx_cli::host_lines(fin, nblocks, delim, fout, first, n, stats);
        if (fout) fclose(fout);
    }
    fclose(fin);
    return r ? 1 : 0;
}
