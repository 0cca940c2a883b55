// find_host_check.cpp — the command line's no-device --find code (fcx_cli_host.h: host_find, parse_hex)
// and the host decoder (fcx_decode.cpp) as a stand-alone host program, for a sanitizer build:
//
//   hipcc -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -Iinclude \
//         -Imy_compress_amd/csrc tools/find_host_check.cpp my_compress_amd/csrc/fcx_decode.cpp -o find_host_check
//   ./find_host_check FILE.fcx HEX [count]   the hits of the pattern's bytes (HEX: an even number of hex
//                                            digits), one line each unless `count` is given, then the totals
//
// Exit status 0 when the file decodes, 1 when the decoder rejects it (a damaged record): both are
// clean runs; a sanitizer report is not.
#include <cstdio>

#include "fcx.h"
#include "fcx_cli_host.h"

int main(int argc, char **argv) {
    if (argc < 3 || argc > 4) {
        fprintf(stderr, "usage: find_host_check FILE.fcx HEX [count]\n");
        return 2;
    }
    std::vector<uint8_t> pat;
    if (!fcx_cli::parse_hex(argv[2], &pat)) {
        fprintf(stderr, "bad pattern %s\n", argv[2]);
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
    uint64_t stats[2] = {0, 0};
    const int r = fcx_cli::host_find(fin, nblocks, pat.data(), (uint32_t)pat.size(), argc == 4, stats);
    fclose(fin);
    return r ? 1 : 0;
}
