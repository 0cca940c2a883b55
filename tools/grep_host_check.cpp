// grep_host_check.cpp — the command line's no-device grep code (fcx_cli_host.h: host_grep, pattern_holds,
// parse_hex, parse_delim) and the host decoder (fcx_decode.cpp) as a stand-alone host program, for a sanitizer
// build:
//
//   hipcc -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -Iinclude \
//         -Imy_compress_amd/csrc tools/grep_host_check.cpp my_compress_amd/csrc/fcx_decode.cpp -o grep_host_check
//   ./grep_host_check FILE.fcx HH HEX OUT     the lines that hold the bytes HEX, delimiter HH (two hex digits), to OUT
//   ./grep_host_check FILE.fcx HH HEX         the totals alone
//
// Exit status 0 when the file decodes, 1 when the decoder rejects it (a damaged record), 2 for arguments the
// parsers refuse (a pattern that holds the delimiter among them): all are clean runs; a sanitizer report is not.
#include <cstdio>
#include <cstring>

#include "fcx.h"
#include "fcx_cli_host.h"

int main(int argc, char **argv) {
    if (argc != 4 && argc != 5) {
        fprintf(stderr, "usage: grep_host_check FILE.fcx HH HEX [OUT]\n");
        return 2;
    }
    uint8_t delim = 0;
    std::vector<uint8_t> pat;
    if (!fcx_cli::parse_delim(argv[2], &delim) || !fcx_cli::parse_hex(argv[3], &pat) || fcx_cli::pattern_holds(pat, delim)) {
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
    FILE *fout = argc == 5 ? fopen(argv[4], "wb") : nullptr;
    if (argc == 5 && !fout) {
        fclose(fin);
        return 2;
    }
    uint64_t stats[4] = {};
    const int r = fcx_cli::host_grep(fin, nblocks, delim, pat.data(), (uint32_t)pat.size(), fout, stats);
    if (fout) fclose(fout);
    fclose(fin);
    return r ? 1 : 0;
}
