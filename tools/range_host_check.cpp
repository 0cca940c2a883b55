// range_host_check.cpp — the command line's no-device --list / --range code (fcx_cli_host.h) and the
// host decoder (fcx_decode.cpp) as a stand-alone host program, for a sanitizer build:
//
//   hipcc -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -Iinclude \
//         -Imy_compress_amd/csrc tools/range_host_check.cpp my_compress_amd/csrc/fcx_decode.cpp -o range_host_check
//   ./range_host_check FILE.fcx            the record list
//   ./range_host_check FILE.fcx OFF:LEN    the decoded bytes of the range, written to /dev/null
//
// Exit status 0 when the file decodes, 1 when the decoder rejects it (a damaged record): both are
// clean runs; a sanitizer report is not.
#include <cstdio>

#include "fcx.h"
#include "fcx_cli_host.h"

int main(int argc, char **argv) {
    if (argc < 2 || argc > 3) {
        fprintf(stderr, "usage: range_host_check FILE.fcx [OFF:LEN]\n");
        return 2;
    }
    uint64_t off = 0, len = 0;
    if (argc == 3 && !fcx_cli::parse_range(argv[2], &off, &len)) {
        fprintf(stderr, "bad range %s\n", argv[2]);
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
    if (argc == 2) r = fcx_cli::host_list(fin, nblocks);
    else {
        FILE *sink = fopen("/dev/null", "wb");
        uint64_t n = 0;
        r = fcx_cli::host_range(fin, sink, nblocks, off, len, &n);
        if (r == 0) printf("range bytes = %llu (offset %llu)\n", (unsigned long long)n, (unsigned long long)off);
        if (sink) fclose(sink);
    }
    fclose(fin);
    return r ? 1 : 0;
}
