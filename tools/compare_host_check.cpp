// compare_host_check.cpp — the command line's no-device --compare code (fcx_cli_host.h) and the host
// decoder (fcx_decode.cpp) as a stand-alone host program, for a sanitizer build:
//
//   hipcc -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -Iinclude \
//         -Imy_compress_amd/csrc tools/compare_host_check.cpp my_compress_amd/csrc/fcx_decode.cpp -o compare_host_check
//   ./compare_host_check FILE.fcx ORIGINAL [BLOCK_BYTES]     (default block size: 1 MiB)
//
// Prints what `my_compress -i FILE.fcx --compare ORIGINAL -b BLOCK_BYTES` prints without a device.
// Exit status 0 when every block comes back, 1 when blocks differ, 3 when the decoder rejects the
// file (a damaged or truncated record): all three are clean runs; a sanitizer report is not.
#include <cstdio>
#include <cstdlib>

#include "fcx.h"
#include "fcx_cli_host.h"

int main(int argc, char **argv) {
    if (argc < 3 || argc > 4) {
        fprintf(stderr, "usage: compare_host_check FILE.fcx ORIGINAL [BLOCK_BYTES]\n");
        return 2;
    }
    const uint32_t block = argc == 4 ? (uint32_t)strtoul(argv[3], nullptr, 0) : FCX_DEFAULT_BLOCK_BYTES;
    if (block == 0 || block > FCX_MAX_BLOCK_BYTES) {
        fprintf(stderr, "block size must be in [1, %u]\n", FCX_MAX_BLOCK_BYTES);
        return 2;
    }
    FILE *fin = fopen(argv[1], "rb"), *forig = fopen(argv[2], "rb");
    if (!fin || !forig) {
        if (fin) fclose(fin);
        if (forig) fclose(forig);
        return 2;
    }
    uint8_t hdr[FCX_HEADER_BYTES];   // "FCX7", u32 total, u16 blocks
    uint16_t nblocks = 0;
    if (fread(hdr, 1, sizeof(hdr), fin) == sizeof(hdr)) memcpy(&nblocks, hdr + 8, 2);
    else memset(hdr, 0, sizeof(hdr));
    int r = 2;
    if (memcmp(hdr, "FCX7", 4) != 0) {
        fprintf(stderr, "not an FCX7 file\n");
    } else {
        uint64_t stats[FCX_VERIFY_STATS];
        r = fcx_cli::host_compare(fin, forig, nblocks, block, stats);
        if (r < 0) r = 3;
    }
    fclose(fin);
    fclose(forig);
    return r;
}
