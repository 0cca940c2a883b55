// repair_host_check.cpp — the command line's no-device --repair code (fcx_cli_host.h, fcx_repair_file.h) and
// the host decoder (fcx_decode.cpp) as a stand-alone host program, for a sanitizer build:
//
//   hipcc -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -Iinclude \
//         -Imy_compress_amd/csrc tools/repair_host_check.cpp my_compress_amd/csrc/fcx_decode.cpp -o repair_host_check
//   ./repair_host_check build FILE.fcx ORIGINAL SIDECAR [BLOCK_BYTES]     (default block size: 1 MiB)
//   ./repair_host_check apply FILE.fcx SIDECAR OUTPUT
//
// `build` writes what `my_compress -i FILE.fcx --compare ORIGINAL --repair SIDECAR -b BLOCK_BYTES` writes without
// a device, `apply` what `my_compress -i FILE.fcx -o OUTPUT --repair SIDECAR` writes.  Exit status 0 on
// success, 3 when the file, the original or the sidecar is refused (a damaged record, a sidecar that does
// not fit): both are clean runs; a sanitizer report is not.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "fcx.h"
#include "fcx_cli_host.h"

static int usage() {
    fprintf(stderr, "usage: repair_host_check build FILE.fcx ORIGINAL SIDECAR [BLOCK_BYTES]\n"
                    "       repair_host_check apply FILE.fcx SIDECAR OUTPUT\n");
    return 2;
}

int main(int argc, char **argv) {
    if (argc < 5) return usage();
    const bool build = strcmp(argv[1], "build") == 0;
    if (!build && strcmp(argv[1], "apply") != 0) return usage();
    if (argc > (build ? 6 : 5)) return usage();
    const uint32_t block = build && argc == 6 ? (uint32_t)strtoul(argv[5], nullptr, 0) : FCX_DEFAULT_BLOCK_BYTES;
    if (block == 0 || block > FCX_MAX_BLOCK_BYTES) {
        fprintf(stderr, "block size must be in [1, %u]\n", FCX_MAX_BLOCK_BYTES);
        return 2;
    }
    FILE *fin = fopen(argv[2], "rb"), *second = fopen(argv[3], "rb"), *out = fopen(argv[4], "wb");
    int r = 2;
    uint8_t hdr[FCX_HEADER_BYTES];   // "FCX7", u32 total, u16 blocks
    uint16_t nblocks = 0;
    if (fin && second && out) {
        if (fread(hdr, 1, sizeof(hdr), fin) == sizeof(hdr)) memcpy(&nblocks, hdr + 8, 2);
        else memset(hdr, 0, sizeof(hdr));
        if (memcmp(hdr, "FCX7", 4) != 0) {
            fprintf(stderr, "not an FCX7 file\n");
        } else if (build) {
            uint64_t stats[FCX_REPAIR_FILE_STATS] = {};
            r = fcx_cli::host_repair_build(fin, second, nblocks, block, out, stats);
            if (r == 0) fcx_cli::repair_totals(stats[2], stats[3], stats[1]);
        } else {
            uint64_t n = 0;
            r = fcx_cli::host_repair_apply(fin, second, out, nblocks, &n);
            if (r == 0) printf("repaired bytes = %llu\n", (unsigned long long)n);
        }
        if (r < 0) r = 3;
    }
    for (FILE *f : {fin, second, out})
        if (f) fclose(f);
    return r;
}
