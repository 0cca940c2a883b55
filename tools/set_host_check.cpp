// set_host_check.cpp — the command line's no-device pattern-set code (fcx_cli_host.h: host_find_set, host_grep_set,
// load_patterns / parse_patterns), the set compiler (fcx_patset.h) and the host decoder (fcx_decode.cpp) as a
// stand-alone host program, for a sanitizer build:
//
//   hipcc -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -Iinclude \
//         -Imy_compress_amd/csrc tools/set_host_check.cpp my_compress_amd/csrc/fcx_decode.cpp -o set_host_check
//   ./set_host_check find FILE.fcx PATTERNS FLAGS          one line per hit, then the totals and "counts: ..."
//   ./set_host_check grep FILE.fcx PATTERNS FLAGS HH [OUT] the lines that hold a pattern, delimiter HH, to OUT
// PATTERNS is a pattern file; FLAGS is made of the letters x (its lines are hex digits), i (fold ASCII case) and
// - (nothing).
//
// Exit status 0 when the file decodes, 1 when the decoder rejects it (a damaged record), 2 for arguments the
// parsers or the set compiler refuse (a pattern that holds the delimiter among them): all are clean runs; a
// sanitizer report is not.
#include <cstdio>
#include <cstring>
#include <memory>

#include "fcx.h"
#include "fcx_cli_host.h"

int main(int argc, char **argv) {
    const bool find = argc == 5 && strcmp(argv[1], "find") == 0;
    const bool grep = (argc == 6 || argc == 7) && strcmp(argv[1], "grep") == 0;
    if (!find && !grep) {
        fprintf(stderr, "usage: set_host_check find FILE.fcx PATTERNS FLAGS | grep FILE.fcx PATTERNS FLAGS HH [OUT]\n");
        return 2;
    }
    const bool hex = strchr(argv[4], 'x') != nullptr, fold = strchr(argv[4], 'i') != nullptr;
    std::vector<uint8_t> bytes;
    std::vector<uint32_t> lens;
    uint8_t delim = 0;
    std::unique_ptr<fcx_pattern_set> set(new fcx_pattern_set());
    if (!fcx_cli::load_patterns(argv[3], hex, &bytes, &lens) ||
        fcx::patset_compile(set.get(), bytes.data(), lens.data(), (uint32_t)lens.size(), fold ? FCX_SET_FOLD_ASCII : 0u) ||
        (grep && (!fcx_cli::parse_delim(argv[5], &delim) || set->holds(delim) || (fold && set->holds(fcx::fold_ascii(delim)))))) {
        fprintf(stderr, "bad arguments\n");
        return 2;
    }
    FILE *fin = fopen(argv[2], "rb");
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
    FILE *fout = argc == 7 ? fopen(argv[6], "wb") : nullptr;
    if (argc == 7 && !fout) {
        fclose(fin);
        return 2;
    }
    uint64_t stats[4] = {}, counts[FCX_SET_MAX_PATTERNS] = {};
    const int r = find ? fcx_cli::host_find_set(fin, nblocks, *set, false, stats, counts)
                       : fcx_cli::host_grep_set(fin, nblocks, delim, *set, fout, stats, counts);
    if (r == 0) {
        printf("counts:");
        for (uint32_t k = 0; k < set->npat; k++) printf(" %llu", (unsigned long long)counts[k]);
        printf("\n");
    }
    if (fout) fclose(fout);
    fclose(fin);
    return r ? 1 : 0;
}
