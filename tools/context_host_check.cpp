// context_host_check.cpp — the command line's no-device context grep (fcx_cli_host.h: host_grep_blocks, parse_context,
// load_patterns), the set compiler (fcx_patset.h) and the host decoder (fcx_decode.cpp) as a stand-alone host
// program, for a sanitizer build:
//
//   c++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -Iinclude \
//       -Imy_compress_amd/csrc tools/context_host_check.cpp my_compress_amd/csrc/fcx_decode.cpp -o context_host_check
//   ./context_host_check FILE.fcx PATTERNS FLAGS HH BEFORE AFTER [OUT]
// PATTERNS is a pattern file; FLAGS is made of the letters x (its lines are hex digits), i (fold ASCII case), v
// (invert) and - (nothing); HH is the delimiter; the blocks' bytes go to OUT with the `--` lines between them, and
// the totals and "counts: ..." to stdout.
//
// Exit status 0 when the file decodes, 1 when the decoder rejects it (a damaged record), 2 for arguments the
// parsers or the set compiler refuse (a pattern that holds the delimiter, a context above 4096 among them): all
// are clean runs; a sanitizer report is not.
#include <cstdio>
#include <cstring>
#include <memory>

#include "fcx.h"
#include "fcx_cli_host.h"

int main(int argc, char **argv) {
    if (argc != 7 && argc != 8) {
        fprintf(stderr, "usage: context_host_check FILE.fcx PATTERNS FLAGS HH BEFORE AFTER [OUT]\n");
        return 2;
    }
    const bool hex = strchr(argv[3], 'x') != nullptr, fold = strchr(argv[3], 'i') != nullptr, invert = strchr(argv[3], 'v') != nullptr;
    std::vector<uint8_t> bytes;
    std::vector<uint32_t> lens;
    uint8_t delim = 0;
    fcx_grep_opts opts = {invert ? FCX_GREP_INVERT : 0u, 0, 0};
    std::unique_ptr<fcx_pattern_set> set(new fcx_pattern_set());
    if (!fcx_cli::load_patterns(argv[2], hex, &bytes, &lens) ||
        fcx::patset_compile(set.get(), bytes.data(), lens.data(), (uint32_t)lens.size(), fold ? FCX_SET_FOLD_ASCII : 0u) ||
        !fcx_cli::parse_delim(argv[4], &delim) || set->holds(delim) || (fold && set->holds(fcx::fold_ascii(delim))) ||
        !fcx_cli::parse_context(argv[5], &opts.before) || !fcx_cli::parse_context(argv[6], &opts.after)) {
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
    FILE *fout = argc == 8 ? fopen(argv[7], "wb") : nullptr;
    if (argc == 8 && !fout) {
        fclose(fin);
        return 2;
    }
    uint64_t stats[6] = {}, counts[FCX_SET_MAX_PATTERNS] = {};
    const int r = fcx_cli::host_grep_blocks(fin, nblocks, delim, *set, opts, fout, stats, counts);
    if (r == 0) {
        printf("counts:");
        for (uint32_t k = 0; k < set->npat; k++) printf(" %llu", (unsigned long long)counts[k]);
        printf("\n");
    }
    if (fout) fclose(fout);
    fclose(fin);
    return r ? 1 : 0;
}
