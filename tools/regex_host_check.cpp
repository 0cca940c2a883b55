// regex_host_check.cpp — the regex compiler (fcx_regex.h), the command line's no-device regex grep (fcx_cli_host.h:
// host_grep_regex) and the host decoder (fcx_decode.cpp) as a stand-alone host program, for a sanitizer build:
//
//   hipcc -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -Iinclude \
//         -Imy_compress_amd/csrc tools/regex_host_check.cpp my_compress_amd/csrc/fcx_decode.cpp -o regex_host_check
//   ./regex_host_check compile EXPRHEX FLAGS HH                    "regex: S states, C classes", or the refusal
//   ./regex_host_check hits EXPRHEX FLAGS HH LINEHEX               the positions of one line's body at which a match ends
//   ./regex_host_check grep FILE.fcx EXPRHEX FLAGS HH BEFORE AFTER [OUT]   the selected lines, delimiter HH, to OUT
// EXPRHEX and LINEHEX are hex digits; FLAGS is made of the letters i (fold ASCII case), v (invert) and - (nothing).
//
// Exit status 0 when the file decodes, 1 when the decoder rejects it (a damaged record), 2 for arguments the parsers
// or the compiler refuse (the compiler's message goes to stdout): all are clean runs; a sanitizer report is not.
#include <cstdio>
#include <cstring>
#include <memory>

#include "fcx.h"
#include "fcx_cli_host.h"

int main(int argc, char **argv) {
    const bool compile = argc == 5 && strcmp(argv[1], "compile") == 0;
    const bool hits = argc == 6 && strcmp(argv[1], "hits") == 0;
    const bool grep = (argc == 8 || argc == 9) && strcmp(argv[1], "grep") == 0;
    if (!compile && !hits && !grep) {
        fprintf(stderr, "usage: regex_host_check compile EXPRHEX FLAGS HH | hits EXPRHEX FLAGS HH LINEHEX | "
                        "grep FILE.fcx EXPRHEX FLAGS HH BEFORE AFTER [OUT]\n");
        return 2;
    }
    const int a = grep ? 3 : 2;   // where EXPRHEX stands
    std::vector<uint8_t> expr, line;
    uint8_t delim = 0;
    fcx_grep_opts opts = {strchr(argv[a + 1], 'v') ? FCX_GREP_INVERT : 0u, 0, 0};
    if (!fcx_cli::parse_hex(argv[a], &expr) || !fcx_cli::parse_delim(argv[a + 2], &delim) || (hits && *argv[5] && !fcx_cli::parse_hex(argv[5], &line)) ||
        (grep && (!fcx_cli::parse_context(argv[6], &opts.before) || !fcx_cli::parse_context(argv[7], &opts.after)))) {
        fprintf(stderr, "bad arguments\n");
        return 2;
    }
    std::unique_ptr<fcx_regex> re(new fcx_regex());
    const std::string why = fcx::regex_compile(re.get(), expr.data(), (uint32_t)expr.size(), delim, strchr(argv[a + 1], 'i') ? FCX_SET_FOLD_ASCII : 0u);
    if (!why.empty()) {
        printf("refused: %s\n", why.c_str());
        return 2;
    }
    if (compile) {
        printf("regex: %u states, %u classes\n", re->nstates, re->nclasses);
        return 0;
    }
    if (hits) {
        uint8_t st = (uint8_t)re->start;
        printf("hits:");
        for (size_t p = 0; p < line.size(); p++) {
            st = re->step(st, line[p]);
            if (line[p] != delim && re->hit(st, p + 1 == line.size() || line[p + 1] == delim)) printf(" %zu", p);
        }
        printf("\n");
        return 0;
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
    FILE *fout = argc == 9 ? fopen(argv[8], "wb") : nullptr;
    if (argc == 9 && !fout) {
        fclose(fin);
        return 2;
    }
    uint64_t stats[6] = {};
    const int r = fcx_cli::host_grep_regex(fin, nblocks, *re, opts, true, fout, stats);
    if (fout) fclose(fout);
    fclose(fin);
    return r ? 1 : 0;
}
