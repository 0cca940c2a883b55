// cut_host_check.cpp — the LIST compiler (fcx_cut.h), the command line's no-device cut (fcx_cli_host.h: host_cut) and
// the host decoder (fcx_decode.cpp) as a stand-alone host program, for a sanitizer build:
//
//   hipcc -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -Iinclude \
//         -Imy_compress_amd/csrc tools/cut_host_check.cpp my_compress_amd/csrc/fcx_decode.cpp -o cut_host_check
//   ./cut_host_check FILE.fcx f|b|F|B LIST SS DD OUT   fields (f) or bytes (b) of LIST, upper case: the complement;
//                                                      SS and DD: separator and delimiter, two hex digits each;
//                                                      OUT: the output file, or - for the totals alone
//   ./cut_host_check - f|b|F|B LIST SS DD              the compiler alone: prints "mn M open O"
//
// Exit status 0 when the file decodes, 1 when the decoder rejects it (a damaged record), 2 for arguments the parsers or
// the compiler refuse (the compiler's reason goes to stderr): all are clean runs; a sanitizer report is not.
#include <cstdio>
#include <cstring>

#include "fcx.h"
#include "fcx_cli_host.h"

int main(int argc, char **argv) {
    const bool compile_only = argc == 6 && strcmp(argv[1], "-") == 0;
    if (!(argc == 7 || compile_only) || strlen(argv[2]) != 1 || !strchr("fbFB", argv[2][0])) {
        fprintf(stderr, "usage: cut_host_check FILE.fcx|- f|b|F|B LIST SS DD [OUT|-]\n");
        return 2;
    }
    uint8_t sep = 0, delim = 0;
    if (!fcx_cli::parse_delim(argv[4], &sep) || !fcx_cli::parse_delim(argv[5], &delim)) {
        fprintf(stderr, "bad separator or delimiter\n");
        return 2;
    }
    const char m = argv[2][0];
    fcx_cut cut;
    const std::string why = fcx::cut_compile(&cut, argv[3], (uint32_t)strlen(argv[3]), m == 'f' || m == 'F' ? FCX_CUT_FIELDS : FCX_CUT_BYTES,
                                             sep, delim, m == 'F' || m == 'B' ? FCX_CUT_COMPLEMENT : 0u);
    if (!why.empty()) {
        fprintf(stderr, "%s\n", why.c_str());
        return 2;
    }
    if (compile_only) {
        printf("mn %u open %u\n", cut.mn, cut.open_end);
        return 0;
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
    FILE *fout = strcmp(argv[6], "-") == 0 ? nullptr : fopen(argv[6], "wb");
    if (!fout && strcmp(argv[6], "-") != 0) {
        fclose(fin);
        return 2;
    }
    uint64_t stats[FCX_CUT_STATS] = {};
    const int r = fcx_cli::host_cut(fin, nblocks, cut, fout, stats);
    if (fout) fclose(fout);
    fclose(fin);
    return r ? 1 : 0;
}
