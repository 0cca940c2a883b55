// digest_host_check.cpp — the command line's no-device --digest / --test code (fcx_cli_host.h,
// fcx_digest_file.h, fcx_crc32.h) and the host decoder (fcx_decode.cpp) as a stand-alone host program, for a
// sanitizer build:
//
//   hipcc -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -Iinclude \
//         -Imy_compress_amd/csrc tools/digest_host_check.cpp my_compress_amd/csrc/fcx_decode.cpp -o digest_host_check
//   ./digest_host_check build ORIGINAL DIGEST [BLOCK_BYTES]        (default block size: 1 MiB)
//   ./digest_host_check check FILE.fcx DIGEST [SIDECAR]
//   ./digest_host_check sweep FILE.fcx DIGEST [SIDECAR]
//
// `build` writes what `my_compress -i X --compare ORIGINAL --digest DIGEST -b BLOCK_BYTES` writes without a
// device, `check` prints what `my_compress -i FILE.fcx --test --digest DIGEST [--repair SIDECAR]` prints.
// `sweep` runs the check with the digest file cut at every length and with every byte of it changed in turn
// (the checks' own lines go to /dev/null) and prints the count of the verdicts: a cut file must be refused, a changed one must not
// pass.  Exit status 0 on success (check: the verdict, 0 or 1), 3 when a file is refused, 4 when the sweep
// finds a cut or changed file that passes: all clean runs; a sanitizer report is not.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include <unistd.h>

#include "fcx.h"
#include "fcx_cli_host.h"

static int usage() {
    fprintf(stderr, "usage: digest_host_check build ORIGINAL DIGEST [BLOCK_BYTES]\n"
                    "       digest_host_check check FILE.fcx DIGEST [SIDECAR]\n"
                    "       digest_host_check sweep FILE.fcx DIGEST [SIDECAR]\n");
    return 2;
}

// the header of an FCX7 file at its start: the record count, or -1
static int records_of(FILE *fin) {
    uint8_t hdr[FCX_HEADER_BYTES];
    uint16_t nblocks = 0;
    rewind(fin);
    if (fread(hdr, 1, sizeof(hdr), fin) != sizeof(hdr) || memcmp(hdr, "FCX7", 4) != 0) return -1;
    memcpy(&nblocks, hdr + 8, 2);
    return nblocks;
}

static std::vector<uint8_t> slurp(FILE *f) {
    std::vector<uint8_t> b;
    uint8_t buf[65536];
    rewind(f);
    for (size_t g; (g = fread(buf, 1, sizeof(buf), f)) > 0;) b.insert(b.end(), buf, buf + g);
    rewind(f);
    return b;
}

int main(int argc, char **argv) {
    if (argc < 4 || argc > 5) return usage();
    if (strcmp(argv[1], "build") == 0) {
        const uint32_t block = argc == 5 ? (uint32_t)strtoul(argv[4], nullptr, 0) : FCX_DEFAULT_BLOCK_BYTES;
        if (block == 0 || block > FCX_MAX_BLOCK_BYTES) {
            fprintf(stderr, "block size must be in [1, %u]\n", FCX_MAX_BLOCK_BYTES);
            return 2;
        }
        FILE *forig = fopen(argv[2], "rb"), *fdig = fopen(argv[3], "wb");
        int r = 2;
        uint64_t stats[FCX_DIGEST_FILE_STATS] = {};
        if (forig && fdig) r = fcx_cli::host_digest_build(forig, block, fdig, stats) ? 3 : 0;
        if (r == 0) fcx_cli::digest_totals(stats[1], (uint32_t)stats[2]);
        for (FILE *f : {forig, fdig})
            if (f) fclose(f);
        return r;
    }
    const bool sweep = strcmp(argv[1], "sweep") == 0;
    if (!sweep && strcmp(argv[1], "check") != 0) return usage();
    FILE *fin = fopen(argv[2], "rb"), *fdig = fopen(argv[3], "rb"), *frep = argc == 5 ? fopen(argv[4], "rb") : nullptr;
    int r = 2;
    const int nblocks = fin ? records_of(fin) : -1;
    if (!fin || !fdig || (argc == 5 && !frep)) {
        fprintf(stderr, "cannot open the files\n");
    } else if (nblocks < 0) {
        fprintf(stderr, "not an FCX7 file\n");
    } else if (!sweep) {
        std::vector<uint32_t> vals;
        r = fcx_cli::load_digest(fdig, &vals) ? -1 : fcx_cli::host_check(fin, frep, fdig, (uint16_t)nblocks, nullptr);
        if (r < 0) r = 3;
    } else {
        const std::vector<uint8_t> whole = slurp(fdig);
        FILE *report = fdopen(dup(1), "w");   // (the checks' own lines go nowhere)
        if (!report || !freopen("/dev/null", "w", stdout) || !freopen("/dev/null", "w", stderr)) return 2;
        auto run = [&](std::vector<uint8_t> &d) {
            FILE *m = d.empty() ? fopen("/dev/null", "rb") : fmemopen(d.data(), d.size(), "rb");
            if (!m) return -2;
            records_of(fin);
            if (frep) rewind(frep);
            const int v = fcx_cli::host_check(fin, frep, m, (uint16_t)nblocks, nullptr);
            fclose(m);
            return v;
        };
        std::vector<uint8_t> d = whole;
        const int base = run(d);
        unsigned long cut_refused = 0, cut_passed = 0, changed_refused = 0, changed_failed = 0, changed_passed = 0;
        for (size_t len = 0; len < whole.size(); len++) {
            d.assign(whole.begin(), whole.begin() + len);
            (run(d) < 0 ? cut_refused : cut_passed)++;
        }
        for (size_t at = 0; at < whole.size(); at++) {
            d = whole;
            d[at] ^= 0x41;
            const int v = run(d);
            (v < 0 ? changed_refused : v == 1 ? changed_failed : changed_passed)++;
        }
        r = cut_passed || (base == 0 && changed_passed) ? 4 : 0;
        fprintf(report, "intact verdict %d; cut at %zu lengths: %lu refused, %lu not; %zu bytes changed: %lu refused, %lu fail, %lu pass\n",
                base, whole.size(), cut_refused, cut_passed, whole.size(), changed_refused, changed_failed, changed_passed);
        fclose(report);
    }
    for (FILE *f : {fin, fdig, frep})
        if (f) fclose(f);
    return r;
}
