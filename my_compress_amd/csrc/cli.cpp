// cli.cpp — the my_compress command line (main(), my_compress.cpp:3726-4213),
// compress path on the GPU through the C ABI.
//
//   my_compress -i IN [-o OUT] -c lz77     compress (FCX7, 1 MiB blocks)
//   my_compress -i IN [-o OUT]             decompress
//
// Same flags, default output "./out" (4040-4042) and byte stream as the
// reference.  Both directions stream through the GPU (fcx_compress_stream /
// fcx_decompress_stream: file reads and writes overlap the device work); without
// a HIP device, compress fails and decompress uses the host decoder.  Superset:
// -b/--block BYTES (<= 1 MiB; the reference fixes 1 MiB, BLOCK_BYTES :113) and
// -d/--device N and -g/--gpus N (-c lz77 over N GPUs of this node, devices d .. d+N-1:
// contiguous block ranges per GPU, segments gathered over RCCL, byte-identical
// output).  `-c lz78` runs the LZ78 codec (FCX8) on the GPU: 256 MiB shards
// through fcx_lz78_compress_host; an FCX8 file decompresses through
// fcx_decompress_stream like an FCX7 one (GPU-only: no host decoder for FCX8).
// Random access, decompress mode only (a usage error with -c, or both together):
//   --range OFF:LEN   writes only the decoded bytes [OFF, OFF + LEN) to -o (fcx_decompress_range_stream:
//                     only the records the range touches are expanded, nothing behind it is read)
//   --list            one line per record (numbered from 0): compressed, decoded bytes, decoded offset
// Without a HIP device both run on the host decoder for FCX7 and fail for FCX8, as decompress does.
// Round-trip verification (fcx_verify_stream: every record decoded and compared with its block):
//   --verify            with -c: compress as usual, close the output, then check it against the input
//   --compare ORIGINAL  decompress mode: check the -i file against ORIGINAL (-b: the block size it was
//                       made with, when not 1 MiB); writes no -o file.  Not with -c, --range, --list, --verify.
// One line per differing block, then the verdict; exit status 0 for OK, 1 for FAIL.  Without a HIP
// device --compare runs on the host decoder for FCX7 and fails for FCX8.
// Repair sidecar (an FCXR file: per block that does not decode back to its input, what restores it):
//   --repair FILE   with -c: compress as usual, close the output, then write the sidecar in a pass over the
//                   finished file and the input (after --verify's pass, when both are given);
//                   with --compare ORIGINAL: also write the sidecar of the -i file against ORIGINAL;
//                   otherwise (decompress): read the sidecar and write the repaired output, the original bytes.
//                   Not with --range or --list.  Prints "repair: E entries, D data bytes for R blocks" when
//                   it writes one.  Without a HIP device both run on the host decoder for FCX7 and fail for FCX8.
// Content digest (an FCXD file: the CRC-32 of every block of the original, and of the whole as crc32 and zip
// print it), and the test that needs no original (fcx_check_stream: every record decoded on the device, a
// repair applied in the sum, each block's CRC-32 against the file's):
//   --digest FILE   with -c: after the output is closed (and after --verify's and --repair's passes), a pass
//                   over the input writes the file; with --compare ORIGINAL: also writes ORIGINAL's;
//                   otherwise (decompress, [--repair R]): the ordinary decompress to -o, then the test in a
//                   second pass over -i.  Prints "digest: B blocks, crc32 XXXXXXXX" when it writes one.
//   --test          decompress mode with --digest FILE [--repair R]: the test alone, no -o file.
//                   Not with -c, --compare, --range or --list; --digest not with --range or --list.
// One line per failing block, then the verdict; exit status 0 for OK, 1 for FAIL.  Without a HIP device the
// FCX7 directions run on the host decoder and the host CRC-32, with the same file bytes and lines; FCX8 fails.
// Search, decompress mode only (fcx_find_stream: the decoded bytes stay on the device, the hit offsets come back):
//   --find STRING     the argument's bytes (1 to 256), anywhere in the decoded file, across record boundaries too
//   --find-hex HEX    the same for any bytes: an even number of hex digits
//   --count           with either: only the totals
// One line "find: offset N" per hit, then "find: H hits, decoded bytes = D"; no -o file; exit status 0 when the
// search ran.  Not with -c, --range, --list, --compare, --verify, --repair, --digest, --test, or both together.
// Without a HIP device an FCX7 file is searched on the host decoder, with the same lines; FCX8 fails.
// Lines, decompress mode only (fcx_lines_*: the decoded bytes stay on the device; a line ends with its delimiter,
// an unterminated tail is a line, lines lie across record boundaries like any other bytes):
//   --count-lines     prints "lines: L lines, N delimiters, decoded bytes = T" (wc -l); no -o file
//   --lines A:N       writes lines A .. A+N-1 to -o, A counted from 1 as sed -n 'A,Bp' counts; "A:" means to the
//                     end (fcx_lines_locate_stream, then the range decode of what it found); --range's twin
//   --line-numbers    with --find / --find-hex: "find: offset P line K" per hit, K counted from 1; a second pass
//                     over the file (fcx_lines_of_stream over the hits of fcx_find_stream)
//   --delim HH        the delimiter byte of the three, two hex digits (default 0a)
// Usage errors: --count-lines or --lines with -c, --range, --list, --compare, --verify, --repair, --digest, --test,
// --find or each other; --line-numbers without --find / --find-hex or with --count; --delim without one of the three.
// Without a HIP device an FCX7 file is served by the host decoder, with the same lines and bytes; FCX8 fails.
// Matching lines, decompress mode only (grep -F; fcx_grep_stream, then fcx_decompress_ranges_stream):
//   --grep STRING     writes every line that holds the argument's bytes (1 to 256, without the delimiter) to -o, each
//                     once and with its delimiter, in order; pass 1 collects the lines' byte ranges (16 bytes a line),
//                     pass 2 decodes the records they touch and writes them
//   --grep-hex HEX    the same for any bytes
//   --count           with either: only the totals, no -o file
//   --delim HH        the delimiter byte (default 0a)
// The last line printed is "grep: L lines, B bytes, H hits, decoded bytes = T".  Usage errors: --grep or --grep-hex with
// -c, --range, --list, --compare, --verify, --repair, --digest, --test, --find, --find-hex, --count-lines, --lines,
// --line-numbers or each other; a pattern that holds the delimiter; an empty or over-long pattern.
//
// Pattern sets, decompress mode only (fcx_find_set_stream / fcx_grep_set_stream: up to 64 patterns in one scan):
//   --find-set FILE   --find for every pattern of FILE: patterns are separated by 0x0A, one trailing 0x0A is allowed;
//                     an offset is printed once however many patterns occur there
//   --grep-set FILE   --grep for every pattern of FILE (grep -F -f): a line is written once
//   --set-hex         every line of FILE is an even number of hex digits
//   --ignore-case     A to Z match a to z and the other way round, nothing else folds (grep -i for ASCII); also with
//                     --find, --find-hex, --grep, --grep-hex, which then run as a set of one
//   --count, --delim  as with --find and --grep
// The totals lines end with ", patterns: P".  Usage errors: an empty pattern line (grep -f would match every line), more
// than 64 patterns, a pattern over 256 bytes, over 4096 bytes in all, bad hex, an unreadable FILE; both set options; a
// set option with --find, --find-hex, --grep or --grep-hex; --set-hex without a set; --ignore-case without a search;
// any of them with --line-numbers; for a grep a pattern that holds the delimiter or, with --ignore-case, that holds it
// after folding both; and whatever is a usage error with --find or --grep.
// Without a HIP device an FCX7 file is cut into lines on the host decoder, with the same bytes and last line; FCX8 fails.
//
// Context and inverted grep, with --grep, --grep-hex or --grep-set only (fcx_grep_blocks_stream, then
// fcx_decompress_ranges_stream over the blocks):
//   --invert          the lines that hold no pattern (grep -v)
//   --before N        N lines in front of every such line too (grep -B), N <= 4096
//   --after N         N lines behind it (grep -A)
//   --context N       both (grep -C)
// They combine with --ignore-case, --delim and --count.  The output is the selected lines in order; with a context a
// line "--" goes between two runs of consecutive selected lines, as GNU grep prints it.  The last line printed is
// "grep: K blocks, L lines, S base lines, B bytes, H hits, decoded bytes = T".  Usage errors: a value that is not a
// number or lies above 4096; one of the four without a grep option.
//
// Regular expressions, decompress mode only (fcx_grep_regex_blocks_stream, then fcx_decompress_ranges_stream):
//   --grep-regex EXPR the lines in which a match of the POSIX ERE subset of include/fcx.h ends (grep -E); with
//                     --count, --delim HH, --ignore-case, --invert, --before / --after / --context N as --grep-set takes
//                     them, and with its output and totals lines ("patterns: 1")
// Usage errors: an expression the compiler refuses (the reason and the offset are printed first); --grep-regex twice or
// with --find, --grep, their -hex and -set forms, --set-hex or --line-numbers.
//
// Cut, decompress mode only (fcx_cut_stream): the fields or byte columns of every line of the decoded bytes, to -o
//   --cut-fields LIST GNU cut's -f LIST: items N, N-M, N- or -M joined by commas; --sep HH the field separator (two hex
//                     digits, default 09)
//   --cut-bytes LIST  GNU cut's -b LIST
//   --complement      what LIST does not select; --delim HH the line delimiter; --count prints the totals and writes nothing
// The last line printed is "cut: N bytes, D delimiters, S separators (K kept), decoded bytes = T".  Two differences from
// GNU cut (include/fcx.h): a line without a separator and with field 1 unselected gives an empty line, and nothing is
// added behind an unterminated last line.  Usage errors: both cut options; a LIST the compiler refuses (the reason and
// the offset are printed first); a separator equal to the delimiter; --sep or --complement without a cut option; a cut
// option with -c, --range, --list, --find*, --count-lines, --compare, --verify, --repair, --digest or --test.
// Together with exactly one grep option (with its modifiers) or with --lines A:N the blocks, lines or line range come as
// they do without the cut (fcx_*_stream), and their cut comes through fcx_cut_ranges_host in a second pass; no `--` line is
// written between blocks, since it is not a byte of the file; the grep's own totals line comes first.
#include <getopt.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "fcx.h"
#include "fcx_cli_host.h"

static int usage() {
    fprintf(stderr,
            "usage: ./my_compress -i[or --file_in] <input file name> [-o[or --file_out] <output file name>] "
            "[-c (or --compress) <lz77/lz78>] [-b (or --block) <bytes>] [-d (or --device) <hip device>] "
            "[-g (or --gpus) <count>] [--verify (with -c)] [--range <offset>:<length> | --list | --compare <original> "
            "(decompress only)] [--repair <sidecar file> (written with -c or --compare, read by a decompress)] "
            "[--digest <digest file> (written with -c or --compare, checked by a decompress)] "
            "[--test (decompress with --digest: check only, no output file)] "
            "[--find <string> | --find-hex <hex digits> [--count | --line-numbers] (decompress only: search the decoded bytes)] "
            "[--count-lines | --lines <first line>:[<count>] (decompress only: the lines of the decoded bytes)] "
            "[--grep <string> | --grep-hex <hex digits> [--count] (decompress only: the lines that hold the bytes, to -o)] "
            "[--delim <two hex digits> (the line delimiter, default 0a)] "
            "[--find-set <pattern file> | --grep-set <pattern file> [--set-hex] [--count] (decompress only: up to 64 patterns, one a line)] "
            "[--ignore-case (with a search: ASCII letters match in either case)] "
            "[--invert] [--before <lines>] [--after <lines>] [--context <lines>] (with a grep: the lines without a pattern, "
            "lines of context, at most 4096) "
            "[--grep-regex <POSIX ERE> [--count] (decompress only: the lines in which a match ends, to -o)] "
            "[--cut-fields <LIST> [--sep <two hex digits, default 09>] | --cut-bytes <LIST> [--complement] [--count] "
            "(decompress only: the fields or byte columns of every line, or of the lines a grep option or --lines selects, to -o)]\n");
    return -1;
}

static int64_t file_read(void *u, uint8_t *buf, uint64_t cap) {
    FILE *f = (FILE *)u;
    const size_t n = fread(buf, 1, (size_t)cap, f);
    return ferror(f) ? -1 : (int64_t)n;
}

struct Files {
    FILE *in, *out;
};
static int64_t files_read(void *u, uint8_t *buf, uint64_t cap) { return file_read(((Files *)u)->in, buf, cap); }
static int files_write(void *u, const uint8_t *buf, uint64_t n) {
    return fwrite(buf, 1, (size_t)n, ((Files *)u)->out) == n ? 0 : -1;
}

static int do_compress(FILE *fin, FILE *fout, uint32_t block, int device) {
    // 256 MiB shards through the pipelined stream path: the next shard is read and the
    // previous one written while the GPU compresses (main()'s loop, 4073-4136)
    const uint64_t shard = (256ull << 20) / block * block;
    fcx_ctx *ctx = nullptr;
    if (fcx_ctx_create(&ctx, device, block, shard)) {
        fprintf(stderr, "fcx: %s\n", fcx_last_error());
        return -1;
    }
    uint8_t hdr[FCX_HEADER_BYTES];
    fcx_write_header(hdr, 0, 0);  // placeholder, rewritten at the end (4079-4086, 4128-4129)
    fwrite(hdr, 1, sizeof(hdr), fout);
    uint64_t total_in = 0, total_out = 0, nblocks = 0;
    Files io{fin, fout};
    auto t0 = std::chrono::steady_clock::now();
    const int r = fcx_compress_stream(ctx, files_read, files_write, &io, shard, &total_in, &total_out, &nblocks);
    if (r) {
        fprintf(stderr, "fcx: %s\n", fcx_last_error());
        fcx_ctx_destroy(ctx);
        return -1;
    }
    fcx_write_header(hdr, total_in, nblocks);
    fseek(fout, 0, SEEK_SET);
    fwrite(hdr, 1, sizeof(hdr), fout);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    printf("<Final>: LZ77 totalBytes = %llu, compress total bytes=%llu, compress rate: %.2f%%\n",
           (unsigned long long)total_in, (unsigned long long)total_out,
           total_in ? 100.0 * (double)total_out / (double)total_in : 0.0);
    printf("[***TIME***]  All block compress spend %.0f ms!!!\n", ms);
    if (nblocks > 65535) fprintf(stderr, "warning: %llu blocks exceed the u16 block count of the format\n",
                                 (unsigned long long)nblocks);
    fcx_ctx_destroy(ctx);
    return 0;
}

// -c lz77 over ngpus devices (fcx_dist_compress_host): the file in rounds of up to
// 1 GiB per GPU, each round's block ranges compressed in parallel and gathered to the
// first device over RCCL, records written in block order (4090-4122)
static int do_compress_dist(FILE *fin, FILE *fout, uint32_t block, int device, int ngpus) {
    std::vector<int> devs(ngpus);
    for (int i = 0; i < ngpus; i++) devs[i] = device + i;
    fcx_dist *d = nullptr;
    if (fcx_dist_init_local(&d, ngpus, devs.data())) {
        fprintf(stderr, "fcx: %s\n", fcx_last_error());
        return -1;
    }
    const uint64_t per = (1ull << 30) / block * block;
    std::vector<uint8_t> buf(per * (uint64_t)ngpus), out(fcx_shard_bound(buf.size(), block));
    uint8_t hdr[FCX_HEADER_BYTES];
    fcx_write_header(hdr, 0, 0);
    fwrite(hdr, 1, sizeof(hdr), fout);
    uint64_t total_in = 0, total_out = 0, nblocks = 0;
    auto t0 = std::chrono::steady_clock::now();
    int rc = 0;
    for (;;) {
        const size_t n = fread(buf.data(), 1, buf.size(), fin);
        if (n == 0) break;
        uint64_t got = 0;
        if (fcx_dist_compress_host(d, buf.data(), n, block, per, out.data(), out.size(), &got)) {
            fprintf(stderr, "fcx: %s\n", fcx_last_error());
            rc = -1;
            break;
        }
        fwrite(out.data(), 1, (size_t)got, fout);
        total_in += n;
        total_out += got;
        nblocks += (n + block - 1) / block;
    }
    fcx_dist_destroy(d);
    if (rc) return rc;
    fcx_write_header(hdr, total_in, nblocks);
    fseek(fout, 0, SEEK_SET);
    fwrite(hdr, 1, sizeof(hdr), fout);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    printf("<Final>: LZ77 totalBytes = %llu, compress total bytes=%llu, compress rate: %.2f%% (%d GPUs)\n",
           (unsigned long long)total_in, (unsigned long long)total_out,
           total_in ? 100.0 * (double)total_out / (double)total_in : 0.0, ngpus);
    printf("[***TIME***]  All block compress spend %.0f ms!!!\n", ms);
    if (nblocks > 65535) fprintf(stderr, "warning: %llu blocks exceed the u16 block count of the format\n",
                                 (unsigned long long)nblocks);
    return 0;
}

// the reference compares sizes only (4198-4201)
static int report(uint64_t got_total, uint32_t total) {
    const bool ok = (uint32_t)got_total == total;
    printf("All block decompress total bytes = %llu, Compress Before bytes = %u [%s]\n",
           (unsigned long long)got_total, total, ok ? "SUCCESS" : "FAIL");
    return ok ? 0 : 1;
}

// with --repair the size that counts is the sidecar's (its trailer was checked against what was written):
// the header's total is that of the bytes that were compressed, which an edited original need not match
static int report_repaired(uint64_t got_total) {
    printf("All block decompress total bytes = %llu, the repair sidecar's bytes = %llu [SUCCESS]\n",
           (unsigned long long)got_total, (unsigned long long)got_total);
    return 0;
}

// host decoder, used when no HIP device is present
static int decompress_host(FILE *fin, FILE *fout, uint32_t total, uint16_t nblocks) {
    uint64_t got_total = 0;
    const int r = fcx_cli::host_each_record(fin, nblocks, [&](uint32_t, uint32_t, const uint8_t *plain, uint64_t n) {
        fwrite(plain, 1, (size_t)n, fout);
        got_total += n;
        return true;
    });
    return r ? r : report(got_total, total);
}

// FCX8 (-c lz78): 256 MiB shards of whole blocks, each through the GPU codec
static int compress_lz78(FILE *fin, FILE *fout, uint32_t block) {
    const uint64_t shard = (256ull << 20) / block * block;
    std::vector<uint8_t> buf(shard), out;
    uint8_t hdr[FCX_HEADER_BYTES];
    memcpy(hdr, "FCX8", 4);
    memset(hdr + 4, 0, 6);
    fwrite(hdr, 1, sizeof(hdr), fout);   // placeholder, rewritten at the end (4079-4086)
    uint64_t total_in = 0, total_out = 0, nblocks = 0;
    auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        const size_t n = fread(buf.data(), 1, buf.size(), fin);
        if (n == 0) break;
        out.resize(FCX_HEADER_BYTES + 10 * n + 4096 * (n / block + 1));
        uint64_t got = 0;
        if (fcx_lz78_compress_host(buf.data(), n, block, out.data(), out.size(), &got)) {
            fprintf(stderr, "fcx: %s\n", fcx_last_error());
            return -1;
        }
        fwrite(out.data() + FCX_HEADER_BYTES, 1, got - FCX_HEADER_BYTES, fout);
        total_in += n;
        total_out += got - FCX_HEADER_BYTES;
        nblocks += (n + block - 1) / block;
    }
    const uint32_t t32 = (uint32_t)total_in;
    const uint16_t nb16 = (uint16_t)nblocks;
    memcpy(hdr + 4, &t32, 4);
    memcpy(hdr + 8, &nb16, 2);
    fseek(fout, 0, SEEK_SET);
    fwrite(hdr, 1, sizeof(hdr), fout);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    printf("<Final>: LZ78 totalBytes = %llu, compress total bytes=%llu, compress rate: %.2f%%\n",
           (unsigned long long)total_in, (unsigned long long)total_out,
           total_in ? 100.0 * (double)total_out / (double)total_in : 0.0);
    printf("[***TIME***]  All block compress spend %.0f ms!!!\n", ms);
    if (nblocks > 65535) fprintf(stderr, "warning: %llu blocks exceed the u16 block count of the format\n",
                                 (unsigned long long)nblocks);
    (void)fcx_lz78_release();   // the codec's cached device scratch
    return 0;
}

// what the decompress mode does: everything, a byte range of the decoded file, or the record list
struct Want {
    bool range = false, list = false;
    uint64_t off = 0, len = 0;
};

static int range_done(uint64_t n, uint64_t off) {
    printf("range decompress bytes = %llu (offset %llu)\n", (unsigned long long)n, (unsigned long long)off);
    return 0;
}

// --list on the GPU: the records in groups (as fcx_decompress_stream forms them: <= 256 records and
// <= 128 MiB), each indexed on the device by fcx_index_shard.  An FCX7 file is read to its end, of
// an FCX8 file the header's counted records.
static int list_gpu(FILE *fin, fcx_dctx *d, char kind, uint16_t counted) {
    constexpr uint32_t kGroup = 256;
    constexpr uint64_t kBytes = 128ull << 20;
    std::vector<uint8_t> buf;
    std::vector<uint64_t> rec(kGroup + 1), dec(kGroup + 1);
    uint8_t *d_in = nullptr;
    uint64_t *d_idx = nullptr, d_cap = 0;
    uint64_t left = kind == '7' ? UINT64_MAX : counted, k0 = 0, pos = 0, comp = 0;
    int rc = 0;
    if (hipMalloc((void **)&d_idx, 16 * (kGroup + 1)) != hipSuccess) return -1;
    bool eof = false;
    while (!eof && left && rc == 0) {
        buf.clear();
        uint32_t nb = 0;
        while (nb < kGroup && left && buf.size() < kBytes) {
            uint32_t sz = 0;
            const size_t g = fread(&sz, 1, 4, fin);
            if (g == 0 && kind == '7') { eof = true; break; }
            if (g != 4 || sz > 10ull * FCX_MAX_BLOCK_BYTES + 4096) { fprintf(stderr, "truncated block record\n"); rc = -1; break; }
            const size_t at = buf.size();
            buf.resize(at + 4 + sz);
            memcpy(buf.data() + at, &sz, 4);
            if (fread(buf.data() + at + 4, 1, sz, fin) != sz) { fprintf(stderr, "truncated block record\n"); rc = -1; break; }
            nb++;
            left--;
        }
        if (rc || nb == 0) break;
        if (buf.size() > d_cap) {
            (void)hipFree(d_in);
            d_in = nullptr;
            d_cap = buf.size();
            if (hipMalloc((void **)&d_in, d_cap) != hipSuccess) { fprintf(stderr, "fcx: hipMalloc failed\n"); rc = -1; break; }
        }
        uint64_t total = 0;
        if (hipMemcpy(d_in, buf.data(), buf.size(), hipMemcpyHostToDevice) != hipSuccess ||
            fcx_index_shard(d, kind, d_in, buf.size(), nb, d_idx, d_idx + kGroup + 1, &total, nullptr) != FCX_OK ||
            hipMemcpy(rec.data(), d_idx, 8 * (nb + 1), hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(dec.data(), d_idx + kGroup + 1, 8 * (nb + 1), hipMemcpyDeviceToHost) != hipSuccess) {
            fprintf(stderr, "fcx: %s\n", fcx_last_error());
            rc = -1;
            break;
        }
        for (uint32_t k = 0; k < nb; k++) {
            fcx_cli::list_line(k0 + k, rec[k + 1] - rec[k] - 4, dec[k + 1] - dec[k], pos + dec[k]);
            comp += rec[k + 1] - rec[k] - 4;
        }
        k0 += nb;
        pos += total;
    }
    (void)hipFree(d_in);
    (void)hipFree(d_idx);
    if (rc == 0) fcx_cli::list_totals(k0, comp, pos);
    return rc;
}

struct Differing {
    uint64_t block, len, dec;
    uint32_t first;
};
static void on_differing(void *u, uint64_t block, uint64_t len, uint64_t dec, uint32_t first) {
    ((std::vector<Differing> *)u)->push_back({block, len, dec, first});
}

// --compare, and the second half of --verify: the compressed file fcomp against the original, by
// fcx_verify_stream on the device, or for an FCX7 file without one by the host decoder
static int do_compare(FILE *fcomp, const char *orig_path, int device, uint32_t block) {
    FILE *forig = fopen(orig_path, "rb");
    if (!forig) { printf("open: %s Fail!!\n", orig_path); return -1; }
    uint8_t hdr[FCX_HEADER_BYTES];
    uint32_t total = 0;
    uint16_t nblocks = 0;
    char kind = 0;
    int r = -1;
    fcx_dctx *d = nullptr;
    if (fread(hdr, 1, sizeof(hdr), fcomp) != sizeof(hdr)) {
        fprintf(stderr, "Read file head infomation error!!!\n");
    } else if (fcx_parse_header(hdr, &total, &nblocks, &kind)) {
        fprintf(stderr, "This file is not support to decompress!!!!\n");
    } else if (fcx_dctx_create(&d, device) != FCX_OK) {
        if (kind != '7') {   // the FCX8 decoder is GPU-only
            fprintf(stderr, "fcx: %s\n", fcx_last_error());
        } else {
            fprintf(stderr, "fcx: %s; decoding on the host\n", fcx_last_error());
            r = fcx_cli::host_compare(fcomp, forig, nblocks, block, nullptr);
        }
    } else {
        uint64_t max_in = 0, stats[FCX_VERIFY_STATS];
        if (fseek(fcomp, 0, SEEK_END) == 0 && ftell(fcomp) > (long)FCX_HEADER_BYTES) max_in = (uint64_t)ftell(fcomp) - FCX_HEADER_BYTES;
        rewind(fcomp);
        std::vector<Differing> bad;
        const int v = fcx_verify_stream(d, file_read, fcomp, file_read, forig, block, max_in, on_differing, &bad, stats);
        fcx_dctx_destroy(d);
        if (v) {
            fprintf(stderr, "fcx: %s\n", fcx_last_error());
        } else {
            for (const Differing &b : bad) {
                if (b.block == stats[0]) fcx_cli::verify_extra(b.len);   // (bytes behind the last record)
                else fcx_cli::verify_line(b.block, b.dec, b.len, b.first);
            }
            r = fcx_cli::verify_totals(stats[1], stats[0], stats[4]);
        }
    }
    fclose(forig);
    return r;
}

// --repair with -c or --compare: the sidecar of the compressed file fcomp (at its start) against the
// original, by fcx_repair_build_stream on the device, or for an FCX7 file without one by the host decoder
static int do_repair_build(FILE *fcomp, const char *orig_path, int device, uint32_t block, const char *repair_path) {
    FILE *forig = fopen(orig_path, "rb");
    if (!forig) { printf("open: %s Fail!!\n", orig_path); return -1; }
    FILE *frep = fopen(repair_path, "wb");
    if (!frep) { printf("open: %s Fail!!\n", repair_path); fclose(forig); return -1; }
    uint8_t hdr[FCX_HEADER_BYTES];
    uint32_t total = 0;
    uint16_t nblocks = 0;
    char kind = 0;
    int r = -1;
    uint64_t stats[FCX_REPAIR_FILE_STATS] = {};
    fcx_dctx *d = nullptr;
    if (fread(hdr, 1, sizeof(hdr), fcomp) != sizeof(hdr)) {
        fprintf(stderr, "Read file head infomation error!!!\n");
    } else if (fcx_parse_header(hdr, &total, &nblocks, &kind)) {
        fprintf(stderr, "This file is not support to decompress!!!!\n");
    } else if (fcx_dctx_create(&d, device) != FCX_OK) {
        if (kind != '7') {   // the FCX8 decoder is GPU-only
            fprintf(stderr, "fcx: %s\n", fcx_last_error());
        } else {
            fprintf(stderr, "fcx: %s; decoding on the host\n", fcx_last_error());
            r = fcx_cli::host_repair_build(fcomp, forig, nblocks, block, frep, stats);
        }
    } else {
        uint64_t max_in = 0;
        if (fseek(fcomp, 0, SEEK_END) == 0 && ftell(fcomp) > (long)FCX_HEADER_BYTES) max_in = (uint64_t)ftell(fcomp) - FCX_HEADER_BYTES;
        rewind(fcomp);
        r = fcx_repair_build_stream(d, file_read, fcomp, file_read, forig, block, max_in, fcx_cli::stdio_write, frep, stats);
        fcx_dctx_destroy(d);
        if (r) {
            fprintf(stderr, "fcx: %s\n", fcx_last_error());
            r = -1;
        }
    }
    fclose(forig);
    if (fclose(frep) != 0 && r == 0) { fprintf(stderr, "write error\n"); r = -1; }
    if (r == 0) fcx_cli::repair_totals(stats[2], stats[3], stats[1]);
    return r;
}

// --digest with -c or --compare: the FCXD file of the original, by fcx_digest_stream on the device, or
// without one by the host CRC-32
static int do_digest_build(const char *orig_path, int device, uint32_t block, const char *digest_path) {
    FILE *forig = fopen(orig_path, "rb");
    if (!forig) { printf("open: %s Fail!!\n", orig_path); return -1; }
    FILE *fdig = fopen(digest_path, "wb");
    if (!fdig) { printf("open: %s Fail!!\n", digest_path); fclose(forig); return -1; }
    uint64_t stats[FCX_DIGEST_FILE_STATS] = {};
    fcx_dctx *d = nullptr;
    int r;
    if (fcx_dctx_create(&d, device) != FCX_OK) {
        fprintf(stderr, "fcx: %s; digesting on the host\n", fcx_last_error());
        r = fcx_cli::host_digest_build(forig, block, fdig, stats);
    } else {
        r = fcx_digest_stream(d, file_read, forig, block, fcx_cli::stdio_write, fdig, stats);
        fcx_dctx_destroy(d);
        if (r) {
            fprintf(stderr, "fcx: %s\n", fcx_last_error());
            r = -1;
        }
    }
    fclose(forig);
    if (fclose(fdig) != 0 && r == 0) { fprintf(stderr, "write error\n"); r = -1; }
    if (r == 0) fcx_cli::digest_totals(stats[1], (uint32_t)stats[2]);
    return r;
}

// --test, and the second pass of a decompress with --digest: the compressed file fcomp (and its repair
// frep, may be null) against the FCXD file, by fcx_check_stream on the device, or for an FCX7 file
// without one by the host decoder
static int do_check(FILE *fcomp, FILE *frep, const char *digest_path, int device) {
    FILE *fdig = fopen(digest_path, "rb");
    if (!fdig) { printf("open: %s Fail!!\n", digest_path); return -1; }
    std::vector<uint32_t> expected;
    if (fcx_cli::load_digest(fdig, &expected)) { fclose(fdig); return -1; }
    rewind(fcomp);
    if (frep) rewind(frep);
    uint8_t hdr[FCX_HEADER_BYTES];
    uint32_t total = 0;
    uint16_t nblocks = 0;
    char kind = 0;
    int r = -1;
    fcx_dctx *d = nullptr;
    if (fread(hdr, 1, sizeof(hdr), fcomp) != sizeof(hdr)) {
        fprintf(stderr, "Read file head infomation error!!!\n");
    } else if (fcx_parse_header(hdr, &total, &nblocks, &kind)) {
        fprintf(stderr, "This file is not support to decompress!!!!\n");
    } else if (fcx_dctx_create(&d, device) != FCX_OK) {
        if (kind != '7') {   // the FCX8 decoder is GPU-only
            fprintf(stderr, "fcx: %s\n", fcx_last_error());
        } else {
            fprintf(stderr, "fcx: %s; decoding on the host\n", fcx_last_error());
            r = fcx_cli::host_check(fcomp, frep, fdig, nblocks, nullptr);
        }
    } else {
        uint64_t max_in = 0, stats[FCX_VERIFY_STATS];
        if (fseek(fcomp, 0, SEEK_END) == 0 && ftell(fcomp) > (long)FCX_HEADER_BYTES) max_in = (uint64_t)ftell(fcomp) - FCX_HEADER_BYTES;
        rewind(fcomp);
        std::vector<Differing> bad;
        const int v = fcx_check_stream(d, file_read, fcomp, frep ? file_read : nullptr, frep, file_read, fdig, max_in, on_differing,
                                       &bad, stats);
        fcx_dctx_destroy(d);
        if (v) {
            fprintf(stderr, "fcx: %s\n", fcx_last_error());
        } else {
            for (const Differing &b : bad) {
                if (b.block == stats[0]) fcx_cli::check_extra(b.len);   // (blocks of the digest file behind the last record)
                else fcx_cli::check_line(b.block, b.dec, b.len, b.first, b.block < expected.size() ? &expected[b.block] : nullptr);
            }
            r = fcx_cli::check_totals(stats[1], stats[0], stats[4]);
        }
    }
    fclose(fdig);
    return r;
}

// ---- a cut behind a grep or --lines: the blocks, lines or line range come as they do without it, their
// cut comes through fcx_cut_ranges_host; without a device the host path's bytes go through the rule of fcx_cut.h ----
static int cli_fail(const char *msg) {
    fprintf(stderr, "fcx: %s\n", msg);
    return -1;
}
struct CutJob {
    const fcx_cut *host;   // the command line's own compilation of LIST
    std::string list;
};

// pass 2 under a cut option: the n ranges of the file at fin, cut, to fout (null: --count); *sum: the ranges' bytes
static int cut_ranges_out(const CutJob *job, fcx_dctx *d, FILE *fin, FILE *fout, const uint64_t *starts, const uint64_t *ends, uint64_t n, uint64_t *sum) {
    *sum = 0;
    for (uint64_t i = 0; i < n; i++) *sum += ends[i] - starts[i];
    std::vector<uint8_t> file;
    if (fseek(fin, 0, SEEK_END) != 0 || ftell(fin) < 0) return cli_fail("cannot size the input file");
    file.resize((size_t)ftell(fin));
    rewind(fin);
    if (fread(file.data(), 1, file.size(), fin) != file.size()) return cli_fail("cannot read the input file");
    const fcx_cut &h = *job->host;
    fcx_cut *cut = nullptr;
    int r = fcx_cut_create(&cut, job->list.data(), (uint32_t)job->list.size(), h.mode, h.sep, h.delim, h.flags);
    uint64_t need = 0, stats[FCX_CUT_STATS] = {};
    std::vector<uint8_t> out;
    if (r == FCX_OK) {   // one call: the cut is a subsequence of the ranges' bytes, so room for those always suffices
        if (fout) out.resize((size_t)*sum);
        r = fcx_cut_ranges_host(d, file.data(), file.size(), starts, ends, n, cut, fout && *sum ? out.data() : nullptr, fout ? *sum : 0, &need,
                                stats);
        if (r == FCX_ERR_CAPACITY && !fout) r = FCX_OK;   // (--count: the size query)
    }
    fcx_cut_destroy(cut);
    if (r) return r;
    if (fout && need && fwrite(out.data(), 1, (size_t)need, fout) != need) return cli_fail("write error");
    fcx_cli::cut_totals(stats);
    return FCX_OK;
}

// a no-device path under a cut option: what fn writes goes to memory, and from there through the rule to fout (null: --count)
template <typename Fn>
static int host_with_cut(const CutJob *job, FILE *fout, Fn fn) {
    if (!job) return fn(fout);
    char *buf = nullptr;
    size_t len = 0;
    FILE *mem = open_memstream(&buf, &len);
    if (!mem) return -1;
    int r = fn(mem);
    if (fclose(mem) != 0) r = -1;
    if (r == 0) {
        uint64_t stats[FCX_CUT_STATS] = {};
        uint32_t ticks = 0;
        std::string kept;
        fcx::cut_host_bytes(*job->host, (const uint8_t *)buf, len, &ticks, fout ? &kept : nullptr, stats);
        stats[5] = len ? 1 : 0;
        if (fout && !kept.empty() && fwrite(kept.data(), 1, kept.size(), fout) != kept.size()) {
            fprintf(stderr, "write error\n");
            r = -1;
        } else {
            fcx_cli::cut_totals(stats);
        }
    }
    free(buf);
    return r;
}

// --find / --find-hex: the pattern's offsets in the decoded file, by fcx_find_stream on the device, or for
// an FCX7 file without one by the host decoder
static int do_find(FILE *fin, int device, const std::vector<uint8_t> &pat, bool count_only) {
    uint8_t hdr[FCX_HEADER_BYTES];
    uint32_t total = 0;
    uint16_t nblocks = 0;
    char kind = 0;
    if (fread(hdr, 1, sizeof(hdr), fin) != sizeof(hdr)) {
        fprintf(stderr, "Read file head infomation error!!!\n");
        return -1;
    }
    if (fcx_parse_header(hdr, &total, &nblocks, &kind)) {
        fprintf(stderr, "This file is not support to decompress!!!!\n");
        return -1;
    }
    fcx_dctx *d = nullptr;
    if (fcx_dctx_create(&d, device) != FCX_OK) {
        if (kind != '7') {   // the FCX8 decoder is GPU-only
            fprintf(stderr, "fcx: %s\n", fcx_last_error());
            return -1;
        }
        fprintf(stderr, "fcx: %s; decoding on the host\n", fcx_last_error());
        return fcx_cli::host_find(fin, nblocks, pat.data(), (uint32_t)pat.size(), count_only, nullptr);
    }
    uint64_t max_in = 0, stats[4] = {};
    if (fseek(fin, 0, SEEK_END) == 0 && ftell(fin) > (long)FCX_HEADER_BYTES) max_in = (uint64_t)ftell(fin) - FCX_HEADER_BYTES;
    rewind(fin);
    const fcx_hit_fn line = [](void *, uint64_t off) { fcx_cli::find_line(off); };
    const int r = fcx_find_stream(d, file_read, fin, max_in, pat.data(), (uint32_t)pat.size(), count_only ? nullptr : line, nullptr,
                                  stats);
    fcx_dctx_destroy(d);
    if (r) {
        fprintf(stderr, "fcx: %s\n", fcx_last_error());
        return -1;
    }
    return fcx_cli::find_totals(stats[0], stats[1]);
}

// --find --line-numbers: the hits as do_find collects them, then a second pass over the file for the line each
// lies on (fcx_lines_of_stream), or for an FCX7 file without a device the host decoder in one pass
static int do_find_numbered(FILE *fin, int device, const std::vector<uint8_t> &pat, uint8_t delim) {
    uint8_t hdr[FCX_HEADER_BYTES];
    uint32_t total = 0;
    uint16_t nblocks = 0;
    char kind = 0;
    if (fread(hdr, 1, sizeof(hdr), fin) != sizeof(hdr)) {
        fprintf(stderr, "Read file head infomation error!!!\n");
        return -1;
    }
    if (fcx_parse_header(hdr, &total, &nblocks, &kind)) {
        fprintf(stderr, "This file is not support to decompress!!!!\n");
        return -1;
    }
    fcx_dctx *d = nullptr;
    if (fcx_dctx_create(&d, device) != FCX_OK) {
        if (kind != '7') {   // the FCX8 decoder is GPU-only
            fprintf(stderr, "fcx: %s\n", fcx_last_error());
            return -1;
        }
        fprintf(stderr, "fcx: %s; decoding on the host\n", fcx_last_error());
        return fcx_cli::host_find_numbered(fin, nblocks, pat.data(), (uint32_t)pat.size(), delim, nullptr);
    }
    uint64_t max_in = 0, stats[4] = {};
    if (fseek(fin, 0, SEEK_END) == 0 && ftell(fin) > (long)FCX_HEADER_BYTES) max_in = (uint64_t)ftell(fin) - FCX_HEADER_BYTES;
    rewind(fin);
    std::vector<uint64_t> hits;
    const fcx_hit_fn keep = [](void *u, uint64_t off) { ((std::vector<uint64_t> *)u)->push_back(off); };
    int r = fcx_find_stream(d, file_read, fin, max_in, pat.data(), (uint32_t)pat.size(), keep, &hits, stats);
    std::vector<uint64_t> lines(hits.size());
    if (r == FCX_OK && !hits.empty()) {
        rewind(fin);
        r = fcx_lines_of_stream(d, file_read, fin, max_in, delim, hits.data(), hits.size(), lines.data());
    }
    fcx_dctx_destroy(d);
    if (r) {
        fprintf(stderr, "fcx: %s\n", fcx_last_error());
        return -1;
    }
    for (size_t i = 0; i < hits.size(); i++) fcx_cli::find_line_numbered(hits[i], lines[i]);
    return fcx_cli::find_totals(stats[0], stats[1]);
}

// --count-lines (fout null) and --lines: fcx_lines_stream, or fcx_lines_locate_stream and then the range decode
// of what it found in a second pass; for an FCX7 file without a device the host decoder
static int do_lines(FILE *fin, FILE *fout, int device, uint8_t delim, uint64_t first, uint64_t count, const CutJob *job) {
    uint8_t hdr[FCX_HEADER_BYTES];
    uint32_t total = 0;
    uint16_t nblocks = 0;
    char kind = 0;
    if (fread(hdr, 1, sizeof(hdr), fin) != sizeof(hdr)) {
        fprintf(stderr, "Read file head infomation error!!!\n");
        return -1;
    }
    if (fcx_parse_header(hdr, &total, &nblocks, &kind)) {
        fprintf(stderr, "This file is not support to decompress!!!!\n");
        return -1;
    }
    fcx_dctx *d = nullptr;
    if (fcx_dctx_create(&d, device) != FCX_OK) {
        if (kind != '7') {   // the FCX8 decoder is GPU-only
            fprintf(stderr, "fcx: %s\n", fcx_last_error());
            return -1;
        }
        fprintf(stderr, "fcx: %s; decoding on the host\n", fcx_last_error());
        return host_with_cut(job, fout, [&](FILE *f) { return fcx_cli::host_lines(fin, nblocks, delim, f, first, count, nullptr); });
    }
    uint64_t max_in = 0, stats[FCX_LINES_STATS] = {}, off = 0, len = 0, got = 0;
    if (fseek(fin, 0, SEEK_END) == 0 && ftell(fin) > (long)FCX_HEADER_BYTES) max_in = (uint64_t)ftell(fin) - FCX_HEADER_BYTES;
    rewind(fin);
    int r;
    if (!fout && !job) {
        r = fcx_lines_stream(d, file_read, fin, max_in, delim, stats);
    } else {
        r = fcx_lines_locate_stream(d, file_read, fin, max_in, delim, first, count, &off, &len);
        if (r == FCX_OK && job) {
            const uint64_t end = off + len;
            r = cut_ranges_out(job, d, fin, fout, &off, &end, len ? 1 : 0, &got);
        } else if (r == FCX_OK && len) {
            rewind(fin);
            Files io{fin, fout};
            r = fcx_decompress_range_stream(d, files_read, files_write, &io, max_in, off, len, &got);
        }
    }
    fcx_dctx_destroy(d);
    if (r) {
        fprintf(stderr, "fcx: %s\n", fcx_last_error());
        return -1;
    }
    return fout || job ? fcx_cli::lines_done(got, off) : fcx_cli::lines_totals(stats[1], stats[0], stats[2]);
}

// --grep / --grep-hex: pass 1 collects the matching lines' byte ranges (fcx_grep_stream), pass 2 decodes them to
// fout (fcx_decompress_ranges_stream; fout null: --count, the totals alone); for an FCX7 file without a device the
// host decoder in one pass
static int do_grep(FILE *fin, FILE *fout, int device, const std::vector<uint8_t> &pat, uint8_t delim, const CutJob *job) {
    uint8_t hdr[FCX_HEADER_BYTES];
    uint32_t total = 0;
    uint16_t nblocks = 0;
    char kind = 0;
    if (fread(hdr, 1, sizeof(hdr), fin) != sizeof(hdr)) {
        fprintf(stderr, "Read file head infomation error!!!\n");
        return -1;
    }
    if (fcx_parse_header(hdr, &total, &nblocks, &kind)) {
        fprintf(stderr, "This file is not support to decompress!!!!\n");
        return -1;
    }
    fcx_dctx *d = nullptr;
    if (fcx_dctx_create(&d, device) != FCX_OK) {
        if (kind != '7') {   // the FCX8 decoder is GPU-only
            fprintf(stderr, "fcx: %s\n", fcx_last_error());
            return -1;
        }
        fprintf(stderr, "fcx: %s; decoding on the host\n", fcx_last_error());
        return host_with_cut(job, fout, [&](FILE *f) { return fcx_cli::host_grep(fin, nblocks, delim, pat.data(), (uint32_t)pat.size(), f, nullptr); });
    }
    uint64_t max_in = 0, stats[FCX_GREP_STATS] = {}, got = 0;
    if (fseek(fin, 0, SEEK_END) == 0 && ftell(fin) > (long)FCX_HEADER_BYTES) max_in = (uint64_t)ftell(fin) - FCX_HEADER_BYTES;
    rewind(fin);
    struct Lines {
        std::vector<uint64_t> starts, ends;
    } lines;
    const fcx_range_fn keep = [](void *u, uint64_t s, uint64_t e) {
        ((Lines *)u)->starts.push_back(s);
        ((Lines *)u)->ends.push_back(e);
    };
    int r = fcx_grep_stream(d, file_read, fin, max_in, delim, pat.data(), (uint32_t)pat.size(), (fout || job) ? keep : nullptr, &lines, stats);
    if (r == FCX_OK && (job || (fout && !lines.starts.empty()))) {
        rewind(fin);
        Files io{fin, fout};
        r = job ? cut_ranges_out(job, d, fin, fout, lines.starts.data(), lines.ends.data(), lines.starts.size(), &got)
                  : fcx_decompress_ranges_stream(d, files_read, files_write, &io, max_in, lines.starts.data(), lines.ends.data(),
                                                 lines.starts.size(), &got);
        if (r == FCX_OK && got != stats[1]) {
            fprintf(stderr, "fcx: the lines' bytes disagree with the grep's sum\n");
            fcx_dctx_destroy(d);
            return -1;
        }
    }
    fcx_dctx_destroy(d);
    if (r) {
        fprintf(stderr, "fcx: %s\n", fcx_last_error());
        return -1;
    }
    return fcx_cli::grep_totals(stats[0], stats[1], stats[2], stats[4]);
}

// --find-set, or --find with --ignore-case: do_find for a pattern set
// (set: the library's, through its public calls alone; host_set: the command line's own compilation of the same
// patterns for the no-device path, fcx_patset.h)
static int do_find_set(FILE *fin, int device, const fcx_pattern_set *set, const fcx_pattern_set &host_set, bool count_only) {
    uint8_t hdr[FCX_HEADER_BYTES];
    uint32_t total = 0;
    uint16_t nblocks = 0;
    char kind = 0;
    if (fread(hdr, 1, sizeof(hdr), fin) != sizeof(hdr)) {
        fprintf(stderr, "Read file head infomation error!!!\n");
        return -1;
    }
    if (fcx_parse_header(hdr, &total, &nblocks, &kind)) {
        fprintf(stderr, "This file is not support to decompress!!!!\n");
        return -1;
    }
    fcx_dctx *d = nullptr;
    if (fcx_dctx_create(&d, device) != FCX_OK) {
        if (kind != '7') {   // the FCX8 decoder is GPU-only
            fprintf(stderr, "fcx: %s\n", fcx_last_error());
            return -1;
        }
        fprintf(stderr, "fcx: %s; decoding on the host\n", fcx_last_error());
        return fcx_cli::host_find_set(fin, nblocks, host_set, count_only, nullptr, nullptr);
    }
    uint64_t max_in = 0, stats[4] = {};
    if (fseek(fin, 0, SEEK_END) == 0 && ftell(fin) > (long)FCX_HEADER_BYTES) max_in = (uint64_t)ftell(fin) - FCX_HEADER_BYTES;
    rewind(fin);
    const fcx_hit_fn line = [](void *, uint64_t off) { fcx_cli::find_line(off); };
    uint32_t npat = 0;
    int r = fcx_pattern_set_info(set, &npat, nullptr, nullptr, nullptr);
    if (r == FCX_OK) r = fcx_find_set_stream(d, file_read, fin, max_in, set, count_only ? nullptr : line, nullptr, stats, nullptr);
    fcx_dctx_destroy(d);
    if (r) {
        fprintf(stderr, "fcx: %s\n", fcx_last_error());
        return -1;
    }
    return fcx_cli::find_set_totals(stats[0], stats[1], npat);
}

// --grep-set, or --grep with --ignore-case: do_grep for a pattern set
static int do_grep_set(FILE *fin, FILE *fout, int device, const fcx_pattern_set *set, const fcx_pattern_set &host_set, uint8_t delim,
                       const CutJob *job) {
    uint8_t hdr[FCX_HEADER_BYTES];
    uint32_t total = 0;
    uint16_t nblocks = 0;
    char kind = 0;
    if (fread(hdr, 1, sizeof(hdr), fin) != sizeof(hdr)) {
        fprintf(stderr, "Read file head infomation error!!!\n");
        return -1;
    }
    if (fcx_parse_header(hdr, &total, &nblocks, &kind)) {
        fprintf(stderr, "This file is not support to decompress!!!!\n");
        return -1;
    }
    fcx_dctx *d = nullptr;
    if (fcx_dctx_create(&d, device) != FCX_OK) {
        if (kind != '7') {   // the FCX8 decoder is GPU-only
            fprintf(stderr, "fcx: %s\n", fcx_last_error());
            return -1;
        }
        fprintf(stderr, "fcx: %s; decoding on the host\n", fcx_last_error());
        return host_with_cut(job, fout, [&](FILE *f) { return fcx_cli::host_grep_set(fin, nblocks, delim, host_set, f, nullptr, nullptr); });
    }
    uint64_t max_in = 0, stats[FCX_GREP_STATS] = {}, got = 0;
    if (fseek(fin, 0, SEEK_END) == 0 && ftell(fin) > (long)FCX_HEADER_BYTES) max_in = (uint64_t)ftell(fin) - FCX_HEADER_BYTES;
    rewind(fin);
    struct Lines {
        std::vector<uint64_t> starts, ends;
    } lines;
    const fcx_range_fn keep = [](void *u, uint64_t s, uint64_t e) {
        ((Lines *)u)->starts.push_back(s);
        ((Lines *)u)->ends.push_back(e);
    };
    uint32_t npat = 0;
    int r = fcx_pattern_set_info(set, &npat, nullptr, nullptr, nullptr);
    if (r == FCX_OK) r = fcx_grep_set_stream(d, file_read, fin, max_in, delim, set, (fout || job) ? keep : nullptr, &lines, stats, nullptr);
    if (r == FCX_OK && (job || (fout && !lines.starts.empty()))) {
        rewind(fin);
        Files io{fin, fout};
        r = job ? cut_ranges_out(job, d, fin, fout, lines.starts.data(), lines.ends.data(), lines.starts.size(), &got)
                  : fcx_decompress_ranges_stream(d, files_read, files_write, &io, max_in, lines.starts.data(), lines.ends.data(),
                                                 lines.starts.size(), &got);
        if (r == FCX_OK && got != stats[1]) {
            fprintf(stderr, "fcx: the lines' bytes disagree with the grep's sum\n");
            fcx_dctx_destroy(d);
            return -1;
        }
    }
    fcx_dctx_destroy(d);
    if (r) {
        fprintf(stderr, "fcx: %s\n", fcx_last_error());
        return -1;
    }
    return fcx_cli::grep_set_totals(stats[0], stats[1], stats[2], stats[4], npat);
}

// --grep, --grep-hex or --grep-set with --invert, --before, --after or --context: the blocks of selected lines
struct BlockOut {
    FILE *in, *out;
    std::vector<uint64_t> starts, ends;
    const char *sep;       // what goes between two blocks ("": nothing)
    uint64_t at = 0;       // bytes of the blocks written so far
    uint64_t sum = 0;      // ... and up to the end of block k
    size_t k = 0;
};
static int64_t blocks_read(void *u, uint8_t *buf, uint64_t cap) { return file_read(((BlockOut *)u)->in, buf, cap); }
// the blocks' bytes arrive back to back: the separator goes in where one block ends and the next begins
static int blocks_write(void *u, const uint8_t *buf, uint64_t n) {
    BlockOut *b = (BlockOut *)u;
    while (n) {
        while (b->k < b->starts.size() && b->at == b->sum) {   // block k begins (empty blocks do not occur)
            if (b->k && fputs(b->sep, b->out) < 0) return -1;
            b->sum += b->ends[b->k] - b->starts[b->k];
            b->k++;
        }
        const uint64_t take = std::min<uint64_t>(n, b->sum - b->at);
        if (take == 0 || fwrite(buf, 1, (size_t)take, b->out) != take) return -1;
        buf += take;
        n -= take;
        b->at += take;
    }
    return 0;
}

static int do_grep_blocks(FILE *fin, FILE *fout, int device, const fcx_pattern_set *set, const fcx_pattern_set &host_set, uint8_t delim,
                          const fcx_grep_opts &opts, const CutJob *job) {
    uint8_t hdr[FCX_HEADER_BYTES];
    uint32_t total = 0;
    uint16_t nblocks = 0;
    char kind = 0;
    if (fread(hdr, 1, sizeof(hdr), fin) != sizeof(hdr)) {
        fprintf(stderr, "Read file head infomation error!!!\n");
        return -1;
    }
    if (fcx_parse_header(hdr, &total, &nblocks, &kind)) {
        fprintf(stderr, "This file is not support to decompress!!!!\n");
        return -1;
    }
    fcx_dctx *d = nullptr;
    if (fcx_dctx_create(&d, device) != FCX_OK) {
        if (kind != '7') {   // the FCX8 decoder is GPU-only
            fprintf(stderr, "fcx: %s\n", fcx_last_error());
            return -1;
        }
        fprintf(stderr, "fcx: %s; decoding on the host\n", fcx_last_error());
        return host_with_cut(job, fout, [&](FILE *f) { return fcx_cli::host_grep_blocks(fin, nblocks, delim, host_set, opts, f, nullptr, nullptr, !job); });
    }
    uint64_t max_in = 0, stats[FCX_GREP_BLOCK_STATS] = {}, got = 0;
    if (fseek(fin, 0, SEEK_END) == 0 && ftell(fin) > (long)FCX_HEADER_BYTES) max_in = (uint64_t)ftell(fin) - FCX_HEADER_BYTES;
    rewind(fin);
    BlockOut io{fin, fout, {}, {}, fcx_cli::block_separator(opts)};
    const fcx_block_fn keep = [](void *u, uint64_t s, uint64_t e, uint64_t, uint64_t) {
        ((BlockOut *)u)->starts.push_back(s);
        ((BlockOut *)u)->ends.push_back(e);
    };
    int r = fcx_grep_blocks_stream(d, file_read, fin, max_in, delim, set, &opts, (fout || job) ? keep : nullptr, &io, stats, nullptr);
    if (r == FCX_OK && (job || (fout && !io.starts.empty()))) {
        rewind(fin);
        r = job ? cut_ranges_out(job, d, fin, fout, io.starts.data(), io.ends.data(), io.starts.size(), &got)
                  : fcx_decompress_ranges_stream(d, blocks_read, blocks_write, &io, max_in, io.starts.data(), io.ends.data(),
                                                 io.starts.size(), &got);
        if (r == FCX_OK && got != stats[2]) {
            fprintf(stderr, "fcx: the blocks' bytes disagree with the grep's sum\n");
            fcx_dctx_destroy(d);
            return -1;
        }
    }
    fcx_dctx_destroy(d);
    if (r) {
        fprintf(stderr, "fcx: %s\n", fcx_last_error());
        return -1;
    }
    return fcx_cli::grep_blocks_totals(stats[0], stats[1], stats[3], stats[2], stats[4], stats[6]);
}

// --grep-regex: do_grep_blocks for a regex; without --invert, --before, --after or --context the totals are the set grep's
static int do_grep_regex(FILE *fin, FILE *fout, int device, const fcx_regex *re, const fcx_regex &host_re, const fcx_grep_opts &opts,
                         bool blocks_form, const CutJob *job) {
    uint8_t hdr[FCX_HEADER_BYTES];
    uint32_t total = 0;
    uint16_t nblocks = 0;
    char kind = 0;
    if (fread(hdr, 1, sizeof(hdr), fin) != sizeof(hdr)) {
        fprintf(stderr, "Read file head infomation error!!!\n");
        return -1;
    }
    if (fcx_parse_header(hdr, &total, &nblocks, &kind)) {
        fprintf(stderr, "This file is not support to decompress!!!!\n");
        return -1;
    }
    fcx_dctx *d = nullptr;
    if (fcx_dctx_create(&d, device) != FCX_OK) {
        if (kind != '7') {   // the FCX8 decoder is GPU-only
            fprintf(stderr, "fcx: %s\n", fcx_last_error());
            return -1;
        }
        fprintf(stderr, "fcx: %s; decoding on the host\n", fcx_last_error());
        return host_with_cut(job, fout, [&](FILE *f) { return fcx_cli::host_grep_regex(fin, nblocks, host_re, opts, blocks_form, f, nullptr, !job); });
    }
    uint64_t max_in = 0, stats[FCX_GREP_BLOCK_STATS] = {}, got = 0;
    if (fseek(fin, 0, SEEK_END) == 0 && ftell(fin) > (long)FCX_HEADER_BYTES) max_in = (uint64_t)ftell(fin) - FCX_HEADER_BYTES;
    rewind(fin);
    BlockOut io{fin, fout, {}, {}, fcx_cli::block_separator(opts)};
    const fcx_block_fn keep = [](void *u, uint64_t s, uint64_t e, uint64_t, uint64_t) {
        ((BlockOut *)u)->starts.push_back(s);
        ((BlockOut *)u)->ends.push_back(e);
    };
    int r = fcx_grep_regex_blocks_stream(d, file_read, fin, max_in, re, &opts, (fout || job) ? keep : nullptr, &io, stats);
    if (r == FCX_OK && (job || (fout && !io.starts.empty()))) {
        rewind(fin);
        r = job ? cut_ranges_out(job, d, fin, fout, io.starts.data(), io.ends.data(), io.starts.size(), &got)
                  : fcx_decompress_ranges_stream(d, blocks_read, blocks_write, &io, max_in, io.starts.data(), io.ends.data(),
                                                 io.starts.size(), &got);
        if (r == FCX_OK && got != stats[2]) {
            fprintf(stderr, "fcx: the blocks' bytes disagree with the grep's sum\n");
            fcx_dctx_destroy(d);
            return -1;
        }
    }
    fcx_dctx_destroy(d);
    if (r) {
        fprintf(stderr, "fcx: %s\n", fcx_last_error());
        return -1;
    }
    return blocks_form ? fcx_cli::grep_blocks_totals(stats[0], stats[1], stats[3], stats[2], stats[4], stats[6])
                       : fcx_cli::grep_set_totals(stats[1], stats[2], stats[4], stats[6], 1);
}

// --cut-fields / --cut-bytes: the whole file through fcx_cut_stream to fout (null: --count, the totals alone); for an
// FCX7 file without a device the host decoder.  host_cut: the command line's own compilation of LIST
static int do_cut(FILE *fin, FILE *fout, int device, const fcx_cut &host_cut, const std::string &list) {
    uint8_t hdr[FCX_HEADER_BYTES];
    uint32_t total = 0;
    uint16_t nblocks = 0;
    char kind = 0;
    if (fread(hdr, 1, sizeof(hdr), fin) != sizeof(hdr)) {
        fprintf(stderr, "Read file head infomation error!!!\n");
        return -1;
    }
    if (fcx_parse_header(hdr, &total, &nblocks, &kind)) {
        fprintf(stderr, "This file is not support to decompress!!!!\n");
        return -1;
    }
    fcx_dctx *d = nullptr;
    if (fcx_dctx_create(&d, device) != FCX_OK) {
        if (kind != '7') {   // the FCX8 decoder is GPU-only
            fprintf(stderr, "fcx: %s\n", fcx_last_error());
            return -1;
        }
        fprintf(stderr, "fcx: %s; decoding on the host\n", fcx_last_error());
        return fcx_cli::host_cut(fin, nblocks, host_cut, fout, nullptr);
    }
    uint64_t max_in = 0, stats[FCX_CUT_STATS] = {};
    if (fseek(fin, 0, SEEK_END) == 0 && ftell(fin) > (long)FCX_HEADER_BYTES) max_in = (uint64_t)ftell(fin) - FCX_HEADER_BYTES;
    rewind(fin);
    fcx_cut *cut = nullptr;
    int r = fcx_cut_create(&cut, list.data(), (uint32_t)list.size(), host_cut.mode, host_cut.sep, host_cut.delim, host_cut.flags);
    Files io{fin, fout};
    if (r == FCX_OK) r = fcx_cut_stream(d, files_read, fout ? files_write : nullptr, &io, max_in, cut, stats);
    fcx_cut_destroy(cut);
    fcx_dctx_destroy(d);
    if (r) {
        fprintf(stderr, "fcx: %s\n", fcx_last_error());
        return -1;
    }
    return fcx_cli::cut_totals(stats);
}

static int do_decompress(FILE *fin, FILE *fout, int device, const Want &want, FILE *frep) {
    uint8_t hdr[FCX_HEADER_BYTES];
    if (fread(hdr, 1, sizeof(hdr), fin) != sizeof(hdr)) {
        fprintf(stderr, "Read file head infomation error!!!\n");
        return -1;
    }
    uint32_t total = 0;
    uint16_t nblocks = 0;
    char kind = 0;
    if (fcx_parse_header(hdr, &total, &nblocks, &kind)) {
        fprintf(stderr, "This file is not support to decompress!!!!\n");
        return -1;
    }
    fcx_dctx *d = nullptr;
    if (fcx_dctx_create(&d, device) != FCX_OK) {
        if (kind != '7') {   // the FCX8 decoder is GPU-only
            fprintf(stderr, "fcx: %s\n", fcx_last_error());
            return -1;
        }
        fprintf(stderr, "fcx: %s; decoding on the host\n", fcx_last_error());
        if (want.list) return fcx_cli::host_list(fin, nblocks);
        if (want.range) {
            uint64_t n = 0;
            const int r = fcx_cli::host_range(fin, fout, nblocks, want.off, want.len, &n);
            return r ? r : range_done(n, want.off);
        }
        if (frep) {
            uint64_t n = 0;
            const int r = fcx_cli::host_repair_apply(fin, frep, fout, nblocks, &n);
            return r ? r : report_repaired(n);
        }
        return decompress_host(fin, fout, total, nblocks);
    }
    if (want.list) {
        const int r = list_gpu(fin, d, kind == '7' ? '7' : '8', nblocks);
        fcx_dctx_destroy(d);
        return r;
    }
    // GPU decoder over whole records, FCX7 and FCX8 alike (the stream path re-reads the header)
    rewind(fin);
    Files io{fin, fout};
    uint64_t got_total = 0, nrec = 0;
    uint32_t htotal = 0;
    if (want.range) {
        // the file's size bounds the staging: a small file does not pin a whole group's buffers
        uint64_t max_in = 0;
        if (fseek(fin, 0, SEEK_END) == 0 && ftell(fin) > (long)FCX_HEADER_BYTES) max_in = (uint64_t)ftell(fin) - FCX_HEADER_BYTES;
        rewind(fin);
        const int r = fcx_decompress_range_stream(d, files_read, files_write, &io, max_in, want.off, want.len, &got_total);
        fcx_dctx_destroy(d);
        if (r) {
            fprintf(stderr, "fcx: %s\n", fcx_last_error());
            return -1;
        }
        return range_done(got_total, want.off);
    }
    const int r = frep ? fcx_repair_apply_stream(d, file_read, fin, file_read, frep, fcx_cli::stdio_write, fout, 0, &got_total)
                       : fcx_decompress_stream(d, files_read, files_write, &io, 0, &htotal, &got_total, &nrec);
    fcx_dctx_destroy(d);
    if (r) {
        fprintf(stderr, "fcx: %s\n", fcx_last_error());
        return -1;
    }
    return frep ? report_repaired(got_total) : report(got_total, total);
}

int main(int argc, char **argv) {
    static struct option long_options[] = {{"file_in", required_argument, nullptr, 'i'},
                                           {"file_out", required_argument, nullptr, 'o'},
                                           {"compress", required_argument, nullptr, 'c'},
                                           {"block", required_argument, nullptr, 'b'},
                                           {"device", required_argument, nullptr, 'd'},
                                           {"gpus", required_argument, nullptr, 'g'},
                                           {"range", required_argument, nullptr, 'R'},
                                           {"list", no_argument, nullptr, 'L'},
                                           {"verify", no_argument, nullptr, 'V'},
                                           {"compare", required_argument, nullptr, 'C'},
                                           {"repair", required_argument, nullptr, 'P'},
                                           {"digest", required_argument, nullptr, 'D'},
                                           {"test", no_argument, nullptr, 'T'},
                                           {"find", required_argument, nullptr, 'F'},
                                           {"find-hex", required_argument, nullptr, 'X'},
                                           {"count", no_argument, nullptr, 'N'},
                                           {"count-lines", no_argument, nullptr, 'W'},
                                           {"lines", required_argument, nullptr, 'S'},
                                           {"line-numbers", no_argument, nullptr, 'K'},
                                           {"delim", required_argument, nullptr, 'M'},
                                           {"grep", required_argument, nullptr, 'G'},
                                           {"grep-hex", required_argument, nullptr, 'H'},
                                           {"find-set", required_argument, nullptr, 1001},
                                           {"grep-set", required_argument, nullptr, 1002},
                                           {"set-hex", no_argument, nullptr, 1003},
                                           {"ignore-case", no_argument, nullptr, 1004},
                                           {"invert", no_argument, nullptr, 1005},
                                           {"before", required_argument, nullptr, 1006},
                                           {"after", required_argument, nullptr, 1007},
                                           {"context", required_argument, nullptr, 1008},
                                           {"grep-regex", required_argument, nullptr, 1009},
                                           {"cut-fields", required_argument, nullptr, 1010},
                                           {"cut-bytes", required_argument, nullptr, 1011},
                                           {"sep", required_argument, nullptr, 1012},
                                           {"complement", no_argument, nullptr, 1013},
                                           {nullptr, 0, nullptr, 0}};
    std::string file_in, file_out = "./out";
    bool compress = false, lz77 = false;
    uint32_t block = FCX_DEFAULT_BLOCK_BYTES;
    int device = 0, ngpus = 1, opt;
    bool dist = false;   // -g given: the RCCL multi-GPU path (also at -g 1)
    bool verify = false, compare = false, test = false;
    std::string original, repair, digest;
    std::vector<uint8_t> pattern;
    int finds = 0;   // --find and --find-hex options seen
    std::vector<uint8_t> grep_pattern;
    int greps = 0;   // --grep and --grep-hex options seen
    bool count_only = false;
    bool count_lines = false, lines = false, line_numbers = false, delim_given = false;
    uint64_t line_first = 0, line_count = 0;
    uint8_t delim = 0x0A;
    std::string find_set, grep_set, grep_regex;
    bool regex_given = false;
    bool set_hex = false, ignore_case = false;
    fcx_grep_opts gopts = {0, 0, 0};
    bool blocks = false;   // --invert, --before, --after or --context seen
    std::string cut_list;
    int cuts = 0;          // --cut-fields and --cut-bytes options seen
    uint32_t cut_mode = 0;
    uint8_t sep = 0x09;
    bool sep_given = false, complement = false;
    Want want;
    if (argc < 3) return usage();
    while ((opt = getopt_long(argc, argv, "i:o:c:b:d:g:", long_options, nullptr)) != -1) {
        switch (opt) {
        case 'i': file_in = optarg; break;
        case 'o': file_out = optarg; break;
        case 'c':
            compress = true;
            lz77 = strncmp(optarg, "lz77", 4) == 0;  // any other value means LZ78 (4034-4038)
            break;
        case 'b': block = (uint32_t)strtoul(optarg, nullptr, 0); break;
        case 'd': device = atoi(optarg); break;
        case 'g': ngpus = atoi(optarg); dist = true; break;
        case 'R':
            if (!fcx_cli::parse_range(optarg, &want.off, &want.len)) return usage();
            want.range = true;
            break;
        case 'L': want.list = true; break;
        case 'V': verify = true; break;
        case 'C': compare = true; original = optarg; break;
        case 'P': repair = optarg; break;
        case 'D': digest = optarg; break;
        case 'T': test = true; break;
        case 'F':
            pattern.assign(optarg, optarg + strlen(optarg));
            if (pattern.empty() || pattern.size() > FCX_FIND_MAX_PATTERN) return usage();
            finds++;
            break;
        case 'X':
            if (!fcx_cli::parse_hex(optarg, &pattern)) return usage();
            finds++;
            break;
        case 'G':
            grep_pattern.assign(optarg, optarg + strlen(optarg));
            if (grep_pattern.empty() || grep_pattern.size() > FCX_FIND_MAX_PATTERN) return usage();
            greps++;
            break;
        case 'H':
            if (!fcx_cli::parse_hex(optarg, &grep_pattern)) return usage();
            greps++;
            break;
        case 'N': count_only = true; break;
        case 'W': count_lines = true; break;
        case 'S':
            if (!fcx_cli::parse_lines(optarg, &line_first, &line_count)) return usage();
            lines = true;
            break;
        case 'K': line_numbers = true; break;
        case 'M':
            if (!fcx_cli::parse_delim(optarg, &delim)) return usage();
            delim_given = true;
            break;
        case 1001: find_set = optarg; break;
        case 1002: grep_set = optarg; break;
        case 1003: set_hex = true; break;
        case 1004: ignore_case = true; break;
        case 1005:
            gopts.flags |= FCX_GREP_INVERT;
            blocks = true;
            break;
        case 1006:
        case 1007:
        case 1008: {
            uint32_t n = 0;
            if (!fcx_cli::parse_context(optarg, &n)) return usage();
            if (opt != 1007) gopts.before = n;
            if (opt != 1006) gopts.after = n;
            blocks = true;
            break;
        }
        case 1009:
            if (regex_given) return usage();
            grep_regex = optarg;
            regex_given = true;
            break;
        case 1010:
        case 1011:
            cut_list = optarg;
            cut_mode = opt == 1010 ? FCX_CUT_FIELDS : FCX_CUT_BYTES;
            cuts++;
            break;
        case 1012:
            if (!fcx_cli::parse_delim(optarg, &sep)) return usage();
            sep_given = true;
            break;
        case 1013: complement = true; break;
        default: return usage();
        }
    }
    if (file_in.empty() || ngpus < 1) return usage();
    // the cut: LIST is compiled here, by the command line's own copy of the compiler (the no-device path reads it)
    fcx_cut host_cut;
    if (cuts > 1 || ((sep_given || complement) && !cuts) || (sep_given && cut_mode == FCX_CUT_BYTES)) return usage();
    if (cuts) {
        if (compress || want.range || want.list || compare || verify || test || finds || !find_set.empty() || count_lines || line_numbers ||
            !repair.empty() || !digest.empty())
            return usage();
        const std::string why = fcx::cut_compile(&host_cut, cut_list.data(), (uint32_t)cut_list.size(), cut_mode, sep, delim,
                                                 complement ? FCX_CUT_COMPLEMENT : 0u);
        if (!why.empty()) {
            fprintf(stderr, "--cut-%s: %s\n", cut_mode == FCX_CUT_FIELDS ? "fields" : "bytes", why.c_str());
            return usage();
        }
    }
    CutJob cut_job{&host_cut, cut_list};
    // --grep-regex: a grep of its own kind; the expression is compiled once the delimiter is known
    std::unique_ptr<fcx_regex, void (*)(fcx_regex *)> regex_own(nullptr, fcx_regex_destroy);
    std::unique_ptr<fcx_regex> host_regex;
    if (regex_given) {
        if (finds || greps || !find_set.empty() || !grep_set.empty() || set_hex || line_numbers) return usage();
        host_regex.reset(new fcx_regex());
        const std::string why = fcx::regex_compile(host_regex.get(), (const uint8_t *)grep_regex.data(), (uint32_t)grep_regex.size(), delim,
                                                   ignore_case ? FCX_SET_FOLD_ASCII : 0u);
        if (!why.empty()) {
            fprintf(stderr, "--grep-regex: %s\n", why.c_str());
            return usage();
        }
        fcx_regex *re = nullptr;
        if (fcx_regex_create(&re, (const uint8_t *)grep_regex.data(), (uint32_t)grep_regex.size(), delim, ignore_case ? FCX_SET_FOLD_ASCII : 0u))
            return usage();
        regex_own.reset(re);
        greps++;
    }
    // the set options: a set file stands for --find or --grep in every rule below
    const bool set_file = !find_set.empty() || !grep_set.empty();
    if ((!find_set.empty() && !grep_set.empty()) || (set_file && (finds || greps)) || (set_hex && !set_file)) return usage();
    if (ignore_case && !(finds || greps || set_file)) return usage();
    if ((set_file || ignore_case) && line_numbers) return usage();
    if (blocks && !(greps || !grep_set.empty())) return usage();   // (the blocks run as a set, of one pattern if need be)
    // the library's set, destroyed when main returns, and the command line's own compilation of the same patterns:
    // the delimiter rule and the no-device path read that one, never the library's object
    std::unique_ptr<fcx_pattern_set, void (*)(fcx_pattern_set *)> pset_own(nullptr, fcx_pattern_set_destroy);
    std::unique_ptr<fcx_pattern_set> host_set;
    fcx_pattern_set *pset = nullptr;
    if (!regex_given && (set_file || ignore_case || blocks)) {
        std::vector<uint8_t> sbytes;
        std::vector<uint32_t> slens;
        if (set_file) {
            if (!fcx_cli::load_patterns((find_set.empty() ? grep_set : find_set).c_str(), set_hex, &sbytes, &slens)) return usage();
        } else {
            sbytes = finds ? pattern : grep_pattern;
            slens.push_back((uint32_t)sbytes.size());
        }
        const uint32_t sflags = ignore_case ? FCX_SET_FOLD_ASCII : 0u;
        host_set.reset(new fcx_pattern_set());
        if (fcx::patset_compile(host_set.get(), sbytes.data(), slens.data(), (uint32_t)slens.size(), sflags)) return usage();
        if (fcx_pattern_set_create(&pset, sbytes.data(), slens.data(), (uint32_t)slens.size(), sflags)) return usage();
        pset_own.reset(pset);
        finds += !find_set.empty();
        greps += !grep_set.empty();
        if (greps && (host_set->holds(delim) || (ignore_case && host_set->holds(fcx::fold_ascii(delim))))) return usage();
    }
    if ((want.range || want.list) && (compress || (want.range && want.list))) return usage();
    if ((compare && (compress || want.range || want.list || verify)) || (verify && !compress)) return usage();
    if (!repair.empty() && (want.range || want.list)) return usage();
    if (!digest.empty() && (want.range || want.list)) return usage();
    if (test && (digest.empty() || compress || compare || want.range || want.list)) return usage();
    if (finds > 1 || greps > 1 || (count_only && !finds && !greps && !cuts) || (cuts && greps && lines)) return usage();
    if (greps && (compress || want.range || want.list || compare || verify || test || finds || count_lines || lines || line_numbers ||
                  !repair.empty() || !digest.empty() || fcx_cli::pattern_holds(grep_pattern, delim)))
        return usage();
    if (finds && (compress || want.range || want.list || compare || verify || test || !repair.empty() || !digest.empty())) return usage();
    if ((count_lines || lines) && (compress || want.range || want.list || compare || verify || test || finds || !repair.empty() ||
                                   !digest.empty() || (count_lines && lines)))
        return usage();
    if (line_numbers && (!finds || count_only)) return usage();
    if (delim_given && !(count_lines || lines || line_numbers || greps || cuts)) return usage();
    if (block == 0 || block > FCX_MAX_BLOCK_BYTES) {
        fprintf(stderr, "block size must be in [1, %u]\n", FCX_MAX_BLOCK_BYTES);
        return -1;
    }
    FILE *fin = fopen(file_in.c_str(), "rb");
    if (!fin) { printf("open: %s Fail!!\n", file_in.c_str()); return -1; }
    // (--list, --compare, --test, --find, --count-lines and --grep --count write no file)
    const bool no_out = want.list || compare || test || finds || count_lines || ((greps || cuts) && count_only);
    FILE *fout = no_out ? nullptr : fopen(file_out.c_str(), "wb");
    if (!fout && !no_out) { printf("open: %s Fail!!\n", file_out.c_str()); fclose(fin); return -1; }
    if (!compress) (void)hipSetDevice(device);   // the FCX8 decoder runs on the current device
    if (compress && !lz77 && hipSetDevice(device) != hipSuccess) {
        fprintf(stderr, "fcx: no HIP device %d\n", device);
        return -1;
    }
    // behind a grep or --lines: those paths cut what they select, no `--` line between blocks
    const CutJob *job = cuts && (greps || lines) ? &cut_job : nullptr;
    if (finds) {
        const int r = pset           ? do_find_set(fin, device, pset, *host_set, count_only)
                      : line_numbers ? do_find_numbered(fin, device, pattern, delim)
                                     : do_find(fin, device, pattern, count_only);
        fclose(fin);
        return r;
    }
    if (greps) {
        const int r = regex_given ? do_grep_regex(fin, fout, device, regex_own.get(), *host_regex, gopts, blocks, job)
                      : blocks ? do_grep_blocks(fin, fout, device, pset, *host_set, delim, gopts, job)
                      : pset ? do_grep_set(fin, fout, device, pset, *host_set, delim, job)
                             : do_grep(fin, fout, device, grep_pattern, delim, job);
        fclose(fin);
        if (fout && fclose(fout) != 0) { fprintf(stderr, "write error\n"); return -1; }
        return r;
    }
    if (cuts && !job) {
        const int r = do_cut(fin, fout, device, host_cut, cut_list);
        fclose(fin);
        if (fout && fclose(fout) != 0) { fprintf(stderr, "write error\n"); return -1; }
        return r;
    }
    if (count_lines || lines) {
        const int r = do_lines(fin, fout, device, delim, line_first, line_count, job);
        fclose(fin);
        if (fout && fclose(fout) != 0) { fprintf(stderr, "write error\n"); return -1; }
        return r;
    }
    if (compare) {
        int r = do_compare(fin, original.c_str(), device, block);
        if (!repair.empty() && r >= 0) {   // the sidecar of the same pair, whatever the verdict
            rewind(fin);
            if (do_repair_build(fin, original.c_str(), device, block, repair.c_str())) r = -1;
        }
        if (!digest.empty() && r >= 0 && do_digest_build(original.c_str(), device, block, digest.c_str())) r = -1;
        fclose(fin);
        return r;
    }
    FILE *frep = nullptr;   // a decompress reads the sidecar
    if (!compress && !repair.empty() && !(frep = fopen(repair.c_str(), "rb"))) {
        printf("open: %s Fail!!\n", repair.c_str());
        return -1;
    }
    int r = compress ? (lz77 ? (dist ? do_compress_dist(fin, fout, block, device, ngpus)
                                     : do_compress(fin, fout, block, device))
                             : compress_lz78(fin, fout, block))
                     : test ? 0 : do_decompress(fin, fout, device, want, frep);
    if (!compress && !digest.empty() && r >= 0) {   // the test: alone, or the second pass over -i after the decompress
        if (fout) fflush(fout);
        const int v = do_check(fin, frep, digest.c_str(), device);
        if (v) r = v;   // (a decompress whose sizes differ keeps its status when the test could pass)
    }
    fclose(fin);
    if (fout) fclose(fout);
    if (frep) fclose(frep);
    if (verify && r == 0) {   // the finished output file against the input, whichever path wrote it
        FILE *fcomp = fopen(file_out.c_str(), "rb");
        if (!fcomp) { printf("open: %s Fail!!\n", file_out.c_str()); return -1; }
        (void)hipSetDevice(device);
        r = do_compare(fcomp, file_in.c_str(), device, block);
        fclose(fcomp);
    }
    if (compress && !repair.empty() && r >= 0) {   // the sidecar of the finished output file, whichever path wrote it
        FILE *fcomp = fopen(file_out.c_str(), "rb");
        if (!fcomp) { printf("open: %s Fail!!\n", file_out.c_str()); return -1; }
        (void)hipSetDevice(device);
        if (do_repair_build(fcomp, file_in.c_str(), device, block, repair.c_str())) r = -1;
        fclose(fcomp);
    }
    if (compress && !digest.empty() && r >= 0) {   // the digest of the input, after the passes above
        (void)hipSetDevice(device);
        if (do_digest_build(file_in.c_str(), device, block, digest.c_str())) r = -1;
    }
    return r;
}
