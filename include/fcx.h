/*
 * fcx.h — C ABI of the MI355X-native LZ77 + Huffman compressor (FCX7 format).
 *
 * The reference (YuBinRen/my_compress) has no plugin/FFI surface; its only seam
 * is the per-block function pair main() calls.  Each entry point below names
 * the reference interface it replaces (my_compress.cpp, lines counted by '\n'):
 *
 *   fcx_compress_block    <- uInt32 my_compress_file_lz77(void*, uInt32, uInt8*)   :2115 (called at :4099)
 *   fcx_decompress_block  <- uInt32 my_decompress_file_lz77(void*, uInt32, FILE*) :2255 (called at :4182)
 *   fcx_write_header      <- stCmpFileHead fwrite/rewrite in main()                :101-111, :4079-4086, :4128-4129
 *   fcx_parse_header      <- header read + "FCX" magic check in main()            :4140-4159
 *   fcx_compress_shard    <- main()'s per-block compress loop                      :4090-4122
 *                            (batched: every block of a device-resident shard in one
 *                             launch sequence, emitting [u32 len][payload]...)
 *   fcx_decompress_shard  <- main()'s per-block decompress loop, my_decompress_file_lz77
 *                            per record                                            :4160-4204, :2255
 *                            (GPU decoder: every record of a device-resident run)
 *   fcx_decompress_host   <- the whole decompress mode of main() on host buffers  :4137-4204
 *                            (FCX7 and FCX8: dispatch on the header's kind, :4140-4159)
 *   fcx_lz78_decompress_shard <- main()'s per-block decompress loop for FCX8,
 *                            my_decompress_file_lz78 per record                    :4160-4204, :3478
 *                            (GPU decoder: every record of a device-resident run)
 *   fcx_dist_*            <- main()'s compress loop (:4090-4122) with the blocks spread over
 *                            several GPUs: contiguous block ranges per GPU, the segments
 *                            concatenated in block order over RCCL (the reference writes the
 *                            blocks to one file in order, :4112-4114)
 *
 * Conventions: plain pointers and sizes, no exceptions cross the ABI, every
 * function returns FCX_OK (0) or a negative FCX_ERR_* code unless stated; the
 * message of the last error on the calling thread is fcx_last_error().  One
 * host thread per context; functions are reentrant across contexts.
 * The compress path is GPU-only: without a usable HIP device every compress
 * entry point fails with FCX_ERR_HIP (there is no CPU fallback).
 */
#ifndef FCX_H
#define FCX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FCX_OK 0
#define FCX_ERR_ARG (-1)       /* NULL pointer, zero/oversize block, bad value */
#define FCX_ERR_CAPACITY (-2)  /* output buffer too small */
#define FCX_ERR_HIP (-3)       /* HIP runtime error / no device */
#define FCX_ERR_FORMAT (-4)    /* malformed compressed stream */
#define FCX_ERR_INTERNAL (-5)  /* device-side invariant violated */
#define FCX_ERR_NOMEM (-6)
#define FCX_ERR_RCCL (-7)      /* RCCL (collective) error */

#define FCX_HEADER_BYTES 10u                 /* "FCX7" + u32 total + u16 blocks (:101-109) */
#define FCX_DEFAULT_BLOCK_BYTES (1u << 20)  /* BLOCK_BYTES (:113) */
#define FCX_MAX_BLOCK_BYTES (1u << 20)      /* reference decoder buffer limit (:2373) */

typedef struct fcx_ctx fcx_ctx;

/* ---- per-block drop-in (host buffers) ------------------------------------ */

/* Same contract as my_compress_file_lz77 (:2115): compresses `len` bytes at `in`
 * (len <= FCX_MAX_BLOCK_BYTES) and writes the block payload to `out`, which the
 * caller sizes at >= 2*len + 1024 (the reference allots 2 MiB per 1 MiB block,
 * :4088).  Returns payload bytes, or 0 if a pointer is NULL (:2122-2123) or on
 * error (see fcx_last_error).  len == 0 is a valid block, as in the reference: its
 * 17-byte payload (N = 0, pCnt = 0, HUFF of one zero byte, G = 0) is written without
 * touching the device.  Runs on the current HIP device through a lazily created
 * per-thread context. */
uint32_t fcx_compress_block(const void *in, uint32_t len, uint8_t *out);

/* Same contract as my_decompress_file_lz77 (:2255) but into memory: decodes one
 * block payload of `len` bytes into `out` (capacity `cap`).  Returns decoded
 * bytes, or a negative FCX_ERR_* code.  Host decoder. */
int64_t fcx_decompress_block(const uint8_t *in, uint32_t len, uint8_t *out, uint64_t cap);

/* ---- container -------------------------------------------------------------- */

/* writes the 10-byte header: "FCX7", u32 total_in mod 2^32, u16 nblocks mod 2^16 */
int fcx_write_header(uint8_t *out10, uint64_t total_in, uint64_t nblocks);
/* parses a header; kind receives '7' (LZ77) or '8' (LZ78); FCX_ERR_FORMAT if not "FCX" */
int fcx_parse_header(const uint8_t *in10, uint32_t *total_in, uint16_t *nblocks, char *kind);
/* worst-case bytes of fcx_compress_shard's output for n input bytes */
uint64_t fcx_shard_bound(uint64_t n, uint32_t block_bytes);

/* ---- batched device path ---------------------------------------------------- */

/* Creates a context on HIP device `device` for blocks of `block_bytes`
 * (1 <= block_bytes <= FCX_MAX_BLOCK_BYTES) and shards up to `max_shard_bytes`;
 * scratch grows on demand if a later call is larger. */
int fcx_ctx_create(fcx_ctx **ctx, int device, uint32_t block_bytes, uint64_t max_shard_bytes);
void fcx_ctx_destroy(fcx_ctx *ctx);

/* Compresses the n device-resident bytes at d_in as consecutive blocks of the
 * context's block size and writes, contiguously at d_out (device, capacity cap),
 * [u32 payload_len][payload] for every block in order (no file header).  Work
 * is enqueued on `stream` (a hipStream_t; NULL = default stream).  If out_len is
 * non-NULL the call synchronises the stream and stores the byte count there;
 * the count is always also left in device memory (fcx_ctx_device_out_len). */
int fcx_compress_shard(fcx_ctx *ctx, const uint8_t *d_in, uint64_t n, uint8_t *d_out, uint64_t cap,
                       uint64_t *out_len, void *stream);
/* device address of the u64 output length written by the last fcx_compress_shard */
const uint64_t *fcx_ctx_device_out_len(fcx_ctx *ctx);
/* waits for the device and reads that length (and the device error bits) */
int fcx_ctx_read_out_len(fcx_ctx *ctx, uint64_t *out_len);

/* Host-to-host convenience: compresses host memory in shards of the context's
 * shard size through the pipelined stream path below and writes the same
 * [u32 len][payload]... stream to host `out` (capacity cap). */
int fcx_compress_host(fcx_ctx *ctx, const uint8_t *in, uint64_t n, uint8_t *out, uint64_t cap,
                      uint64_t *out_len);
/* device, block size and shard capacity of a context (any pointer may be NULL) */
int fcx_ctx_info(fcx_ctx *ctx, int *device, uint32_t *block_bytes, uint64_t *shard_bytes);

/* ---- pipelined host I/O (main()'s read / code / write loop, :4073-4204) ----- */

/* read: fill up to cap bytes, return the count (0 = end of input) or < 0 on error;
 * write: consume n bytes, return 0 or < 0 on error */
typedef int64_t (*fcx_read_fn)(void *user, uint8_t *buf, uint64_t cap);
typedef int (*fcx_write_fn)(void *user, const uint8_t *buf, uint64_t n);

/* Streams input through the GPU in shards of shard_bytes (rounded down to whole
 * blocks): two pinned/device slots, H2D / compute / D2H on separate streams, the
 * next shard read and the previous shard's records written while the GPU
 * compresses.  Emits the [u32 len][payload]... records (no file header; the
 * caller writes it from *total_in and *nblocks). */
int fcx_compress_stream(fcx_ctx *ctx, fcx_read_fn read, fcx_write_fn write, void *user, uint64_t shard_bytes,
                        uint64_t *total_in, uint64_t *total_out, uint64_t *nblocks);

/* ---- introspection ---------------------------------------------------------- */

/* Enables per-kernel hipEvent timing of subsequent fcx_compress_shard calls. */
int fcx_ctx_set_profiling(fcx_ctx *ctx, int enable);
/* Testing: forces how the match search runs in later calls — 0 auto (default: every
 * tile goes to the match unit its own sampled bytes call for, fcx_ctx_route_stats), 1 the
 * general kernel with the bucket search for every tile (unknown positions via the run table /
 * the stitch), 2 the general kernel with the run table for whole tiles, 3 the general kernel,
 * 4 the 4-byte-key unit, 5 the unit without the repeat filter, 6 the unit with the run-mode
 * walk inlined, 7 the unit without the bucket search — modes 1-7 unrouted, every tile of the
 * call through that one kernel.  The output is identical in every mode; only the speed
 * differs. */
int fcx_ctx_set_match_mode(fcx_ctx *ctx, int mode);
/* After a profiled call: number of stages, and stage i's name and device ms. */
int fcx_ctx_stage_count(fcx_ctx *ctx);
int fcx_ctx_stage(fcx_ctx *ctx, int i, const char **name, float *ms);
/* statistics of the last call (device counters copied back on request):
 * tokens, matches, lazily evaluated positions, lazy tiles, total tiles */
int fcx_ctx_stats(fcx_ctx *ctx, uint64_t *tokens, uint64_t *matches, uint64_t *lazy_evals,
                  uint64_t *lazy_tiles, uint64_t *tiles);
/* The match kernel the last fcx_compress_shard call ran (routed: the unit given the most
 * tiles): 0 general, 1 4-byte keys (small alphabets), 2 without the repeat filter
 * (match-dense data), 3 run-mode walk inlined (long matches), 4 without the bucket search
 * (few matches), 5 the uniform unit (one byte value over the window); -1 for a NULL ctx. */
int fcx_ctx_match_kernel(fcx_ctx *ctx);
/* Routing of the last (routed) call, after a device synchronize: out[0..3] tiles filed to the
 * sparse, runs, 4-byte-key and no-filter units (the runs and no-filter counts include the tiles
 * handed on to them), out[4] tiles handed on (sparse / runs units to the no-filter unit, the
 * uniform unit to the runs unit), out[5] tiles with bytes, out[6] tiles past the units' grids
 * (searched by the units' looped remainder kernels), out[7] 1 when the call waited for its own
 * counts (a context's first call), out[8] tiles filed to the uniform unit (one byte value over
 * the window: closed form).  Writes min(n, FCX_ROUTE_STATS) values; FCX_ERR_ARG when the last
 * call had a forced unit (fcx_ctx_set_match_mode). */
#define FCX_ROUTE_STATS 9
int fcx_ctx_route_stats(fcx_ctx *ctx, uint64_t *out, int n);

/* ---- GPU decoder ------------------------------------------------------------ */

typedef struct fcx_dctx fcx_dctx;

/* Decoder context on HIP device `device`; scratch grows on demand. */
int fcx_dctx_create(fcx_dctx **ctx, int device);
void fcx_dctx_destroy(fcx_dctx *ctx);

/* Decodes `nblocks` consecutive block records ([u32 len][payload]..., an FCX7
 * file without its 10-byte header) of in_len device-resident bytes at d_in into
 * d_out (device, capacity cap), blocks back to back in order.  The bytes equal
 * the reference decoder's (my_decompress_file_lz77 :2255), including its
 * single-symbol sub-stream and early-stop behaviour.  Synchronises `stream` (a
 * hipStream_t; NULL = default) once after the header pass (to size scratch) and
 * once at the end; stores the decoded byte count in *out_len.  FCX_ERR_FORMAT
 * for malformed input, FCX_ERR_CAPACITY if cap is too small. */
int fcx_decompress_shard(fcx_dctx *ctx, const uint8_t *d_in, uint64_t in_len, uint32_t nblocks, uint8_t *d_out,
                         uint64_t cap, uint64_t *out_len, void *stream);
/* Host-to-host: a whole FCX7 or FCX8 file (header included) into `out` (capacity cap),
 * through fcx_decompress_stream. */
int fcx_decompress_host(fcx_dctx *ctx, const uint8_t *in, uint64_t in_len, uint8_t *out, uint64_t cap,
                        uint64_t *out_len);
/* Streams an FCX7 or FCX8 file (header first; the header's kind selects the decoder, as
 * main() does, :4140-4159) through the GPU decoder in groups of up to 256 whole records;
 * max_in (0 = unknown) bounds the staging buffers.  An FCX7 file is read to its end; of an
 * FCX8 file the header's counted records are read (main() reads block_num records), in
 * groups that also close when the next record (<= 10 len + 4096 bytes) would not fit the
 * 128 MiB staging.  Reports the header's total (mod 2^32), the decoded bytes and the records. */
int fcx_decompress_stream(fcx_dctx *ctx, fcx_read_fn read, fcx_write_fn write, void *user, uint64_t max_in,
                          uint32_t *hdr_total, uint64_t *total_out, uint64_t *nblocks);
int fcx_dctx_device(fcx_dctx *ctx, int *device);
/* per-stage hipEvent timing of subsequent fcx_decompress_shard / fcx_lz78_decompress_shard calls;
 * the stage functions report the last such call (FCX8: ms summed over its record batches) */
int fcx_dctx_set_profiling(fcx_dctx *ctx, int enable);
int fcx_dctx_stage_count(fcx_dctx *ctx);
int fcx_dctx_stage(fcx_dctx *ctx, int i, const char **name, float *ms);
/* Counters of the segment decoder (the Jacobi-synchronised symbol decode) for the last
 * fcx_decompress_shard call, read-only: writes min(n, FCX_DSYMBOL_STATS) values in this order:
 * Huffman settle rounds (summed over the sub-streams), Huffman sub-streams that took the serial
 * fallback, of those per kind (flags, chars, packed distances, Golomb bytes), Golomb settle
 * rounds, Golomb streams that took the serial fallback.  All zero when the call failed in its
 * header pass.  FCX_ERR_ARG for a NULL ctx or out, or n < 0. */
#define FCX_DSYMBOL_STATS 8
int fcx_dctx_symbol_stats(fcx_dctx *ctx, uint64_t *out, int n);

/* ---- -c lz78 (FCX8): the reference's second block codec ---------------------
 *   fcx_lz78_compress_block  <- uInt32 my_compress_file_lz78(void*, uInt32, uInt8*)  :3127 (called at :4106)
 *   fcx_lz78_compress_shard  <- main()'s per-block loop with -c lz78                 :4090-4122
 *   fcx_lz78_compress_host   <- the whole -c lz78 compress mode of main()            :4073-4136
 * Same record framing as FCX7 ([u32 len][payload] per block); the payload layout is
 * my_compress_file_lz78's.  GPU-only like the LZ77 path (FCX_ERR_HIP without a device).
 * Compress scratch (~40 B per input byte of a batch of <= 1 GiB) is kept per device
 * between calls; calls on one device are serialised; fcx_lz78_release() frees it. */
/* d_in / d_out device pointers; writes the records (no header) and their length. */
int fcx_lz78_compress_shard(const uint8_t *d_in, uint64_t n, uint32_t block_bytes, uint8_t *d_out, uint64_t cap,
                            uint64_t *out_len, void *stream);
/* host buffers; writes the "FCX8" header (total mod 2^32, u16 block count) + records. */
int fcx_lz78_compress_host(const uint8_t *in, uint64_t n, uint32_t block_bytes, uint8_t *out, uint64_t cap,
                           uint64_t *out_len);
/* frees the current device's LZ78 compress scratch */
int fcx_lz78_release(void);
/* one block: payload bytes (no length prefix), 0 on NULL / error; out >= 10*len + 4096. */
uint32_t fcx_lz78_compress_block(const void *in, uint32_t len, uint8_t *out);
/*   fcx_lz78_decompress_block <- my_decompress_file_lz78(void*, uInt32, FILE*)       :3478 (called at :4189)
 *   fcx_lz78_decompress_host  <- the whole decompress mode of main() for FCX8        :4137-4204
 * Both run the token-parallel GPU decoder below through a per-thread, lazily created fcx_dctx on
 * the current device; it keeps the reference's quirks (a block whose decoded bytes end in 0x00
 * loses that byte, 3701-3703; a one-symbol char stream decodes as zeros; symbols a stream runs
 * out of are 0).  decompress_block returns decoded bytes or a negative FCX_ERR_*;
 * decompress_host reads the header's counted records and ignores bytes after them. */
int64_t fcx_lz78_decompress_block(const uint8_t *in, uint32_t len, uint8_t *out, uint64_t cap);
int fcx_lz78_decompress_host(const uint8_t *in, uint64_t in_len, uint8_t *out, uint64_t cap, uint64_t *out_len);
/* FCX8 twin of fcx_decompress_shard: nblocks records ([u32 len][payload]..., the file
 * without its header) of in_len device bytes at d_in -> decoded blocks back to back at
 * d_out (device, capacity cap).  Bytes equal my_decompress_file_lz78's (:3478).  Runs on
 * `stream`; records are decoded in batches of fcx_lz78_decode_batch_records(), with scratch (in
 * the context, grown on demand) per token of the batch in flight, and the stream is synchronised
 * once per batch (to size that scratch) and at the end.  FCX_ERR_ARG for a NULL ctx, d_in, d_out
 * or out_len (before the device is touched); FCX_ERR_FORMAT "malformed record k" (1-based);
 * FCX_ERR_CAPACITY when the decoded bytes exceed cap.
 * The record named is the first one that fails the earliest stage that fails: the framing of the
 * whole run is checked first, then, batch after batch, the headers, the trees, the links and
 * sizes, and a stage is not run once an earlier one failed.  It is the first bad record of the
 * run unless a record before it in the same batch fails a later stage.
 * Domain: the streams the reference's encoder can write for a block of <= 1 MiB.  FCX_ERR_FORMAT
 * also for these streams, which the reference decoder would take: wcnt above 1 MiB + 10 used
 * indices; more than 4100 groups; N above 1 MiB + 8 tokens; a decoded size above 1 MiB + 8 bytes
 * counted before the tail-zero rule takes its byte (a parent chain deeper than 1447); a group code
 * of more than 32 bits; a group tree in which a node has two parents or none, the root is a child,
 * or a child id is >= 2G - 1, whether a code walks there or not; a char tree outside the domain of
 * fcx_decompress_shard (two parents, no parent, a child that does not precede its parent, a code
 * of more than 32 bits). */
int fcx_lz78_decompress_shard(fcx_dctx *ctx, const uint8_t *d_in, uint64_t in_len, uint32_t nblocks,
                              uint8_t *d_out, uint64_t cap, uint64_t *out_len, void *stream);
/* records per internal batch of fcx_lz78_decompress_shard */
uint32_t fcx_lz78_decode_batch_records(void);

/* ---- random access: decoded-size index and range decode (FCX7 and FCX8) -------------------
 * A record stores neither its decoded size nor its block size, and the decoded size is not the
 * encoder's block size: an incompressible FCX7 block may decode to 0 bytes (the early stop,
 * :2331-2335), an FCX8 block whose bytes end in 0x00 loses that byte (:3701-3703).  So byte x of
 * the decoded run is not in record x / block; the index below says where it is.
 *
 * The decoded bytes are the full decoders' bytes (fcx_decompress_shard, fcx_lz78_decompress_shard),
 * quirks and all: one-symbol sub-streams decode as zeros, the early stop, the tail-zero rule.  The
 * streams rejected are the full decoders' too, as far as a pass reads them:
 * the FCX7 size pass decodes the flags and the Golomb bytes only, so a bad chars or distance
 * *tree*, or a distance before the block start, is seen by the expansion of that record and not by
 * the index.  (The FCX8 size pass decodes every stream of a record: it sees all the expansion sees.)
 *
 * Error codes: FCX_ERR_ARG for a NULL ctx, d_in (with in_len > 0 or nblocks > 0) or out_len, a
 * kind other than '7' or '8', exactly one of the two index pointers NULL; FCX_ERR_CAPACITY when
 * cap < *out_len (*out_len is set); FCX_ERR_FORMAT for a malformed stream. */

/* Index of a device-resident run of nblocks records (kind '7' or '8'): two device arrays of
 * nblocks + 1 u64 each.  rec_off[k] = byte offset in d_in of record k's u32 length prefix,
 * rec_off[nblocks] = bytes the nblocks records span; dec_off[k] = decoded bytes of records
 * 0..k-1 (the bytes fcx_decompress_shard / fcx_lz78_decompress_shard would write before record k),
 * dec_off[nblocks] = the decoded total, also stored in *total when non-NULL.  Checks the framing,
 * the headers and the size-bearing streams of every record.  Synchronises `stream`. */
int fcx_index_shard(fcx_dctx *ctx, char kind, const uint8_t *d_in, uint64_t in_len, uint32_t nblocks,
                    uint64_t *d_rec_off, uint64_t *d_dec_off, uint64_t *total, void *stream);

/* pread on the decoded run: bytes [off, off + len) of what the full decode would produce, written
 * to d_out[0 ..).  *out_len = min(len, total - off), 0 when off >= total (not an error).  Nothing
 * past d_out[*out_len) is written.  Only the records the range touches are expanded (records of
 * decoded size 0 are skipped), and only the bytes inside the range are stored: there is no staging
 * copy of whole records.
 * d_rec_off / d_dec_off: an index from fcx_index_shard over the same run, or both NULL.
 *  - Both NULL: the call builds an index in the context's scratch first, which checks the framing,
 *    headers and size-bearing streams of *every* record of the run: a malformed record anywhere in
 *    the run fails the call.
 *  - An index given: only the records the call expands are read and checked.  A record outside
 *    the range may be arbitrarily damaged and the call still succeeds.
 * A given index is trusted for where things are, not for safety.  A touched record's rec_off must
 * point at a length prefix that fits in_len, the touched records must chain (each length prefix
 * leads to the next inside in_len), and each one's decoded size must equal dec_off[k + 1] -
 * dec_off[k]: otherwise FCX_ERR_FORMAT.  An index that disagrees with the run in a way these
 * checks do not see gives wrong bytes or FCX_ERR_FORMAT, never an access outside d_in[0, in_len),
 * the two index arrays or d_out[0, *out_len).  Synchronises `stream`. */
int fcx_decompress_range_shard(fcx_dctx *ctx, char kind, const uint8_t *d_in, uint64_t in_len, uint32_t nblocks,
                               const uint64_t *d_rec_off, const uint64_t *d_dec_off, uint64_t off, uint64_t len,
                               uint8_t *d_out, uint64_t cap, uint64_t *out_len, void *stream);

/* whole file (header + records) in host memory -> the range in host memory, through
 * fcx_decompress_range_stream */
int fcx_decompress_range_host(fcx_dctx *ctx, const uint8_t *in, uint64_t in_len, uint64_t off, uint64_t len,
                              uint8_t *out, uint64_t cap, uint64_t *out_len);

/* fcx_decompress_stream's twin: reads record groups as it does, indexes each group, decodes only the
 * part of the range that falls in the group and writes it, and stops reading once the range is
 * served (a range past the end reads the whole file and writes nothing).  Every record of the
 * groups read is checked as by fcx_index_shard.  *total_out = bytes written. */
int fcx_decompress_range_stream(fcx_dctx *ctx, fcx_read_fn read, fcx_write_fn write, void *user, uint64_t max_in,
                                uint64_t off, uint64_t len, uint64_t *total_out);

/* Counters of the last fcx_index_shard / fcx_decompress_range_shard call on the context (the host
 * and stream forms: of their last group), read-only, min(n, FCX_RANGE_STATS) values: records whose
 * sizes the size pass computed (0 when an index was given), records expanded, bytes stored to
 * d_out (counted by the kernels that store them), 1 if the call built its own index. */
#define FCX_RANGE_STATS 4
int fcx_dctx_range_stats(fcx_dctx *ctx, uint64_t *out, int n);

/* ---- round-trip verification: does each record decode back to its block? (FCX7 and FCX8) -----
 * The byte stream is the reference's, and the reference's decoder does not return every input:
 *  - a Huffman sub-stream with one distinct symbol stores no symbol identity and decodes as zeros
 *    (:930-984), so a block of one repeated byte value decodes to the right length of zeros;
 *  - an all-literal FCX7 block of 16 or more bytes has flag bytes that are all 0xFF, one distinct
 *    symbol: its flags decode as "all matches", and with pCnt = 0 the block stops at once and decodes
 *    to 0 bytes (the early stop, :2331-2335): an incompressible stretch of a file is lost;
 *  - an FCX8 block whose bytes end in 0x00 loses that byte (:3701-3703).
 * The decompress mode's own check compares total sizes only, modulo 2^32.  The calls below decode
 * the records with the full decoders and compare them, block by block, with what was compressed.
 *
 * What is compared: record k with original block k, the bytes [k B, min(n, (k + 1) B)) of the
 * original for the block size B the run was compressed with, wherever record k's bytes fall in the
 * decoded run.  Per record a pair of u32: the decoded byte count, and the first difference: the
 * smallest i < min(decoded, block length) at which the bytes differ; if there is none and the sizes
 * differ, min(decoded, block length); otherwise FCX_VERIFY_SAME.
 * stats[0 .. FCX_VERIFY_STATS): blocks, blocks that differ, the first differing block (UINT64_MAX if
 * none), blocks whose decoded size is not the block's length, original bytes lying in differing
 * blocks, decoded bytes in total.
 *
 * Return codes: FCX_OK whether or not blocks differ (the verdict is in the data); FCX_ERR_ARG for a
 * NULL ctx or stats, a kind other than '7' or '8', block_bytes outside [1, FCX_MAX_BLOCK_BYTES],
 * nblocks != ceil(n / block_bytes); FCX_ERR_FORMAT exactly where the full decoders give it. */
#define FCX_VERIFY_SAME 0xFFFFFFFFu
#define FCX_VERIFY_STATS 6

/* Verifies the nblocks records (no file header) of rec_len device bytes at d_rec against the n
 * device bytes at d_orig that were compressed in blocks of block_bytes.  d_blocks (device, 2 * nblocks
 * u32, or NULL) receives the pairs, stats (host) the summary.  The run is indexed
 * (fcx_index_shard), then decoded in groups of consecutive records whose decoded bytes fit a
 * buffer the context keeps (256 MiB by default, grown on demand; a record of no bytes counts as one
 * byte, a record larger than the bound is a group of its own), each group through fcx_decompress_shard / fcx_lz78_decompress_shard and then
 * compared.  Only d_blocks is written.  nblocks == 0 with n == 0 gives zero stats (the first
 * differing block UINT64_MAX) and touches no device memory.  Synchronises `stream`.  With
 * fcx_dctx_set_profiling the stage table of the call is index, decode, compare, summary. */
int fcx_verify_shard(fcx_dctx *ctx, char kind, const uint8_t *d_rec, uint64_t rec_len, uint32_t nblocks,
                     const uint8_t *d_orig, uint64_t n, uint32_t block_bytes, uint32_t *d_blocks, uint64_t *stats,
                     void *stream);
/* Host buffers: `rec` the records without the file header, `orig` what was compressed; blocks_host
 * (2 * nblocks u32) may be NULL.  Copies in and calls fcx_verify_shard. */
int fcx_verify_host(fcx_dctx *ctx, char kind, const uint8_t *rec, uint64_t rec_len, uint32_t nblocks,
                    const uint8_t *orig, uint64_t n, uint32_t block_bytes, uint32_t *blocks_host, uint64_t *stats);
/* one differing block: its number in the file, its length in the original, its decoded bytes, the
 * first difference */
typedef void (*fcx_verify_fn)(void *user, uint64_t block, uint64_t block_len, uint64_t decoded, uint32_t first_diff);
/* fcx_decompress_stream's twin: reads a whole FCX7 or FCX8 file (header first) from read_comp in the
 * same record groups (<= 256 records, <= 128 MiB; an FCX7 file to its end, of an FCX8 file the
 * counted records), for each group the matching records * block_bytes bytes of the original from
 * read_orig, and verifies the group.  on_block (may be NULL) is called for every differing block, in
 * order.  A record for which the original has no bytes left differs, with block length 0, whatever
 * it decodes to.  Original bytes left after the last record are reported too: they are added to
 * stats[4], and on_block is called once more, last, with block = stats[0] (the number of records),
 * their count as block_len, decoded 0 and first_diff 0.  So the file round-trips exactly when
 * stats[1] == 0 and stats[4] == 0.  Stats are summed over the groups; the first differing block is
 * numbered over the whole file. */
int fcx_verify_stream(fcx_dctx *ctx, fcx_read_fn read_comp, void *user_comp, fcx_read_fn read_orig, void *user_orig,
                      uint32_t block_bytes, uint64_t max_in, fcx_verify_fn on_block, void *user_cb, uint64_t *stats);
/* Testing: bound of a group's decoded bytes in later fcx_verify_* calls (0 = the default, 256 MiB),
 * so that small inputs cross group boundaries; and the groups the last fcx_verify_shard call made
 * (-1 for a NULL ctx).  The results do not depend on the bound. */
int fcx_dctx_set_verify_group(fcx_dctx *ctx, uint64_t bytes);
int fcx_dctx_verify_groups(fcx_dctx *ctx);

/* ---- repair sidecar: every FCX7 and FCX8 file decodes back to its input -----------------------
 * The records stay the reference's bytes, so what its decoder does not return (above) cannot be
 * mended inside them.  A repair is a second, small piece of data made from the records and the
 * original while both are at hand: one entry per block that does not come back, which says what to
 * keep of the decoded record and what to write behind it.  A decompress that is given the repair
 * returns the original exactly; without it nothing changes.
 *
 * Record k with (decoded bytes dlen, first difference fd) as fcx_verify_shard computes them and its
 * block of blen bytes: no entry when fd == FCX_VERIFY_SAME; otherwise one entry that keeps the decoded
 * prefix [0, from) with from = fd and writes len = blen - from bytes: FCX_REPAIR_FILL when those bytes
 * of the original are all one value (len <= 1 included; len == 0 only truncates), else FCX_REPAIR_RAW
 * with the bytes appended to the repair's data.  Always from <= min(dlen, blen).
 * The entry is the same 32 little-endian bytes on the device, in the FCXR file and in Python. */
typedef struct fcx_repair_entry {
    uint64_t block;     /* run-relative in the shard calls, file-wide in the file */
    uint64_t data_off;  /* RAW: offset of its bytes in the data (of the call / of its section); FILL: 0 */
    uint32_t from, len;
    uint32_t kind;      /* FCX_REPAIR_RAW or FCX_REPAIR_FILL */
    uint32_t fill;      /* low 8 bits; 0 for RAW */
} fcx_repair_entry;
#define FCX_REPAIR_RAW 0u
#define FCX_REPAIR_FILL 1u

/* Builds the repair of a device-resident run: fcx_verify_shard's index, decode and compare, then the
 * entries of the differing blocks in block order at d_entries (nblocks slots, or NULL) and the RAW
 * bytes back to back in entry order at d_data (capacity data_cap).  *nentries and *data_bytes are set
 * whenever the call gets as far as the plan (every return but FCX_ERR_ARG / FCX_ERR_FORMAT / a
 * HIP error).  data_cap < *data_bytes: FCX_ERR_CAPACITY, nothing is gathered, so d_data == NULL with
 * data_cap == 0 is the size query.  d_entries == NULL only together with d_data == NULL: the counts
 * alone.  stats (FCX_VERIFY_STATS values, may be NULL): fcx_verify_shard's.  Only d_entries[0,
 * *nentries) and d_data[0, *data_bytes) are written, and of the original only [d_orig, d_orig + n) is
 * read.  FCX_ERR_ARG as fcx_verify_shard.  The result does not depend on fcx_dctx_set_verify_group.
 * Stage table with profiling: index, decode, compare, summary, plan, gather. */
int fcx_repair_build_shard(fcx_dctx *ctx, char kind, const uint8_t *d_rec, uint64_t rec_len, uint32_t nblocks,
                           const uint8_t *d_orig, uint64_t n, uint32_t block_bytes, fcx_repair_entry *d_entries,
                           uint8_t *d_data, uint64_t data_cap, uint32_t *nentries, uint64_t *data_bytes, uint64_t *stats,
                           void *stream);
/* Decodes the run and applies the repair: the n original bytes, block k at d_out + k block_bytes.
 * The run is indexed, the entries are validated against it and every record without an entry is
 * checked, and only then is d_out written.  FCX_ERR_FORMAT, naming the first bad entry or else the first
 * bad record (numbered from 0), when an entry's block is >= nblocks or not strictly ascending, kind > 1,
 * from > the record's decoded bytes, from + len != the block's length, a RAW range lies outside
 * [0, data_bytes), or a record without an entry does not decode to its block's length.  cap < n:
 * FCX_ERR_CAPACITY with *out_len = n.  FCX_ERR_ARG as fcx_verify_shard (nblocks != ceil(n / block_bytes)
 * included).  With nentries == 0 the call is the index plus one full decode straight into d_out;
 * otherwise record groups are formed as fcx_verify_shard forms them: a group without entries decodes
 * straight to its place in d_out, a group with entries into the context's bounded buffer, from where
 * its blocks are assembled.  On an error d_out[0, n) is unspecified; d_out[n, cap) is never written.
 * What these checks cannot see: a repair made for another file whose entries happen to fit gives wrong
 * bytes.  The FCXR file's header and trailer (kind, block size, n, records) guard the file forms, and a
 * content digest (fcx_check_*, below) tells such a repair from the right one.
 * Stage table with profiling: index, check, decode, assemble. */
int fcx_repair_apply_shard(fcx_dctx *ctx, char kind, const uint8_t *d_rec, uint64_t rec_len, uint32_t nblocks, uint64_t n,
                           uint32_t block_bytes, const fcx_repair_entry *d_entries, uint32_t nentries,
                           const uint8_t *d_data, uint64_t data_bytes, uint8_t *d_out, uint64_t cap, uint64_t *out_len,
                           void *stream);
/* Counters of the last fcx_repair_build_shard / fcx_repair_apply_shard call on the context (the host
 * and stream forms: of their last group), min(n, FCX_REPAIR_STATS) values: entries, FILL entries, data
 * bytes, groups decoded straight into d_out, groups staged and assembled (both 0 after a build). */
#define FCX_REPAIR_STATS 5
int fcx_dctx_repair_stats(fcx_dctx *ctx, uint64_t *out, int n);

/* The FCXR file.  Header, 16 bytes: "FCXR", u8 version 1, u8 kind '7' / '8', u16 0, u32 block_bytes,
 * u32 0.  Sections: u32 nentries (1..256), u32 0, u64 data_bytes, the entries (block file-wide,
 * data_off into the section's data), the data.  Trailer: u32 0xFFFFFFFF, u32 0, u64 n, u64 records,
 * u64 entries, u64 data_bytes.  The writer is canonical: a section holds exactly the entries whose
 * block >> 8 is equal, everything ascends, the RAW bytes lie back to back in entry order; so the bytes
 * do not depend on how a path groups the records.  The reader takes any sectioning that ascends
 * strictly with 1..256 entries per section, and reads sections as the record groups need them. */
#define FCX_REPAIR_HEADER_BYTES 16u
#define FCX_REPAIR_TRAILER_BYTES 40u
#define FCX_REPAIR_FILE_STATS 4   /* the trailer: original bytes, records, entries, data bytes */
/* fcx_verify_stream's twin: reads the FCX7 / FCX8 file and the original in the same record groups and
 * writes the canonical FCXR file through write_repair.  Original bytes after the last record, or
 * records the original has no bytes for, are FCX_ERR_ARG: a repair cannot express them.
 * stats (FCX_REPAIR_FILE_STATS values, may be NULL): the trailer's. */
int fcx_repair_build_stream(fcx_dctx *ctx, fcx_read_fn read_comp, void *user_comp, fcx_read_fn read_orig, void *user_orig,
                            uint32_t block_bytes, uint64_t max_in, fcx_write_fn write_repair, void *user_repair,
                            uint64_t *stats);
/* fcx_decompress_stream's twin: reads the file in its record groups, for each group the sections of
 * the FCXR file that hold its entries, and writes the repaired bytes.  FCX_ERR_FORMAT for an FCXR file
 * of another kind than the FCX file's, a malformed one, a trailer that disagrees with the records read
 * or the bytes written, or a block shorter than the block size that is not the last record. */
int fcx_repair_apply_stream(fcx_dctx *ctx, fcx_read_fn read_comp, void *user_comp, fcx_read_fn read_repair,
                            void *user_repair, fcx_write_fn write_out, void *user_out, uint64_t max_in,
                            uint64_t *total_out);
/* on memory, through the stream forms: `in` a whole FCX7 / FCX8 file, `repair` a whole FCXR file */
int fcx_repair_build_host(fcx_dctx *ctx, const uint8_t *in, uint64_t in_len, const uint8_t *orig, uint64_t n,
                          uint32_t block_bytes, uint8_t *repair, uint64_t cap, uint64_t *repair_len);
int fcx_repair_apply_host(fcx_dctx *ctx, const uint8_t *in, uint64_t in_len, const uint8_t *repair, uint64_t repair_len,
                          uint8_t *out, uint64_t cap, uint64_t *out_len);

/* ---- content digests: one CRC-32 per block of the original, and a test that needs no original ----
 * The verification and the repair above read the original again.  A digest is what stays of it: the
 * CRC-32 (CRC-32/ISO-HDLC, zlib's crc32) of every block, made while the bytes are at hand.  With it the
 * records, and a repair if there is one, can be tested at any later time: does block k, decoded and
 * repaired, still have its length and its CRC-32?  The values are computed on the device; only compressed
 * bytes cross to it for a test, and no decoded byte leaves it. */

/* CRC-32 (zlib's) of every block of n device bytes cut at block_bytes: d_crc[0, ceil(n/B)); *whole (host,
 * may be NULL) = the CRC-32 of all n bytes.  n == 0: no block, *whole = 0, no device memory touched.
 * Only [d_data, d_data + n) is read.  With whole the call synchronises `stream`; without, the values are
 * ready when the stream's work is.  FCX_ERR_ARG for a NULL ctx, d_data or d_crc with n > 0, block_bytes
 * outside [1, FCX_MAX_BLOCK_BYTES], more than 2^31 - 1 blocks. */
int fcx_digest_shard(fcx_dctx *ctx, const uint8_t *d_data, uint64_t n, uint32_t block_bytes, uint32_t *d_crc,
                     uint32_t *whole, void *stream);

/* The same sum over nseg segments [d_off[k], d_off[k + 1]) of d_data (d_off: nseg + 1 ascending u64 on the
 * device; a segment starts at any byte and holds fewer than 2^32): d_crc[k], 0 for an empty segment.  Only
 * the bytes of the segments are read.  Reads the offsets back first (synchronises `stream`), then enqueues. */
int fcx_digest_segments(fcx_dctx *ctx, const uint8_t *d_data, const uint64_t *d_off, uint32_t nseg, uint32_t *d_crc,
                        void *stream);
/* The host mirror: zlib's crc32(crc, p, n) (start with 0; the sum continues) and crc32_combine, the CRC-32
 * of A | B from those of A and B and the length of B.  No device. */
uint32_t fcx_crc32(uint32_t crc, const uint8_t *p, uint64_t n);
uint32_t fcx_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b);

/* fcx_verify_shard with digests in place of the original.  Record k, decoded, and when an entry of the
 * given repair names block k, repaired as fcx_repair_apply_shard would, is block k.  It passes when its
 * length is the block's length (from n and block_bytes) and its CRC-32 equals d_crc[k].
 * d_blocks (2*nblocks u32 or NULL): the block's resulting length, its CRC-32.
 * stats[FCX_VERIFY_STATS]: blocks, failing blocks, first failing block (UINT64_MAX: none), blocks whose
 * length is wrong, original bytes in failing blocks, decoded bytes in total.
 * nentries == 0: no repair.  Entries are validated exactly as fcx_repair_apply_shard validates them
 * (same FCX_ERR_FORMAT texts).  But a record without an entry whose size is wrong is a failing block here,
 * not an error: that is what a test is for.  FCX_ERR_ARG / FCX_ERR_FORMAT otherwise as fcx_verify_shard.
 * The records are indexed and decoded in fcx_verify_shard's groups into the context's bounded buffer
 * (fcx_dctx_set_verify_group applies; the result does not depend on it); nothing is assembled: a repaired
 * block's CRC-32 is combined from that of its decoded prefix and that of its RAW bytes, or of its fill
 * byte, which is computed without memory.  Only d_blocks is written.  Synchronises `stream`.  Stage table
 * with profiling: index, decode, digest, summary. */
int fcx_check_shard(fcx_dctx *ctx, char kind, const uint8_t *d_rec, uint64_t rec_len, uint32_t nblocks, uint64_t n,
                    uint32_t block_bytes, const fcx_repair_entry *d_entries, uint32_t nentries,
                    const uint8_t *d_data, uint64_t data_bytes, const uint32_t *d_crc,
                    uint32_t *d_blocks, uint64_t *stats, void *stream);
/* Counters of the last fcx_digest_shard / fcx_check_shard call on the context (the host and stream forms:
 * of their last shard or group), min(n, FCX_DIGEST_STATS) values: segments digested, bytes digested (a
 * check: the decoded bytes and the repair's data, of which a repaired record's kept prefix is a part),
 * groups decoded, blocks repaired before digesting. */
#define FCX_DIGEST_STATS 4
int fcx_dctx_digest_stats(fcx_dctx *ctx, uint64_t *out, int n);
/* Testing and timing: the bytes a lane puts through the slicing tables per round in later digest and check
 * calls: 4 (the default, also for 0), 8 or 16, with as many 1 KiB tables in LDS.  The values are the same. */
int fcx_dctx_set_digest_slice(fcx_dctx *ctx, uint32_t bytes);

/* The FCXD file, all fields little endian.  Header, 16 bytes: "FCXD", u8 version 1, u8 0, u16 0, u32
 * block_bytes, u32 0.  Sections: u32 count (1..4096), u32 0, then count u32 CRC-32 values in block order;
 * a count of 0 (with its u32 0) ends the sections.  Trailer: u64 n, u64 blocks, u32 CRC-32 of the whole
 * original (what crc32, zip and zlib.crc32 give for it), u32 CRC-32 of the values as written.  The writer is
 * canonical: every section but the last holds exactly 4096 values.  The reader takes any sectioning within
 * 1..4096, needs no seek and holds one section at a time; FCX_ERR_FORMAT for a bad magic or version,
 * nonzero reserved fields, a count above 4096, truncation anywhere, a trailer whose n, blocks or CRCs
 * disagree with what was read, blocks != ceil(n / block_bytes), bytes behind the trailer. */
#define FCX_DIGEST_HEADER_BYTES 16u
#define FCX_DIGEST_TRAILER_BYTES 24u
#define FCX_DIGEST_SECTION 4096u
#define FCX_DIGEST_FILE_STATS 3   /* the trailer: original bytes, blocks, CRC-32 of the whole */
/* Reads the original to its end in shards of whole blocks, digests each on the device and writes the
 * canonical FCXD file.  stats (FCX_DIGEST_FILE_STATS values, may be NULL): the trailer's. */
int fcx_digest_stream(fcx_dctx *ctx, fcx_read_fn read_orig, void *user_orig, uint32_t block_bytes,
                      fcx_write_fn write_digest, void *user_digest, uint64_t *stats);
/* fcx_verify_stream's twin without the original: reads the FCX7 / FCX8 file in its record groups, for each
 * group the FCXD values of its blocks and, when read_repair is given, the FCXR sections that hold its
 * entries, and checks the group (fcx_check_shard).  on_block (may be NULL) is called for every failing
 * block in order with the block's number, its length by the digest file, its resulting length and, in the
 * place of the first difference, its CRC-32.  A record behind the digest file's last block fails, with
 * block length 0.  Blocks of the digest file behind the last record are reported as fcx_verify_stream
 * reports bytes behind the last record: their bytes are added to stats[4], and on_block is called once more,
 * last, with block = stats[0], their bytes as block_len, 0 and 0.  So the file passes exactly when
 * stats[1] == 0 and stats[4] == 0.  FCX_ERR_FORMAT for a malformed FCXD or FCXR file, an FCXR file of the
 * other codec or of another block size than the FCXD file's, or a trailer of either that disagrees. */
int fcx_check_stream(fcx_dctx *ctx, fcx_read_fn read_comp, void *user_comp, fcx_read_fn read_repair, void *user_repair,
                     fcx_read_fn read_digest, void *user_digest, uint64_t max_in, fcx_verify_fn on_block, void *user_cb,
                     uint64_t *stats);
/* on memory, through the stream forms: `orig` the original, `in` a whole FCX7 / FCX8 file, `repair` a whole
 * FCXR file or NULL, `digest` a whole FCXD file */
int fcx_digest_host(fcx_dctx *ctx, const uint8_t *orig, uint64_t n, uint32_t block_bytes, uint8_t *digest, uint64_t cap,
                    uint64_t *digest_len);
int fcx_check_host(fcx_dctx *ctx, const uint8_t *in, uint64_t in_len, const uint8_t *repair, uint64_t repair_len,
                   const uint8_t *digest, uint64_t digest_len, fcx_verify_fn on_block, void *user_cb, uint64_t *stats);

/* ---- search: where does a byte string occur in the decoded run? (FCX7 and FCX8) ----------------
 * The decoded run is what fcx_decompress_shard / fcx_lz78_decompress_shard write for the records, quirks
 * included: the bytes and the coordinates of the index and the range calls above.  A hit is an offset p
 * with decoded[p, p + plen) == pattern; overlapping occurrences all count; record and block boundaries do
 * not exist for the search, so a match may lie across any number of records.  Hits come in ascending
 * order.  The decoded bytes stay on the device: only the pattern goes to it and the hit offsets come
 * back.  A repair sidecar is not applied: the search is over the bytes the records decode to. */
#define FCX_FIND_MAX_PATTERN 256u
#define FCX_FIND_STATS 6
/* Searches the nblocks records (no file header) of rec_len device bytes at d_rec for the plen bytes at
 * pattern (host, 1 <= plen <= FCX_FIND_MAX_PATTERN).  *nhits is always the number of hits in the run;
 * d_hits[0, min(cap, *nhits)) (device) receives the first of them, ascending, and nothing else is
 * written; d_hits == NULL with cap == 0 is the count alone.  FCX_OK whether or not cap was reached.
 * nblocks == 0 gives *nhits = 0 and touches no device memory.  The run is indexed, then decoded in
 * fcx_verify_shard's groups into the context's bounded buffer (fcx_dctx_set_verify_group applies; the
 * result does not depend on it) and each group is scanned together with the last plen - 1 bytes before
 * it.  Synchronises `stream`.  FCX_ERR_ARG, before the device is touched, for a NULL ctx, pattern or
 * nhits, a NULL d_rec with nblocks > 0, a NULL d_hits with cap > 0, a kind other than '7' or '8', plen
 * outside [1, FCX_FIND_MAX_PATTERN]; FCX_ERR_FORMAT exactly where the index and the full decoders give
 * it.  Stage table with profiling: index, decode, scan, summary. */
int fcx_find_shard(fcx_dctx *ctx, char kind, const uint8_t *d_rec, uint64_t rec_len, uint32_t nblocks,
                   const uint8_t *pattern /* host */, uint32_t plen,
                   uint64_t *d_hits, uint64_t cap, uint64_t *nhits, void *stream);
typedef void (*fcx_hit_fn)(void *user, uint64_t offset);
/* fcx_decompress_stream's twin: reads the header, then the records in that function's groups, and
 * searches them as one run: a match that lies across two groups is found like any other.  on_hit (may
 * be NULL) is called for every hit of the file, in order, with file-wide offsets.  stats (4 values, may
 * be NULL): hits, decoded bytes, records, positions judged, summed over the file. */
int fcx_find_stream(fcx_dctx *ctx, fcx_read_fn read_comp, void *user_comp, uint64_t max_in,
                    const uint8_t *pattern, uint32_t plen, fcx_hit_fn on_hit, void *user_cb, uint64_t *stats);
/* a whole file (header + records) in host memory, through fcx_find_stream: *nhits the hits of the file,
 * hits[0, min(cap, *nhits)) (host, NULL with cap == 0: the count alone) the first of them */
int fcx_find_host(fcx_dctx *ctx, const uint8_t *in, uint64_t in_len, const uint8_t *pattern, uint32_t plen,
                  uint64_t *hits, uint64_t cap, uint64_t *nhits);
/* Counters of the last fcx_find_shard call on the context (the stream and host forms: of their last
 * group), min(n, FCX_FIND_STATS) values: start positions judged, positions that passed the prefix filter
 * (the first min(plen, 4) bytes), hits, groups decoded, carry bytes kept across group ends, write
 * windows run.  After a whole run positions judged = max(decoded bytes - plen + 1, 0): no position is
 * judged twice or skipped. */
int fcx_dctx_find_stats(fcx_dctx *ctx, uint64_t *out, int n);
/* Testing: hits per window of the stream form's hit buffer in later calls (0 = the default, 1 Mi); a
 * group with more hits is delivered in several windows.  The results do not depend on it. */
int fcx_dctx_set_find_window(fcx_dctx *ctx, uint32_t hits);

/* ---- lines: count, locate, decode and number the lines of the decoded run (FCX7 and FCX8) --------
 * D is the decoded run: what fcx_decompress_shard / fcx_lz78_decompress_shard write for the records,
 * quirks included; the bytes and coordinates of the index, the range and the search calls.  It has T
 * bytes.  A repair sidecar is not applied.  The delimiter d is one byte value chosen by the caller, any
 * of the 256 (the tools default to 0x0A).
 *   nl(x), 0 <= x <= T: the number of i < x with D[i] == d.
 *   Line j (0-based here and in Python) starts at s_j: s_0 = 0, s_j = 1 + the position of the j-th
 *   delimiter for 1 <= j <= nl(T).
 *   The number of lines is L = nl(T) + (T > 0 && D[T-1] != d): an unterminated tail is a line, T == 0 has none.
 *   Line j < L is D[s_j, e_j) with e_j = s_{j+1} when j < nl(T), else T: the delimiter belongs to the line it ends.
 *   The line of an offset x <= T is nl(x).
 * Record and block boundaries do not exist for lines.  The decoded bytes stay on the device.
 * Argument checks come before the device is touched and give FCX_ERR_ARG: a NULL ctx, a NULL output or
 * count pointer, a NULL d_rec with nblocks > 0, a kind other than '7' or '8', a partial set of index
 * pointers.  FCX_ERR_FORMAT exactly where the index and the full decoders give it.  The shard calls run
 * in fcx_verify_shard's groups through the context's bounded buffer (fcx_dctx_set_verify_group applies;
 * the results do not depend on it) and synchronise `stream`.  Stage table with profiling: index, decode,
 * count, summary. */
#define FCX_LINES_STATS 4
#define FCX_LINES_CALL_STATS 5
/* The line column of the index: d_line_off[k] = nl(dec_off[k]), the delimiters in the decoded bytes before
 * record k, d_line_off[nblocks] = nl(T); nblocks + 1 u64 on the device beside fcx_index_shard's rec_off /
 * dec_off, or NULL for the counts alone.  stats (host, FCX_LINES_STATS values): nl(T), L, T, the bytes
 * behind the last delimiter.  nblocks == 0 gives zeros and touches no device memory.  Nothing but
 * d_line_off is written. */
int fcx_lines_index_shard(fcx_dctx *ctx, char kind, const uint8_t *d_rec, uint64_t rec_len, uint32_t nblocks, uint8_t delim,
                          uint64_t *d_line_off, uint64_t *stats, void *stream);
/* The byte range of lines [first, first + count): *off = s_first, *len reaches to e of the last line
 * taken.  first + count saturates, so count = UINT64_MAX means "to the end"; first >= L gives *off = T,
 * *len = 0, not an error.  Pass all three index arrays (fcx_index_shard's and fcx_lines_index_shard's
 * for the same delimiter) or none of them.  With none the call indexes the run, counts group by group and
 * decodes no group behind the one that holds the second boundary.  With an index its arrays are copied
 * to the host (24 bytes per record), the records that hold the two boundary delimiters are found by
 * bisection on line_off, and only those, two at most, are decoded and scanned.  A given index is trusted
 * for where things are, not for safety (the rule of fcx_decompress_range_shard): FCX_ERR_FORMAT when it
 * does not ascend, when a touched record does not decode to dec_off[k+1] - dec_off[k] bytes or does not
 * hold the delimiters line_off promises, or when the arrays do not start at 0; never an access outside d_rec[0, rec_len), the arrays or the
 * context's buffer.  A damaged record the call does not touch does not fail it.  The call with an index
 * publishes no stage table (it has no index or group stage): fcx_dctx_stage_count is 0 after it. */
int fcx_lines_locate_shard(fcx_dctx *ctx, char kind, const uint8_t *d_rec, uint64_t rec_len, uint32_t nblocks, uint8_t delim,
                           const uint64_t *d_rec_off, const uint64_t *d_dec_off, const uint64_t *d_line_off,
                           uint64_t first, uint64_t count, uint64_t *off, uint64_t *len, void *stream);
/* The bytes of lines [first, first + count) to d_out: the locate above, then fcx_decompress_range_shard with
 * the same index, or the one the call built.  cap < their length: FCX_ERR_CAPACITY with *out_len set to it.
 * Nothing past d_out[*out_len) is written. */
int fcx_decompress_lines_shard(fcx_dctx *ctx, char kind, const uint8_t *d_rec, uint64_t rec_len, uint32_t nblocks,
                               uint8_t delim, const uint64_t *d_rec_off, const uint64_t *d_dec_off,
                               const uint64_t *d_line_off, uint64_t first, uint64_t count, uint8_t *d_out, uint64_t cap,
                               uint64_t *out_len, void *stream);
/* d_lines[i] = nl(d_offsets[i]) for noff non-decreasing decoded offsets <= T on the device, such as
 * fcx_find_shard's d_hits.  An offset above T or a descending pair is found on the device: FCX_ERR_ARG
 * naming the first bad index.  Only d_lines[0, noff) is written.  noff == 0 is FCX_OK and touches nothing. */
int fcx_lines_of_shard(fcx_dctx *ctx, char kind, const uint8_t *d_rec, uint64_t rec_len, uint32_t nblocks, uint8_t delim,
                       const uint64_t *d_offsets, uint64_t noff, uint64_t *d_lines, void *stream);
/* fcx_find_stream's twins: the file is read in that function's groups and treated as one run; a line that
 * spans two groups is handled like any other, the delimiters so far are carried from group to group.
 * fcx_lines_stream: the FCX_LINES_STATS values over the file (wc -l).
 * fcx_lines_locate_stream: one pass, file-wide *off / *len; reading stops once both boundaries are known
 * (a range that reaches the last line reads to the end, for T).
 * fcx_lines_of_stream: noff host offsets, ascending, to host line numbers; per group only the offsets
 * inside the group's decoded range go to the device; FCX_ERR_ARG naming the first bad index. */
int fcx_lines_stream(fcx_dctx *ctx, fcx_read_fn read_comp, void *user_comp, uint64_t max_in, uint8_t delim, uint64_t *stats);
int fcx_lines_locate_stream(fcx_dctx *ctx, fcx_read_fn read_comp, void *user_comp, uint64_t max_in, uint8_t delim,
                            uint64_t first, uint64_t count, uint64_t *off, uint64_t *len);
int fcx_lines_of_stream(fcx_dctx *ctx, fcx_read_fn read_comp, void *user_comp, uint64_t max_in, uint8_t delim,
                        const uint64_t *offsets, uint64_t noff, uint64_t *lines);
/* a whole file (header + records) in host memory, through the stream forms; fcx_decompress_lines_host is
 * fcx_lines_locate_stream over the memory, then fcx_decompress_range_host (cap < the length:
 * FCX_ERR_CAPACITY with *out_len set to it) */
int fcx_lines_host(fcx_dctx *ctx, const uint8_t *in, uint64_t in_len, uint8_t delim, uint64_t *stats);
int fcx_decompress_lines_host(fcx_dctx *ctx, const uint8_t *in, uint64_t in_len, uint8_t delim, uint64_t first,
                              uint64_t count, uint8_t *out, uint64_t cap, uint64_t *out_len);
int fcx_lines_of_host(fcx_dctx *ctx, const uint8_t *in, uint64_t in_len, uint8_t delim, const uint64_t *offsets,
                      uint64_t noff, uint64_t *lines);
/* Counters of the last line call on the context (the stream and host forms: of their last group),
 * min(n, FCX_LINES_CALL_STATS) values: bytes counted, records decoded, groups decoded, offsets ranked,
 * selects run.  After a whole-run index bytes counted == T: no byte is counted twice or skipped. */
int fcx_dctx_lines_stats(fcx_dctx *ctx, uint64_t *out, int n);

/* ---- grep: which lines of the decoded run hold a byte string, and a decode of many ranges (FCX7 and FCX8) ----
 * D, T, the delimiter d and the lines s_j / e_j are those of the line calls above, a hit is the search's: an
 * offset p with D[p, p + plen) == pattern.  A pattern that holds d is FCX_ERR_ARG (grep -F cannot express it
 * either), so every hit lies wholly inside one line.  Line j is selected iff some hit p has s_j <= p < e_j.
 * The result is the selected lines in ascending order, each exactly once however many hits it holds, as
 * (start = s_j, end = e_j): the delimiter belongs to the line it ends, an unterminated tail line ends at T, a
 * run without a delimiter is one line [0, T).  Record, block, tile and group boundaries do not exist for
 * this: a line may be longer than a record or a decode group, hold hits on both sides of any boundary and
 * span records that decode to no bytes.  A repair sidecar is not applied. */
#define FCX_GREP_STATS 5   /* lines, bytes (sum of end - start), hits, judged, decoded */
/* The selected lines of the nblocks records at d_rec: stats[0] (host, FCX_GREP_STATS values) is always their
 * number in the run, d_start / d_end[0, min(cap, stats[0])) (device, two separate arrays: d_start feeds
 * fcx_lines_of_shard, both feed fcx_decompress_ranges_shard) receive the first of them and nothing behind
 * is written; both NULL with cap == 0 is the count alone; FCX_OK whether or not cap was reached.  stats[3],
 * the start positions judged, is max(T - plen + 1, 0) after every call, stats[4] is T.  nblocks == 0 gives
 * zeros and touches no device.  The run is indexed, then decoded in fcx_verify_shard's groups into the
 * context's bounded buffer (fcx_dctx_set_verify_group applies; the result does not depend on it); each group
 * is scanned once together with the last plen - 1 bytes before it, and what goes from group to group is a
 * few words (the last delimiter, the last hit, the lines so far, whether the open line is selected), never
 * bytes of the open line.  Device scratch beyond the decoded group is two bitmaps of group bytes / 8 each
 * and 48 bytes per 4096 decoded bytes, whatever the number of hits or lines.  Synchronises `stream`.
 * FCX_ERR_ARG before the device is touched: a NULL ctx, pattern or stats, a NULL d_rec with nblocks > 0, a
 * NULL d_start or d_end with cap > 0, a kind other than '7' or '8', plen outside [1, FCX_FIND_MAX_PATTERN],
 * a pattern that holds delim; a decode group of 4 GiB or more is FCX_ERR_ARG as in fcx_find_shard.
 * Stage table with profiling: index, decode, scan, select, summary. */
int fcx_grep_shard(fcx_dctx *ctx, char kind, const uint8_t *d_rec, uint64_t rec_len, uint32_t nblocks, uint8_t delim,
                   const uint8_t *pattern /* host */, uint32_t plen, uint64_t *d_start, uint64_t *d_end, uint64_t cap,
                   uint64_t *stats, void *stream);
/* Device bytes the last fcx_grep_shard call on the context reserved beside the decoded group (the bitmaps and the
 * tile words of its largest group; 0 after a call without records).  After a fcx_grep_blocks_* call: those
 * and what the select stage reserved beside them (its bitmaps, tile words, ring and words). */
int fcx_dctx_grep_scratch(fcx_dctx *ctx, uint64_t *bytes);
/* Decodes nranges byte ranges [d_start[i], d_end[i]) of D (device arrays) in one call: d_out[0, sum) is the
 * concatenation of D[start_i, end_i) in order, *out_len is always the sum.  Rules: start_i <= end_i <= T and
 * end_i <= start_{i+1} (ascending and disjoint; empty and touching ranges are allowed).  They are checked on
 * the device before anything is stored: FCX_ERR_ARG naming the first range that breaks one.  sum > cap:
 * FCX_ERR_CAPACITY with nothing stored, so d_out == NULL with cap == 0 is the size query.  nranges == 0
 * stores nothing, decodes nothing and touches no device.  The ranges never visit the host: a device pass
 * scans their lengths into output offsets and leaves one flag per record that holds a byte of a range, and
 * only those nblocks flags come back.  Of each of fcx_verify_shard's groups only the touched records are
 * decoded, stretch by stretch, to their places in the context's bounded buffer (a group without one is
 * skipped), and the pieces of the ranges inside are copied to their output offsets.  Pass fcx_index_shard's arrays or NULL
 * for both (the call then indexes the run itself); a given index is trusted for where things are, not for
 * safety, as in fcx_decompress_range_shard: FCX_ERR_FORMAT when it does not start at 0, does not ascend or
 * leaves the run, or a decoded record has another size than it says.  With an index a damaged record that no
 * range touches does not fail the call.  FCX_ERR_ARG before the device is touched: a NULL ctx or out_len, a
 * NULL d_rec with nblocks > 0, NULL ranges with nranges > 0, a NULL d_out with cap > 0, half an index, a
 * kind other than '7' or '8'.  Synchronises `stream`.  Stage table with profiling: index, map, decode, gather. */
int fcx_decompress_ranges_shard(fcx_dctx *ctx, char kind, const uint8_t *d_rec, uint64_t rec_len, uint32_t nblocks,
                                const uint64_t *d_rec_off, const uint64_t *d_dec_off,
                                const uint64_t *d_start, const uint64_t *d_end, uint64_t nranges,
                                uint8_t *d_out, uint64_t cap, uint64_t *out_len, void *stream);
/* Counters of the last fcx_decompress_ranges_shard call on the context, min(n, FCX_RANGES_STATS) values:
 * ranges, bytes stored, records touched, records decoded, groups decoded. */
#define FCX_RANGES_STATS 5
int fcx_dctx_ranges_stats(fcx_dctx *ctx, uint64_t *out, int n);
/* A whole file (header + records) in host memory.  fcx_grep_host: the bytes of the selected lines to out (grep
 * -F): the records go to the device once, fcx_grep_shard's arrays feed fcx_decompress_ranges_shard there, and
 * only the lines' bytes come back; *out_len is always their number, cap < *out_len is FCX_ERR_CAPACITY, out ==
 * NULL with cap == 0 the size query; stats (FCX_GREP_STATS values, may be NULL).  fcx_decompress_ranges_host:
 * nranges host ranges under fcx_decompress_ranges_shard's rules. */
int fcx_grep_host(fcx_dctx *ctx, const uint8_t *in, uint64_t in_len, uint8_t delim, const uint8_t *pattern, uint32_t plen,
                  uint8_t *out, uint64_t cap, uint64_t *out_len, uint64_t *stats);
typedef void (*fcx_range_fn)(void *user, uint64_t start, uint64_t end);
/* fcx_find_stream's twin: reads the header, then the records in that function's groups of 256, and treats the
 * file as one run: the words above and the decoded base go from group to group, so a line across two stream
 * groups with a hit on either side is one line.  on_line (may be NULL: the totals alone) is called for every
 * selected line of the file once, in order, with its file-wide start and its true end: a selected line still
 * open at a stream group's end is held back (two words) until a later group closes it or the file ends.  The
 * lines come to the host by windows of fcx_dctx_set_find_window lines.  stats (FCX_GREP_STATS values, may be
 * NULL) over the file.  Argument checks as fcx_grep_shard, before anything is read. */
int fcx_grep_stream(fcx_dctx *ctx, fcx_read_fn read_comp, void *user_comp, uint64_t max_in, uint8_t delim,
                    const uint8_t *pattern, uint32_t plen, fcx_range_fn on_line, void *user_line, uint64_t *stats);
/* fcx_decompress_range_stream's twin for many ranges: n host ranges under fcx_decompress_ranges_shard's rules,
 * checked on the host before anything is read (FCX_ERR_ARG naming the first that descends, overlaps or has end <
 * start).  Each stream group is indexed, gets the slice of the ranges that meets its decoded bytes, clipped to
 * them, gathers it on the device and writes it; a range across groups is written in pieces.  Reading stops
 * behind the group that holds the last range's end.  A range that ends behind the file's end is FCX_ERR_ARG once
 * the end is reached; what lay inside the file has been written by then.  *out_len (may be NULL): bytes written. */
int fcx_decompress_ranges_stream(fcx_dctx *ctx, fcx_read_fn read_comp, fcx_write_fn write_out, void *user, uint64_t max_in,
                                 const uint64_t *starts, const uint64_t *ends, uint64_t n, uint64_t *out_len);
int fcx_decompress_ranges_host(fcx_dctx *ctx, const uint8_t *in, uint64_t in_len, const uint64_t *starts, const uint64_t *ends,
                               uint64_t nranges, uint8_t *out, uint64_t cap, uint64_t *out_len);

/* ---- pattern sets: many patterns and ASCII case folding in one scan (FCX7 and FCX8) -------------------------
 * D, T, the delimiter d and the lines s_j / e_j are those of the search, the line calls and the grep above.
 * A set holds npat patterns pat_k of len_k bytes.  fold(b) = b + 0x20 for 0x41 <= b <= 0x5A and b otherwise
 * with FCX_SET_FOLD_ASCII (bytes >= 0x80 are never folded), the identity without it.  Pattern k occurs at p iff
 * p + len_k <= T and fold(D[p + i]) == fold(pat_k[i]) for all i < len_k.  A hit is a position p at which at
 * least one pattern occurs; hits are reported ascending, each position once however many patterns occur
 * there.  counts[k] (host, npat values, may be NULL) is the number of positions at which pattern k occurs,
 * over the whole run whatever cap is, so sum(counts) >= hits; duplicates and prefixes of one another are
 * allowed and each counts for itself.  Positions judged after a whole run = max(T - min_len + 1, 0): no
 * position is judged twice or skipped.  Grep: line j is selected iff a hit p has s_j <= p < e_j; a pattern
 * that holds d, or with the flag a folded pattern that holds fold(d), is FCX_ERR_ARG (`a` against the
 * delimiter `A` would match across a line end).  A set of one pattern without the flag gives exactly
 * fcx_find_shard's and fcx_grep_shard's hits, lines and judged positions.
 * How a run is scanned: every record group is scanned behind the last min(max_len - 1, bytes seen) bytes; a
 * group that is not the run's last judges the positions p with p + max_len <= group end against all
 * patterns, the last max_len - 1 positions wait for the next group, and at the run's end they are judged
 * with pattern k admitted iff p + len_k <= T (the stream forms: a final pass over the carry alone once the
 * reader has ended). */
#define FCX_SET_MAX_PATTERNS 64u
#define FCX_SET_MAX_BYTES    4096u      /* sum of the lengths */
#define FCX_SET_FOLD_ASCII   1u         /* flags */
#define FCX_SET_SCAN_STATS   6          /* judged, candidate positions, full compares, hits, groups, final passes */
typedef struct fcx_pattern_set fcx_pattern_set;
/* Compiles npat patterns (bytes: their concatenation, lens[k] in [1, FCX_FIND_MAX_PATTERN], npat in
 * [1, FCX_SET_MAX_PATTERNS], sum of the lengths <= FCX_SET_MAX_BYTES) into what the scan kernel reads: the
 * folded pattern bytes padded to dwords, their offsets and lengths, the two filter tables.  Pure host code:
 * no device is touched.  FCX_ERR_ARG for NULL arguments, npat, a length or the sum out of range, unknown
 * flag bits. */
int fcx_pattern_set_create(fcx_pattern_set **set, const uint8_t *bytes, const uint32_t *lens, uint32_t npat, uint32_t flags);
void fcx_pattern_set_destroy(fcx_pattern_set *set);
/* any of the outputs may be NULL */
int fcx_pattern_set_info(const fcx_pattern_set *set, uint32_t *npat, uint32_t *min_len, uint32_t *max_len, uint32_t *flags);
/* fcx_find_shard / fcx_find_stream / fcx_find_host for a set: the same arguments, checks, cap rule, windows
 * (fcx_dctx_set_find_window) and stage table, with `set` in the place of (pattern, plen) and counts behind
 * nhits / stats.  nblocks == 0 gives zeros and touches no device.  Scratch is the search's own plus the set's
 * device copy (8.7 KB) and 64 counters: it does not grow with hits or patterns. */
int fcx_find_set_shard(fcx_dctx *ctx, char kind, const uint8_t *d_rec, uint64_t rec_len, uint32_t nblocks,
                       const fcx_pattern_set *set, uint64_t *d_hits, uint64_t cap, uint64_t *nhits, uint64_t *counts,
                       void *stream);
int fcx_find_set_stream(fcx_dctx *ctx, fcx_read_fn read_comp, void *user_comp, uint64_t max_in, const fcx_pattern_set *set,
                        fcx_hit_fn on_hit, void *user_cb, uint64_t *stats, uint64_t *counts);
int fcx_find_set_host(fcx_dctx *ctx, const uint8_t *in, uint64_t in_len, const fcx_pattern_set *set, uint64_t *hits,
                      uint64_t cap, uint64_t *nhits, uint64_t *counts);
/* fcx_grep_shard / fcx_grep_stream / fcx_grep_host for a set: stats are FCX_GREP_STATS values with stats[3],
 * the positions judged, max(T - min_len + 1, 0); the held-back open line, the windows and the chaining into
 * fcx_decompress_ranges_shard are the one-pattern calls'.  FCX_ERR_ARG also when a pattern holds delim or,
 * with FCX_SET_FOLD_ASCII, a folded pattern holds fold(delim). */
int fcx_grep_set_shard(fcx_dctx *ctx, char kind, const uint8_t *d_rec, uint64_t rec_len, uint32_t nblocks, uint8_t delim,
                       const fcx_pattern_set *set, uint64_t *d_start, uint64_t *d_end, uint64_t cap, uint64_t *stats,
                       uint64_t *counts, void *stream);
int fcx_grep_set_stream(fcx_dctx *ctx, fcx_read_fn read_comp, void *user_comp, uint64_t max_in, uint8_t delim,
                        const fcx_pattern_set *set, fcx_range_fn on_line, void *user_line, uint64_t *stats, uint64_t *counts);
int fcx_grep_set_host(fcx_dctx *ctx, const uint8_t *in, uint64_t in_len, uint8_t delim, const fcx_pattern_set *set,
                      uint8_t *out, uint64_t cap, uint64_t *out_len, uint64_t *stats, uint64_t *counts);
/* Counters of the last set call on the context, summed over its groups (the stream and host forms: over the
 * file), min(n, FCX_SET_SCAN_STATS) values: positions judged; of those, positions whose candidate mask
 * T0[b0] & T1[b1] was not zero; (position, pattern) pairs of more than two bytes taken to the full compare;
 * hits; groups scanned; final passes run: 1 after every call that had records, in the shard forms the scan of the
 * last group and in the stream and host forms the pass behind the last group, which scans nothing when no
 * position is left (max_len == 1, or nothing was decoded); 0 after a call without records. */
int fcx_dctx_set_scan_stats(fcx_dctx *ctx, uint64_t *out, int n);

/* ---- context and inverted grep: grep -v, -A, -B, -C on a run (FCX7 and FCX8) ------------------------------
 * D, T, the delimiter d, the lines s_j / e_j and their number L are those of the line calls; a hit is the
 * pattern sets' hit.  Line j matches iff a hit p has s_j <= p < e_j.  Line j is a base line iff it matches, or
 * with FCX_GREP_INVERT iff it does not.  Line j is selected iff some base line k has j - after <= k <= j +
 * before: `after` lines follow a base line, `before` lines precede one; with the invert flag the context
 * surrounds the lines that do not match, as in GNU grep.  The result is the blocks: the maximal runs of
 * consecutive selected lines, ascending, each as (start = s of its first line, end = e of its last line, line =
 * the 0-based number of its first line).  Two selected lines that touch are one block (GNU grep prints its
 * `--` between blocks).  Blocks are disjoint and ascending, so d_start / d_end feed
 * fcx_decompress_ranges_shard unchanged.  Blocks and not lines, because -v on a run with few hits selects
 * nearly every line: that is one range per gap between hits, at most hits + 1 of them, instead of 16 bytes
 * per line.  T == 0 has no lines and no blocks; an unterminated tail is a line like any other (with the invert
 * flag it can be a base line); a run without a delimiter is one line; empty lines are lines that never match,
 * so with the invert flag they are base lines.
 * stats (FCX_GREP_BLOCK_STATS values): blocks, selected lines, bytes (sum of end - start), base lines, hits,
 * positions judged, decoded bytes T, lines L; all over the whole run whatever cap is.  The answer does not
 * depend on record, tile, decode-group or stream-group boundaries (fcx_dctx_set_verify_group,
 * fcx_dctx_set_find_window); the run is decoded once; scratch beside the grep's own is three bitmaps and 56
 * bytes per tile of a decode group plus a ring of before + 1 line starts (at most 32 KiB), whatever the hits,
 * the lines or the blocks, and nothing of a line's bytes travels between groups. */
#define FCX_GREP_INVERT 1u
#define FCX_GREP_MAX_CONTEXT 4096u
typedef struct fcx_grep_opts { uint32_t flags, before, after; } fcx_grep_opts;
#define FCX_GREP_BLOCK_STATS 8  /* blocks, selected lines, bytes (sum of end - start), base lines,
                                   hits, judged, decoded (T), lines (L) */
/* fcx_grep_set_shard's arguments, checks, cap rule and size query, with the options and a third array: the
 * first min(cap, blocks) blocks to d_start / d_end / d_line (device; all three NULL with cap == 0 for the
 * counts alone); FCX_OK whether or not cap was reached, and nothing behind min(cap, blocks) is written.  A set
 * of one pattern without flags and zero options is the plain grep.  nblocks == 0 gives zeros and touches no
 * device.  FCX_ERR_ARG also, before the device is touched: NULL opts, unknown flag bits, before or after above
 * FCX_GREP_MAX_CONTEXT.  Synchronises `stream`.  Stage table with profiling: index, decode, scan, select,
 * summary. */
int fcx_grep_blocks_shard(fcx_dctx *ctx, char kind, const uint8_t *d_rec, uint64_t rec_len, uint32_t nblocks, uint8_t delim,
                          const fcx_pattern_set *set, const fcx_grep_opts *opts, uint64_t *d_start, uint64_t *d_end,
                          uint64_t *d_line, uint64_t cap, uint64_t *stats, uint64_t *counts, void *stream);
typedef void (*fcx_block_fn)(void *user, uint64_t start, uint64_t end, uint64_t line, uint64_t nlines);
/* fcx_grep_set_stream's twin: the file is one run.  on_block (may be NULL: the totals alone) is called for every
 * block once, in order, with its true end and the number of its lines: a block still open at a stream group's
 * end is held back (its start and first line), and lines that only a base line of a later group can select
 * wait on the device (the ring) until that group shows whether and where their block starts. */
int fcx_grep_blocks_stream(fcx_dctx *ctx, fcx_read_fn read_comp, void *user_comp, uint64_t max_in, uint8_t delim,
                           const fcx_pattern_set *set, const fcx_grep_opts *opts, fcx_block_fn on_block, void *user_block,
                           uint64_t *stats, uint64_t *counts);
/* fcx_grep_set_host's twin: the records go to the device once, the blocks feed fcx_decompress_ranges_shard
 * there, and only the blocks' bytes come back, concatenated; the size query and FCX_ERR_CAPACITY as there. */
int fcx_grep_blocks_host(fcx_dctx *ctx, const uint8_t *in, uint64_t in_len, uint8_t delim, const fcx_pattern_set *set,
                         const fcx_grep_opts *opts, uint8_t *out, uint64_t cap, uint64_t *out_len, uint64_t *stats,
                         uint64_t *counts);

/* ---- regular-expression grep: grep -E with -v, -A, -B, -C on a run (FCX7 and FCX8) ---------------------------
 * The expression is a subset of POSIX ERE over bytes (LC_ALL=C), compiled on the host into a DFA of at most
 * FCX_REGEX_MAX_STATES states over byte classes.  The delimiter d is fixed at compile time, since `.` and negated
 * sets exclude it; the grep calls take no delimiter of their own.
 *   literal bytes; \ and a punctuation byte as that byte; . (any byte but d)
 *   [...] and [^...] with ranges and [:alpha:] [:digit:] [:alnum:] [:upper:] [:lower:] [:space:] [:punct:]
 *   [:xdigit:] (inside a set a backslash is a backslash, as in POSIX); a negated set never matches d
 *   \w \W \s \S        ( ) and |        * + ? {m} {m,} {m,n} with n <= 255
 *   ^ only as the first and $ only as the last item of a top-level alternative (which the whole expression is
 *   when it has no top-level |)
 * FCX_ERR_ARG, the message naming the offset: a back-reference, \b \B \< \>, any other escape of a letter or digit,
 * an anchor elsewhere, an empty alternative or group, {0} and {0,0}, d as a literal or inside a range or single byte of a set
 * that is not negated (with the fold flag: also a byte that folds to what d folds to; the named classes and the
 * shorthands leave d out instead), an expression that matches the empty string (a*, ^$: it would select every
 * line, and an empty line has no position to carry a hit), more than 1024 positions after expanding the counted
 * repetitions, more than 4096 states during subset construction, more than FCX_REGEX_MAX_STATES after
 * minimisation.  With FCX_SET_FOLD_ASCII letters of literals and sets match both ASCII cases (bytes >= 0x80
 * never fold): in the byte classes, the scan reads the bytes as they are.
 * Semantics.  D, T, d and the lines s_j / e_j are those of the line calls; the body of line j is D[s_j, b_j) with
 * b_j = e_j - 1 if the line is terminated and e_j otherwise.  A position p, s_j <= p < b_j, is a hit iff for some
 * top-level alternative A and some q: s_j <= q <= p, D[q..p] is in L(A), q == s_j if A begins with ^, and
 * p == b_j - 1 if A ends with $.  A hit is the position at which a match ends, always a byte of the matching line
 * that is not d.  A line matches iff it holds a hit; base lines, selected lines, blocks and the eight stats are
 * those of the blocks calls above, `hits` the number of hit positions, `judged` T after a whole run.  The answer
 * does not depend on record, tile, decode-group or stream-group boundaries. */
#define FCX_REGEX_MAX_PATTERN 1024u   /* bytes of the expression */
#define FCX_REGEX_MAX_STATES  64u     /* DFA states after minimisation, dead state included */
#define FCX_REGEX_SCAN_STATS  4       /* judged, hits, groups, final passes */
typedef struct fcx_regex fcx_regex;
/* flags: FCX_SET_FOLD_ASCII or 0.  *re is NULL on failure. */
int  fcx_regex_create(fcx_regex **re, const uint8_t *expr, uint32_t len, uint8_t delim, uint32_t flags);
void fcx_regex_destroy(fcx_regex *re);
/* any of the outputs may be NULL: DFA states, byte classes, the flags, the delimiter */
int  fcx_regex_info(const fcx_regex *re, uint32_t *states, uint32_t *classes, uint32_t *flags, uint8_t *delim);
/* fcx_grep_blocks_shard / _stream / _host with a regex for the set, its delimiter, and no counts array: the same
 * argument checks before the device is touched, cap rule and size query, nblocks == 0 touching no device, 4 GiB
 * group refusal, stage table (index, decode, scan, select, summary), held-back open block in the stream form and
 * chaining into the multi-range decode in the host form.  With zero options the blocks are the matching lines
 * of grep -E, runs of adjacent ones merged, and `selected lines` is their count.  Between groups one byte ($
 * looks one byte ahead) and the DFA state in front of it stay on the device.  Scratch beside the blocks calls'
 * (fcx_dctx_grep_scratch counts it): states + 1 bytes per tile of a decode group. */
int fcx_grep_regex_blocks_shard(fcx_dctx *ctx, char kind, const uint8_t *d_rec, uint64_t rec_len, uint32_t nblocks,
                                const fcx_regex *re, const fcx_grep_opts *opts, uint64_t *d_start, uint64_t *d_end,
                                uint64_t *d_line, uint64_t cap, uint64_t *stats, void *stream);
int fcx_grep_regex_blocks_stream(fcx_dctx *ctx, fcx_read_fn read_comp, void *user_comp, uint64_t max_in, const fcx_regex *re,
                                 const fcx_grep_opts *opts, fcx_block_fn on_block, void *user_block, uint64_t *stats);
int fcx_grep_regex_blocks_host(fcx_dctx *ctx, const uint8_t *in, uint64_t in_len, const fcx_regex *re, const fcx_grep_opts *opts,
                               uint8_t *out, uint64_t cap, uint64_t *out_len, uint64_t *stats);
/* counters of the last regex call (the stream form: of the whole file), min(n, FCX_REGEX_SCAN_STATS) values:
 * positions judged, hits, ranges scanned, final passes */
int fcx_dctx_regex_scan_stats(fcx_dctx *ctx, uint64_t *out, int n);

/* ---- cut: fields and byte columns of the lines of the decoded run (FCX7 and FCX8) ---------------------------
 * D, T, the delimiter d and the lines s_j / e_j are those of the line calls.  A repair sidecar is not applied.
 * A cut is compiled once on the host from a mode (FCX_CUT_FIELDS or FCX_CUT_BYTES), a LIST, a separator byte sep
 * (fields mode only; sep == d is FCX_ERR_ARG), d and flags (FCX_CUT_COMPLEMENT or 0).
 * LIST is GNU cut's: items joined by `,`, each N, N-M, N- or -M with N >= 1 and N <= M, no blanks.  Closed numbers
 * are at most FCX_CUT_MAX_COLUMN; an open item N- selects every column from N on, beyond the maximum too, and its
 * N is at most FCX_CUT_MAX_COLUMN + 1.  sel(k) is "k is in LIST", negated under the complement flag; all columns
 * above the maximum are selected or not together, so the device counts a line's ticks up to FCX_CUT_MAX_COLUMN + 1
 * and no further.  mn is the smallest k with sel(k).  FCX_ERR_ARG, the message naming the offset in LIST: an empty
 * list or item, a 0, a descending range, a number above its maximum, any other byte, a list whose effective
 * selection is empty (the complement of `1-`).
 * Column of a byte.  For a byte at p in line j with D[p] != d, ticks(p) is the number of i in [s_j, p) that tick.
 * Bytes mode: every byte ticks, col(p) = ticks(p) + 1.  Fields mode: a byte ticks iff it equals sep; a byte that
 * is not sep has col(p) = ticks(p) + 1, a separator byte opens column k = ticks(p) + 2.  A line without a
 * separator is a line of one field.
 * Keep rule.  The output is a subsequence of D: a delimiter byte is always kept; a byte that is neither d nor (in
 * fields mode) sep is kept iff sel(col(p)); a separator byte is kept iff sel(k) and k > mn for the column k it
 * opens.  So `a,b,c,d\n` with the list 2,4 gives `b,d\n`, and with 5 gives `\n`.  The result does not depend on
 * record, tile, decode-group or buffer-piece boundaries; a line may be longer than any of them.
 * Relation to GNU cut (LC_ALL=C).  -b: the same bytes for every input whose last line is terminated.  -f: the same
 * bytes for every such input in which each line holds a separator or field 1 is selected.  Two differences, on
 * purpose: (1) a line with no separator and field 1 not selected is printed whole by cut (dropped with -s); here
 * it gives an empty line, as awk -F would: cut's rule needs a look-ahead over a line of unbounded length before
 * the line's first byte can be judged.  (2) No byte is added behind an unterminated tail.  Not built: -s,
 * --output-delimiter, reordering or repeating fields, multi-byte separators and characters. */
#define FCX_CUT_FIELDS 1u
#define FCX_CUT_BYTES 2u
#define FCX_CUT_COMPLEMENT 1u     /* flags */
#define FCX_CUT_MAX_COLUMN 4096u
#define FCX_CUT_STATS 6   /* output bytes (whatever cap is), bytes judged (T after a whole run), delimiters seen,
                           * separators seen (0 in bytes mode), separators kept, groups */
typedef struct fcx_cut fcx_cut;
/* Pure host code.  *cut is NULL on failure. */
int  fcx_cut_create(fcx_cut **cut, const char *list, uint32_t len, uint32_t mode, uint8_t sep, uint8_t delim, uint32_t flags);
void fcx_cut_destroy(fcx_cut *cut);
/* any of the outputs may be NULL: the mode, sep, d, the flags, mn (FCX_CUT_MAX_COLUMN + 1: a column above the
 * maximum), whether LIST has an open item */
int  fcx_cut_info(const fcx_cut *cut, uint32_t *mode, uint8_t *sep, uint8_t *delim, uint32_t *flags, uint32_t *mn, uint32_t *open_end);
/* Cap rule of the device calls below (the search's): *out_len is always the output's total, d_out[0, min(cap,
 * total)) receives its first bytes and nothing behind is written, FCX_OK whether or not cap was reached; d_out ==
 * NULL with cap == 0 is the size query (it skips the gather).  The output is a subsequence, so cap >= T always
 * suffices.  stats: FCX_CUT_STATS values on the host, may be NULL.  All synchronise `stream`.
 * fcx_cut_buffer cuts the n plain device bytes at d_in as one text.  d_in and d_out may have any alignment; only
 * [d_in, d_in + n) is read.  n == 0 gives zeros and touches no device.  FCX_ERR_ARG before the device is touched:
 * a NULL ctx, cut or out_len, a NULL d_in with n > 0, a NULL d_out with cap > 0. */
int fcx_cut_buffer(fcx_dctx *ctx, const uint8_t *d_in, uint64_t n, const fcx_cut *cut, uint8_t *d_out, uint64_t cap,
                   uint64_t *out_len, uint64_t *stats, void *stream);
/* Cuts the whole run: it is indexed, then decoded in fcx_verify_shard's groups into the context's bounded buffer
 * (fcx_dctx_set_verify_group applies; the result does not depend on it; a group of 4 GiB or more is FCX_ERR_ARG).
 * What goes from group to group is words on the device: the saturated tick count of the open line, the output
 * bytes so far and the counters; no byte and no state visits the host between groups.  Scratch beside the decoded
 * group: a keep bitmap (group bytes / 8) and 16 bytes per 4096-byte tile, whatever the lines or the output.
 * nblocks == 0 gives zeros and touches no device.  FCX_ERR_ARG before the device is touched: a NULL ctx, cut or
 * out_len, a NULL d_rec with nblocks > 0, a NULL d_out with cap > 0, a kind other than '7' or '8'.  Stage table
 * with profiling: index, decode, cut, summary. */
int fcx_cut_shard(fcx_dctx *ctx, char kind, const uint8_t *d_rec, uint64_t rec_len, uint32_t nblocks, const fcx_cut *cut,
                  uint8_t *d_out, uint64_t cap, uint64_t *out_len, uint64_t *stats, void *stream);
/* Cuts the concatenation of the ranges' bytes as one text, under fcx_decompress_ranges_shard's rules and errors
 * (an index or NULL for both arrays): with a grep's blocks as ranges this is `zgrep ... | cut`.  It runs that call
 * into a buffer of the context of `sum` bytes and then the buffer cut: scratch that grows with the selection,
 * unlike fcx_cut_shard's (fcx_dctx_cut_scratch counts it).  nranges == 0 gives zeros and touches no device. */
int fcx_cut_ranges_shard(fcx_dctx *ctx, char kind, const uint8_t *d_rec, uint64_t rec_len, uint32_t nblocks,
                         const uint64_t *d_rec_off, const uint64_t *d_dec_off, const uint64_t *d_start, const uint64_t *d_end,
                         uint64_t nranges, const fcx_cut *cut, uint8_t *d_out, uint64_t cap, uint64_t *out_len, uint64_t *stats,
                         void *stream);
/* fcx_decompress_stream's twin: reads the header, then the records in that function's groups of 256, and treats the
 * file as one run: the tick count of the open line and the counters stay on the device across stream groups, each
 * group's kept bytes go through write_out (NULL: the totals alone, no gather).  `user` goes to both callbacks.
 * stats (FCX_CUT_STATS values, may be NULL) over the file.  FCX_ERR_ARG before anything is read: a NULL ctx,
 * read_comp or cut. */
int fcx_cut_stream(fcx_dctx *ctx, fcx_read_fn read_comp, fcx_write_fn write_out, void *user, uint64_t max_in, const fcx_cut *cut,
                   uint64_t *stats);
/* A whole file (header + records) in host memory.  fcx_cut_host cuts all of it through the stream form;
 * fcx_cut_ranges_host takes host ranges: the records go to the device once and only the cut bytes come back.
 * *out_len is always the output's total, cap < *out_len is FCX_ERR_CAPACITY (fcx_cut_host has stored the first cap
 * bytes by then, fcx_cut_ranges_host nothing), out == NULL with cap == 0 the size query, as fcx_grep_host. */
int fcx_cut_host(fcx_dctx *ctx, const uint8_t *in, uint64_t in_len, const fcx_cut *cut, uint8_t *out, uint64_t cap, uint64_t *out_len,
                 uint64_t *stats);
int fcx_cut_ranges_host(fcx_dctx *ctx, const uint8_t *in, uint64_t in_len, const uint64_t *starts, const uint64_t *ends,
                        uint64_t nranges, const fcx_cut *cut, uint8_t *out, uint64_t cap, uint64_t *out_len, uint64_t *stats);
/* the last cut call's FCX_CUT_STATS values, min(n, FCX_CUT_STATS) of them; the device bytes it reserved beside the
 * decoded group (bitmap, tile words, and the ranges form's buffer) */
int fcx_dctx_cut_stats(fcx_dctx *ctx, uint64_t *out, int n);
int fcx_dctx_cut_scratch(fcx_dctx *ctx, uint64_t *bytes);

/* ---- multi-GPU: block ranges per GPU + RCCL over xGMI -------------------------
 * Blocks are independent (the window and the parse restart per block, :1675-1703), so
 * rank r of N compresses the contiguous block range fcx_dist_block_range(nb, r, N) of the
 * input and the only exchange is the concatenation of the per-rank segments
 * ([u32 len][payload]... each) in rank order: an all-gather of the u64 segment sizes,
 * then either a gather to rank 0 (grouped point-to-point receives, every xGMI link at
 * once, 1/N of the all-gather's traffic) or an all-gather-v (one broadcast per source
 * rank with its exact size), straight into the output buffer at each segment's offset.
 * The 10-byte header is the caller's (fcx_write_header from the global totals). */
typedef struct fcx_dist fcx_dist;
#define FCX_DIST_ID_BYTES 128u   /* ncclUniqueId */
#define FCX_DIST_GATHER 0        /* concat to rank 0 only */
#define FCX_DIST_ALLGATHER 1     /* concat on every rank */

/* contiguous block range [b0, b1) of rank r of n (the partition of my_compress_amd.dist) */
void fcx_dist_block_range(uint64_t nblocks, int rank, int nranks, uint64_t *b0, uint64_t *b1);
/* gather-aware partition: rank 0 (the receiver) takes floor(nblocks * share0_ppm / 10^6)
 * blocks first, ranks 1..N-1 split the rest near-evenly (share0_ppm 0 = the even split
 * above).  Equals my_compress_amd.dist.block_range(nblocks, rank, N, share0_ppm). */
void fcx_dist_block_range_w(uint64_t nblocks, int rank, int nranks, uint32_t share0_ppm, uint64_t *b0,
                            uint64_t *b1);
/* a fresh RCCL unique id (rank 0 creates it; the caller hands it to every rank) */
int fcx_dist_unique_id(uint8_t *id);
/* one rank of an N-process job (one process per GPU, on HIP device `device`) */
int fcx_dist_init_rank(fcx_dist **d, int nranks, int rank, const uint8_t *id, int device);
/* one process driving ndev devices (rank i on devices[i]; ncclCommInitAll) */
int fcx_dist_init_local(fcx_dist **d, int ndev, const int *devices);
void fcx_dist_destroy(fcx_dist *d);
/* ranks of the job and ranks driven by this process */
int fcx_dist_size(fcx_dist *d, int *nranks, int *nlocal);
/* Concatenates the segments of every rank in rank order (process-per-GPU form: local
 * index 0).  d_seg/seg_len: this rank's segment (device); d_out/cap: the destination
 * (device; on rank 0 for FCX_DIST_GATHER it may be the buffer d_seg lives in, with
 * d_seg == d_out).  *total receives the concatenated length on every rank.  Enqueued on
 * `stream` (a hipStream_t of the rank's device) and synchronised. */
int fcx_dist_concat(fcx_dist *d, int local, const uint8_t *d_seg, uint64_t seg_len, uint8_t *d_out, uint64_t cap,
                    uint64_t *total, int mode, void *stream);
/* The strong-scaling step of one rank, compress and concatenation overlapped (process-per-GPU
 * form).  Every rank passes rank_bytes[0..N) (each rank's input bytes, e.g. from
 * fcx_dist_block_range_w; the same array everywhere) and its own n = rank_bytes[rank] device
 * bytes at d_in.  A peer (rank > 0) compresses its range as `nsub` sub-batches of whole blocks
 * (1 <= nsub <= FCX_DIST_MAX_SUB), each at its bound offset of d_out (capacity >=
 * fcx_dist_gather_bound(n, block, nsub)), and sends each piece to rank 0 as soon as it is done
 * (its u64 length and error word, then its bytes) while the next piece compresses.  Rank 0
 * compresses its range into d_out at offset 0 while the pieces arrive in a staging buffer the
 * handle keeps, then moves them behind its own segment: d_out[0, *total) on rank 0 is every
 * rank's [u32 len][payload] records in block order (capacity >= fcx_shard_bound of the whole
 * input).  A peer whose compress fails sends failure words instead of pieces, so rank 0 always
 * completes the exchange; rank 0 then sends the job's verdict to every peer, so every rank
 * returns an error when any rank failed.  *total: the concatenation on rank 0, the bytes sent on
 * a peer.  Collective over the job; `stream` is the compress stream; returns after both streams
 * are synchronised. */
#define FCX_DIST_MAX_SUB 64u
int fcx_dist_compress_gather(fcx_dist *d, fcx_ctx *ctx, const uint8_t *d_in, uint64_t n, const uint64_t *rank_bytes,
                             uint32_t nsub, uint8_t *d_out, uint64_t cap, uint64_t *total, void *stream);
/* d_out capacity fcx_dist_compress_gather needs for n input bytes in nsub sub-batches */
uint64_t fcx_dist_gather_bound(uint64_t n, uint32_t block_bytes, uint32_t nsub);
/* The whole job in one process (fcx_dist_init_local): host input, rounds of up to
 * round_bytes per device (0 = 1 GiB) split into block ranges, every device compresses
 * its range with one host thread each, the segments are gathered to local rank 0 over
 * RCCL and copied to `out` ([u32 len][payload] records, no header); *out_len = bytes. */
int fcx_dist_compress_host(fcx_dist *d, const uint8_t *in, uint64_t n, uint32_t block_bytes, uint64_t round_bytes,
                           uint8_t *out, uint64_t cap, uint64_t *out_len);
/* name of the transport under a handle: "rccl" or "loopback" */
const char *fcx_dist_transport(fcx_dist *d);

/* ---- loopback transport: the protocols above between thread ranks of one process ------
 * The multi-rank protocols (fcx_dist_concat, fcx_dist_compress_gather, fcx_dist_compress_host)
 * talk to a transport seam (group start/end, send/recv of device bytes, all-gather,
 * broadcast); RCCL is the product transport.  The loopback transport runs the same protocol
 * code between host threads of one process on one device -- each thread rank with its own
 * fcx_dist, fcx_ctx and streams -- so the N > 1 exchange runs on a one-GPU box: a matched
 * send/recv pair is one device-to-device copy on the hub's stream, ordered after both sides'
 * stream positions, and both streams wait for it.  An operation left unmatched for
 * timeout_ms (0 = 60 s) aborts the hub, and every rank then fails instead of hanging. */
typedef struct fcx_loop fcx_loop;
int fcx_loop_create(fcx_loop **hub, int nranks, int device, uint32_t timeout_ms);
/* drops the creator's reference; the hub lives until its last fcx_dist is destroyed */
void fcx_loop_destroy(fcx_loop *hub);
/* rank `rank` of the hub's job, one rank per handle (the fcx_dist_init_rank form) */
int fcx_dist_init_loop(fcx_dist **d, fcx_loop *hub, int rank);
/* every rank of an nranks job in one handle on one device (the fcx_dist_init_local form) */
int fcx_dist_init_loop_local(fcx_dist **d, int nranks, int device, uint32_t timeout_ms);
/* Rank 0 of the last fcx_dist_compress_gather: device ms of its final moves of the peers' bytes
 * behind its own segment (N - 1 copies, hipEvents on its stream); -1 on a peer or before any. */
int fcx_dist_gather_copy_ms(fcx_dist *d, float *ms);
/* Testing: a peer of fcx_dist_compress_gather treats sub-batch `piece` as failed after the
 * earlier pieces are queued (as device error bits would); -1 = off. */
int fcx_dist_debug_fail(fcx_dist *d, int piece);

const char *fcx_last_error(void);
const char *fcx_version(void);

#ifdef __cplusplus
}
#endif
#endif /* FCX_H */
