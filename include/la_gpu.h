/*
 * la_gpu.h -- C ABI of the MI355X (gfx950) data plane behind libarchive's
 * lz4 / gzip read filters.
 *
 * This is the `extern "C"` shim the host filters (include/la_filter.h,
 * libarchive_amd/host/) call from inside their vtable read() -- the ONLY place
 * a device boundary is crossed.  Plain pointers and sizes,
 * no C++ or framework types.  Each entry point cites the reference code whose
 * arithmetic it replaces (paths relative to the reference tree).
 *
 * Conventions
 *   - Functions return LA_OK (0) or a negative la_rc.  Nothing throws.
 *   - Pointers named d_* are DEVICE pointers; h_* are host pointers.
 *   - Work is enqueued on the context's HIP stream; results are valid after
 *     la_gpu_sync() (or after the caller synchronises that stream itself).
 *   - A context is owned by one host thread (one `struct archive` = one
 *     thread, reference README.md:194-221); any number of contexts may exist.
 */
#ifndef LA_GPU_H
#define LA_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LA_GPU_ABI_VERSION 3

typedef enum la_rc {
	LA_OK            = 0,
	LA_ERR_NO_DEVICE = -1,	/* no usable gfx950 device / HIP runtime failure at open */
	LA_ERR_HIP       = -2,	/* a HIP call failed; see la_gpu_last_error() */
	LA_ERR_ARG       = -3,
	LA_ERR_NOMEM     = -4
} la_rc;

typedef struct la_gpu_ctx la_gpu_ctx;

/* ---- context ---- */
int         la_gpu_abi_version(void);
int         la_gpu_device_count(void);
/* Opens device `device`, creates a private stream and a small workspace. */
int         la_gpu_open(int device, la_gpu_ctx **out);
void        la_gpu_close(la_gpu_ctx *ctx);
/* Run on a caller-owned hipStream_t instead of the private one (NULL = back to private). */
int         la_gpu_set_stream(la_gpu_ctx *ctx, void *hip_stream);
int         la_gpu_sync(la_gpu_ctx *ctx);
const char *la_gpu_last_error(const la_gpu_ctx *ctx);
/* Pre-size the context's device workspace (sequence tables, scan scratch) so that
 * no allocation happens inside a decode call.  Optional. */
int         la_gpu_reserve(la_gpu_ctx *ctx, uint64_t workspace_bytes);

/* Raw device memory helpers for C hosts that do not own an allocator. */
int         la_gpu_malloc(la_gpu_ctx *ctx, void **d_ptr, uint64_t bytes);
int         la_gpu_free(la_gpu_ctx *ctx, void *d_ptr);
int         la_gpu_malloc_host(la_gpu_ctx *ctx, void **h_ptr, uint64_t bytes);	/* pinned */
int         la_gpu_free_host(la_gpu_ctx *ctx, void *h_ptr);
int         la_gpu_memcpy_h2d(la_gpu_ctx *ctx, void *d_dst, const void *h_src, uint64_t bytes);
int         la_gpu_memcpy_d2h(la_gpu_ctx *ctx, void *h_dst, const void *d_src, uint64_t bytes);
int         la_gpu_memcpy_d2d(la_gpu_ctx *ctx, void *d_dst, const void *d_src, uint64_t bytes);

/* A marker in the stream: la_gpu_mark() notes the point reached so far, la_gpu_wait_mark()
 * blocks the host until everything queued BEFORE the marker is done -- work queued after it
 * keeps running (how the filters wait for a slab copy while the next window decodes). */
int         la_gpu_mark(la_gpu_ctx *ctx);
int         la_gpu_wait_mark(la_gpu_ctx *ctx);

/* Stream-ordered timer (HIP events on the context's stream). */
int         la_gpu_timer_start(la_gpu_ctx *ctx);
int         la_gpu_timer_stop(la_gpu_ctx *ctx, float *elapsed_ms);	/* synchronises */

/* Per-phase timing of the most recent batch call (HIP events between the kernels,
 * on the work stream).  la_gpu_profile_read() synchronises on the last event and
 * returns the number of phases filled in (0 when profiling is off). */
#define LA_PROF_MAX_PHASES 12
int         la_gpu_profile_enable(la_gpu_ctx *ctx, int on);
int         la_gpu_profile_read(la_gpu_ctx *ctx, float *ms, const char **names, int cap);

/* ---- per-unit status words written by the device ---- */
enum {
	LA_ST_OK                  = 0,
	LA_ST_LZ4_BAD_BLOCK_SUM   = 1,	/* lz4.c:517-526  -> "malformed lz4 data" */
	LA_ST_LZ4_DECODE          = 2,	/* lz4.c:594-598  -> "lz4 decompression failed" */
	LA_ST_LZ4_BAD_HEADER_SUM  = 3,	/* lz4.c:446-451  -> "malformed lz4 data" */
	LA_ST_LZ4_BAD_CONTENT_SUM = 4,	/* lz4.c:655-660  -> "lz4 stream checksum error" */
	LA_ST_GZ_DATA             = 5,	/* gzip.c:494-499 -> "gzip decompression failed" */
	LA_ST_GZ_TRUNCATED        = 6,	/* gzip.c:464-469 -> "truncated gzip input" */
	LA_ST_GZ_BAD_CRC          = 7,	/* NEW (reference never checks, gzip.c:423) */
	LA_ST_GZ_BAD_ISIZE        = 8,	/* NEW */
	LA_ST_GZ_OUT_FULL         = 9,	/* member produced more than dst_cap bytes: host retries with a larger slot */
	LA_ST_GZ_NO_TRAILER       = 10,	/* deflate body complete, fewer than 8 trailer bytes inside src_len (gzip.c:419-421) */
	/* zstd.c:226-231 -> "Zstd decompression failed: <libzstd's name of the error>" */
	LA_ST_ZSTD_CORRUPT        = 11,	/* "Corrupted block detected" */
	LA_ST_ZSTD_TRUNCATED      = 12,	/* the frame needs more bytes than src_len (zstd.c:213-217 "Truncated zstd input") */
	LA_ST_ZSTD_BAD_CHECKSUM   = 13,	/* "Restored data doesn't match checksum" */
	LA_ST_ZSTD_OUT_FULL       = 14,	/* the frame produces more than dst_cap bytes: host retries with a larger slot */
	LA_ST_ZSTD_UNSUPPORTED    = 15,	/* reserved header bit: "Unsupported frame parameter" */
	LA_ST_ZSTD_WINDOW         = 16,	/* window above 2^27 + 1 (ZSTD_decompressStream's default limit): "Frame requires too much memory for decoding" */
	LA_ST_ZSTD_DICTIONARY     = 17,	/* the frame names a dictionary: "Dictionary mismatch" */
	/* LA_GZ_OPT_PIECES only: how a PIECE of one raw-deflate stream ends when its stream does not end in it */
	LA_ST_GZ_PIECE_END        = 18,	/* a non-final block ended on a byte boundary and on the last byte of the span:
					 * the next piece starts right behind it (consumed == src_len) */
	LA_ST_GZ_NEEDS_HISTORY    = 19,	/* a match reaches in front of the piece's first output byte: the blocks behind this
					 * flush point depend on earlier output (Z_SYNC_FLUSH), the piece cannot be decoded alone */
	/* bzip2.c:326-329 -> "bzip decompression failed", :282-286 -> "truncated bzip2 input" */
	LA_ST_BZ2_DATA            = 20,	/* what libbz2 answers BZ_DATA_ERROR for inside a block: a table, selector or symbol
					 * that cannot be, more symbols than the level allows, origPtr outside the block */
	LA_ST_BZ2_TRUNCATED       = 21,	/* the candidate's decode runs off the end of d_src */
	LA_ST_BZ2_BAD_CRC         = 22,	/* a block's bytes do not give its header's CRC (the bytes are delivered, as libbz2 emits
					 * them before it compares), or a stream's combined CRC is not the stored one */
	LA_ST_BZ2_REFUTED         = 23,	/* the chain of confirmed blocks does not pass through this candidate: 48 bits of
					 * compressed data that look like a magic, or an entry behind the point where the walk ended */
	LA_ST_BZ2_RANDOMISED      = 24,	/* the block's randomised bit is set (bzip2 0.9.0 and older): not decoded, a data error */
	/* xz.c:443-451 -> "Lzma library error: Corrupted input data", "Lzma library error:  No progress is possible" */
	LA_ST_XZ_DATA             = 25,	/* refused at a chunk boundary: control 3 .. 0x7F, a first chunk without a dictionary reset,
					 * an LZMA chunk without the properties it owes, a bad properties byte, a range decoder that
					 * does not end on the chunk's two sizes (liblzma reports these in the call that emitted the
					 * last valid byte) */
	LA_ST_XZ_LZMA             = 26,	/* refused inside an LZMA chunk: a distance beyond the data, a range decoder that asks for
					 * bytes behind the chunk's compressed size (liblzma reports these in a call of their own) */
	LA_ST_XZ_TRUNCATED        = 27,	/* the block, its padding or its check field runs off the end of d_src */
	LA_ST_XZ_SIZE             = 28,	/* the data disagrees with a size of the block header */
	LA_ST_XZ_BAD_CHECK        = 29,	/* the check field is not the CRC32 / CRC64 / SHA-256 of the block's bytes */
	LA_ST_XZ_PADDING          = 30,	/* a non-zero byte in the block padding */
	LA_ST_XZ_OUT_FULL         = 31,	/* a block of unknown size produces more than dst_cap bytes: the host retries with more */
	/* lzip (xz.c:443-451 for the first, :605-632 "Lzip: ..." for the last two; the others are questions to the host) */
	LA_ST_LZIP_DATA           = 32,	/* refused inside the LZMA stream: a distance beyond the data or the dictionary, a code that
					 * is not 0 behind the end-of-payload marker */
	LA_ST_LZIP_SRC_END        = 33,	/* the stream asks for a byte at or behind the member's tentative end (src_end) */
	LA_ST_LZIP_TRUNCATED      = 34,	/* no tentative end, and the stream asks for a byte behind d_src */
	LA_ST_LZIP_EARLY_END      = 35,	/* the marker ends the stream in front of the tentative end */
	LA_ST_LZIP_SIZE_OVER      = 36,	/* the stream produces more than the tentative data size */
	LA_ST_LZIP_OUT_FULL       = 37,	/* no tentative size, and the stream produces more than dst_cap: the host retries with more */
	LA_ST_LZIP_BAD_SIZE       = 38,	/* the stream ended with fewer bytes than the tentative data size */
	LA_ST_LZIP_BAD_CRC        = 39,	/* the bytes do not give the trailer's CRC32 */
	LA_ST_LZIP_REFUSED        = 40,	/* the entry points outside d_src or d_dst, or its dst_cap is above LA_XZ_DST_CAP_MAX: not decoded */
	/* lzop (archive_read_support_filter_lzop.c; the numbers in brackets are liblzo2's lzo1x_decompress_safe codes, which
	 * the reference prints) */
	LA_ST_LZOP_BAD_SUM_C      = 41,	/* lzop.c:425-429 -> "Corrupted data": the compressed bytes do not give the block's sum; not decoded */
	LA_ST_LZOP_INPUT_OVERRUN  = 42,	/* lzop.c:459-462 -> "lzop decompression failed: -4": the stream asks for a byte behind src_len */
	LA_ST_LZOP_OUTPUT_OVERRUN = 43,	/* lzop.c:459-462 -> "lzop decompression failed: -5": a literal run or match passes dst_len */
	LA_ST_LZOP_LOOKBEHIND     = 44,	/* lzop.c:459-462 -> "lzop decompression failed: -6": a match starts in front of the block */
	LA_ST_LZOP_NOT_CONSUMED   = 45,	/* lzop.c:459-462 -> "lzop decompression failed: -8": the end marker stands in front of src_len */
	LA_ST_LZOP_SHORT_OUTPUT   = 46,	/* lzop.c:449-454 -> "Corrupted data": the stream ends well with fewer than dst_len bytes */
	LA_ST_LZOP_BAD_SUM_U      = 47,	/* lzop.c:473-477 -> "Corrupted data": the decoded bytes do not give the block's sum */
	LA_ST_LZOP_REFUSED        = 48,	/* the entry points outside d_src or d_dst, src_len > dst_len (lzop.c:332-333 "Corrupted lzop
					 * header" is the host's) or dst_len is above LA_LZOP_MAX_BLOCK (lzop.c:324-325): not touched */
	/* uu (archive_read_support_filter_uu.c): why the walk over a window's lines stopped at result.stop_off */
	LA_ST_UU_IGNORED          = 49,	/* uu.c:515-519: a bad byte while looking for a head, behind decoded bytes: the rest of the
					 * stream is ignored (ST_IGNORE) and the stream ends without an error */
	LA_ST_UU_BAD_BYTE_HEAD    = 50,	/* uu.c:521-524 -> "Insufficient compressed data": the same with nothing decoded so far */
	LA_ST_UU_BAD_BYTE         = 51,	/* uu.c:521-524 -> "Insufficient compressed data": a bad byte in a data line or an `end` line */
	LA_ST_UU_BAD_LINE         = 52,	/* uu.c:607-656, :706-711 -> "Insufficient compressed data": a data line breaks its rules */
	LA_ST_UU_BAD_END          = 53,	/* uu.c:659-666 -> "Insufficient compressed data": the line behind the zero-length line is not `end` */
	LA_ST_UU_TOO_LONG         = 54,	/* uu.c:559-563 -> "Invalid format data": a line over LA_UU_MAX_HEAD_LINE / LA_UU_MAX_DATA_LINE */
	LA_ST_UU_UNTERMINATED     = 55	/* uu.c:527-533 -> "Missing format data": the stream ends inside a line that is not `end` */
};

/* =====================================================================
 * XXH32 -- replaces __archive_xxhash.XXH32 (libarchive/xxhash.c:234-319) for
 * MANY independent hashes at once (one hash is a serial chain).
 * ===================================================================== */
typedef struct la_hash_job {
	uint64_t off;	/* byte offset of the range inside d_base */
	uint32_t len;
	uint32_t seed;
} la_hash_job;

int la_gpu_xxh32_many(la_gpu_ctx *ctx, const uint8_t *d_base,
    const la_hash_job *d_jobs, uint32_t n_jobs, uint32_t *d_out);

/* =====================================================================
 * CRC32 -- replaces crc32() (libarchive/archive_crc32.h:43-84, zlib-compatible)
 * for many ranges; each range is reduced wave-parallel with GF(2) combines.
 * `seed` of a job is the running crc to continue from (0 for a fresh one).
 * ===================================================================== */
int la_gpu_crc32_many(la_gpu_ctx *ctx, const uint8_t *d_base,
    const la_hash_job *d_jobs, uint32_t n_jobs, uint32_t *d_out);

/* =====================================================================
 * Adler-32 -- replaces adler32() (zlib's, as archive_read_support_filter_lzop.c:51, :282, :422, :469 calls it) for many
 * ranges; each range is cut into lane chunks whose (a, b) pairs are combined.  `seed` of a job is the running value to
 * continue from (1 for a fresh one).  Addition under ABI version 3.
 * ===================================================================== */
int la_gpu_adler32_many(la_gpu_ctx *ctx, const uint8_t *d_base,
    const la_hash_job *d_jobs, uint32_t n_jobs, uint32_t *d_out);

/* =====================================================================
 * LZ4 -- replaces the data plane of lz4_filter_read_data_block /
 * lz4_filter_read_default_stream / _legacy_stream
 * (libarchive/archive_read_support_filter_lz4.c:471-613, :615-668, :670-721):
 * block checksum XXH32, LZ4_decompress_safe[_usingDict], content checksum,
 * header check byte -- for a whole batch of blocks/frames per call.
 * The host walks the size words (cheap pointer chase) and fills these tables.
 * ===================================================================== */
#define LA_LZ4B_STORED    1u	/* size word had bit 31: payload is the data (lz4.c:500-504, :530-552) */
#define LA_LZ4B_CHECKSUM  2u	/* block_sum holds the LE32 that followed the payload (lz4.c:517-526) */
#define LA_LZ4B_DEPENDENT 4u	/* frame without the independence bit: matches may reach the previous block (lz4.c:562-591) */
#define LA_LZ4B_FIRST     8u	/* first block of its frame: dictionary is 64 KiB of zeros (lz4.c:260-261) */
#define LA_LZ4B_HIST     16u	/* dependent block that continues a frame from the previous batch: its dictionary is
					 * the la_lz4_batch.hist_len bytes in FRONT of d_dst (d_dst[-hist_len .. 0)) */

typedef struct la_lz4_block {
	uint64_t src_off;	/* first payload byte inside d_src (after the 4-byte size word) */
	uint32_t src_len;	/* payload bytes (size word & 0x7fffffff) */
	uint32_t dst_cap;	/* frame's block maximum size, or 8 MiB for legacy blocks */
	uint32_t flags;		/* LA_LZ4B_* */
	uint32_t block_sum;	/* expected XXH32 of the payload when LA_LZ4B_CHECKSUM */
} la_lz4_block;

#define LA_LZ4F_CONTENT_SUM 1u	/* content_sum holds the LE32 after the EndMark (lz4.c:639-662) */
#define LA_LZ4F_HEADER_SUM  2u	/* verify descriptor check byte (lz4.c:446-451) */
#define LA_LZ4F_CONT        4u	/* the frame began in an earlier batch: no descriptor here, its content hash
					 * continues from d_carry_in */
#define LA_LZ4F_OPEN        8u	/* the frame goes on in the next batch: its content hash state goes to d_carry_out */
#define LA_LZ4F_HASHED     16u	/* the frame carries a content checksum (set on every piece of such a frame) */

typedef struct la_lz4_frame {
	uint64_t desc_off;	/* offset of FLG inside d_src */
	uint32_t desc_len;	/* descriptor bytes INCLUDING the trailing check byte (3..15) */
	uint32_t first_block;	/* index of the frame's first block in the block table */
	uint32_t n_blocks;
	uint32_t flags;		/* LA_LZ4F_* */
	uint32_t content_sum;	/* expected XXH32 of the frame's decoded bytes */
	uint32_t reserved;
} la_lz4_frame;

/* Batch summary reduced on the device (first failing event in STREAM order). */
typedef struct la_batch_summary {
	uint64_t total_out;		/* decoded bytes of the whole batch */
	uint32_t n_bad_units;		/* blocks / members with status != 0 */
	uint32_t n_bad_frames;
	uint32_t first_bad_unit;	/* 0xFFFFFFFF if none */
	uint32_t first_bad_frame;	/* 0xFFFFFFFF if none */
	uint32_t first_zero_unit;	/* first unit that decoded to 0 bytes (ends the stream, SURVEY F11 i); 0xFFFFFFFF if none */
	uint32_t reserved;
} la_batch_summary;

#define LA_LZ4_OPT_GENERAL_ONLY 1u	/* force the general (any block size / dependent) expand kernel */
#define LA_LZ4_OPT_NO_VERIFY    2u	/* skip the three XXH32 checks (the reference's `!stream-checksum` shape) */
#define LA_LZ4_OPT_PARSE_V1     4u	/* first-generation parse: block checksums and token walk as two kernels
					 * reading global memory per lane (kept as a cross-check of the staged one) */

#define LA_LZ4_OPT_EXPAND_INORDER 8u	/* second implementation of the LDS-window expand step (la_lz4_inorder.hip, round 3: one
					 * matcher wave takes the sequences in stream order, literal waves run ahead of it, a flush wave
					 * behind it; no per-sequence flags, no polling in the match phase); same results, kept as the
					 * cross-check of the default kernel (la_lz4_fast.hip), which is still the faster one */

#define LA_LZ4_OPT_SEARCH_IN_EXPAND 16u	/* the default LDS-window kernel finds what each match has to wait for by itself, in
					 * front of its match phase, as it did before the dependency kernel (la_lz4_deps.hip) took
					 * that search out of it; same results, kept as the cross-check of the dependency words */

#define LA_LZ4_OPT_SPLIT_SMALL 32u	/* a batch below the slicing threshold takes the split form of the last expand slice
					 * (la_lz4_slices.h: launches by position in the frame, frame checksums advancing between
					 * them) with the whole batch as that slice, wherever a batch at size would split its last
					 * quarter; same results, so that tests reach the path with a few dozen blocks */

typedef struct la_lz4_batch {
	const uint8_t      *d_src;	/* compressed image (or batch window) in HBM */
	uint64_t            src_bytes;
	const la_lz4_block *d_blocks;
	uint32_t            n_blocks;
	const la_lz4_frame *d_frames;	/* may be NULL when n_frames == 0 */
	uint32_t            n_frames;
	uint8_t            *d_dst;	/* decoded slab: blocks are packed back to back in table order */
	uint64_t            dst_cap;
	/* outputs */
	uint32_t           *d_out_len;		/* [n_blocks]  decoded bytes per block */
	uint64_t           *d_dst_off;		/* [n_blocks+1] exclusive prefix sums of d_out_len */
	uint32_t           *d_block_status;	/* [n_blocks]  LA_ST_* */
	uint32_t           *d_frame_status;	/* [n_frames]  LA_ST_* */
	la_batch_summary   *d_summary;		/* one record */
	uint32_t            options;		/* LA_LZ4_OPT_* */
	uint32_t            hist_len;		/* bytes of carried-over output in front of d_dst (LA_LZ4B_HIST), else 0 */
	/* XXH32 state of a content checksum that spans batches (one frame at most enters a batch
	 * and one at most leaves it unfinished): LA_XXH_CARRY_BYTES each, may be NULL when no
	 * frame has LA_LZ4F_CONT / LA_LZ4F_OPEN.  Must be two different buffers. */
	const void         *d_carry_in;
	void               *d_carry_out;
} la_lz4_batch;
#define LA_XXH_CARRY_BYTES 64u

/* Workspace bytes la_gpu_lz4_decode() needs for this shape (for la_gpu_reserve). */
uint64_t la_gpu_lz4_workspace_bytes(uint32_t n_blocks, uint64_t src_bytes);

int la_gpu_lz4_decode(la_gpu_ctx *ctx, const la_lz4_batch *batch);

/* Debugging aid: after la_gpu_lz4_decode(ctx, batch) and before the next call on ctx, copies the sequence-table
 * entries of block `block` (lit_src | lit_len << 16 | dst << 32 | off << 48) and the dependency words the dependency
 * kernel wrote for them (first sequence to wait for | number of sequences << 16) to the host, `cap` of each at most.
 * Synchronises.  Returns the block's sequence count (0: the block has no table), or LA_ERR_ARG when that decode
 * computed no words (LA_LZ4_OPT_GENERAL_ONLY, _SEARCH_IN_EXPAND, _EXPAND_INORDER).  The words mean something only for a
 * block the LDS-window kernel took in one piece: not stored, not failed, at most 4096 sequences, not routed to the general
 * kernel for its long sequences; the others' are never written.  A word that waits for too little shows in the
 * decoded bytes only as a race; here it can be compared with the rule. */
int la_gpu_lz4_debug_deps(la_gpu_ctx *ctx, const la_lz4_batch *batch, uint32_t block, uint64_t *seq_out,
    uint32_t *deps_out, uint32_t cap);

/* Debugging aid, the same contract: the LITERAL PLAN the dependency kernel wrote for block `block`, `cap` entries at
 * most.  Entry c, for c < ceil(src_len / 32), is the first sequence of the block whose literals end beyond payload
 * offset 32 c, or 0xFFFF when no literal byte lies at or behind that offset; one more entry behind them holds the number
 * of chunks that hold literals.  The LDS-window kernel starts each payload chunk's literal placement from its entry.
 * Synchronises.  Returns the number of entries, ceil(src_len / 32) + 1; 0 for a block the window kernel did not take
 * in one piece (stored, failed, no table, more than 4096 sequences, routed to the general kernel): nothing was
 * written for it; LA_ERR_ARG when that decode computed no plan (the options named above). */
int la_gpu_lz4_debug_literal_plan(la_gpu_ctx *ctx, const la_lz4_batch *batch, uint32_t block, uint16_t *plan_out,
    uint32_t cap);

/* =====================================================================
 * gzip / DEFLATE -- replaces the inflate() loop of gzip_filter_read
 * (libarchive/archive_read_support_filter_gzip.c:431-511; zlib inflate with
 * windowBits -15) for a batch of independent members, plus the trailer
 * CRC32/ISIZE check the reference leaves as a TODO (gzip.c:423).
 * ===================================================================== */
typedef struct la_gz_member {
	uint64_t src_off;	/* first byte of the raw deflate body inside d_src */
	uint32_t src_len;	/* bytes available for body + trailer (up to the next member / end) */
	uint32_t dst_cap;	/* capacity reserved for this member's output */
	uint64_t dst_off;	/* where its output goes inside d_dst */
} la_gz_member;

typedef struct la_gz_result {
	uint32_t status;	/* LA_ST_* (a CRC/ISIZE mismatch is reported here but the bytes are still delivered) */
	uint32_t out_len;	/* bytes produced (also on error: what zlib would have emitted) */
	uint32_t consumed;	/* deflate body bytes consumed (trailer follows) */
	uint32_t crc32;		/* CRC32 of the produced bytes */
} la_gz_result;

typedef struct la_gz_batch {
	const uint8_t      *d_src;
	uint64_t            src_bytes;
	const la_gz_member *d_members;
	uint32_t            n_members;
	uint8_t            *d_dst;
	uint64_t            dst_cap;
	la_gz_result       *d_results;	/* [n_members] */
	la_batch_summary   *d_summary;
	uint32_t            options;
	union {
		uint32_t    hist_len;	/* LA_GZ_OPT_CHAIN: bytes (0 .. 32768) of the same stream's earlier output that the caller
					 * has placed in d_dst directly in FRONT of d_members[0].dst_off; not read otherwise */
		uint32_t    reserved;	/* the field's name before it had a meaning: same place, kept for sources that zero it */
	};
} la_gz_batch;

#define LA_GZ_OPT_NO_VERIFY   1u	/* do not compare the trailer (reference behaviour) */
#define LA_GZ_OPT_WAVE_KERNEL 2u	/* force the wave-per-member kernel (default: lane-per-member from 8192 members up) */
#define LA_GZ_OPT_LANE_KERNEL 4u	/* force the in-place lane-per-member kernel */
#define LA_GZ_OPT_TWO_PHASE   8u	/* force entropy decode + LDS-window expand (the default from 8192 members up) */

#define LA_GZ_OPT_EXPAND_INORDER 32u	/* two-phase path: build the output with the in-order expand kernel (cross-check) */
#define LA_GZ_OPT_RAW        16u	/* members are bare raw-deflate streams (ZIP entries, archive_read_support_format_zip.c:2536-2700):
					 * no gzip trailer follows the body, nothing is compared; status, out_len, consumed and
					 * the CRC32 of the produced bytes are reported */

#define LA_GZ_OPT_PIECES     64u	/* every la_gz_member is a span that CLAIMS to start on a byte-aligned block boundary of one
					 * raw-deflate stream (behind a flush marker 00 00 FF FF, a stored block, or the member header).
					 * Verified as LA_GZ_OPT_RAW (no trailer is read, crc32 is that of the bytes produced).  A piece
					 * ends with LA_ST_OK (a final block ended; consumed points behind it, rounded up to the byte),
					 * LA_ST_GZ_PIECE_END (see there; tested before the next block header is asked for, so a
					 * non-final block that ends mid-byte at the end of the span is LA_ST_GZ_TRUNCATED),
					 * LA_ST_GZ_NEEDS_HISTORY (out_len = the whole symbols in front of the match), or as any member
					 * does.  Nothing in the claim is trusted: the caller confirms a chain of pieces in stream order
					 * (la_gz_pieces_build, la_host.h). */

#define LA_GZ_OPT_CHAIN      128u	/* with LA_GZ_OPT_PIECES only (alone, or with LA_GZ_OPT_LANE_KERNEL, LA_GZ_OPT_TWO_PHASE or
					 * LA_GZ_OPT_EXPAND_INORDER: LA_ERR_ARG, as are hist_len > 32768 and dst_cap + hist_len >= 2^32): the
					 * members are the pieces of ONE raw-deflate stream in stream order, claimed as for LA_GZ_OPT_PIECES,
					 * and they are decoded as one stream -- a distance may reach over the piece's first byte into the
					 * pieces before it and into the hist_len bytes in front of the chain (Z_SYNC_FLUSH, pigz).
					 *   Output is PACKED: piece i's bytes start at d_members[0].dst_off + the sum of out_len of the
					 * pieces before it; d_members[i].dst_off is ignored for i > 0, d_members[i].dst_cap stays the
					 * piece's own bound, and batch.dst_cap counts from d_members[0].dst_off.
					 *   A distance in front of byte -hist_len of the chain is LA_ST_GZ_DATA (out_len = the whole symbols
					 * in front of the match); LA_ST_GZ_NEEDS_HISTORY is never reported.  The first piece whose packed end
					 * would pass batch.dst_cap is LA_ST_GZ_OUT_FULL (out_len 0), the pieces in front of it are intact.
					 * LA_ST_GZ_PIECE_END, LA_ST_OK, LA_ST_GZ_TRUNCATED and consumed are as in piece mode; crc32 is that
					 * of the piece's own packed bytes (fold with la_crc32_combine).  Behind the first piece that is
					 * neither LA_ST_GZ_PIECE_END nor LA_ST_OK results are unspecified.  Nothing outside
					 * [dst_off[0] - hist_len, dst_off[0] + dst_cap) and the workspace is touched, whatever the claims.
					 *   Workspace: 4 bytes per byte of batch.dst_cap and about 40 bytes per piece (la_gpu_reserve). */

#define LA_GZ_OPT_BLOCK_STARTS 256u	/* with LA_GZ_OPT_PIECES | LA_GZ_OPT_CHAIN and n_members == 1 only (else LA_ERR_ARG, as are the chain's
					 * own refusals and src_bytes >= 2^29: bit offsets are 32-bit words): d_members[0] is the span from a
					 * TRUE block boundary of one raw-deflate stream to the end of the window, and the boundary lies at
					 * bit LA_GZ_OPT_START_BIT(options) of the span's first byte.  The device finds the candidate starts
					 * of non-final dynamic blocks behind it, decodes a piece from every one of them, confirms in stream
					 * order those a confirmed piece ended on exactly, and decodes the confirmed pieces as a chain:
					 * hist_len, the packed output from d_members[0].dst_off and batch.dst_cap are the chain's.
					 *   d_results has THREE entries.  [0]: status of the chain -- LA_ST_OK (the final block ended),
					 * LA_ST_GZ_PIECE_END (a non-final block ended on the last bit of the span), LA_ST_GZ_OUT_FULL (the
					 * next piece does not fit: out_len and consumed stand in front of it), or what the last piece earned
					 * (LA_ST_GZ_TRUNCATED, LA_ST_GZ_DATA); out_len: the packed bytes, those of the last piece in front
					 * of its error included; consumed: in BITS from the span's first byte, the bit behind the last block
					 * that ended (for an error: where the decoder's bit buffer stood); crc32: of the out_len bytes.
					 * [1]: out_len = candidates found, consumed = pieces confirmed (the first piece included).
					 * [2]: the chain as far as it stands on a block boundary, for a caller with more input behind the
					 * span: [0] itself when that is LA_ST_OK, LA_ST_GZ_PIECE_END or LA_ST_GZ_OUT_FULL; else the chain
					 * without its last piece -- LA_ST_GZ_PIECE_END, out_len and crc32 of the pieces in front of it,
					 * consumed = the bit that piece starts at (the next call's first byte and start bit).
					 *   Workspace (la_gpu_reserve), from src_bytes and dst_cap alone: 4 B per byte of dst_cap and about
					 * 2 B per byte of src_bytes. */
#define LA_GZ_OPT_START_BIT_SHIFT 16
#define LA_GZ_OPT_START_BIT(options) (((options) >> LA_GZ_OPT_START_BIT_SHIFT) & 7u)

int la_gpu_gzip_decode(la_gpu_ctx *ctx, const la_gz_batch *batch);

/* =====================================================================
 * Zstandard -- replaces, for a batch of whole frames per call, the ZSTD_decompressStream loop of
 * zstd_filter_read (libarchive/archive_read_support_filter_zstd.c:171-260; libzstd is the reference's
 * external dependency for this codec): frame header, raw / RLE / compressed blocks, XXH64 content checksum.
 * The host walks the frame and block headers (la_zstd_index_build, include/la_host.h), drops skippable
 * frames and fills this table; one frame = one unit (a frame is one serial chain).
 * ===================================================================== */
typedef struct la_zstd_frame {
	uint64_t src_off;	/* the frame's magic number inside d_src */
	uint64_t src_len;	/* bytes of the whole frame (header .. last block / checksum) */
	uint64_t dst_off;	/* where its output goes inside d_dst */
	uint64_t dst_cap;	/* capacity reserved for it: Frame_Content_Size when the header carries one, else the walker's bound */
} la_zstd_frame;

typedef struct la_zstd_result {
	uint32_t status;	/* LA_ST_* */
	union {
		uint32_t path;		/* who gave the verdict: 0 the wave or lane kernel (always, without LA_ZSTD_OPT_BLOCK_PARALLEL),
					 * 1 the block path */
		uint32_t reserved;	/* the field's name before it had a meaning: same place, kept for sources that read it */
	};
	uint64_t out_len;	/* bytes produced (0 on error) */
} la_zstd_result;

typedef struct la_zstd_batch {
	const uint8_t       *d_src;
	uint64_t             src_bytes;
	const la_zstd_frame *d_frames;
	uint32_t             n_frames;
	uint32_t             options;	/* LA_ZSTD_OPT_* */
	uint8_t             *d_dst;
	uint64_t             dst_cap;
	la_zstd_result      *d_results;	/* [n_frames] */
} la_zstd_batch;

#define LA_ZSTD_OPT_NO_VERIFY 1u	/* skip the content checksum */
#define LA_ZSTD_OPT_LANE_KERNEL 2u	/* first-generation kernel, one LANE per frame (default: one wave per frame); same results, kept as a cross-check */
/* Decode the BLOCKS of every frame in parallel (a wave per block, matches resolved by pointer jumping; la_zstd_blocks.hip).
 * The block path only ever reports success (result.path = 1): a frame it cannot finish -- damaged, truncated, too small
 * a slot, wrong checksum, more blocks / sequences / literals than its workspace rules hold -- is decoded by the wave
 * kernel (or the lane kernel, with LA_ZSTD_OPT_LANE_KERNEL) behind it in the same call, with path = 0: statuses and
 * bytes are those of options 0 and 2. */
#define LA_ZSTD_OPT_BLOCK_PARALLEL 4u

uint64_t la_gpu_zstd_workspace_bytes(uint32_t n_frames);
int      la_gpu_zstd_decode(la_gpu_ctx *ctx, const la_zstd_batch *batch);

/* =====================================================================
 * LZ4 compression -- the data plane of the lz4 WRITE filter: replaces, for a whole
 * stream per call, LZ4_compress_default per independent block, the stored-block fallback, the block
 * checksum, the frame descriptor with its check byte, the EndMark and the content checksum of
 * libarchive/archive_write_add_filter_lz4.c:394-447, :484-532.  d_src[0, src_bytes) is cut into blocks
 * of block_size bytes (at most 64 KiB), blocks_per_frame of them form one frame; d_out receives the
 * concatenated frames, *d_out_bytes their total size (if it exceeds out_cap nothing past out_cap was
 * written: call again with a larger buffer; src_bytes + src_bytes/255 + 27 bytes per block always fit).
 * The bytes are not liblz4's (an LZ4 stream is not unique); every conforming decoder returns the input.
 * ===================================================================== */
#define LA_LZ4C_BLOCK_SUM   1u	/* FLG bit 4: XXH32 of every block's payload as written */
#define LA_LZ4C_CONTENT_SUM 2u	/* FLG bit 2: XXH32 of every frame's input bytes after its EndMark */

typedef struct la_lz4c_batch {
	const uint8_t *d_src;
	uint64_t       src_bytes;
	uint32_t       block_size;		/* 1 .. 65536 */
	uint32_t       blocks_per_frame;	/* >= 1 */
	uint32_t       flags;			/* LA_LZ4C_* */
	uint32_t       reserved;
	uint8_t       *d_out;
	uint64_t       out_cap;
	uint64_t      *d_out_bytes;		/* one u64 on the device */
} la_lz4c_batch;

uint64_t la_gpu_lz4_compress_workspace_bytes(uint64_t src_bytes, uint32_t block_size, uint32_t blocks_per_frame);
/* upper bound of the stream la_gpu_lz4_compress writes for this shape */
uint64_t la_gpu_lz4_compress_bound(uint64_t src_bytes, uint32_t block_size, uint32_t blocks_per_frame);
int      la_gpu_lz4_compress(la_gpu_ctx *ctx, const la_lz4c_batch *batch);

/* =====================================================================
 * gzip compression -- the data plane of the gzip WRITE filter: replaces, for a whole stream per
 * call, deflate() through zlib, the hand-built header, the CRC32 of the input and the trailer of
 * libarchive/archive_write_add_filter_gzip.c:201-237, :263-266, :293-345.  d_src[0, src_bytes) is cut into chunks of
 * chunk_bytes (at most 49152); every chunk becomes one gzip member of one deflate block, whose header carries the
 * BGZF-compatible "BC" size subfield.  `options` selects the block: LA_GZC_FIXED a fixed-Huffman block, or a stored
 * one when that would not shrink; LA_GZC_DYNAMIC the smallest of a dynamic-Huffman, the fixed-Huffman and the stored
 * block of the same tokens, chosen per chunk from their exact sizes, so never larger than LA_GZC_FIXED gives;
 * LA_GZC_STORED stored blocks only (zlib level 0).  Any other value is LA_ERR_ARG; a zeroed struct means
 * LA_GZC_FIXED.  d_out receives the concatenated members, *d_out_bytes their size (beyond out_cap nothing is written;
 * la_gpu_gzip_compress_bound() always fits, in every mode).  The two fields joined the end of the struct under ABI
 * version 3.
 *
 * `framing` selects the shape of the output.  LA_GZC_FRAME_MEMBERS (a zeroed field) is the above.  With
 * LA_GZC_FRAME_STREAM d_out receives a byte-aligned piece of ONE raw-deflate stream of any length: no gzip header, no
 * trailer, no "BC" field, no CRC32 (la_gpu_crc32_many's jobs take a running seed), and `mtime` is ignored.  The chunks
 * are cut and compressed in parallel as before, `options` keeps its meaning, and each chunk contributes either
 *   - a Huffman block with BFINAL = 0, its end-of-block symbol, then zlib's sync-flush shape: the three zero bits that
 *     open an empty non-final stored block, zero bits up to the next byte boundary and the bytes 00 00 FF FF; or
 *   - a stored block 00 LEN NLEN data (byte-aligned as it is), whenever the Huffman form with that tail would take
 *     n + 5 bytes or more: a chunk of n bytes never takes more than n + 5, and la_gpu_gzip_compress_bound() still fits.
 * No block of the piece has BFINAL set: the caller continues the stream with the next piece or ends it, for example
 * with the empty fixed block 03 00.  Input of length 0 gives 0 bytes.  No match crosses a chunk boundary, so a
 * chunk's bytes do not depend on its neighbours, and every chunk starts on a byte after a sync marker.  Any other
 * value of `framing` is LA_ERR_ARG and nothing is written.
 * ===================================================================== */
#define LA_GZC_FIXED    0u   /* as before: fixed-Huffman block, stored when that would not shrink */
#define LA_GZC_DYNAMIC  1u   /* smallest of dynamic-Huffman, fixed-Huffman and stored, per chunk */
#define LA_GZC_STORED   2u   /* stored blocks only (zlib level 0) */

#define LA_GZC_FRAME_MEMBERS 0u   /* one gzip member per chunk */
#define LA_GZC_FRAME_STREAM  1u   /* a continuable piece of one raw-deflate stream */

typedef struct la_gzc_batch {
	const uint8_t *d_src;
	uint64_t       src_bytes;
	uint32_t       chunk_bytes;	/* 1 .. 49152 */
	uint32_t       mtime;		/* MTIME of every member header (0 = none, gzip.c:213-220 writes time(NULL) unless "!timestamp") */
	uint8_t       *d_out;
	uint64_t       out_cap;
	uint64_t      *d_out_bytes;	/* one u64 on the device */
	uint32_t       options;		/* LA_GZC_FIXED, LA_GZC_DYNAMIC or LA_GZC_STORED */
	union {
		uint32_t framing;	/* LA_GZC_FRAME_MEMBERS or LA_GZC_FRAME_STREAM */
		uint32_t reserved;	/* the field's name before it had a meaning: same place, kept for sources that zero it */
	};
} la_gzc_batch;

uint64_t la_gpu_gzip_compress_workspace_bytes(uint64_t src_bytes, uint32_t chunk_bytes);
uint64_t la_gpu_gzip_compress_bound(uint64_t src_bytes, uint32_t chunk_bytes);
int      la_gpu_gzip_compress(la_gpu_ctx *ctx, const la_gzc_batch *batch);

/* =====================================================================
 * ZIP entries -- the data plane of the ZIP writer (host/la_write_zip.c): replaces, for a whole write window of
 * entries per call, the deflate() loop and the crc32() of libarchive/archive_write_set_format_zip.c (:1271-1301 the
 * data of a deflated entry, :1245-1266 of a stored one, :1324-1349 the end of its stream).  The window is a table of
 * SEGMENTS on the device; a segment is an entry's bytes, or the part of an entry that lies in this window.
 *
 * Output.  For segment i, in table order and back to back: gap_before[i] bytes that are left untouched (the host
 * writes the local file header there), the segment's stream bytes at d_results[i].out_off, out_len long, then
 * gap_after[i] untouched bytes (the data descriptor).  *d_out_bytes is the total.
 *   The stream bytes of a segment are exactly what la_gpu_gzip_compress gives with LA_GZC_FRAME_STREAM for
 * d_src[src_off, src_off + src_len) alone with the same chunk_bytes and options -- chunks are cut from the segment's
 * first byte, none crosses a segment -- followed, if LA_ZIPC_LAST is set, by the empty final fixed block 03 00.  So a
 * last segment of length 0 is 03 00 and any other of length 0 is nothing, and the segments of one entry, in
 * consecutive calls or in one, concatenate to one raw-deflate stream.  With LA_ZIPC_STORE (method 0) the stream bytes
 * are the segment's bytes, copied; LA_ZIPC_LAST adds nothing to them.
 *   crc32 is the CRC32 of the segment's input continued from crc_seed (0 for an entry's first segment, the previous
 * segment's crc32 after that), whatever the method.
 *
 * Errors.  LA_ERR_ARG, with nothing written to d_out, d_results or d_out_bytes, for chunk_bytes 0 or above 49152, an
 * unknown value of `options`, a non-zero `reserved`, and for a segment with unknown flag bits, a non-zero `reserved`,
 * src_len >= 2^31, a range outside d_src, or gaps and worst-case stream bytes (src_len + 5 per chunk + 2) that
 * together pass 2^32 - 1.  Launches are sized by ceil(src_bytes / chunk_bytes) + n_segs chunks, which segments that do
 * not overlap never exceed; a table that does is LA_ERR_ARG too, and so are n_segs >= 2^31 and a chunk bound above
 * 2^31 - 1.  Because the table is device memory, the call waits for the stream once, for this verdict (one 4-byte read
 * behind the kernels that build the chunk table): everything queued on the context's stream before the call is
 * therefore complete when it returns, which matters to a caller that overlaps other work on that stream; the
 * compression itself is then queued as every other call's is.  A write is made only if it ends inside out_cap, so with an
 * out_cap that is too small nothing lies beyond it and *d_out_bytes says what was needed;
 * la_gpu_zip_compress_bound() always fits, gap_bytes_total being the sum of all gaps.
 * These are additions under ABI version 3: no earlier struct or function changed.
 * ===================================================================== */
#define LA_ZIPC_LAST  1u	/* the entry ends with this segment */
#define LA_ZIPC_STORE 2u	/* method 0: the bytes are copied as they are */

typedef struct la_zipc_seg {
	uint64_t src_off;	/* in d_src */
	uint32_t src_len;	/* 0 allowed; below 2^31 */
	uint32_t crc_seed;	/* running CRC32 of the entry's earlier segments, 0 for its first */
	uint32_t gap_before;	/* bytes left untouched in front of the segment's stream bytes (local header) */
	uint32_t gap_after;	/* ... and behind them (data descriptor) */
	uint32_t flags;		/* LA_ZIPC_* */
	uint32_t reserved;	/* 0 */
} la_zipc_seg;

typedef struct la_zipc_result {
	uint64_t out_off;	/* first stream byte inside d_out */
	uint32_t out_len;	/* stream bytes, 03 00 included */
	uint32_t crc32;
} la_zipc_result;

typedef struct la_zipc_batch {
	const uint8_t     *d_src;
	uint64_t           src_bytes;
	const la_zipc_seg *d_segs;
	uint32_t           n_segs;
	uint32_t           chunk_bytes;	/* 1 .. 49152 */
	uint32_t           options;	/* LA_GZC_FIXED, LA_GZC_DYNAMIC or LA_GZC_STORED: the blocks of a deflated segment */
	uint32_t           reserved;	/* 0 */
	uint8_t           *d_out;
	uint64_t           out_cap;
	la_zipc_result    *d_results;	/* [n_segs] */
	uint64_t          *d_out_bytes;	/* one u64 on the device */
} la_zipc_batch;

/* workspace of the largest mode (for la_gpu_reserve; the call reserves what it needs itself) */
uint64_t la_gpu_zip_compress_workspace_bytes(uint64_t src_bytes, uint32_t n_segs, uint32_t chunk_bytes);
/* upper bound of *d_out_bytes: the input, 5 bytes per chunk (at most ceil(src_bytes / chunk_bytes) + n_segs of them), 2 per
 * segment, the gaps */
uint64_t la_gpu_zip_compress_bound(uint64_t src_bytes, uint32_t n_segs, uint32_t chunk_bytes, uint64_t gap_bytes_total);
int      la_gpu_zip_compress(la_gpu_ctx *ctx, const la_zipc_batch *batch);

/* =====================================================================
 * zstd compression -- the data plane of the zstd WRITE filter (host/la_write_zstd.c): replaces, for a whole stream
 * per call, what libarchive/archive_write_add_filter_zstd.c gets from libzstd's ZSTD_compressStream2.  d_src[0,
 * src_bytes) is cut into blocks of block_size bytes (at most 128 KiB, Block_Maximum_Size), blocks_per_frame of them
 * form one frame (Single_Segment_Flag set, Frame_Content_Size present).  Blocks are independent (no match reaches an
 * earlier block, no repeat offsets, every block states its own tables).  Empty input is one frame with one empty raw
 * block.  d_out receives the concatenated frames, *d_out_bytes their total size (if it exceeds out_cap nothing past
 * out_cap was written: call again with a larger buffer; la_gpu_zstd_compress_bound() always fits).  The bytes are not
 * libzstd's (a zstd stream is not unique); every conforming decoder returns the input.
 *
 * Entropy stage.  Without the two flags below a block's literals are Huffman-coded only when their largest byte is at
 * most 128 (the tree description is the direct 4-bit form, which holds 128 weights) and the sequences use the
 * predefined tables; the bytes written for such flags never change.  LA_ZSTDC_FULL_ALPHABET Huffman-codes literals of
 * any alphabet: the weights go out in the direct form or FSE-coded (RFC 8878 4.2.1.1), whichever is allowed and
 * smaller; literals whose sent weights are all equal have no FSE form and stay raw above 128 weights.
 * LA_ZSTDC_FIT_TABLES chooses per block and per field (LL, OF, ML) between Predefined_Mode, RLE_Mode (one code in the
 * whole block) and FSE_Compressed_Mode with counts normalised from the block's own histogram (accuracy log 5 .. 9, 8
 * for offsets), by estimated cost; Repeat_Mode is never written.  LA_ZSTDC_RAW_LITERALS wins over FULL_ALPHABET.
 * ===================================================================== */
#define LA_ZSTDC_CHECKSUM      1u	/* Content_Checksum_Flag + XXH64 (low 32 bits) of every frame's input */
#define LA_ZSTDC_RAW_LITERALS  2u	/* no Huffman literals (the filter's negative / zero levels) */
#define LA_ZSTDC_FULL_ALPHABET 4u	/* Huffman literals for any alphabet (FSE-coded weights where needed or smaller) */
#define LA_ZSTDC_FIT_TABLES    8u	/* sequence tables per block: predefined, RLE or fitted to the block's histogram */

typedef struct la_zstdc_batch {
	const uint8_t *d_src;
	uint64_t       src_bytes;
	uint32_t       block_size;		/* 1 .. 131072 */
	uint32_t       blocks_per_frame;	/* >= 1; block_size * blocks_per_frame < 2^31 */
	uint32_t       flags;			/* LA_ZSTDC_* */
	uint32_t       reserved;
	uint8_t       *d_out;
	uint64_t       out_cap;
	uint64_t      *d_out_bytes;		/* one u64 on the device */
} la_zstdc_batch;

uint64_t la_gpu_zstd_compress_workspace_bytes(uint64_t src_bytes, uint32_t block_size, uint32_t blocks_per_frame);
/* upper bound of the stream la_gpu_zstd_compress writes for this shape: the input, 3 bytes per block, 13 per frame */
uint64_t la_gpu_zstd_compress_bound(uint64_t src_bytes, uint32_t block_size, uint32_t blocks_per_frame);
int      la_gpu_zstd_compress(la_gpu_ctx *ctx, const la_zstdc_batch *batch);

/* =====================================================================
 * bzip2 -- replaces, for a window of a stream per call, the BZ2_bzDecompress loop of bzip2_filter_read
 * (libarchive/archive_read_support_filter_bzip2.c:214-332; libbz2 is the reference's external dependency for this
 * codec).  A bzip2 stream is "BZh" + level digit, then blocks of at most 100 000 x level bytes, each behind the 48-bit
 * magic 0x314159265359 at ANY bit position, then the end magic 0x177245385090 + the 32-bit combined CRC, padded to a
 * byte.  Blocks are independent, so the block is the parallel unit: one workgroup per block.
 *
 * la_gpu_bzip2_scan finds every bit position of d_src[0, src_bytes) where one of the two magics starts (all 48 bits
 * inside the source) and writes them in ascending order to d_cands[0, min(count, cand_cap)); *d_count is the number
 * found.  A match is a CANDIDATE: 48 bits of compressed data can look like a magic.
 *
 * la_gpu_bzip2_decode runs twice over one candidate table, workspace kept between the calls (no other call on the
 * context in between; n, slot_level and options the same).
 *   LA_BZ2_MEASURE decodes every block candidate from its own bit position up to its end-of-block symbol (entropy
 * decode, inverse BWT by a parallel chase, length of the run-length expansion), then confirms candidates in stream
 * order from state_in: candidate k + 1 is confirmed only if it starts where the confirmed candidate in front of it
 * ends; behind an end-of-stream candidate the walk takes the stored CRC, goes to the next byte and asks for "BZh[1-9]"
 * and a candidate 32 bits on (the bid rule, bzip2.c:112-148).  Results: status, level, out_len, end_bit, dst_off (the
 * exclusive scan of out_len over confirmed blocks) per entry; an entry the walk does not pass through is
 * LA_ST_BZ2_REFUTED with out_len 0.  d_state_out says where and why the walk ended.
 *   LA_BZ2_EMIT expands the confirmed blocks among entries [0, n_emit) whose packed end lies inside dst_cap into
 * d_dst, fills in crc, compares block CRCs with their headers and combined CRCs with the end-of-stream entries
 * (LA_ST_BZ2_BAD_CRC in the entry's status), and writes d_state_out again: the stream state behind the last entry it
 * took, first_bad = the first failing entry in stream order.  A block that ends on four equal bytes without their count
 * is emitted as libbz2 emits it (with the count it makes up from the byte behind the block's last) and then fails with
 * LA_ST_BZ2_DATA; it is the first_bad entry as a wrong CRC is, its bytes count in total_out.
 * Blocks with the randomised bit are LA_ST_BZ2_RANDOMISED.  Additions under ABI version 3.
 * ===================================================================== */
#define LA_BZ2_KIND_BLOCK 0u
#define LA_BZ2_KIND_END   1u
typedef struct la_bz2_cand {
	uint64_t bit_off;	/* first bit of the magic, counted from the most significant bit of d_src[0] */
	uint32_t kind;		/* LA_BZ2_KIND_* */
	uint32_t reserved;
} la_bz2_cand;

typedef struct la_bz2_result {
	uint32_t status;	/* LA_ST_* */
	uint32_t level;		/* level digit (1 .. 9) of the stream the entry belongs to; 0 if refuted */
	uint64_t out_len;	/* decoded bytes of a confirmed block; 0 for everything else */
	uint64_t end_bit;	/* block: the bit behind its end-of-block symbol; end of stream: the byte boundary behind the CRC */
	uint64_t dst_off;	/* where a confirmed block's bytes go in d_dst */
	uint32_t crc;		/* EMIT: bzip2 CRC of the block's bytes; end of stream: the combined CRC of its blocks */
	uint32_t stored_crc;	/* the CRC the header (or the end of stream) carries */
} la_bz2_result;

/* how the walk ended (la_bz2_state.stop) */
#define LA_BZ2_STOP_TABLE   0u	/* every entry of the table was passed or refuted and the stream goes on at stop_bit: no
				 * candidate there (the host decides: more input, a damaged magic, the end of the input) */
#define LA_BZ2_STOP_ENTRY   1u	/* entry stop_entry is the next unit and cannot be taken: see its status (a block that
				 * is damaged, truncated or randomised; an end of stream whose CRC lies outside d_src) */
#define LA_BZ2_STOP_BID     2u	/* behind an end of stream, 14 bytes are there and are no "BZh[1-9]" + magic */
#define LA_BZ2_STOP_SHORT   3u	/* behind an end of stream (or at the start), fewer than 14 bytes are left */
#define LA_BZ2_STOP_LEVEL   4u	/* a stream begins at stop_bit whose level is above slot_level: decode on from there */

typedef struct la_bz2_state {
	uint32_t open;		/* 1: inside a stream (a block or end magic is next); 0: a stream header is next */
	uint32_t level;		/* open: the stream's level digit 1 .. 9 */
	uint32_t crc;		/* open: the combined CRC of the stream's blocks so far */
	uint32_t stop;		/* out: LA_BZ2_STOP_* */
	uint64_t start_bit;	/* in: where the next unit starts in d_src.  out (stop_bit): where the walk ended */
	uint64_t total_out;	/* out: decoded bytes of the confirmed (MEASURE) / emitted (EMIT) blocks */
	uint32_t n_taken;	/* out: entries [0, n_taken) were passed: confirmed or refuted */
	uint32_t stop_entry;	/* out: LA_BZ2_STOP_ENTRY */
	uint32_t first_bad;	/* out, EMIT: first entry that failed behind its bytes (LA_ST_BZ2_BAD_CRC, or LA_ST_BZ2_DATA for the
				 * missing count), 0xFFFFFFFF if none */
	uint32_t reserved;
} la_bz2_state;

#define LA_BZ2_MEASURE 0u
#define LA_BZ2_EMIT    1u
#define LA_BZ2_OPT_SERIAL_CHASE 1u	/* inverse BWT by the plain serial chase (the fallback of the parallel one, and its cross-check) */

typedef struct la_bz2_batch {
	const uint8_t     *d_src;
	uint64_t           src_bytes;
	const la_bz2_cand *d_cands;	/* device-resident, ascending bit_off */
	uint32_t           n;		/* at most la_gpu_bzip2_max_blocks(slot_level) */
	uint32_t           phase;	/* LA_BZ2_MEASURE, LA_BZ2_EMIT */
	uint8_t           *d_dst;	/* EMIT */
	uint64_t           dst_cap;
	la_bz2_result     *d_results;	/* [n] */
	const la_bz2_state *state_in;	/* HOST memory, read during the call */
	la_bz2_state      *d_state_out;	/* one record on the device */
	uint32_t           options;	/* LA_BZ2_OPT_* */
	uint32_t           slot_level;	/* 1 .. 9: every block gets a workspace slot for 100 000 x slot_level bytes */
	uint32_t           n_emit;	/* EMIT: entries [0, n_emit) */
	uint32_t           reserved;
} la_bz2_batch;

/* how many candidates one decode call slots at this level (the table may be longer: pass its front) */
uint32_t la_gpu_bzip2_max_blocks(uint32_t slot_level);
uint64_t la_gpu_bzip2_workspace_bytes(uint32_t n, uint32_t slot_level);
/* ws: counts of the compaction, src_bytes / 16 words and the scan's scratch */
int      la_gpu_bzip2_scan(la_gpu_ctx *ctx, const uint8_t *d_src, uint64_t src_bytes, la_bz2_cand *d_cands, uint32_t cand_cap,
    uint32_t *d_count);
int      la_gpu_bzip2_decode(la_gpu_ctx *ctx, const la_bz2_batch *batch);

/* ------------------------------------------------------------------------------------------------------------------
 * xz -- replaces, for a table of blocks per call, what lzma_code does inside a block for xz_filter_read
 * (libarchive/archive_read_support_filter_xz.c:651-735; liblzma is the reference's external dependency for this codec):
 * the LZMA2 chunk layer, the LZMA decoder, the block padding and the block check.  The container (stream header, block
 * headers, index, footer, stream padding) is walked on the host (host/la_filter_xz.c).  Every xz block starts with a
 * dictionary reset, so blocks are independent: one workgroup per block, the probability model in LDS, the dictionary is
 * the block's own output in d_dst.  csrc/la_xz_dev.h states the decode rules and the verdicts.
 * A block whose header carries no compressed size is bounded by src_bytes (and LA_ST_XZ_TRUNCATED says it ran into
 * that bound); one without an uncompressed size is bounded by dst_cap (LA_ST_XZ_OUT_FULL).  On every failure out_len
 * (= valid) bytes in front of it are in d_dst.  Checks: None, CRC32, CRC64 and SHA-256 are verified, other IDs are
 * passed over, as liblzma's stream decoder does without LZMA_TELL_UNSUPPORTED_CHECK.  A block's dst_cap is at most
 * LA_XZ_DST_CAP_MAX (the CRC32 of a block is one la_hash_job, whose 32-bit length is rounded up to whole 64-byte
 * rows); an entry above it, or one that points outside d_src or d_dst, is LA_ST_XZ_SIZE and is not decoded.
 * Additions under ABI version 3. */
#define LA_XZ_UNKNOWN (~(uint64_t)0)
#define LA_XZ_DST_CAP_MAX ((uint64_t)0xFFFFFFC0u)
typedef struct la_xz_block {
	uint64_t src_off;	/* first byte of the block's LZMA2 data inside d_src (behind the block header) */
	uint64_t comp_size;	/* of the block header, or LA_XZ_UNKNOWN: bounded by the end of the source */
	uint64_t uncomp_size;	/* of the block header, or LA_XZ_UNKNOWN: bounded by dst_cap */
	uint64_t dst_off;	/* where the block's bytes go inside d_dst */
	uint64_t dst_cap;	/* the block's output budget (the uncompressed size when that is known) */
	uint64_t check_off;	/* offset of the check field inside d_src, or LA_XZ_UNKNOWN: behind the end marker and the padding */
	uint32_t dict_size;	/* of the LZMA2 filter's properties */
	uint32_t check_id;	/* of the stream header: 0 none, 1 CRC32, 4 CRC64, 10 SHA-256 */
} la_xz_block;

typedef struct la_xz_result {
	uint32_t status;	/* LA_ST_OK or LA_ST_XZ_* */
	uint32_t reserved;
	uint64_t out_len;	/* bytes produced */
	uint64_t consumed;	/* source bytes of the LZMA2 data, up to and including the 0x00 end marker */
	uint64_t valid;		/* a failed block: the bytes in front of the failure that are valid (they are in d_dst) */
} la_xz_result;

/* Filter chains (still ABI version 3; no layout above changes).  la_xz_batch.reserved is a flag word: with
 * LA_XZ_BATCH_CHAINS, d_blocks[n] is followed in the same device buffer by la_xz_chain chains[n], the filters that stand
 * in front of LZMA2 in each block's chain, in chain order: delta (prop: the distance 1 .. 256) and the BCJ filters x86,
 * PowerPC, IA-64, ARM, ARM-Thumb, SPARC (prop: start_offset).  csrc/la_xz_filters_dev.h states the transforms.  They are
 * undone in reverse order over the block's out_len bytes (a failed block: over its valid bytes) between decode and
 * verify, so the check is taken over the unfiltered bytes.  An entry with a count above LA_XZ_CHAIN_MAX, an id outside
 * 0x03 .. 0x09 or a start_offset the filter's alignment does not divide is LA_ST_XZ_SIZE for its block, which is not
 * decoded (its bytes of d_dst are not touched, as for an entry that points outside a buffer).  Any other
 * non-zero flag word is LA_ERR_ARG.  The filters' scratch (16 bytes per block, 256 per 16 KiB of dst_cap) is reserved
 * in the context's workspace by the call itself, beside la_gpu_xz_workspace_bytes(n). */
#define LA_XZ_BATCH_CHAINS 1u
#define LA_XZ_CHAIN_MAX 3u
typedef struct la_xz_chain {
	uint32_t count;			/* 0 .. LA_XZ_CHAIN_MAX filters in front of LZMA2 */
	uint32_t id[LA_XZ_CHAIN_MAX];
	uint32_t prop[LA_XZ_CHAIN_MAX];
	uint32_t reserved;
} la_xz_chain;

typedef struct la_xz_batch {
	const uint8_t     *d_src;
	uint64_t           src_bytes;
	const la_xz_block *d_blocks;	/* device-resident */
	uint32_t           n;
	uint32_t           reserved;	/* 0, or LA_XZ_BATCH_CHAINS */
	uint8_t           *d_dst;
	uint64_t           dst_cap;	/* every block's [dst_off, dst_off + dst_cap) lies inside it */
	la_xz_result      *d_results;	/* [n] */
} la_xz_batch;

uint64_t la_gpu_xz_workspace_bytes(uint32_t n);
int      la_gpu_xz_decode(la_gpu_ctx *ctx, const la_xz_batch *batch);

/* ------------------------------------------------------------------------------------------------------------------
 * lzip -- replaces, for a table of members per call, what lzma_code does for xz_filter_read on a .lz stream
 * (libarchive/archive_read_support_filter_xz.c:533-646, :651-735: lzma_raw_decoder with one LZMA1 filter, lc 3, lp 0,
 * pb 2).  A member is "LZIP", a version byte (0, 1), a dictionary byte, ONE LZMA stream that ends at its end-of-payload
 * marker, and a trailer: CRC32, data size, and (version 1) member size.  Members are independent: one workgroup per
 * member, the probability model in LDS, the dictionary is the member's own output.  csrc/la_lzip_dev.h states the rules
 * (through csrc/la_xz_dev.h's symbol loop).
 *
 * la_gpu_lzip_scan finds every offset of d_src[0, src_bytes) at which a member header can stand: "LZIP", a version of 0
 * or 1, a dictionary byte b with 12 <= (b & 31) <= 29 (xz.c:343-374), all six bytes inside the source.  The offsets go in
 * ascending order to d_offs[0, min(count, cap)); *d_count is the number found.  A match is a CANDIDATE: the host chains
 * members by their trailers' member sizes (host/la_filter_lzip.c).
 *
 * la_gpu_lzip_decode decodes a table of members.  Either end of a member may be unknown (LA_LZIP_UNKNOWN): the source is
 * then bounded by src_bytes (LA_ST_LZIP_TRUNCATED) instead of src_end (LA_ST_LZIP_SRC_END), the output by dst_cap
 * (LA_ST_LZIP_OUT_FULL) instead of data_size (LA_ST_LZIP_SIZE_OVER).  A stream that ends elsewhere than a tentative end
 * says is LA_ST_LZIP_EARLY_END / LA_ST_LZIP_BAD_SIZE.  With LA_LZIP_HAS_CRC the CRC32 of the bytes is compared with
 * `crc32` (LA_ST_LZIP_BAD_CRC); the computed value is in the result either way.  On every failure out_len (= valid)
 * bytes in front of it are in d_dst.  A tentative end or size that proves wrong is no verdict on the stream: the host
 * decodes that member again with both unknown.  dst_cap is at most LA_XZ_DST_CAP_MAX, as for an xz block and for the same
 * reason; such an entry, or one that points outside d_src or d_dst, is LA_ST_LZIP_REFUSED.  Additions under ABI version 3. */
#define LA_LZIP_UNKNOWN (~(uint64_t)0)
#define LA_LZIP_HAS_CRC 1u
typedef struct la_lzip_member {
	uint64_t src_off;	/* first byte of the LZMA stream inside d_src (behind the 6-byte header) */
	uint64_t src_end;	/* tentative: the offset of the trailer (the byte behind the marker), or LA_LZIP_UNKNOWN */
	uint64_t data_size;	/* tentative: the trailer's data size, or LA_LZIP_UNKNOWN */
	uint64_t dst_off;	/* where the member's bytes go inside d_dst */
	uint64_t dst_cap;	/* the member's output budget (at least data_size when that is given) */
	uint32_t dict_size;	/* from the header's dictionary byte (la_lzip_dict_size) */
	uint32_t crc32;		/* LA_LZIP_HAS_CRC: the trailer's CRC32 */
	uint32_t flags;		/* LA_LZIP_HAS_CRC */
	uint32_t reserved;
} la_lzip_member;

typedef struct la_lzip_result {
	uint32_t status;	/* LA_ST_OK or LA_ST_LZIP_* */
	uint32_t crc32;		/* CRC32 of the out_len bytes (0 for an entry that was refused) */
	uint64_t out_len;	/* bytes produced */
	uint64_t consumed;	/* source bytes of the LZMA stream through the marker; what was read so far on a failure */
	uint64_t valid;		/* = out_len: the bytes in front of a failure are valid */
} la_lzip_result;

typedef struct la_lzip_batch {
	const uint8_t        *d_src;
	uint64_t              src_bytes;
	const la_lzip_member *d_members;	/* device-resident */
	uint32_t              n;
	uint32_t              reserved;	/* 0 */
	uint8_t              *d_dst;
	uint64_t              dst_cap;		/* every member's [dst_off, dst_off + dst_cap) lies inside it */
	la_lzip_result       *d_results;	/* [n] */
} la_lzip_batch;

uint64_t la_gpu_lzip_workspace_bytes(uint32_t n);
int      la_gpu_lzip_scan(la_gpu_ctx *ctx, const uint8_t *d_src, uint64_t src_bytes, uint64_t *d_offs, uint32_t cap, uint32_t *d_count);
int      la_gpu_lzip_decode(la_gpu_ctx *ctx, const la_lzip_batch *batch);

/* ------------------------------------------------------------------------------------------------------------------
 * lzop -- replaces, for a table of blocks per call, what lzop_filter_read does with one block
 * (libarchive/archive_read_support_filter_lzop.c:412-482): the sum over the compressed bytes, lzo1x_decompress_safe (or
 * the plain copy of a stored block, src_len == dst_len), the sum over the decoded bytes.  Blocks are independent and
 * both of their sizes stand in the block header, so the host hops from header to header (host/la_filter_lzop.c) and the
 * device decodes one block per wave in ONE pass.  csrc/la_lzo_dev.h states the LZO1X rules.
 *
 * A block whose compressed sum fails is not decoded (LA_ST_LZOP_BAD_SUM_C, out_len 0).  The host hands over sum_c and
 * sum_u as the reference would hold them when it compares (a stale value included, lzop.c:335-350); without a flag for
 * a side nothing is computed or compared for it and the result's field is 0.  On every failure out_len bytes in front of
 * it are in d_dst.  An entry that points outside d_src or d_dst, with src_len > dst_len or dst_len above
 * LA_LZOP_MAX_BLOCK, is LA_ST_LZOP_REFUSED and not touched.  Additions under ABI version 3. */
#define LA_LZOP_C_ADLER32 1u	/* sum_c is the Adler-32 of the compressed bytes (ADLER32_COMPRESSED) */
#define LA_LZOP_C_CRC32   2u	/* sum_c is their CRC32 (CRC32_COMPRESSED); wins over LA_LZOP_C_ADLER32 */
#define LA_LZOP_U_ADLER32 4u	/* sum_u is the Adler-32 of the decoded bytes (ADLER32_UNCOMPRESSED) */
#define LA_LZOP_U_CRC32   8u	/* sum_u is their CRC32 (CRC32_UNCOMPRESSED); wins over LA_LZOP_U_ADLER32 */
#define LA_LZOP_MAX_BLOCK ((uint32_t)64 << 20)	/* MAX_BLOCK_SIZE, lzop.c:92 */
typedef struct la_lzop_block {
	uint64_t src_off;	/* first byte of the block's data inside d_src (behind its header words) */
	uint64_t dst_off;	/* where the block's bytes go inside d_dst */
	uint32_t src_len;	/* the header's compressed size */
	uint32_t dst_len;	/* the header's uncompressed size; equal to src_len: a stored block */
	uint32_t flags;		/* LA_LZOP_* */
	uint32_t sum_c;
	uint32_t sum_u;		/* (not looked at for a stored block, lzop.c:435-440) */
	uint32_t reserved;
} la_lzop_block;

typedef struct la_lzop_result {
	uint32_t status;	/* LA_ST_OK or LA_ST_LZOP_* */
	uint32_t sum_c;		/* the computed sums (0 where no flag asks for one, or the block was not decoded) */
	uint32_t sum_u;
	uint32_t out_len;	/* bytes produced: the bytes in front of a failure are valid */
	uint32_t consumed;	/* source bytes read, through the end marker when one was found */
} la_lzop_result;

typedef struct la_lzop_batch {
	const uint8_t       *d_src;
	uint64_t             src_bytes;
	const la_lzop_block *d_blocks;	/* device-resident */
	uint32_t             n;
	uint32_t             reserved;	/* 0 */
	uint8_t             *d_dst;
	uint64_t             dst_cap;		/* every block's [dst_off, dst_off + dst_len) lies inside it */
	la_lzop_result      *d_results;	/* [n] */
} la_lzop_batch;

uint64_t la_gpu_lzop_workspace_bytes(uint32_t n);
int      la_gpu_lzop_decode(la_gpu_ctx *ctx, const la_lzop_batch *batch);

/* ------------------------------------------------------------------------------------------------------------------
 * uu -- replaces, for a window of the stream per call, the line loop of uudecode_filter_read
 * (libarchive/archive_read_support_filter_uu.c:508-714): get_line, the four states and the two decoders.  A line decodes
 * on its own once its start and the state in front of it are known, so the device finds the line starts, gives every
 * line its transition function over the five states, resolves the states by a scan under composition from the state in
 * front of the window, and decodes all lines at once.  csrc/la_uu_dev.h states the per-line rules.
 *
 * The call takes whole lines only.  In a window that is not `final`, a last line without its line end -- or whose only
 * line end so far is a '\r' in the window's last byte -- is left to the next window: `consumed` stops in front of it.
 * In a `final` window such a line is a line (uu.c:527-533: only `end` may stand there).  The walk stops at the first
 * line that its state refuses; the bytes of the lines in front of it are in d_dst, `consumed` and `stop_off` are that
 * line's offset and `state` is LA_UU_STOP.  Without a stop, status is LA_ST_OK and stop_off == consumed.
 * The host parses mode and name from its own copy of d_src[head_off, head_off + head_len), the last header line the
 * walk accepted.  src_bytes is at most LA_UU_MAX_SRC_BYTES; dst_cap >= src_bytes always suffices and is required.
 * The workspace holds a line table sized for a window of '\n' alone, about 12 bytes per source byte.
 * Additions under ABI version 3. */
#define LA_UU_FIND_HEAD   0u	/* ST_FIND_HEAD, uu.c:57 */
#define LA_UU_READ_UU     1u	/* ST_READ_UU */
#define LA_UU_UUEND       2u	/* ST_UUEND */
#define LA_UU_READ_BASE64 3u	/* ST_READ_BASE64 */
#define LA_UU_STOP        4u	/* absorbing: the walk ended (ST_IGNORE, or one of the reference's errors) */
#define LA_UU_MAX_HEAD_LINE 131072u	/* a line of this many bytes or more, line end included, while looking for a head (uu.c:559) */
#define LA_UU_MAX_DATA_LINE 32768u	/* a data line of more bytes than this, line end included (uu.c:604, :669) */
#define LA_UU_MAX_SRC_BYTES ((uint64_t)1 << 31)
typedef struct la_uu_state {
	uint32_t state;		/* LA_UU_FIND_HEAD .. LA_UU_READ_BASE64 */
	uint32_t decoded;	/* nonzero: the stream has produced bytes in front of this window (uudecode->total > 0) */
} la_uu_state;

typedef struct la_uu_result {
	uint32_t status;	/* LA_ST_OK or LA_ST_UU_* */
	uint32_t state;		/* behind the lines taken; LA_UU_STOP with every status but LA_ST_OK */
	uint32_t decoded;	/* in.decoded, or out_len > 0 */
	uint32_t n_headers;	/* header lines accepted in this window */
	uint64_t out_len;	/* bytes in d_dst */
	uint64_t consumed;	/* source bytes of the whole lines taken */
	uint64_t stop_off;	/* first byte of the line that stopped the walk (== consumed) */
	uint64_t head_off;	/* the last accepted header line, line end included; 0, 0 when n_headers == 0 */
	uint32_t head_len;
	uint32_t reserved;
} la_uu_result;

typedef struct la_uu_batch {
	const uint8_t *d_src;
	uint64_t       src_bytes;
	uint32_t       final;		/* nonzero: the window ends the stream */
	uint32_t       reserved;	/* 0 */
	la_uu_state    in;		/* the state in front of the window (host memory, read by the call) */
	uint8_t       *d_dst;
	uint64_t       dst_cap;		/* >= src_bytes */
	la_uu_result  *d_result;	/* one record, device-resident */
} la_uu_batch;

uint64_t la_gpu_uu_workspace_bytes(uint64_t src_bytes);
int      la_gpu_uu_decode(la_gpu_ctx *ctx, const la_uu_batch *batch);

/* ------------------------------------------------------------------------------------------------------------------
 * bzip2 compression -- replaces the BZ2_bzCompress loop of libarchive/archive_write_add_filter_bzip2.c (libbz2 is the
 * reference's external dependency for this codec).  d_src[0, src_bytes) is cut every
 * la_gpu_bzip2_compress_block_bytes(level) = 4 * ((100000 * level - 19) / 5) input bytes; every cut is one block (block
 * magic, block CRC, origPtr, symbol map, 2..6 tables, selectors, symbols), sorted and coded on the device.  The blocks are
 * concatenated at bit granularity behind the pending bits of *d_state; whole bytes go to d_out, the remaining 0..7 bits
 * and the running combined CRC go back to *d_state, which lives on the device and is read and written there only.
 * LA_BZ2C_FIRST resets *d_state and writes "BZh" + level digit in front; LA_BZ2C_LAST writes the end magic, the
 * combined CRC and zero padding to a byte behind the blocks, so FIRST | LAST with src_bytes == 0 is the 14-byte empty
 * stream and a call without LAST writes a piece the next call continues.  *d_out_bytes is the size needed; nothing is
 * written past out_cap; la_gpu_bzip2_compress_bound() always fits.  The bytes are not libbz2's: the cut is fixed (libbz2
 * fills a block to its limit) and the tables are fitted differently; every conforming reader returns the input.
 * A call whose piece does not fit (*d_out_bytes > out_cap) leaves *d_state as it found it, so the same call can be made
 * again with more room; a call whose piece fits moves *d_state on.
 * src_bytes is at most LA_BZ2C_MAX_SRC_BYTES (1 GiB: positions inside the run-length coded window are 32-bit).  The
 * workspace is about 46 bytes per input byte (two key and two order buffers of the sort, ranks, the three byte stages,
 * symbols, the staged bit buffers): 2.9 GiB for a 64 MiB window, about 46 GiB at the limit;
 * la_gpu_bzip2_compress_workspace_bytes() gives the exact figure, 0 above the limit.
 * la_gpu_bzip2_compress_sort_rounds() (measurement) synchronises and returns how many sort rounds the context's last
 * compress call ran before every rank was distinct; 0 without one.
 * Additions under ABI version 3. */
#define LA_BZ2C_MAX_SRC_BYTES ((uint64_t)1 << 30)
#define LA_BZ2C_FIRST 1u	/* reset *d_state, write "BZh" + level digit in front */
#define LA_BZ2C_LAST  2u	/* behind the blocks: end magic 0x177245385090, combined CRC, zero-pad to a byte */
typedef struct la_bz2c_state {	/* device-resident, read and rewritten by every call */
	uint32_t crc;		/* combined CRC of the stream's blocks so far */
	uint32_t nbits;		/* 0..7 bits of the stream not yet part of a whole byte */
	uint32_t bits;		/* those bits, most significant first, in the low byte's top */
	uint32_t reserved;
} la_bz2c_state;
typedef struct la_bz2c_batch {
	const uint8_t *d_src;
	uint64_t       src_bytes;
	uint32_t       level;	/* 1..9 */
	uint32_t       flags;	/* LA_BZ2C_* */
	la_bz2c_state *d_state;
	uint8_t       *d_out;
	uint64_t       out_cap;
	uint64_t      *d_out_bytes;
} la_bz2c_batch;
uint32_t la_gpu_bzip2_compress_block_bytes(uint32_t level);	/* 0 for a level outside 1..9 */
uint64_t la_gpu_bzip2_compress_workspace_bytes(uint64_t src_bytes, uint32_t level);
uint64_t la_gpu_bzip2_compress_bound(uint64_t src_bytes, uint32_t level);
int      la_gpu_bzip2_compress(la_gpu_ctx *ctx, const la_bz2c_batch *batch);
uint32_t la_gpu_bzip2_compress_sort_rounds(la_gpu_ctx *ctx);

/* ------------------------------------------------------------------------------------------------------------------
 * xz compression -- replaces the lzma_code loop of libarchive/archive_write_add_filter_xz.c (liblzma is the reference's
 * external dependency for this codec) for the blocks of ONE .xz stream.  d_src[0, src_bytes) is cut every
 * LA_XZC_BLOCK_BYTES input bytes, at every level; every cut is one complete block: a 16-byte block header with both sizes
 * and one LZMA2 filter (dictionary 1 MiB), LZMA2 chunks of LA_XZC_CHUNK_BYTES input bytes each, the end marker, zero
 * padding to four bytes and the CRC64.  The chunk is the parallel unit: each one resets state and properties (control
 * 0xE0 for a block's first chunk, 0xC0 otherwise; lc 3, lp 0, pb 2), and one whose coding is not smaller than its input is
 * stored (0x01 / 0x02), so a chunk takes at most its input + 5 bytes.  Levels 0..3 match a chunk against itself; levels
 * 4..9 also against the up to 64 KiB of the same block in front of it.  csrc/la_xz_enc_dev.h states the rules.
 * The blocks are written back to back into d_out; LA_XZC_FIRST puts the 12-byte stream header (check CRC64) in front.
 * Index and footer are the host's (host/la_write_xz.c), which reads the sizes back out of the block headers.
 * *d_out_bytes is the size needed; nothing is written at or behind out_cap; la_gpu_xz_compress_bound(), exact arithmetic
 * from the shape above, always fits.  The bytes are not liblzma's; every conforming reader returns the input.
 * src_bytes is at most LA_XZC_MAX_SRC_BYTES (positions are 32-bit).  The workspace is one slot per chunk, about the size
 * of the input.  Additions under ABI version 3. */
#define LA_XZC_BLOCK_BYTES   ((uint32_t)1 << 20)
#define LA_XZC_CHUNK_BYTES   ((uint32_t)1 << 16)
#define LA_XZC_MAX_SRC_BYTES ((uint64_t)1 << 30)
#define LA_XZC_FIRST 1u		/* the stream header goes in front */
typedef struct la_xzc_batch {
	const uint8_t *d_src;
	uint64_t       src_bytes;
	uint32_t       level;	/* 0..9 */
	uint32_t       flags;	/* LA_XZC_* */
	uint8_t       *d_out;
	uint64_t       out_cap;
	uint64_t      *d_out_bytes;
} la_xzc_batch;
uint64_t la_gpu_xz_compress_block_bytes(uint32_t level);	/* LA_XZC_BLOCK_BYTES; 0 for a level above 9 */
uint64_t la_gpu_xz_compress_workspace_bytes(uint64_t src_bytes);
uint64_t la_gpu_xz_compress_bound(uint64_t src_bytes, uint32_t level);
int      la_gpu_xz_compress(la_gpu_ctx *ctx, const la_xzc_batch *batch);

/* ------------------------------------------------------------------------------------------------------------------
 * lzip compression -- replaces the lzma_code loop of libarchive/archive_write_add_filter_xz.c for its lzip filter
 * (liblzma's raw LZMA1 encoder is the reference's external dependency for this codec).  d_src[0, src_bytes) is cut every
 * la_gpu_lzip_compress_member_bytes(level) input bytes: 64 KiB at levels 0..6 (dictionary byte 0x10), 256 KiB at levels
 * 7..9 (0x12).  Every cut is one complete MEMBER: "LZIP", version 1, the dictionary byte; one raw LZMA1 stream (lc 3,
 * lp 0, pb 2) that ends with the end marker; CRC32, data size and member size.  The members are written back to back into
 * d_out, which is a whole lzip stream (the shape plzip writes) and may be followed by the next call's; src_bytes == 0
 * writes one member of no data.  The member is the parallel unit and is coded without knowing its neighbours; within a
 * level group every level writes the same bytes.  csrc/la_lzip_enc_dev.h states the rules.
 * lzip has no uncompressed member, so la_gpu_lzip_compress_bound() is arithmetic from the coder's worst case and not from
 * a stored fallback: 7 * m + 64 stream bytes and 26 of framing per member of m input bytes, about SEVEN times the input
 * (measured expansion on noise: 1.4 %).  The workspace is one slot of that size per member, so workspace and d_out are
 * about 448 MiB each for a 64 MiB window.  *d_out_bytes is the size needed; nothing is written at or behind out_cap.
 * The bytes are not liblzma's; every conforming reader returns the input.  src_bytes is at most LA_LZC_MAX_SRC_BYTES;
 * level is 0..9 and flags 0, anything else is LA_ERR_ARG.  Additions under ABI version 3. */
#define LA_LZC_MAX_SRC_BYTES ((uint64_t)1 << 30)
typedef struct la_lzc_batch {
	const uint8_t *d_src;
	uint64_t       src_bytes;
	uint32_t       level;	/* 0..9 */
	uint32_t       flags;	/* 0 */
	uint8_t       *d_out;
	uint64_t       out_cap;
	uint64_t      *d_out_bytes;
} la_lzc_batch;
uint64_t la_gpu_lzip_compress_member_bytes(uint32_t level);	/* 0 for a level above 9 */
uint64_t la_gpu_lzip_compress_workspace_bytes(uint64_t src_bytes, uint32_t level);	/* 0 above the limit or for a level above 9 */
uint64_t la_gpu_lzip_compress_bound(uint64_t src_bytes, uint32_t level);	/* 0 for a level above 9 */
int      la_gpu_lzip_compress(la_gpu_ctx *ctx, const la_lzc_batch *batch);

/* ------------------------------------------------------------------------------------------------------------------
 * lzop compression -- replaces, for a window per call, what drive_compressor of
 * libarchive/archive_write_add_filter_lzop.c:314-386 does per block (liblzo2's lzo1x_1_compress is the reference's external
 * dependency for this codec).  d_src[0, src_bytes) is cut every block_size bytes; every cut is one complete lzop BLOCK:
 * BE32 uncompressed size, BE32 compressed size, BE32 Adler-32 of the uncompressed bytes, then one LZO1X stream -- or the
 * input itself, with both sizes equal, where the stream is not shorter than the block (:364-381).  The output is
 * d_out[0, lead_bytes), left untouched for the caller (the filter writes the part's header there), then the blocks back to
 * back.  No header and no closing size word are written: those are the host's.  src_bytes == 0 writes nothing behind the gap.
 * The block is the parallel unit; csrc/la_lzo_enc_dev.h states how its sequences become bytes.  There is one coder: the
 * method and level bytes of a part's header do not reach this call.  The bytes are not liblzo2's; every conforming reader
 * returns the input.  *d_out_bytes is the size needed, the gap counted; nothing is written at or behind out_cap.
 * block_size is 1 .. LA_LZOPC_BLOCK_BYTES, anything else is LA_ERR_ARG.  Additions under ABI version 3. */
#define LA_LZOPC_BLOCK_BYTES 65536u
typedef struct la_lzopc_batch {
	const uint8_t *d_src;
	uint64_t       src_bytes;
	uint32_t       block_size;	/* 1 .. 65536; the filter passes LA_LZOPC_BLOCK_BYTES */
	uint32_t       lead_bytes;	/* d_out[0, lead_bytes) is left untouched for the caller (the header); counted in *d_out_bytes */
	uint8_t       *d_out;
	uint64_t       out_cap;
	uint64_t      *d_out_bytes;
} la_lzopc_batch;
uint64_t la_gpu_lzop_compress_workspace_bytes(uint64_t src_bytes, uint32_t block_size);	/* 0 for a bad block_size */
uint64_t la_gpu_lzop_compress_bound(uint64_t src_bytes, uint32_t block_size);	/* src_bytes + 12 per block; 0 for block_size 0 */
int      la_gpu_lzop_compress(la_gpu_ctx *ctx, const la_lzopc_batch *batch);

#ifdef __cplusplus
}
#endif
#endif /* LA_GPU_H */
