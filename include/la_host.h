/*
 * la_host.h -- host-side (plain C) helpers of the GPU read filters: the frame /
 * member walkers that turn a compressed image into the job tables of
 * include/la_gpu.h, and the mapping from device status words back to the
 * reference's return codes and error strings.
 *
 * The walkers restate ONLY the framing of the reference filters (the cheap,
 * sequential pointer chase); every checksum and every decoded byte is produced
 * on the device.
 *   lz4 : libarchive/archive_read_support_filter_lz4.c:289-368 (frame select),
 *         :370-469 (descriptor), :471-613 (block header), :670-721 (legacy)
 *   gzip: libarchive/archive_read_support_filter_gzip.c:128-239 (header),
 *         :398-429 (trailer), :431-511 (member loop)
 */
#ifndef LA_HOST_H
#define LA_HOST_H

#include <stddef.h>
#include <stdint.h>
#include <sys/types.h>	/* ssize_t */
#include "la_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* How the walked region ends (what the reference does AFTER the last indexed unit) */
enum {
	LA_END_EOF = 0,		/* end of input, unrecognised trailing data, or another silent end: rc 0 */
	LA_END_TRUNCATED,	/* "truncated lz4 input" / "truncated gzip input" */
	LA_END_MALFORMED,	/* "malformed lz4 data" (descriptor / block size word) */
	LA_END_MALFORMED_SKIP,	/* "Malformed lz4 data" (skippable frame without a length, lz4.c:349-353) */
	LA_END_EMPTY_FRAME,	/* a frame without blocks: its checksum is verified, then the stream ends (SURVEY F11 i) */
	LA_END_NEED_MORE,	/* window ended inside an item and more input may follow (at_eof == 0) */
	LA_END_GZ_NO_TRAILER,	/* deflate body complete, trailer short: ARCHIVE_FATAL without message (gzip.c:419-421) */
	LA_END_GZ_TOO_LARGE,	/* a gzip member of 4 GiB or more (compressed span or decoded size): beyond the 32-bit member
				 * table of this data plane -- an explicit error, never a wrong byte (the reference streams such
				 * members; a deployment keeps the reference filter for them) */
	LA_END_ZSTD_BAD_MAGIC,	/* bytes that are neither a zstd nor a skippable frame where a frame must start: libzstd's
				 * "Unknown frame descriptor" (zstd.c:226-231) */
	LA_END_ZSTD_BAD_BLOCK	/* the last indexed frame stops at a reserved block type / oversized block: the device names it */
};

typedef struct la_lz4_index {
	la_lz4_block *blocks;
	uint32_t      n_blocks, cap_blocks;
	la_lz4_frame *frames;
	uint32_t      n_frames, cap_frames;
	int           end_kind;		/* LA_END_* */
	uint64_t      consumed;		/* bytes of the image covered by complete items */
	uint64_t      max_out;		/* sum of dst_cap over blocks (upper bound of decoded bytes) */
} la_lz4_index;

/* Walk img[0..len).  at_eof: no more input follows this window.  Returns 0, or
 * -1 on allocation failure.  The index owns its arrays (la_lz4_index_free). */
int  la_lz4_index_build(const uint8_t *img, uint64_t len, int at_eof, la_lz4_index *idx);

/* A frame of independent blocks may be larger than one window: with a resume record the walker
 * indexes the complete blocks it sees, marks the frame LA_LZ4F_OPEN and continues it at the start
 * of the next window (frame record flagged LA_LZ4F_CONT, no descriptor).  Zero the record before
 * the first window.  Legacy frames continue the same way (their blocks share nothing).  In a frame
 * of dependent blocks the first block of a continuation is flagged LA_LZ4B_HIST: the caller must
 * put the tail of the previous window's output in front of the next slab (la_lz4_batch.hist_len). */
typedef struct la_lz4_resume {
	uint32_t in_frame;	/* the next window starts inside a frame (1) / a legacy frame (2) */
	uint32_t bmax;		/* its block maximum */
	uint32_t flags;		/* bit 0: block checksums, bit 1: content checksum, bit 2: dependent blocks */
	uint32_t blocks_so_far;	/* blocks of the frame indexed in earlier windows */
} la_lz4_resume;
/* Full entry point (the filter's).  rs: resume record, NULL = none.  out_budget: stop indexing in front of the
 * block that would take the window's decoded bytes (sum of dst_cap) past it (0 = no bound); the rest of the stream
 * is the next window's.  la_lz4_index_build is this with rs NULL and no budget. */
int  la_lz4_index_build_ex(const uint8_t *img, uint64_t len, int at_eof, la_lz4_resume *rs, uint64_t out_budget,
         la_lz4_index *idx);
void la_lz4_index_free(la_lz4_index *idx);

/* Bid functions (lz4.c:138-183, gzip.c:244-255) over a peeked buffer */
int  la_lz4_bid_bytes(const uint8_t *p, size_t avail);

/* ---- gzip ---- */
typedef struct la_gz_header {	/* what peek_at_header (gzip.c:128-239) extracts */
	uint64_t off;		/* where the member starts in the image */
	uint32_t len;		/* header bytes */
	uint32_t mtime;
	uint32_t name_off;	/* offset of the FNAME string inside the image, 0 if absent */
	uint32_t bgzf_size;	/* total member size from a BGZF "BC" extra subfield, 0 if absent */
} la_gz_header;

typedef struct la_gz_index {
	la_gz_member *members;	/* src_off/src_len = deflate body + trailer (+ slack when speculative) */
	la_gz_header *headers;
	uint32_t      n, cap;
	int           end_kind;	/* LA_END_* : EOF (silent end / trailing garbage), TRUNCATED, NEED_MORE */
	uint64_t      consumed;	/* bytes of the image covered by the indexed members */
	uint64_t      max_out;	/* sum of dst_cap */
	int           speculative;	/* 1: some boundaries come from the 1f 8b 08 scan and must be confirmed by the decode */
} la_gz_index;

/* Header length (0 = not a gzip header / not enough bytes), gzip.c:128-239 */
size_t la_gz_header_parse(const uint8_t *p, size_t avail, la_gz_header *h);
int    la_gz_bid_bytes(const uint8_t *p, size_t avail);
/* Walk img[0..len): member table with per-member output slots (dst_off assigned back to
 * back from each member's ISIZE claim).  The plain entry point is la_gz_index_build_ex with
 * no hints, no flags, no budget and the span limit LA_GZ_SPAN_LIMIT. */
int    la_gz_index_build(const uint8_t *img, uint64_t len, int at_eof, la_gz_index *idx);
/* flags: LA_GZ_INDEX_STRICT = a speculative boundary must also carry the XFL / OS bytes real writers emit
 * (XFL 0, 2 or 4; OS 0..13 or 255) -- a few thousand times fewer false boundaries inside deflate data.  A stream
 * whose headers do not look like that is still read correctly: the decode of the member in front ends early, the
 * filter sees a header there and goes on without the flag (la_filter_gzip.c). */
#define LA_GZ_INDEX_STRICT 1u
/* Largest compressed span of ONE member the 32-bit member table can express */
#define LA_GZ_SPAN_LIMIT 0xFFFFFFFFull
/* Full entry point (the filter's).
 * first_skip: candidate boundaries to pass over for the first member (refuted by a decode);
 * first_cap: minimum output slot of the first member (its ISIZE claim proved too small);
 * out_budget: stop indexing once the members taken ask for this many decoded bytes (0 = no bound);
 * span_limit: a member whose compressed span passes it ends the walk with LA_END_GZ_TOO_LARGE
 * (LA_GZ_SPAN_LIMIT, or lower in tests). */
int    la_gz_index_build_ex(const uint8_t *img, uint64_t len, int at_eof, uint32_t first_skip,
           uint32_t first_cap, uint32_t flags, uint64_t out_budget, uint64_t span_limit, la_gz_index *idx);
void   la_gz_index_free(la_gz_index *idx);

/* ---- pieces of ONE gzip member (flush points; la_gzip_index.c) ----
 * Any byte-aligned block boundary of a deflate stream is a place to start a decoder, provided the blocks behind it
 * reach no further back than the boundary.  zlib's Z_FULL_FLUSH, pigz -i and this project's gzip:single-member write
 * filter leave such boundaries behind the four bytes 00 00 FF FF (an empty stored block's LEN / NLEN).  The walker
 * cuts img[from .. len) -- `from` on a true block boundary: behind the member header, or behind a confirmed piece --
 * at every such four bytes: piece k is [end of piece k-1, marker + 4), a la_gz_member for la_gpu_gzip_decode with
 * LA_GZ_OPT_PIECES.  NOTHING is trusted: 00 00 FF FF also occurs inside stored data and Huffman bits.  The caller
 * walks the results in stream order and confirms piece k only when it answers LA_ST_GZ_PIECE_END with consumed ==
 * src_len; piece 0 starts on a true boundary and a confirmed piece ends on one, so a confirmed chain is correct by
 * induction.  A piece that answers LA_ST_GZ_TRUNCATED with bytes behind it ended in a false marker: the caller comes
 * back with `from` = that piece's start and first_skip one higher, which merges it with the next one.
 *   The span behind the last marker runs to the end of the window; it is queued only with at_eof (last_open = 1: it
 *   holds the final block, or the stream was cut) -- otherwise its bytes are the next window's and `consumed` stops
 *   in front of them.
 *   first_skip  markers to pass over for the first piece (refuted by a decode)
 *   min_cap     no slot below this (a piece answered LA_ST_GZ_OUT_FULL: doubled from that piece on, like hint_cap)
 *   out_budget  stop in front of the piece that would take the sum of slots past it (0 = no bound; one is always taken)
 *   span_limit  as la_gz_index_build_ex
 * end_kind: LA_END_EOF (at_eof and everything is queued), LA_END_NEED_MORE (bytes behind `consumed` wait for the
 * next window), LA_END_GZ_TOO_LARGE. */
typedef struct la_gz_pieces {
	la_gz_member *pieces;
	uint32_t      n, cap;
	int           end_kind;
	int           last_open;	/* the last piece queued is the span behind the last marker */
	uint64_t      consumed;		/* img offset behind the last piece queued (`from` when none is) */
	uint64_t      max_out;		/* sum of the slots (each rounded up to 16 bytes) */
} la_gz_pieces;
int      la_gz_pieces_build(const uint8_t *img, uint64_t len, uint64_t from, int at_eof, uint32_t first_skip,
             uint32_t min_cap, uint64_t out_budget, uint64_t span_limit, la_gz_pieces *x);
void     la_gz_pieces_free(la_gz_pieces *x);
/* offset of the first 00 00 FF FF at or behind `from`, or len */
uint64_t la_gz_next_marker(const uint8_t *img, uint64_t len, uint64_t from);
/* LA_GZIP_FLUSH_POINTS=1 or =chain: the gzip read filter and its bid policy look for flush points */
int      la_gz_flush_points_enabled(void);
int      la_zstd_blocks_enabled(void);	/* LA_ZSTD_BLOCKS=1: one zstd frame decodes block-parallel (LA_ZSTD_OPT_BLOCK_PARALLEL) */
/* LA_GZIP_FLUSH_POINTS=chain: the pieces may depend on each other, the filter decodes them with LA_GZ_OPT_CHAIN */
int      la_gz_flush_points_chain(void);
/* LA_GZIP_BLOCK_STARTS=1: a member without flush points is decoded from the block starts the device finds
 * (LA_GZ_OPT_BLOCK_STARTS); the bid policy then takes a lone member */
int      la_gz_block_starts_enabled(void);

/* ---- zstd (host/la_zstd_index.c) ---- */
typedef struct la_zstd_index_result {
	uint32_t n_frames;	/* entries written to frames[] (skippable frames are passed over) */
	int      end_kind;	/* LA_END_EOF, _TRUNCATED, _NEED_MORE, _ZSTD_BAD_MAGIC, _ZSTD_BAD_BLOCK */
	uint64_t consumed;	/* bytes of the image covered by the indexed frames (and the skippable ones between them) */
	uint64_t dst_bytes;	/* decoded bytes the slots ask for (16-byte aligned slots back to back) */
	int      window_full;	/* stopped because of cap / out_budget, not because of the input */
} la_zstd_index_result;
/* zstd.c:107-131 over a peeked buffer */
int la_zstd_bid_bytes(const uint8_t *p, size_t avail);
/* Frame table of img[0..len): frame and block headers only.  out_budget as for the other walkers. */
int la_zstd_index_build(const uint8_t *img, uint64_t len, int at_eof, uint64_t out_budget, la_zstd_frame *frames,
        uint32_t cap, la_zstd_index_result *res);

/* ---- bid policy (host/la_bid_policy.c): does the stream hold many independent units, or ONE serial one that the
 * reference's own filter decodes faster on a host core?  Used by the bidders; LA_GPU_BID=all switches it off. ---- */
struct archive_read_filter;
/* 1: the policy is on and a look-ahead of 1024 KiB shows one serial unit (`parallel`, a la_bid_*_parallel below, says 0) */
int    la_bid_declines(struct archive_read_filter *filter, int (*parallel)(const unsigned char *, size_t, size_t));
int    la_bid_take_all(void);
size_t la_bid_lookahead(size_t default_kib);
const unsigned char *la_bid_peek(struct archive_read_filter *filter, size_t want, size_t *got);
int    la_bid_gzip_parallel(const unsigned char *p, size_t n, size_t hdr_len, size_t lookahead);
int    la_bid_lz4_parallel(const unsigned char *p, size_t n, size_t lookahead);
int    la_bid_zstd_parallel(const unsigned char *p, size_t n, size_t lookahead);
int    la_bid_xz_parallel(const unsigned char *p, size_t n, size_t lookahead);
int    la_bid_lzip_parallel(const unsigned char *p, size_t n, size_t lookahead);
int    la_bid_lzop_parallel(const unsigned char *p, size_t n, size_t lookahead);

/* ---- read-filter window plumbing (host/la_bid_policy.c), shared by the read filters; the held-back delivery and the
 * reader base at its end by the bzip2, xz, lzip and lzop ones ---- */
/* LA_GPU_DEVICE: the device ordinal every filter, the ZIP reader and the hash drop-in open (default 0) */
int  la_env_device(void);

/* One filter's window: its device, its size (read once, at init) and whether upstream has ended */
typedef struct la_window {
	la_gpu_ctx *gpu;
	const char *name;		/* "lz4", "gzip", "zstd", "bzip2", "xz", "lzip", "lzop": in the error strings */
	size_t      batch_bytes;	/* compressed bytes of the next window: min(16 MiB, target), then ramped */
	size_t      target_bytes;	/* LA_GPU_BATCH_MIB, default 64 */
	size_t      max_batch_bytes;	/* LA_GPU_MAX_BATCH_MIB, default 2048: how far a window may widen */
	uint64_t    out_budget;		/* LA_GPU_OUT_BUDGET_MIB, default 4096: decoded bytes one window may ask for */
	int         upstream_eof;
} la_window;
/* Read the knobs and open the device; on failure "Can't initialize <name> GPU data plane ..." and ARCHIVE_FATAL */
int  la_window_open(struct archive_read_filter *self, la_window *w, const char *name);
/* batch = min(2 x batch, target) */
void la_window_ramp(la_window *w);
/* "<name> GPU data plane: <what> failed: <device error>"; returns ARCHIVE_FATAL */
int  la_window_fail(struct archive_read_filter *self, const la_window *w, const char *what);

/* A grown buffer: pinned host, device or malloc'ed host memory.  The growers start at 1 MiB and double;
 * 0, or -1 when the allocation failed.  la_buf_pinned copies the first `keep` bytes over. */
enum { LA_BUF_HOST = 0, LA_BUF_PINNED, LA_BUF_DEV };
typedef struct la_buf {
	uint8_t *p;
	size_t   cap;
	int      kind;	/* LA_BUF_*, set by the grower */
} la_buf;
int  la_buf_pinned(la_gpu_ctx *gpu, la_buf *b, size_t need, size_t keep);
int  la_buf_dev(la_gpu_ctx *gpu, la_buf *b, size_t need);
int  la_buf_host(la_buf *b, size_t need);
void la_buf_release(la_gpu_ctx *gpu, la_buf *b);

/* Append upstream bytes to the pinned stage[0..*len) until it holds a window (w->batch_bytes) or upstream
 * ends (w->upstream_eof).  ARCHIVE_FATAL with upstream's error left in place, or after la_window_fail. */
int  la_window_gather(struct archive_read_filter *self, la_window *w, la_buf *stage, size_t *len);
/* Drop stage[0, used): the unfinished unit opens the next window.  When that unit needs more bytes (`more`), nothing
 * was dropped and the window was full, the unit is larger than the window: double it up to max_batch_bytes, or refuse
 * "<name> <unit> too large for the GPU data plane (more than %llu compressed bytes; LA_GPU_MAX_BATCH_MIB)". */
int  la_window_carry(struct archive_read_filter *self, la_window *w, la_buf *stage, size_t *len, size_t used, int more,
         const char *unit);

/* A verdict reported after the bytes in front of it: rc (ARCHIVE_OK = none) and the message to set with it.
 * fmt NULL: no message (upstream already set the error, or the reference returns ARCHIVE_FATAL without one). */
typedef struct la_verdict {
	int  rc;
	int  has_msg;
	char msg[256];
} la_verdict;
#if defined(__GNUC__)
__attribute__((format(printf, 3, 4)))
#endif
void la_verdict_set(la_verdict *v, int rc, const char *fmt, ...);
/* sets the message, if any, and returns rc */
int  la_verdict_report(struct archive_read_filter *self, const la_verdict *v);

/* Decoded bytes held back in front of a possible error (the bzip2, xz, lzip and lzop filters).  The reference hands out whole
 * blocks of LA_OUT_BLOCK bytes and loses the partial block on an error, so with T bytes decoded everything up to the
 * last block boundary strictly below T is safe to hand out; the rest (at most one block) waits for the next window's
 * verdict.  Each filter's head comment derives T and which of its errors is early or late. */
#define LA_OUT_BLOCK ((uint64_t)65536)	/* bzip2.c:186, xz.c:474 */
typedef struct la_holdback {
	la_buf   out; size_t out_len, out_pos;	/* pinned: what the current window decoded (the window appends, read takes) */
	uint8_t *tail; size_t tail_len;		/* held back from earlier windows, at most one block */
	uint64_t total, delivered;		/* T (the window adds to it), bytes handed out */
	la_verdict verdict; uint64_t end_limit; int ended;	/* the stream's end is known: reported once end_limit bytes are out */
	int      finished;
	uint64_t base;				/* where the grid of output blocks starts: 0, or the last la_holdback_rebase */
} la_holdback;
enum {
	LA_HB_EARLY,	/* the error arrives in the call that emitted byte T: floor((T-1)/64Ki)*64Ki bytes go out, 0 for T = 0 */
	LA_HB_LATE,	/* it arrives in a call of its own: floor(T/64Ki)*64Ki */
	LA_HB_ALL	/* a clean end: T */
};
int     la_holdback_open(la_holdback *h);	/* the tail block; -1: no memory */
/* The stream ends here, T being h->total: rc and msg (NULL: none) are reported behind the bytes `how` lets out.  A
 * later call replaces an earlier one. */
void    la_holdback_end(la_holdback *h, int rc, const char *msg, int how);
/* The reference's output block starts afresh here, T being h->total (the lzip filter, at every member's confirmed end:
 * xz.c:693-734 hands out the partial block there).  All T bytes may go out; the early / late arithmetic counts from
 * here on.  A filter that never calls it keeps one grid from byte 0. */
void    la_holdback_rebase(la_holdback *h);
/* The filter's read(): hands out what may go, then the verdict once, then 0; runs window(self) -- which appends to
 * `out`, adds to `total` and may call la_holdback_end -- whenever it needs more.  A window that does not return
 * ARCHIVE_OK has set its error: that code is returned and the read is over. */
ssize_t la_holdback_read(struct archive_read_filter *self, const la_window *w, la_holdback *h, const void **p,
            int (*window)(struct archive_read_filter *));
void    la_holdback_release(la_gpu_ctx *gpu, la_holdback *h);

/* What a filter that decodes a window of units in one launch and hands the bytes out through la_holdback keeps: each
 * of the four embeds one as the first member of its private struct.  The walker, the launch and the walk of its
 * results stay in the filter. */
typedef struct la_reader {
	la_window w;
	la_buf stage; size_t stage_len;	/* pinned: the stream from the first byte of the unfinished unit on */
	la_buf d_src, d_dst, d_tabs;	/* the window on the device, the decoded bytes, the filter's tables */
	la_buf h_tabs;			/* the filter's host tables, one zeroed block of the size it asked for */
	la_holdback hb;
} la_reader;
/* The host block, the holdback, the window and its device; out_budget is clamped to max_out_budget (0: left alone).
 * r NULL (the filter had no memory for its struct) or no memory here: ENOMEM with nomem_msg; no device: la_window_open's
 * message.  Either way everything is released again and ARCHIVE_FATAL returned. */
int     la_reader_open(struct archive_read_filter *self, la_reader *r, const char *name, size_t host_tab_bytes,
            uint64_t max_out_budget, const char *nomem_msg);
/* la_window_gather, then stage[0, stage_len) uploaded to d_src */
int     la_reader_gather(struct archive_read_filter *self, la_reader *r);
/* Append d_dst[0, bytes) to hb.out; T grows by as much */
int     la_reader_take(struct archive_read_filter *self, la_reader *r, uint64_t bytes);
/* The window's end: ramp, then nothing more when the stream has ended, else la_window_carry */
int     la_reader_finish(struct archive_read_filter *self, la_reader *r, size_t used, int more, const char *unit);
ssize_t la_reader_read(struct archive_read_filter *self, la_reader *r, const void **p, int (*window)(struct archive_read_filter *));
/* Everything la_reader_open and the windows allocated, and the device; the filter's struct is the filter's to free */
void    la_reader_close(la_reader *r);
/* A unit whose decoded size nothing states is given *solo_cap bytes of output: max(8 x the `have` compressed bytes at
 * hand, 1 MiB) when it is 0, at most out_budget.  la_reader_solo_full, when `cap` proved too small ("output full"):
 * *solo_cap = 2 x cap, or at the budget "<name> <unit> too large for the GPU data plane (more than %llu decoded bytes;
 * LA_GPU_OUT_BUDGET_MIB)" and ARCHIVE_FATAL. */
uint64_t la_reader_solo_cap(const la_reader *r, uint64_t *solo_cap, uint64_t have);
int     la_reader_solo_full(struct archive_read_filter *self, const la_reader *r, uint64_t *solo_cap, uint64_t cap, const char *unit);

/* ---- hash drop-ins (host/la_hash_dropin.c) ----
 * The 4-pointer table of libarchive/archive_xxhash.h:37-46 (defined as `__archive_xxhash` when built
 * inside libarchive with -DLA_IN_LIBARCHIVE) and crc32() with zlib's signature
 * (libarchive/archive_crc32.h:43-52).  One-buffer XXH32 calls run on the calling thread (a single
 * XXH32 is one serial chain); la_crc32 sends buffers of 8 MiB and more through la_gpu_crc32_many. */
struct la_archive_xxhash {
	unsigned int (*XXH32)(const void *input, unsigned int len, unsigned int seed);
	void        *(*XXH32_init)(unsigned int seed);			/* malloc'ed, free()-able */
	int          (*XXH32_update)(void *state, const void *input, unsigned int len);	/* 0 = XXH_OK */
	unsigned int (*XXH32_digest)(void *state);			/* frees the state */
};
#ifdef LA_IN_LIBARCHIVE
extern const struct la_archive_xxhash __archive_xxhash;
#else
extern const struct la_archive_xxhash la_archive_xxhash;
#endif
unsigned long la_crc32(unsigned long crc, const void *buf, size_t len);
unsigned long la_crc32_host(unsigned long crc, const void *buf, size_t len);
/* crc32(A || B) from crc32(A), crc32(B) and len(B): the GF(2) combine (the drop-in's ranges, the gzip filter's pieces) */
uint32_t la_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b);

/* The reference's error string for a device status word / an end kind */
const char *la_status_message(uint32_t la_st);
const char *la_end_message(int end_kind, int is_gzip);

#ifdef __cplusplus
}
#endif
#endif
