/*
 * la_bid_policy.c -- the host code the read filters (la_filter_lz4.c, la_filter_gzip.c, la_filter_zstd.c,
 * la_filter_bzip2.c, la_filter_xz.c, la_filter_lzip.c, la_filter_lzop.c) share: the bid policy, below it the window
 * plumbing, and at the end the held-back delivery and the reader base (la_reader) of the bzip2, xz, lzip and lzop filters.
 *
 * Bid policy: should the GPU filter take this stream at all?
 *
 * The device decodes INDEPENDENT units in parallel (lz4 frames / blocks, gzip members, zstd frames); ONE serial
 * unit -- a plain single-member .gz (gzip.c:431-511), a one-frame .zst (zstd.c:196-260), a single lz4 frame whose
 * content checksum is one XXH32 chain (lz4.c:615-668) -- runs on one wave and is 1.5 to 100 times slower than the
 * reference's own filter on one host core (known limits).  The product has no CPU path, so the honest
 * answer for such a stream is NOT TO BID: with libarchive's own bidder registered beside this one
 * (archive_read.c:557-565 takes the highest bid) the reference's filter then decodes it.
 *
 * The decision is made in bid() from a bounded look-ahead (bid() may only peek, archive_read_private.h:43-51):
 *   - fewer bytes than the look-ahead in the whole stream: small, taken (nothing to win or lose);
 *   - evidence of many units inside the look-ahead (a BGZF size subfield, a second member header, a frame that
 *     ends inside it): taken;
 *   - otherwise the first unit is larger than the look-ahead: declined (bid 0).
 * An .lz stream (la_filter_lzip.c) is taken when the look-ahead shows a second member header that the member size in
 * front of it confirms: a first member longer than the look-ahead is one serial chain.
 * An .lzo stream (la_filter_lzop.c) is taken when its first block ends inside the look-ahead: every block header carries
 * both of its sizes, and a block longer than the look-ahead is one serial chain.
 * An .xz stream (la_filter_xz.c) is taken when its first block header carries a compressed size (xz -T, pixz: the
 * host hops from header to header); a block without one is a serial chain of unknown extent.
 * LA_ZSTD_BLOCKS=1 makes one long zstd frame a parallel unit (its blocks), and the zstd bidder takes it.
 * LA_GPU_BID=all switches the policy off (every stream with the right magic is taken: the stand-alone test core
 * has no other bidder); LA_GPU_BID_LOOKAHEAD_KIB sets the look-ahead (default 1024, gzip 256).
 */
#include "la_read_private.h"
#include "la_host.h"
#include <errno.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

int la_bid_take_all(void)
{
	const char *m = getenv("LA_GPU_BID");
	return m != NULL && strcmp(m, "all") == 0;
}

size_t la_bid_lookahead(size_t dflt_kib)
{
	const char *v = getenv("LA_GPU_BID_LOOKAHEAD_KIB");
	size_t kib = dflt_kib;
	if (v != NULL && atol(v) > 0)
		kib = (size_t)atol(v);
	if (kib > (64u << 10))
		kib = 64u << 10;
	return kib << 10;
}

/* as many bytes as upstream has, at most `want`; *got = how many (0: none) */
const unsigned char *la_bid_peek(struct archive_read_filter *filter, size_t want, size_t *got)
{
	ssize_t avail = 0;
	const unsigned char *p = __archive_read_filter_ahead(filter, want, &avail);
	if (p == NULL && avail > 0)
		p = __archive_read_filter_ahead(filter, (size_t)avail, &avail);
	if (p == NULL || avail <= 0) {
		*got = 0;
		return NULL;
	}
	*got = (size_t)avail < want ? (size_t)avail : want;
	return p;
}

int la_bid_declines(struct archive_read_filter *filter, int (*parallel)(const unsigned char *, size_t, size_t))
{
	if (la_bid_take_all())
		return 0;
	const size_t la = la_bid_lookahead(1024);
	size_t got = 0;
	const unsigned char *w = la_bid_peek(filter, la, &got);
	return w != NULL && !parallel(w, got, la);
}

int la_gz_flush_points_enabled(void)
{
	const char *v = getenv("LA_GZIP_FLUSH_POINTS");
	return v != NULL && (v[0] == '1' || strcmp(v, "chain") == 0);
}

/* LA_ZSTD_BLOCKS=1: the zstd filter decodes the blocks of a frame in parallel (LA_ZSTD_OPT_BLOCK_PARALLEL) on windows
 * of large frames, so ONE long frame is no serial unit any more and the bidder takes it.  Read from the environment at
 * every call, as la_gz_flush_points_enabled is: the bidder asks at bid time, the filter once in its init, so a process
 * that changes the variable between the two gets a filter that took the stream and decodes it on the frame kernels
 * (or the reverse): slow, never wrong */
int la_zstd_blocks_enabled(void)
{
	const char *v = getenv("LA_ZSTD_BLOCKS");
	return v != NULL && v[0] == '1';
}

/* LA_GZIP_FLUSH_POINTS=chain: piece mode as for =1 (the same bid evidence), and the pieces are decoded as one stream
 * (LA_GZ_OPT_CHAIN): blocks behind a flush point may reach back over it (Z_SYNC_FLUSH, pigz without -i) */
int la_gz_flush_points_chain(void)
{
	const char *v = getenv("LA_GZIP_FLUSH_POINTS");
	return v != NULL && strcmp(v, "chain") == 0;
}

/* LA_GZIP_BLOCK_STARTS=1: ONE ordinary member -- no flush point, no second header -- is no serial unit any more: the
 * filter lets the device find its block starts and decodes it as a chain of pieces (LA_GZ_OPT_BLOCK_STARTS), so the
 * bidder takes it.  Read at every call, as la_gz_flush_points_enabled is. */
int la_gz_block_starts_enabled(void)
{
	const char *v = getenv("LA_GZIP_BLOCK_STARTS");
	return v != NULL && v[0] == '1';
}

/* LA_GZIP_FLUSH_POINTS=1: ONE member whose body is a chain of flush points (00 00 FF FF, la_gz_pieces_build) decodes a
 * piece per lane.  Evidence inside the look-ahead: at least LA_BID_GZ_MARKERS markers behind the header, none further
 * than LA_BID_GZ_GAP from the one before (the first: from the header) -- the pieces of zlib's Z_FULL_FLUSH writers,
 * pigz -i and gzip:single-member are that close; four stray 00 00 FF FF in 256 KiB of a plain deflate stream, each
 * within 128 KiB of the last, are not impossible, and such a stream then costs what LA_GPU_BID=all costs. */
#define LA_BID_GZ_MARKERS 4u
#define LA_BID_GZ_GAP     ((size_t)128 << 10)
static int gzip_flush_points(const unsigned char *p, size_t n, size_t hdr_len)
{
	size_t prev = hdr_len;
	for (unsigned k = 0; k < LA_BID_GZ_MARKERS; k++) {
		const size_t mk = (size_t)la_gz_next_marker(p, n, prev);
		if (mk >= n || mk - prev > LA_BID_GZ_GAP)
			return 0;
		prev = mk + 4;
	}
	return 1;
}

/* gzip: p[0..n) starts with a member whose header (hdr_len bytes, parsed by the caller) carries no BGZF size.
 * 1 = take it.  A second member header inside the look-ahead counts as evidence of a many-member stream; the
 * candidate test is the strict one of the boundary search (XFL / OS bytes that real writers emit).  With
 * LA_GZIP_FLUSH_POINTS=1 a chain of flush points counts too; with LA_GZIP_BLOCK_STARTS=1 a lone member needs no
 * evidence at all. */
int la_bid_gzip_parallel(const unsigned char *p, size_t n, size_t hdr_len, size_t lookahead)
{
	if (n < lookahead)
		return 1;	/* the whole stream is smaller than the look-ahead */
	if (la_gz_block_starts_enabled())
		return 1;
	if (la_gz_flush_points_enabled() && gzip_flush_points(p, n, hdr_len))
		return 1;
	for (size_t i = hdr_len + 1; i + 10 <= n; i++) {
		const unsigned char *q = memchr(p + i, 0x1f, n - 10 - i + 1);
		if (q == NULL)
			break;
		i = (size_t)(q - p);
		if (q[1] == 0x8b && q[2] == 0x08 && (q[3] & 0xE0) == 0 && (q[8] == 0 || q[8] == 2 || q[8] == 4) &&
		    (q[9] <= 13 || q[9] == 255))
			return 1;
	}
	return 0;
}

/* lz4: 1 = take it.  A frame without a content checksum decodes block-parallel whatever its size; a frame WITH one is
 * bound by its XXH32 chain, so it has to end inside the look-ahead (then the stream is made of frames that small). */
int la_bid_lz4_parallel(const unsigned char *p, size_t n, size_t lookahead)
{
	if (n < lookahead || n < 11)
		return 1;
	const uint32_t magic = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
	if (magic != 0x184D2204u)
		return 1;	/* legacy frame: no checksums */
	const unsigned flg = p[4];
	if (!(flg & 0x04))
		return 1;	/* no content checksum */
	size_t pos = 4 + 3 + ((flg & 0x08) ? 8 : 0) + ((flg & 0x01) ? 4 : 0);
	const int bsum = (flg & 0x10) != 0;
	while (pos + 4 <= n) {
		const uint32_t w = (uint32_t)p[pos] | (uint32_t)p[pos + 1] << 8 | (uint32_t)p[pos + 2] << 16 | (uint32_t)p[pos + 3] << 24;
		if (w == 0)
			return 1;	/* EndMark inside the look-ahead */
		pos += 4 + (size_t)(w & 0x7FFFFFFFu) + (bsum ? 4 : 0);
	}
	return 0;
}

/* zstd: 1 = take it: the first frame (skippable frames in front of it passed over) ends inside the look-ahead; with
 * LA_ZSTD_BLOCKS=1 a longer frame too (it is by construction many blocks of at most 128 KiB) */
int la_bid_zstd_parallel(const unsigned char *p, size_t n, size_t lookahead)
{
	if (n < lookahead || la_zstd_blocks_enabled())
		return 1;
	la_zstd_frame fr[4];
	la_zstd_index_result r;
	memset(&r, 0, sizeof(r));
	if (la_zstd_index_build(p, n, 0, ~0ull, fr, 4, &r) != 0)
		return 1;	/* let the filter report what is wrong with it */
	return r.n_frames >= 1;
}

/* xz: 1 = take it: the first block header carries a compressed size (a threaded writer: every block does, and the host
 * hops from header to header), the stream has no block at all, or the look-ahead already holds the whole stream.  A
 * block without a compressed size is one serial chain whose end only its decoder finds. */
int la_bid_xz_parallel(const unsigned char *p, size_t n, size_t lookahead)
{
	if (n < lookahead || n < 14)
		return 1;
	return p[12] == 0 || (p[13] & 0x40) != 0;
}

/* lzip: 1 = take it: the look-ahead holds the whole stream, or it shows a confirmed second member -- the first header
 * shape at an offset o whose preceding 8 bytes, the member size of a version 1 trailer, say o (la_filter_lzip.c chains
 * members by the same rule).  A first member longer than the look-ahead is one serial chain. */
int la_bid_lzip_parallel(const unsigned char *p, size_t n, size_t lookahead)
{
	if (n < lookahead)
		return 1;
	for (size_t o = 6 + 5 + 20; o + 6 <= n; o++) {
		const unsigned char *q = memchr(p + o, 'L', n - 6 - o + 1);
		if (q == NULL)
			break;
		o = (size_t)(q - p);
		if (memcmp(q, "LZIP", 4) != 0 || q[4] > 1 || (q[5] & 31) < 12 || (q[5] & 31) > 29)
			continue;
		uint64_t msize = 0;
		for (unsigned k = 0; k < 8; k++)
			msize |= (uint64_t)(q - 8)[k] << (8 * k);
		if (msize == o)
			return 1;
	}
	return 0;
}

/* lzop: 1 = take it: the look-ahead holds the whole stream, or the first block ends inside it (`lzop` writes blocks of
 * 256 KiB, and a stream is then thousands of them).  A first block longer than the look-ahead is one serial chain: the
 * format allows blocks of up to 64 MiB.  p[0, 9) is the magic.  The header's fields are walked as la_filter_lzop.c walks
 * them (lzop.c:221-296), its checksum and refusals left to the filter: a header the walk cannot follow is taken, so
 * that the filter says what is wrong with it. */
int la_bid_lzop_parallel(const unsigned char *p, size_t n, size_t lookahead)
{
	if (n < lookahead || n < 9 + 29)
		return 1;
	size_t at = 9;
	const unsigned version = ((unsigned)p[at] << 8) | p[at + 1];
	at += 4;
	if (version >= 0x940)
		at += 2;
	at += 1;
	if (version >= 0x940)
		at += 1;
	const uint32_t flags = (uint32_t)p[at] << 24 | (uint32_t)p[at + 1] << 16 | (uint32_t)p[at + 2] << 8 | p[at + 3];
	at += 4;
	if (flags & 0x0800u)
		at += 4;
	at += 4 + (version >= 0x940 ? 8 : 4);
	at += 1 + (size_t)p[at] + 4;	/* the name and the header's checksum */
	if (flags & 0x0040u) {
		if (at > n || n - at < 4)
			return 0;
		const uint64_t skip = ((uint64_t)p[at] << 24 | (uint64_t)p[at + 1] << 16 | (uint64_t)p[at + 2] << 8 | p[at + 3]) + 8;
		if (skip > n - at)
			return 0;
		at += (size_t)skip;
	}
	if (at > n || n - at < 8)
		return 0;
	const uint32_t usize = (uint32_t)p[at] << 24 | (uint32_t)p[at + 1] << 16 | (uint32_t)p[at + 2] << 8 | p[at + 3];
	const uint32_t csize = (uint32_t)p[at + 4] << 24 | (uint32_t)p[at + 5] << 16 | (uint32_t)p[at + 6] << 8 | p[at + 7];
	if (usize == 0 || usize > ((uint32_t)64 << 20) || csize > usize)
		return 1;	/* an empty part, or a header the filter refuses */
	/* (at most two checksum words stand between the sizes and the data) */
	return (uint64_t)csize + 16 <= n - at;
}

/*
 * Window plumbing: the window configuration and its ramp, opening the device, the "GPU data plane" error strings,
 * the buffer growers, the gather loop, the carry of the unfinished unit, the deferred verdict and the held-back
 * delivery.  What differs between the filters -- the walker, the launch, the stream-order walk of the results --
 * stays in each filter.
 */
#define MIB ((size_t)1 << 20)

int la_env_device(void)
{
	const char *d = getenv("LA_GPU_DEVICE");
	return d ? atoi(d) : 0;
}

static size_t env_mib(const char *name, int dflt)
{
	const char *v = getenv(name);
	return (size_t)(v && atoi(v) > 0 ? atoi(v) : dflt) << 20;
}

int la_window_open(struct archive_read_filter *self, la_window *w, const char *name)
{
	w->name = name;
	/* The window RAMPS: the first one holds 16 MiB of the stream, the next 32, up to the target.  What a window
	 * costs before its first byte comes back -- pinned staging and slab of its size (about half a millisecond
	 * per MiB), the gather, the upload -- is paid before anything overlaps, so a stream of 1 GiB took 1.0 s
	 * with fixed 256 MiB windows and 0.48 s with 16 MiB ones, and 16 GiB 1.70 s against 1.41 s at 64 MiB
	 * (profiles/r03_alevel.txt): small streams want small windows, long ones 64-128 MiB. */
	w->target_bytes = env_mib("LA_GPU_BATCH_MIB", 64);
	w->batch_bytes = w->target_bytes < 16 * MIB ? w->target_bytes : 16 * MIB;
	w->max_batch_bytes = env_mib("LA_GPU_MAX_BATCH_MIB", 2048);
	w->out_budget = env_mib("LA_GPU_OUT_BUDGET_MIB", 4096);
	const int rc = la_gpu_open(la_env_device(), &w->gpu);
	if (rc != LA_OK) {
		w->gpu = NULL;
		archive_set_error(&self->archive->archive, ARCHIVE_ERRNO_MISC,
		    "Can't initialize %s GPU data plane (la_gpu_open: %d); no CPU fallback is built", name, rc);
		return ARCHIVE_FATAL;
	}
	return ARCHIVE_OK;
}

void la_window_ramp(la_window *w)
{
	if (w->batch_bytes < w->target_bytes)
		w->batch_bytes = w->batch_bytes * 2 < w->target_bytes ? w->batch_bytes * 2 : w->target_bytes;
}

int la_window_fail(struct archive_read_filter *self, const la_window *w, const char *what)
{
	archive_set_error(&self->archive->archive, ARCHIVE_ERRNO_MISC,
	    "%s GPU data plane: %s failed: %s", w->name, what, w->gpu ? la_gpu_last_error(w->gpu) : "no device");
	return ARCHIVE_FATAL;
}

/* Growers: the capacity starts at 1 MiB and doubles until it holds `need`.  0, or -1 when the allocation failed. */
static size_t grown(size_t cap, size_t need)
{
	size_t nc = cap ? cap : MIB;
	while (nc < need)
		nc *= 2;
	return nc;
}

int la_buf_pinned(la_gpu_ctx *gpu, la_buf *b, size_t need, size_t keep)
{
	if (b->cap >= need)
		return 0;
	const size_t nc = grown(b->cap, need);
	void *np = NULL;
	if (la_gpu_malloc_host(gpu, &np, nc) != LA_OK)
		return -1;	/* (the old buffer stays) */
	if (keep)
		memcpy(np, b->p, keep);
	if (b->p)
		la_gpu_free_host(gpu, b->p);
	b->p = np;
	b->cap = nc;
	b->kind = LA_BUF_PINNED;
	return 0;
}

int la_buf_dev(la_gpu_ctx *gpu, la_buf *b, size_t need)
{
	if (b->cap >= need)
		return 0;
	const size_t nc = grown(b->cap, need);
	la_buf_release(gpu, b);
	void *np = NULL;
	if (la_gpu_malloc(gpu, &np, nc) != LA_OK)
		return -1;
	b->p = np;
	b->cap = nc;
	b->kind = LA_BUF_DEV;
	return 0;
}

int la_buf_host(la_buf *b, size_t need)
{
	if (b->cap >= need)
		return 0;
	const size_t nc = grown(b->cap, need);
	la_buf_release(NULL, b);
	if ((b->p = malloc(nc)) == NULL)
		return -1;
	b->cap = nc;
	b->kind = LA_BUF_HOST;
	return 0;
}

void la_buf_release(la_gpu_ctx *gpu, la_buf *b)
{
	if (b->p) {
		if (b->kind == LA_BUF_PINNED)
			la_gpu_free_host(gpu, b->p);
		else if (b->kind == LA_BUF_DEV)
			la_gpu_free(gpu, b->p);
		else
			free(b->p);
	}
	b->p = NULL;
	b->cap = 0;
}

int la_window_gather(struct archive_read_filter *self, la_window *w, la_buf *stage, size_t *len)
{
	const size_t want = w->batch_bytes;
	while (!w->upstream_eof && *len < want) {
		ssize_t avail;
		const void *up = __archive_read_filter_ahead(self->upstream, 1, &avail);
		if (up == NULL) {
			if (avail < 0)
				return ARCHIVE_FATAL;	/* upstream already set the error */
			w->upstream_eof = 1;
			break;
		}
		size_t n = (size_t)avail;
		if (n > want - *len)
			n = want - *len;
		/* a stream that has already filled 8 MiB gets the whole window at once instead of
		 * five more rounds of pin-a-bigger-buffer-and-copy */
		size_t need = *len + n;
		if (need > 8 * MIB && need < want)
			need = want;
		if (la_buf_pinned(w->gpu, stage, need, *len) < 0)
			return la_window_fail(self, w, "pinned staging allocation");
		memcpy(stage->p + *len, up, n);
		*len += n;
		__archive_read_filter_consume(self->upstream, (int64_t)n);
	}
	return ARCHIVE_OK;
}

int la_window_carry(struct archive_read_filter *self, la_window *w, la_buf *stage, size_t *len, size_t used, int more,
    const char *unit)
{
	if (more && used == 0 && *len >= w->batch_bytes) {
		/* one unit larger than the window: widen it, as the other filters do */
		if (*len >= w->max_batch_bytes) {
			archive_set_error(&self->archive->archive, ARCHIVE_ERRNO_MISC,
			    "%s %s too large for the GPU data plane (more than %llu compressed bytes; LA_GPU_MAX_BATCH_MIB)",
			    w->name, unit, (unsigned long long)w->max_batch_bytes);
			return ARCHIVE_FATAL;
		}
		w->batch_bytes = *len * 2 < w->max_batch_bytes ? *len * 2 : w->max_batch_bytes;
	}
	memmove(stage->p, stage->p + used, *len - used);
	*len -= used;
	return ARCHIVE_OK;
}

void la_verdict_set(la_verdict *v, int rc, const char *fmt, ...)
{
	v->rc = rc;
	v->has_msg = fmt != NULL;
	if (fmt) {
		va_list ap;
		va_start(ap, fmt);
		vsnprintf(v->msg, sizeof(v->msg), fmt, ap);
		va_end(ap);
	}
}

int la_verdict_report(struct archive_read_filter *self, const la_verdict *v)
{
	if (v->has_msg)
		archive_set_error(&self->archive->archive, ARCHIVE_ERRNO_MISC, "%s", v->msg);
	return v->rc;
}

int la_holdback_open(la_holdback *h)
{
	return (h->tail = malloc((size_t)LA_OUT_BLOCK)) != NULL ? 0 : -1;
}

static uint64_t block_floor(uint64_t n)
{
	return n / LA_OUT_BLOCK * LA_OUT_BLOCK;
}

void la_holdback_end(la_holdback *h, int rc, const char *msg, int how)
{
	if (msg)
		la_verdict_set(&h->verdict, rc, "%s", msg);
	else
		la_verdict_set(&h->verdict, rc, NULL);
	h->ended = 1;
	const uint64_t t = h->total - h->base;	/* (base is 0 unless the filter moved it: la_holdback_rebase) */
	h->end_limit = how == LA_HB_ALL ? h->total : h->base + block_floor(how == LA_HB_EARLY && t ? t - 1 : t);
}

void la_holdback_rebase(la_holdback *h)
{
	h->base = h->total;
}

/* bytes that may be handed out: while the stream goes on, whatever follows is at best an early error */
static uint64_t holdback_limit(const la_holdback *h)
{
	return h->ended ? h->end_limit : h->base + block_floor(h->total > h->base ? h->total - h->base - 1 : 0);
}

ssize_t la_holdback_read(struct archive_read_filter *self, const la_window *w, la_holdback *h, const void **p,
    int (*window)(struct archive_read_filter *))
{
	*p = NULL;
	if (h->finished)
		return 0;
	for (;;) {
		const uint64_t limit = holdback_limit(h);
		if (h->tail_len && h->delivered + h->tail_len <= limit) {
			const size_t k = h->tail_len;
			*p = h->tail;
			h->tail_len = 0;
			h->delivered += k;
			return (ssize_t)k;
		}
		if (h->tail_len == 0 && h->out_pos < h->out_len && h->delivered < limit) {
			size_t k = h->out_len - h->out_pos;
			if (k > limit - h->delivered)
				k = (size_t)(limit - h->delivered);
			*p = h->out.p + h->out_pos;
			h->out_pos += k;
			h->delivered += k;
			return (ssize_t)k;
		}
		if (h->ended) {
			h->finished = 1;
			if (h->verdict.rc != ARCHIVE_OK)
				return la_verdict_report(self, &h->verdict);
			return 0;
		}
		/* what the window holds beyond `limit` (with the tail, at most one block) waits for the next window's verdict */
		if (h->out_pos < h->out_len) {
			const size_t k = h->out_len - h->out_pos;
			if (h->tail_len + k > LA_OUT_BLOCK) {
				archive_set_error(&self->archive->archive, ARCHIVE_ERRNO_MISC, "%s filter: held-back bytes exceed one block", w->name);
				h->finished = 1;
				return ARCHIVE_FATAL;
			}
			memcpy(h->tail + h->tail_len, h->out.p + h->out_pos, k);
			h->tail_len += k;
		}
		h->out_len = h->out_pos = 0;
		const int r = window(self);
		if (r != ARCHIVE_OK) {
			h->finished = 1;
			return r;
		}
	}
}

void la_holdback_release(la_gpu_ctx *gpu, la_holdback *h)
{
	la_buf_release(gpu, &h->out);
	free(h->tail);
	h->tail = NULL;
}

int la_reader_open(struct archive_read_filter *self, la_reader *r, const char *name, size_t host_tab_bytes,
    uint64_t max_out_budget, const char *nomem_msg)
{
	if (r == NULL || (r->h_tabs.p = calloc(1, host_tab_bytes)) == NULL || la_holdback_open(&r->hb) < 0)
		archive_set_error(&self->archive->archive, ENOMEM, "%s", nomem_msg);
	else if (la_window_open(self, &r->w, name) == ARCHIVE_OK) {
		if (max_out_budget && (r->w.out_budget == 0 || r->w.out_budget > max_out_budget))
			r->w.out_budget = max_out_budget;
		return ARCHIVE_OK;
	}
	if (r) {
		la_holdback_release(NULL, &r->hb);
		la_buf_release(NULL, &r->h_tabs);
	}
	return ARCHIVE_FATAL;
}

int la_reader_gather(struct archive_read_filter *self, la_reader *r)
{
	const int rc = la_window_gather(self, &r->w, &r->stage, &r->stage_len);
	if (rc != ARCHIVE_OK || r->stage_len == 0)
		return rc;
	if (la_buf_dev(r->w.gpu, &r->d_src, r->stage_len + 64) < 0)
		return la_window_fail(self, &r->w, "la_gpu_malloc");
	if (la_gpu_memcpy_h2d(r->w.gpu, r->d_src.p, r->stage.p, r->stage_len) != LA_OK)
		return la_window_fail(self, &r->w, "la_gpu_memcpy_h2d");
	return ARCHIVE_OK;
}

int la_reader_take(struct archive_read_filter *self, la_reader *r, uint64_t bytes)
{
	la_holdback *h = &r->hb;
	if (bytes) {
		if (la_buf_pinned(r->w.gpu, &h->out, h->out_len + (size_t)bytes + 64, h->out_len) < 0)
			return la_window_fail(self, &r->w, "la_gpu_malloc_host");
		if (la_gpu_memcpy_d2h(r->w.gpu, h->out.p + h->out_len, r->d_dst.p, bytes) != LA_OK || la_gpu_sync(r->w.gpu) != LA_OK)
			return la_window_fail(self, &r->w, "la_gpu_memcpy_d2h");
	}
	h->out_len += (size_t)bytes;
	h->total += bytes;
	return ARCHIVE_OK;
}

int la_reader_finish(struct archive_read_filter *self, la_reader *r, size_t used, int more, const char *unit)
{
	la_window_ramp(&r->w);
	if (r->hb.ended)
		return ARCHIVE_OK;
	return la_window_carry(self, &r->w, &r->stage, &r->stage_len, used, more, unit);
}

ssize_t la_reader_read(struct archive_read_filter *self, la_reader *r, const void **p, int (*window)(struct archive_read_filter *))
{
	return la_holdback_read(self, &r->w, &r->hb, p, window);
}

void la_reader_close(la_reader *r)
{
	la_gpu_ctx *gpu = r->w.gpu;
	(void)la_gpu_sync(gpu);
	la_buf_release(gpu, &r->d_src);
	la_buf_release(gpu, &r->d_dst);
	la_buf_release(gpu, &r->d_tabs);
	la_holdback_release(gpu, &r->hb);
	la_buf_release(gpu, &r->stage);
	la_gpu_close(gpu);
	la_buf_release(NULL, &r->h_tabs);
}

uint64_t la_reader_solo_cap(const la_reader *r, uint64_t *solo_cap, uint64_t have)
{
	if (*solo_cap == 0)
		*solo_cap = have * 8 > MIB ? have * 8 : MIB;
	if (*solo_cap > r->w.out_budget)
		*solo_cap = r->w.out_budget;
	return *solo_cap;
}

int la_reader_solo_full(struct archive_read_filter *self, const la_reader *r, uint64_t *solo_cap, uint64_t cap, const char *unit)
{
	if (cap >= r->w.out_budget) {
		archive_set_error(&self->archive->archive, ARCHIVE_ERRNO_MISC,
		    "%s %s too large for the GPU data plane (more than %llu decoded bytes; LA_GPU_OUT_BUDGET_MIB)",
		    r->w.name, unit, (unsigned long long)r->w.out_budget);
		return ARCHIVE_FATAL;
	}
	*solo_cap = cap * 2;
	return ARCHIVE_OK;
}
