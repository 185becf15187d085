/*
 * la_filter_lzop.c -- the lzop read filter on the MI355X data plane.
 *
 * Mirrors libarchive/archive_read_support_filter_lzop.c: the same bidder (lzop.c:131-148: the nine magic bytes, 72
 * bits), filter code and name (ARCHIVE_FILTER_LZOP, "lzop", lzop.c:185-186), vtable shape (read / close, lzop.c:171-175),
 * consume_header (lzop.c:201-308) and consume_block_info (lzop.c:310-360) restated field for field, and the strings and
 * return codes of lzop_filter_read (lzop.c:362-483).  Where the reference hands liblzo2 one block per read, this filter
 * gathers a window of the stream, hops from block header to block header on the host -- both sizes and the checksums of
 * a block stand in front of it, so nothing is scanned or guessed -- and sends ALL blocks of the window to the device in
 * ONE la_gpu_lzop_decode call: the sum over the compressed bytes, the LZO1X decode (or the copy of a stored block), the
 * sum over the decoded bytes.  What the window did not finish (a header or a block that runs off its end) opens the
 * next one.  A block larger than LA_GPU_MAX_BATCH_MIB compressed is refused by name.  No CPU fallback.
 *
 * Restated as they stand in the reference:
 *   - the 29-byte look-ahead behind the magic (a header is at most 29 bytes up to its name), so a stream that ends
 *     sooner is "Truncated lzop data" even where its header is shorter;
 *   - a part ends at a block of size 0; then another magic starts a part, and anything else -- junk, fewer than nine
 *     bytes -- ends the stream without an error;
 *   - CRC32 wins over Adler-32 where both flags are set;
 *   - the stale checksum: with a *_COMPRESSED flag and no *_UNCOMPRESSED one a stored block reads no checksum word, and
 *     its bytes are compared with the value the block in front of it left, or 0 (lzop.c:335-350, :419-429).  The walk
 *     keeps both words as the reference does and hands the device what the reference would compare with;
 *   - an extra field that runs off the stream is skipped blind (lzop.c:294-295 ignores the consume's answer), and the
 *     next block header is what is truncated.
 *
 * Bytes in front of an error.  The reference hands out one block per read, so every block in front of the failing one
 * is out when the error is returned, and nothing of the failing block is: the filter takes the bytes of the good blocks,
 * restarts the hold-back grid there (la_holdback_rebase) and ends the stream with LA_HB_ALL.
 */
#include "la_read_private.h"
#include "la_host.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define LZOP_HEADER_MAGIC "\x89\x4c\x5a\x4f\x00\x0d\x0a\x1a\x0a"
#define LZOP_HEADER_MAGIC_LEN 9

/* lzop.c:85-92 */
#define FILTER			0x0800
#define CRC32_HEADER		0x1000
#define EXTRA_FIELD		0x0040
#define ADLER32_UNCOMPRESSED	0x0001
#define ADLER32_COMPRESSED	0x0002
#define CRC32_UNCOMPRESSED	0x0100
#define CRC32_COMPRESSED	0x0200
#define MAX_BLOCK_SIZE		(64 * 1024 * 1024)

#define LZO_TAB_CAP 4096u	/* blocks one launch takes; a window with more is taken in parts */

struct lzop_private {
	la_reader r;			/* stage: from the first byte of the unfinished header or block on; d_tabs: block table, results */
	la_lzop_block *tab;		/* host copies of the tables (LZO_TAB_CAP entries each), in r.h_tabs */
	la_lzop_result *res;
	/* struct read_lzop's fields (lzop.c:71-83) at the walk's position */
	char in_stream;
	unsigned flags;
	uint32_t compressed_cksum, uncompressed_cksum;
	/* how the stream ends, once the walk or a result has shown it; reported behind the bytes of the blocks in front */
	int end_rc;
	char end_msg[64];
};

static int lzop_bidder_bid(struct archive_read_filter_bidder *, struct archive_read_filter *);
static int lzop_bidder_init(struct archive_read_filter *);
static ssize_t lzop_filter_read(struct archive_read_filter *, const void **);
static int lzop_filter_close(struct archive_read_filter *);

static const struct archive_read_filter_bidder_vtable lzop_bidder_vtable = {
	.bid = lzop_bidder_bid,
	.init = lzop_bidder_init,
};
static const struct archive_read_filter_vtable lzop_reader_vtable = {
	.read = lzop_filter_read,
	.close = lzop_filter_close,
};

int archive_read_support_filter_lzop(struct archive *_a)
{
	struct archive_read *a = (struct archive_read *)_a;
	if (__archive_read_register_bidder(a, NULL, "lzop", &lzop_bidder_vtable) != ARCHIVE_OK)
		return ARCHIVE_FATAL;
	return ARCHIVE_OK;
}

/* lzop.c:131-148 */
static int lzop_bidder_bid(struct archive_read_filter_bidder *self, struct archive_read_filter *filter)
{
	ssize_t avail;
	(void)self;
	const unsigned char *p = __archive_read_filter_ahead(filter, LZOP_HEADER_MAGIC_LEN, &avail);
	if (p == NULL || avail == 0)
		return 0;
	if (memcmp(p, LZOP_HEADER_MAGIC, LZOP_HEADER_MAGIC_LEN))
		return 0;
	/* Default policy (la_bid_policy.c): one block is one serial chain; a stream whose first block does not end inside the
	 * look-ahead is left to liblzo2 on a host core. */
	if (la_bid_declines(filter, la_bid_lzop_parallel))
		return 0;
	return LZOP_HEADER_MAGIC_LEN * 8;
}

static int lzop_bidder_init(struct archive_read_filter *self)
{
	self->code = ARCHIVE_FILTER_LZOP;
	self->name = "lzop";
	struct lzop_private *st = calloc(1, sizeof(*st));
	if (la_reader_open(self, st ? &st->r : NULL, "lzop", (sizeof(la_lzop_block) + sizeof(la_lzop_result)) * LZO_TAB_CAP, 0,
	    "Can't allocate data for lzop decompression") != ARCHIVE_OK) {	/* lzop.c:190-191 */
		free(st);
		return ARCHIVE_FATAL;
	}
	st->tab = (la_lzop_block *)st->r.h_tabs.p;
	st->res = (la_lzop_result *)(st->tab + LZO_TAB_CAP);
	self->data = st;
	self->vtable = &lzop_reader_vtable;
	return ARCHIVE_OK;
}

/* adler32() over a header (at most 29 + 255 bytes): zlib's, from the fresh value 1 */
static uint32_t lzop_adler32(const uint8_t *p, size_t n)
{
	uint32_t a = 1, b = 0;
	for (size_t i = 0; i < n; i++) {
		a = (a + p[i]) % 65521u;
		b = (b + a) % 65521u;
	}
	return (b << 16) | a;
}

enum { WK_OK, WK_MORE, WK_END };

static int wk_end(struct lzop_private *st, int rc, const char *msg)
{
	st->end_rc = rc;
	snprintf(st->end_msg, sizeof(st->end_msg), "%s", msg ? msg : "");
	return WK_END;
}

/* `need` bytes at *pos: WK_OK; they are not there: WK_MORE while upstream goes on, else the reference's "truncated" */
static int wk_ahead(struct lzop_private *st, size_t len, int eof, size_t pos, size_t need)
{
	if (len - pos >= need)
		return WK_OK;
	return eof ? wk_end(st, ARCHIVE_FAILED, "Truncated lzop data") : WK_MORE;
}

/* consume_header, lzop.c:201-308, over src[*pos, len).  *pos moves only on WK_OK. */
static int wk_header(struct lzop_private *st, const uint8_t *src, size_t len, int eof, size_t *pos)
{
	size_t at = *pos;
	int r;
	if (len - at < LZOP_HEADER_MAGIC_LEN)
		return eof ? wk_end(st, ARCHIVE_OK, NULL) : WK_MORE;
	if (memcmp(src + at, LZOP_HEADER_MAGIC, LZOP_HEADER_MAGIC_LEN))
		return wk_end(st, ARCHIVE_OK, NULL);
	at += LZOP_HEADER_MAGIC_LEN;
	if ((r = wk_ahead(st, len, eof, at, 29)) != WK_OK)
		return r;
	const unsigned char *p = src + at, *_p = p;
	const unsigned version = archive_be16dec(p);
	p += 4;	/* version(2 bytes) + library version(2 bytes) */
	if (version >= 0x940) {
		const unsigned reqversion = archive_be16dec(p); p += 2;
		if (reqversion < 0x900)
			return wk_end(st, ARCHIVE_FAILED, "Invalid required version");
	}
	const unsigned method = *p++;
	if (method < 1 || method > 3)
		return wk_end(st, ARCHIVE_FAILED, "Unsupported method");
	if (version >= 0x940) {
		const unsigned level = *p++;
		if (level > 9)
			return wk_end(st, ARCHIVE_FAILED, "Invalid level");
	}
	const unsigned flags = archive_be32dec(p); p += 4;
	if (flags & FILTER)
		p += 4;	/* Skip filter */
	p += 4;	/* Skip mode */
	p += version >= 0x940 ? 8 : 4;	/* Skip mtime */
	size_t hlen = *p++;	/* Read filename length */
	hlen += (size_t)(p - _p);
	if ((r = wk_ahead(st, len, eof, at, hlen + 4)) != WK_OK)
		return r;
	const uint32_t checksum = (flags & CRC32_HEADER) ? (uint32_t)la_crc32_host(0, _p, hlen) : lzop_adler32(_p, hlen);
	if (archive_be32dec(_p + hlen) != checksum)
		return wk_end(st, ARCHIVE_FAILED, "Corrupted lzop header");
	at += hlen + 4;
	if (flags & EXTRA_FIELD) {
		/* Skip extra field */
		if ((r = wk_ahead(st, len, eof, at, 4)) != WK_OK)
			return r;
		const uint64_t skip = (uint64_t)archive_be32dec(src + at) + 4 + 4;
		if (skip > len - at) {
			if (!eof)
				return WK_MORE;
			at = len;	/* (the reference skips blind; the block header behind it is what is missing) */
		} else
			at += (size_t)skip;
	}
	st->flags = flags;
	st->in_stream = 1;
	*pos = at;
	return WK_OK;
}

/* consume_block_info, lzop.c:310-360, and the look-ahead for the block's bytes (lzop.c:412-418), over src[*pos, len).
 * WK_OK: *b is the block (dst_off is the caller's) and *pos stands behind it; *b with dst_len 0: the part ended.  The
 * filter's state and *pos move only on WK_OK. */
static int wk_block(struct lzop_private *st, const uint8_t *src, size_t len, int eof, size_t *pos, la_lzop_block *b)
{
	size_t at = *pos;
	const unsigned flags = st->flags;
	uint32_t ccksum = st->compressed_cksum, ucksum = st->uncompressed_cksum;
	int r;
	memset(b, 0, sizeof(*b));
	if ((r = wk_ahead(st, len, eof, at, 4)) != WK_OK)
		return r;
	const uint32_t usize = archive_be32dec(src + at);
	at += 4;
	if (usize == 0) {
		st->in_stream = 0;
		*pos = at;
		return WK_OK;
	}
	if (usize > MAX_BLOCK_SIZE)
		return wk_end(st, ARCHIVE_FAILED, "Corrupted lzop header");
	if ((r = wk_ahead(st, len, eof, at, 4)) != WK_OK)
		return r;
	const uint32_t csize = archive_be32dec(src + at);
	at += 4;
	if (csize > usize)
		return wk_end(st, ARCHIVE_FAILED, "Corrupted lzop header");
	if (flags & (CRC32_UNCOMPRESSED | ADLER32_UNCOMPRESSED)) {
		if ((r = wk_ahead(st, len, eof, at, 4)) != WK_OK)
			return r;
		ccksum = ucksum = archive_be32dec(src + at);
		at += 4;
	}
	if ((flags & (CRC32_COMPRESSED | ADLER32_COMPRESSED)) && csize < usize) {
		if ((r = wk_ahead(st, len, eof, at, 4)) != WK_OK)
			return r;
		ccksum = archive_be32dec(src + at);
		at += 4;
	}
	if (len - at < csize) {
		if (!eof)
			return WK_MORE;
		/* (the block info is consumed by then, and its words are the stream's state) */
		st->compressed_cksum = ccksum; st->uncompressed_cksum = ucksum;
		return wk_end(st, ARCHIVE_FATAL, "Truncated lzop data");
	}
	b->src_off = at;
	b->src_len = csize;
	b->dst_len = usize;
	b->flags = (flags & CRC32_COMPRESSED ? LA_LZOP_C_CRC32 : 0u) | (flags & ADLER32_COMPRESSED ? LA_LZOP_C_ADLER32 : 0u);
	if (csize != usize)	/* a stored block is handed out before the second sum is looked at (lzop.c:435-440) */
		b->flags |= (flags & CRC32_UNCOMPRESSED ? LA_LZOP_U_CRC32 : 0u) | (flags & ADLER32_UNCOMPRESSED ? LA_LZOP_U_ADLER32 : 0u);
	b->sum_c = ccksum;
	b->sum_u = ucksum;
	st->compressed_cksum = ccksum; st->uncompressed_cksum = ucksum;
	*pos = at + csize;
	return WK_OK;
}

/* Decode tab[0, n) in one call; the results are in st->res. */
static int lzo_launch(struct archive_read_filter *self, struct lzop_private *st, uint32_t n, uint64_t dst_bytes)
{
	la_reader *r = &st->r;
	la_gpu_ctx *gpu = r->w.gpu;
	const size_t o_res = sizeof(la_lzop_block) * LZO_TAB_CAP;
	if (la_buf_dev(gpu, &r->d_dst, (size_t)dst_bytes + 64) < 0)
		return la_window_fail(self, &r->w, "la_gpu_malloc");
	la_lzop_batch bt;
	memset(&bt, 0, sizeof(bt));
	bt.d_src = r->d_src.p; bt.src_bytes = r->stage_len;
	bt.d_blocks = (const la_lzop_block *)r->d_tabs.p; bt.n = n;
	bt.d_dst = r->d_dst.p; bt.dst_cap = dst_bytes;
	bt.d_results = (la_lzop_result *)(r->d_tabs.p + o_res);
	if (la_gpu_memcpy_h2d(gpu, r->d_tabs.p, st->tab, sizeof(la_lzop_block) * n) != LA_OK) return la_window_fail(self, &r->w, "la_gpu_memcpy_h2d");
	if (la_gpu_lzop_decode(gpu, &bt) != LA_OK) return la_window_fail(self, &r->w, "la_gpu_lzop_decode");
	if (la_gpu_memcpy_d2h(gpu, st->res, bt.d_results, sizeof(la_lzop_result) * n) != LA_OK || la_gpu_sync(gpu) != LA_OK)
		return la_window_fail(self, &r->w, "la_gpu_memcpy_d2h");
	return ARCHIVE_OK;
}

/* what the reference says about a block the device did not pass (lzop.c:425-477) */
static void lzo_block_failed(struct lzop_private *st, uint32_t status)
{
	int code = 0;
	switch (status) {
	case LA_ST_LZOP_INPUT_OVERRUN:  code = -4; break;	/* LZO_E_INPUT_OVERRUN */
	case LA_ST_LZOP_OUTPUT_OVERRUN: code = -5; break;	/* LZO_E_OUTPUT_OVERRUN */
	case LA_ST_LZOP_LOOKBEHIND:     code = -6; break;	/* LZO_E_LOOKBEHIND_OVERRUN */
	case LA_ST_LZOP_NOT_CONSUMED:   code = -8; break;	/* LZO_E_INPUT_NOT_CONSUMED */
	default: break;	/* the two sums, a short output; a refused entry cannot be: the walk made the same checks */
	}
	st->end_rc = ARCHIVE_FATAL;
	if (code)
		snprintf(st->end_msg, sizeof(st->end_msg), "lzop decompression failed: %d", code);
	else
		snprintf(st->end_msg, sizeof(st->end_msg), "Corrupted data");
}

/* One window: gather, upload, walk and launch; says how the stream ends if this window shows it.
 * ARCHIVE_OK, or a fatal code with the error set. */
static int lzo_window(struct archive_read_filter *self)
{
	struct lzop_private *st = (struct lzop_private *)self->data;
	int r = la_reader_gather(self, &st->r);
	if (r != ARCHIVE_OK)
		return r;
	const uint8_t *src = st->r.stage.p;
	const size_t len = st->r.stage_len;
	const int eof = st->r.w.upstream_eof;
	if (la_buf_dev(st->r.w.gpu, &st->r.d_tabs, (sizeof(la_lzop_block) + sizeof(la_lzop_result)) * LZO_TAB_CAP) < 0)
		return la_window_fail(self, &st->r.w, "la_gpu_malloc");
	size_t pos = 0;		/* the first byte of the header or block info the walk stands at */
	int wk = WK_OK;
	while (wk == WK_OK) {
		/* the blocks from here on that one launch takes; a verdict the walk meets waits behind them */
		uint32_t n = 0;
		uint64_t dst_bytes = 0;
		while (n < LZO_TAB_CAP) {
			if (!st->in_stream) {
				if ((wk = wk_header(st, src, len, eof, &pos)) != WK_OK)
					break;
			}
			la_lzop_block *b = &st->tab[n];
			if (n && dst_bytes + MAX_BLOCK_SIZE > st->r.w.out_budget)
				break;
			if ((wk = wk_block(st, src, len, eof, &pos, b)) != WK_OK)
				break;
			if (b->dst_len == 0)
				continue;	/* the part ended */
			b->dst_off = dst_bytes;
			dst_bytes += b->dst_len;
			n++;
		}
		if (n == 0)
			continue;
		if ((r = lzo_launch(self, st, n, dst_bytes)) != ARCHIVE_OK)
			return r;
		uint32_t good = 0;
		while (good < n && st->res[good].status == LA_ST_OK)
			good++;
		if ((r = la_reader_take(self, &st->r, good < n ? st->tab[good].dst_off : dst_bytes)) != ARCHIVE_OK)
			return r;
		la_holdback_rebase(&st->r.hb);	/* every block of them is out before the next one is read */
		if (good < n) {
			lzo_block_failed(st, st->res[good].status);	/* (replaces a verdict the walk met behind it) */
			wk = WK_END;
		}
	}
	if (wk == WK_END)
		la_holdback_end(&st->r.hb, st->end_rc, st->end_rc != ARCHIVE_OK ? st->end_msg : NULL, LA_HB_ALL);
	return la_reader_finish(self, &st->r, pos, wk == WK_MORE, "block");
}

static ssize_t lzop_filter_read(struct archive_read_filter *self, const void **p)
{
	return la_reader_read(self, &((struct lzop_private *)self->data)->r, p, lzo_window);
}

static int lzop_filter_close(struct archive_read_filter *self)
{
	struct lzop_private *st = (struct lzop_private *)self->data;
	if (st == NULL)
		return ARCHIVE_OK;
	la_reader_close(&st->r);
	free(st);
	self->data = NULL;
	return ARCHIVE_OK;
}
