/*
 * la_filter_lzip.c -- the lzip read filter on the MI355X data plane.
 *
 * Mirrors the lzip half of libarchive/archive_read_support_filter_xz.c: the same bidder (xz.c:343-383: "LZIP", a version
 * of 0 or 1, a dictionary exponent of 12 .. 29: 32 + 8 + 8 bits), filter code and name (ARCHIVE_FILTER_LZIP, "lzip",
 * xz.c:409-410), vtable shape (read / close, xz.c:462-466), set_error's strings for the stream (xz.c:443-451,
 * ARCHIVE_FATAL) and lzip_tail's strings, order and ARCHIVE_FAILED for the trailer (xz.c:589-646).  Where the reference
 * feeds lzma_code (a raw LZMA1 decoder per member, xz.c:533-586) whatever __archive_read_filter_ahead returns, this
 * filter gathers a window of the stream that starts at a member header and
 *   - has the device find every offset with the shape of a member header (la_gpu_lzip_scan);
 *   - chains members: from a member start S, the first candidate o with le64(o - 8) == o - S -- the member size of a
 *     version 1 trailer -- is the member's end; the end of the input counts as a candidate once upstream has ended.  The
 *     trailer in front of o gives the member's compressed extent, its data size and its CRC32 before a bit is decoded;
 *   - sends all chained members to the device in ONE la_gpu_lzip_decode call, output offsets from a prefix sum of the
 *     data sizes.
 * Such an end and size are TENTATIVE (eight bytes of compressed data can look like a member size).  The device says
 * whether the stream really ends there with that many bytes and that CRC; a member it refutes is no error: it is decoded
 * again ALONE with both ends unknown, bounded by the window and by a budget that grows on "output full", its end learnt
 * from `consumed`, and lzip_tail's checks run on the host against the trailer that is really there.  A member whose end
 * no candidate gives goes the same way: a version 0 member (12-byte trailer, no member size), a last member followed by
 * junk, a broken chain.  Behind a trailer the next six bytes either have the header shape, which starts a member, or
 * the data ends cleanly there: junk is ignored (xz.c:636-645).  What the window did not finish opens the next one at
 * that member's first byte.  A member larger than LA_GPU_MAX_BATCH_MIB compressed, or min(LA_GPU_OUT_BUDGET_MIB, 4095)
 * MiB decoded, is refused by name.  No CPU fallback.
 *
 * Bytes in front of an error.  The reference hands out its 64 KiB block when lzma_code has filled it and, at every
 * member's end, the partial block (LZMA_STREAM_END sets eof, which ends the fill loop, xz.c:669-734); lzip_tail runs in
 * that same call, and the next member starts a fresh block.  So the 64 KiB grid restarts at every member boundary, and
 * everything up to a member end whose trailer held is out (la_holdback_rebase).  Inside a member, with M its bytes that
 * liblzma has emitted when the reference returns the error -- liblzma's LZMA1 decoder with an unknown uncompressed size
 * goes on to decode the next symbol when the output block is full (only its write waits), so the marker, or a damaged
 * symbol, behind a full block is met in the call that filled it:
 *   - a data error inside the stream, and every trailer verdict ("Lzip: ..."), arrive in the call that emitted byte M,
 *     so that byte's block is not handed out (LA_HB_EARLY);
 *   - input that ends inside a stream is LZMA_BUF_ERROR from a lzma_code call without input ("No progress is possible",
 *     not "truncated input"); behind a full block that call is made by the next read (LA_HB_LATE);
 *   - a clean end (no header shape behind a trailer, or fewer than six bytes) hands out everything (LA_HB_ALL).
 * (tests/lzip_support.py restates the reference's loop over the real liblzma; the rule above is what that emulator
 * gives when upstream hands the reference the whole input at once, as a memory reader does.  With small reads the
 * symbol behind a full block may arrive with the next read, and an early error becomes a late one.)
 */
#include "la_read_private.h"
#include "la_host.h"
#include "../csrc/la_lzip_dev.h"	/* la_lzip_header_shape, la_lzip_dict_size: the rules header is plain C too */
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define LZ_TAB_CAP   4096u			/* members one launch takes; a window with more is taken in parts */
#define LZ_CAND_CAP  ((uint32_t)1 << 16)	/* candidates one scan keeps; a window with more is scanned in parts */

static const char LZ_MSG_DATA[] = "Lzma library error: Corrupted input data";
static const char LZ_MSG_BUF[] = "Lzma library error:  No progress is possible";

struct lzip_private {
	la_reader r;			/* stage: from the first byte of the next member on; d_tabs: candidates, count, member table, results */
	uint64_t *cands; size_t n_cands, cands_cap;	/* the window's header shapes, ascending */
	la_lzip_member *tab;		/* host copies of the tables (LZ_TAB_CAP entries each), in r.h_tabs */
	la_lzip_result *res;
	size_t *ends;			/* tab[i]'s member ends inside the window */
	int force_solo;			/* the member at stage[0 ...] was refuted as chained: decode it alone */
	uint64_t solo_cap;		/* output budget of the next member decoded alone (grows on LA_ST_LZIP_OUT_FULL) */
};

static int lzip_reader_bid(struct archive_read_filter_bidder *, struct archive_read_filter *);
static int lzip_reader_init(struct archive_read_filter *);
static ssize_t lzip_filter_read(struct archive_read_filter *, const void **);
static int lzip_filter_close(struct archive_read_filter *);

static const struct archive_read_filter_bidder_vtable lzip_bidder_vtable = {
	.bid = lzip_reader_bid,
	.init = lzip_reader_init,
};
static const struct archive_read_filter_vtable lzip_reader_vtable = {
	.read = lzip_filter_read,
	.close = lzip_filter_close,
};

int archive_read_support_filter_lzip(struct archive *_a)
{
	struct archive_read *a = (struct archive_read *)_a;
	if (__archive_read_register_bidder(a, NULL, "lzip", &lzip_bidder_vtable) != ARCHIVE_OK)
		return ARCHIVE_FATAL;
	return ARCHIVE_OK;
}

/* xz.c:343-383 */
static int lzip_reader_bid(struct archive_read_filter_bidder *self, struct archive_read_filter *filter)
{
	ssize_t avail;
	(void)self;
	const unsigned char *p = __archive_read_filter_ahead(filter, 6, &avail);
	if (p == NULL)
		return 0;
	if (!la_lzip_header_shape(p))
		return 0;
	/* Default policy (la_bid_policy.c): one member is one serial chain; a stream whose first member does not end inside
	 * the look-ahead is left to liblzma on a host core. */
	if (la_bid_declines(filter, la_bid_lzip_parallel))
		return 0;
	return 32 + 8 + 8;
}

static int lzip_reader_init(struct archive_read_filter *self)
{
	self->code = ARCHIVE_FILTER_LZIP;
	self->name = "lzip";
	struct lzip_private *st = calloc(1, sizeof(*st));
	/* (a member's dst_cap is at most LA_XZ_DST_CAP_MAX: 4095 MiB) */
	if (la_reader_open(self, st ? &st->r : NULL, "lzip", (sizeof(la_lzip_member) + sizeof(la_lzip_result) + sizeof(size_t)) * LZ_TAB_CAP,
	    (uint64_t)4095 << 20, "Can't allocate data for xz decompression") != ARCHIVE_OK) {	/* xz.c:482-483 */
		free(st);
		return ARCHIVE_FATAL;
	}
	st->tab = (la_lzip_member *)st->r.h_tabs.p;
	st->res = (la_lzip_result *)(st->tab + LZ_TAB_CAP);
	st->ends = (size_t *)(st->res + LZ_TAB_CAP);
	self->data = st;
	self->vtable = &lzip_reader_vtable;
	return ARCHIVE_OK;
}

static uint64_t le64(const uint8_t *p)
{
	uint64_t v = 0;
	for (unsigned k = 0; k < 8; k++)
		v |= (uint64_t)p[k] << (8 * k);
	return v;
}

/* The header shapes of the window, in parts of LZ_CAND_CAP: st->cands[0, n_cands). */
static int lz_scan(struct archive_read_filter *self, struct lzip_private *st, size_t len)
{
	la_reader *r = &st->r;
	la_gpu_ctx *gpu = r->w.gpu;
	uint64_t *d_offs = (uint64_t *)r->d_tabs.p;
	uint32_t *d_count = (uint32_t *)(r->d_tabs.p + sizeof(uint64_t) * LZ_CAND_CAP);
	size_t from = 0;
	st->n_cands = 0;
	for (;;) {
		uint32_t count = 0;
		if (la_gpu_lzip_scan(gpu, r->d_src.p + from, len - from, d_offs, LZ_CAND_CAP, d_count) != LA_OK)
			return la_window_fail(self, &r->w, "la_gpu_lzip_scan");
		if (la_gpu_memcpy_d2h(gpu, &count, d_count, 4) != LA_OK || la_gpu_sync(gpu) != LA_OK)
			return la_window_fail(self, &r->w, "la_gpu_memcpy_d2h");
		const uint32_t k = count < LZ_CAND_CAP ? count : LZ_CAND_CAP;
		if (st->n_cands + k > st->cands_cap) {
			const size_t nc = (st->n_cands + k) * 2;
			uint64_t *np = realloc(st->cands, sizeof(uint64_t) * nc);
			if (np == NULL) {
				archive_set_error(&self->archive->archive, ENOMEM, "Can't allocate data for xz decompression");
				return ARCHIVE_FATAL;
			}
			st->cands = np;
			st->cands_cap = nc;
		}
		if (k && (la_gpu_memcpy_d2h(gpu, st->cands + st->n_cands, d_offs, sizeof(uint64_t) * k) != LA_OK || la_gpu_sync(gpu) != LA_OK))
			return la_window_fail(self, &r->w, "la_gpu_memcpy_d2h");
		for (uint32_t i = 0; i < k; i++)
			st->cands[st->n_cands + i] += from;
		st->n_cands += k;
		if (count <= LZ_CAND_CAP)
			return ARCHIVE_OK;
		from = (size_t)st->cands[st->n_cands - 1] + 1;	/* the table was full: on behind its last entry */
	}
}

/* The end of the version 1 member that starts at S: the first candidate o behind it (*ci: where to start looking; the
 * end of the input is one when upstream has ended) with le64(o - 8) == o - S.  0: none. */
static size_t lz_chain_end(const struct lzip_private *st, const uint8_t *src, size_t len, int eof, size_t S, size_t *ci)
{
	while (*ci < st->n_cands && st->cands[*ci] <= S)
		(*ci)++;
	for (size_t k = *ci; k <= st->n_cands; k++) {
		if (k == st->n_cands && !eof)
			break;
		const size_t o = k < st->n_cands ? (size_t)st->cands[k] : len;
		if (o - S >= 6 + 20 && le64(src + o - 8) == o - S)
			return o;
	}
	return 0;
}

/* Decode tab[0, n) in one call; the results are in st->res. */
static int lz_launch(struct archive_read_filter *self, struct lzip_private *st, uint32_t n, uint64_t dst_bytes)
{
	la_reader *r = &st->r;
	la_gpu_ctx *gpu = r->w.gpu;
	const size_t o_tab = sizeof(uint64_t) * LZ_CAND_CAP + 256, o_res = o_tab + sizeof(la_lzip_member) * LZ_TAB_CAP;
	if (la_buf_dev(gpu, &r->d_dst, (size_t)dst_bytes + 64) < 0)
		return la_window_fail(self, &r->w, "la_gpu_malloc");
	la_lzip_batch bt;
	memset(&bt, 0, sizeof(bt));
	bt.d_src = r->d_src.p; bt.src_bytes = r->stage_len;
	bt.d_members = (const la_lzip_member *)(r->d_tabs.p + o_tab); bt.n = n;
	bt.d_dst = r->d_dst.p; bt.dst_cap = dst_bytes;
	bt.d_results = (la_lzip_result *)(r->d_tabs.p + o_res);
	if (la_gpu_memcpy_h2d(gpu, r->d_tabs.p + o_tab, st->tab, sizeof(la_lzip_member) * n) != LA_OK) return la_window_fail(self, &r->w, "la_gpu_memcpy_h2d");
	if (la_gpu_lzip_decode(gpu, &bt) != LA_OK) return la_window_fail(self, &r->w, "la_gpu_lzip_decode");
	if (la_gpu_memcpy_d2h(gpu, st->res, bt.d_results, sizeof(la_lzip_result) * n) != LA_OK || la_gpu_sync(gpu) != LA_OK)
		return la_window_fail(self, &r->w, "la_gpu_memcpy_d2h");
	return ARCHIVE_OK;
}

static void lz_end_failed(struct lzip_private *st, const char *msg)
{
	la_holdback_end(&st->r.hb, ARCHIVE_FAILED, msg, LA_HB_EARLY);
}

/* One window: gather, upload, scan, walk; updates T, and says how the stream ends if this window shows it.
 * ARCHIVE_OK, or a fatal code with the error set. */
static int lz_window(struct archive_read_filter *self)
{
	struct lzip_private *st = (struct lzip_private *)self->data;
	la_holdback *hb = &st->r.hb;
	const uint64_t out_budget = st->r.w.out_budget;
	int r = la_reader_gather(self, &st->r);
	if (r != ARCHIVE_OK)
		return r;
	const uint8_t *src = st->r.stage.p;
	const size_t len = st->r.stage_len;
	const int eof = st->r.w.upstream_eof;
	const size_t tabs_bytes = sizeof(uint64_t) * LZ_CAND_CAP + 256 + (sizeof(la_lzip_member) + sizeof(la_lzip_result)) * LZ_TAB_CAP;
	if (la_buf_dev(st->r.w.gpu, &st->r.d_tabs, tabs_bytes) < 0) return la_window_fail(self, &st->r.w, "la_gpu_malloc");
	st->n_cands = 0;
	if (len && (r = lz_scan(self, st, len)) != ARCHIVE_OK)
		return r;
	size_t pos = 0;		/* the first byte of the member the walk stands at */
	size_t ci = 0;		/* the first candidate that may lie behind pos */
	int more = 0;		/* that member needs bytes the window does not hold */
	while (!hb->ended && !more) {
		if (len - pos < 6) {	/* xz.c:350-352: no six bytes, no member */
			if (eof) la_holdback_end(hb, ARCHIVE_OK, NULL, LA_HB_ALL); else more = 1;
			break;
		}
		if (!la_lzip_header_shape(src + pos)) {	/* junk behind a member is ignored (xz.c:636-645) */
			la_holdback_end(hb, ARCHIVE_OK, NULL, LA_HB_ALL);
			break;
		}
		/* the run of members that chain from here, each with a trailer whose sizes fit a launch */
		uint32_t n = 0;
		uint64_t dst_bytes = 0;
		size_t at = pos;
		while (!st->force_solo && n < LZ_TAB_CAP && len - at >= 6 && la_lzip_header_shape(src + at) && src[at + 4] == 1) {
			const size_t o = lz_chain_end(st, src, len, eof, at, &ci);
			if (o == 0)
				break;
			const uint64_t data_size = le64(src + o - 16);
			if (data_size > out_budget || (n && dst_bytes + data_size > out_budget))
				break;
			la_lzip_member *m = &st->tab[n];
			m->src_off = at + 6; m->src_end = o - 20; m->data_size = data_size;
			m->dst_off = dst_bytes; m->dst_cap = data_size;
			m->dict_size = la_lzip_dict_size(src[at + 5]);
			m->crc32 = archive_le32dec(src + o - 20); m->flags = LA_LZIP_HAS_CRC; m->reserved = 0;
			st->ends[n++] = o;
			dst_bytes += data_size;
			at = o;
		}
		if (n) {
			if ((r = lz_launch(self, st, n, dst_bytes)) != ARCHIVE_OK)
				return r;
			uint32_t good = 0;
			while (good < n && st->res[good].status == LA_ST_OK)
				good++;
			if (good) {
				/* every one of them ends where its trailer says, with that size and CRC: lzip_tail would pass them */
				if ((r = la_reader_take(self, &st->r, st->tab[good - 1].dst_off + st->res[good - 1].out_len)) != ARCHIVE_OK)
					return r;
				la_holdback_rebase(hb);
				pos = st->ends[good - 1];
			}
			st->force_solo = good < n;	/* a tentative end, size or CRC did not hold: that member alone says what is wrong */
			continue;
		}
		/* the member at pos alone, both ends unknown */
		if (!st->force_solo && !eof && pos > 0) {
			more = 1;	/* no end in this window: the next one opens at this member and holds more of it */
			break;
		}
		const unsigned tail = src[pos + 4] == 0 ? 12 : 20;
		const uint64_t cap = la_reader_solo_cap(&st->r, &st->solo_cap, len - pos - 6);
		la_lzip_member *m = &st->tab[0];
		m->src_off = pos + 6; m->src_end = LA_LZIP_UNKNOWN; m->data_size = LA_LZIP_UNKNOWN;
		m->dst_off = 0; m->dst_cap = cap;
		m->dict_size = la_lzip_dict_size(src[pos + 5]);
		m->crc32 = 0; m->flags = 0; m->reserved = 0;
		if ((r = lz_launch(self, st, 1, cap)) != ARCHIVE_OK)
			return r;
		const la_lzip_result q = st->res[0];
		if (q.status == LA_ST_LZIP_OUT_FULL) {
			if ((r = la_reader_solo_full(self, &st->r, &st->solo_cap, cap, "member")) != ARCHIVE_OK)
				return r;
			continue;	/* again, with twice the room */
		}
		const size_t trailer = pos + 6 + (size_t)q.consumed;
		if (!eof && (q.status == LA_ST_LZIP_TRUNCATED || (q.status == LA_ST_OK && len - trailer < tail))) {
			more = 1;	/* the stream, or its trailer, runs off the window */
			break;
		}
		st->solo_cap = 0;
		st->force_solo = 0;
		if ((r = la_reader_take(self, &st->r, q.out_len)) != ARCHIVE_OK)
			return r;
		if (q.status == LA_ST_LZIP_TRUNCATED)
			la_holdback_end(hb, ARCHIVE_FATAL, LZ_MSG_BUF, LA_HB_LATE);
		else if (q.status != LA_ST_OK)
			la_holdback_end(hb, ARCHIVE_FATAL, LZ_MSG_DATA, LA_HB_EARLY);
		/* lzip_tail, xz.c:589-646 */
		else if (len - trailer < tail)
			lz_end_failed(st, "Lzip: Remaining data is less bytes");
		else if (q.crc32 != archive_le32dec(src + trailer))
			lz_end_failed(st, "Lzip: CRC32 error");
		else if (q.out_len != le64(src + trailer + 4))
			lz_end_failed(st, "Lzip: Uncompressed size error");
		else if (tail == 20 && 6 + q.consumed + 20 != le64(src + trailer + 12))
			lz_end_failed(st, "Lzip: Member size error");
		else {
			la_holdback_rebase(hb);
			pos = trailer + tail;
		}
	}
	return la_reader_finish(self, &st->r, pos, more, "member");
}

static ssize_t lzip_filter_read(struct archive_read_filter *self, const void **p)
{
	return la_reader_read(self, &((struct lzip_private *)self->data)->r, p, lz_window);
}

static int lzip_filter_close(struct archive_read_filter *self)
{
	struct lzip_private *st = (struct lzip_private *)self->data;
	if (st == NULL)
		return ARCHIVE_OK;
	la_reader_close(&st->r);
	free(st->cands);
	free(st);
	self->data = NULL;
	return ARCHIVE_OK;
}
