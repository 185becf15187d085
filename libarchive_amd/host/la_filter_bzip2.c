/*
 * la_filter_bzip2.c -- the bzip2 read filter on the MI355X data plane.
 *
 * Mirrors libarchive/archive_read_support_filter_bzip2.c: the same bidder (bzip2.c:112-148: 14 bytes ahead, 24 bits
 * for "BZh", 5 for the level digit, 48 for a block or end-of-stream magic), filter code and name
 * (ARCHIVE_FILTER_BZIP2, "bzip2", bzip2.c:183-209), vtable shape (read / close, bzip2.c:174-178, :337-362) and error
 * strings ("truncated bzip2 input", bzip2.c:282-286; "bzip decompression failed", bzip2.c:326-329).  Where the
 * reference feeds BZ2_bzDecompress whatever __archive_read_filter_ahead returns (bzip2.c:214-332), this filter gathers
 * a window of the stream, has the device find every block and end-of-stream magic in it (la_gpu_bzip2_scan), decode all
 * block candidates at once and confirm them in stream order (la_gpu_bzip2_decode, LA_BZ2_MEASURE), expand the confirmed
 * blocks that fit the decoded-bytes budget (LA_BZ2_EMIT) and copies them back in one piece.  What the window did not
 * finish -- the first unconfirmed, truncated or over-budget unit and everything behind it -- opens the next window at
 * that unit's byte; the stream state (inside a stream or between two, level, combined CRC, bit offset 0 .. 7) goes
 * with it.  A bzip2 stream is never one large serial unit, so there is no LA_GPU_BID policy here.  No CPU fallback.
 *
 * Bytes in front of an error.  The reference hands out its 64 KiB block only when BZ2_bzDecompress has filled it
 * (avail_out == 0, bzip2.c:317-324) and, at the end, the partial block (bzip2.c:236-241, :291-296); on an error it
 * returns ARCHIVE_FATAL and the partial block is lost.  libbz2 decodes a block completely before it emits its first
 * byte, emits all of a block's bytes before it compares the block's CRC, and, having emitted a block's last byte, goes
 * on to read the next header in the same call even when the output block is full.  With T the bytes libbz2 has emitted
 * when it reports the error (through the block in front of a damaged header, table or symbol; through the block
 * itself for a wrong block CRC; everything for a wrong combined CRC):
 *   - a data error arrives in the call that emitted byte T or later, so the block that holds byte T is not handed out
 *     (LA_HB_EARLY);
 *   - truncated input is found by the NEXT look at upstream (bzip2.c:280-287), after a full block has been returned
 *     (LA_HB_LATE);
 *   - a clean end (end of input between streams, or bytes behind a stream that fail the bid) hands out all T (LA_HB_ALL).
 * What each kind lets out, and the holding back until the next window says which it is, is la_holdback's (la_host.h,
 * la_bid_policy.c).  (tests/bzip2_support.py restates the reference's loop over the real libbz2; the rule above is
 * what that emulator gives.  For T a multiple of 64 KiB the first case assumes that upstream hands the reference the
 * damaged unit together with byte T's block, as a memory reader does.)
 */
#include "la_read_private.h"
#include "la_host.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define BZ_CAND_CAP    ((uint32_t)1 << 16)	/* candidates one scan keeps; a window with more is taken in parts */

struct bzip2_private {
	la_reader r;			/* stage: from the byte of the next unit on; d_tabs: candidates, results, state, count */
	uint32_t options;		/* LA_BZIP2_SERIAL_CHASE=1: LA_BZ2_OPT_SERIAL_CHASE */
	la_bz2_state st;		/* where the stream stands at stage[0] */
	la_bz2_result *res;		/* the window's results on the host (4096 entries), r.h_tabs */
};

static int bzip2_reader_bid(struct archive_read_filter_bidder *, struct archive_read_filter *);
static int bzip2_reader_init(struct archive_read_filter *);
static ssize_t bzip2_filter_read(struct archive_read_filter *, const void **);
static int bzip2_filter_close(struct archive_read_filter *);

static const struct archive_read_filter_bidder_vtable bzip2_bidder_vtable = {
	.bid = bzip2_reader_bid,
	.init = bzip2_reader_init,
};
static const struct archive_read_filter_vtable bzip2_reader_vtable = {
	.read = bzip2_filter_read,
	.close = bzip2_filter_close,
};

int archive_read_support_filter_bzip2(struct archive *_a)
{
	struct archive_read *a = (struct archive_read *)_a;
	if (__archive_read_register_bidder(a, NULL, "bzip2", &bzip2_bidder_vtable) != ARCHIVE_OK)
		return ARCHIVE_FATAL;
	return ARCHIVE_OK;
}

/* bzip2.c:112-148 */
static int bzip2_reader_bid(struct archive_read_filter_bidder *self, struct archive_read_filter *filter)
{
	ssize_t avail;
	(void)self;
	const unsigned char *p = __archive_read_filter_ahead(filter, 14, &avail);
	if (p == NULL)
		return 0;
	if (memcmp(p, "BZh", 3) != 0)
		return 0;
	if (p[3] < '1' || p[3] > '9')
		return 0;
	if (memcmp(p + 4, "\x31\x41\x59\x26\x53\x59", 6) != 0 && memcmp(p + 4, "\x17\x72\x45\x38\x50\x90", 6) != 0)
		return 0;
	return 24 + 5 + 48;
}

static int bzip2_reader_init(struct archive_read_filter *self)
{
	self->code = ARCHIVE_FILTER_BZIP2;
	self->name = "bzip2";
	struct bzip2_private *st = calloc(1, sizeof(*st));
	if (la_reader_open(self, st ? &st->r : NULL, "bzip2", sizeof(la_bz2_result) * 4096, 0,
	    "Can't allocate data for bzip2 decompression") != ARCHIVE_OK) {
		free(st);
		return ARCHIVE_FATAL;
	}
	st->res = (la_bz2_result *)st->r.h_tabs.p;
	const char *sc = getenv("LA_BZIP2_SERIAL_CHASE");
	st->options = (sc && atoi(sc) > 0) ? LA_BZ2_OPT_SERIAL_CHASE : 0u;
	self->data = st;
	self->vtable = &bzip2_reader_vtable;
	return ARCHIVE_OK;
}

/* the stream ends here, T being hb.total */
static void bz_end_data(struct bzip2_private *st)
{
	la_holdback_end(&st->r.hb, ARCHIVE_FATAL, "bzip decompression failed", LA_HB_EARLY);
}
static void bz_end_truncated(struct bzip2_private *st)
{
	la_holdback_end(&st->r.hb, ARCHIVE_FATAL, "truncated bzip2 input", LA_HB_LATE);
}
static void bz_end_clean(struct bzip2_private *st)
{
	la_holdback_end(&st->r.hb, ARCHIVE_OK, NULL, LA_HB_ALL);
}

/* the byte that starts at bit `bit` of p[0, n): caller keeps bit + 8 <= 8 n */
static unsigned bz_byte_at(const uint8_t *p, size_t n, uint64_t bit)
{
	const size_t b = (size_t)(bit >> 3);
	const unsigned sh = (unsigned)(bit & 7);
	const unsigned hi = p[b], lo = b + 1 < n ? p[b + 1] : 0;
	return ((hi << 8 | lo) >> (8 - sh)) & 0xFFu;
}

/* What stands at bit `bit` where a block or end-of-stream magic has to: 1 a whole magic, 0 the front of one that the
 * window cuts off, -1 something else.  libbz2 compares the six bytes one at a time and fails at the first that
 * differs (decompress.c, BZ_X_BLKHDR_1 .. 6 and BZ_X_ENDHDR_2 .. 6), so a cut-off front that differs is a data error. */
static int bz_magic_at(const uint8_t *p, size_t n, uint64_t bit)
{
	static const uint8_t blk[6] = { 0x31, 0x41, 0x59, 0x26, 0x53, 0x59 }, end[6] = { 0x17, 0x72, 0x45, 0x38, 0x50, 0x90 };
	const uint64_t left = (uint64_t)n * 8 > bit ? (uint64_t)n * 8 - bit : 0;
	const unsigned k = left >= 48 ? 6 : (unsigned)(left / 8);
	int mb = 1, me = 1;
	for (unsigned i = 0; i < k; i++) {
		const unsigned c = bz_byte_at(p, n, bit + 8 * i);
		if (c != blk[i]) mb = 0;
		if (c != end[i]) me = 0;
	}
	if (!mb && !me)
		return -1;
	return k == 6;
}

/* One window: gather, upload, scan, measure, emit, copy back; updates the stream state and T, and says how the stream
 * ends if this window shows it.  ARCHIVE_OK, or a fatal code with the error set. */
static int bz_window(struct archive_read_filter *self)
{
	struct bzip2_private *st = (struct bzip2_private *)self->data;
	la_reader *rd = &st->r;
	la_gpu_ctx *gpu = rd->w.gpu;
	int r = la_reader_gather(self, rd);
	if (r != ARCHIVE_OK)
		return r;
	if (rd->stage_len == 0) {	/* (upstream has ended) */
		if (st->st.open)
			bz_end_truncated(st);
		else
			bz_end_clean(st);
		return ARCHIVE_OK;
	}
	const uint8_t *src = rd->stage.p;
	const size_t len = rd->stage_len;
	/* every block of the window gets a slot for the largest block its stream may hold */
	uint32_t slot_level = st->st.open ? st->st.level : 9;
	if (!st->st.open && len >= 4 && src[3] >= '1' && src[3] <= '9')
		slot_level = (uint32_t)(src[3] - '0');
	const uint32_t max_n = la_gpu_bzip2_max_blocks(slot_level);
	const size_t o_res = sizeof(la_bz2_cand) * BZ_CAND_CAP, o_state = o_res + sizeof(la_bz2_result) * 4096, o_count = o_state + 64;
	if (la_buf_dev(gpu, &rd->d_tabs, o_count + 64) < 0)
		return la_window_fail(self, &rd->w, "la_gpu_malloc");
	la_bz2_cand *d_cands = (la_bz2_cand *)rd->d_tabs.p;
	la_bz2_result *d_results = (la_bz2_result *)(rd->d_tabs.p + o_res);
	la_bz2_state *d_state = (la_bz2_state *)(rd->d_tabs.p + o_state);
	uint32_t *d_count = (uint32_t *)(rd->d_tabs.p + o_count);
	uint32_t count = 0;
	if (la_gpu_bzip2_scan(gpu, rd->d_src.p, len, d_cands, BZ_CAND_CAP, d_count) != LA_OK) return la_window_fail(self, &rd->w, "la_gpu_bzip2_scan");
	if (la_gpu_memcpy_d2h(gpu, &count, d_count, 4) != LA_OK || la_gpu_sync(gpu) != LA_OK) return la_window_fail(self, &rd->w, "la_gpu_memcpy_d2h");
	uint32_t n = count < BZ_CAND_CAP ? count : BZ_CAND_CAP;
	if (n > max_n)
		n = max_n;	/* the table never holds more blocks than the workspace slots: the rest waits for the next window */
	la_bz2_batch bt;
	la_bz2_state ms, es;
	memset(&bt, 0, sizeof(bt));
	bt.d_src = rd->d_src.p; bt.src_bytes = len;
	bt.d_cands = d_cands; bt.n = n;
	bt.d_results = d_results;
	bt.state_in = &st->st; bt.d_state_out = d_state;
	bt.options = st->options; bt.slot_level = slot_level;
	bt.phase = LA_BZ2_MEASURE;
	if (la_gpu_bzip2_decode(gpu, &bt) != LA_OK) return la_window_fail(self, &rd->w, "la_gpu_bzip2_decode");
	if (la_gpu_memcpy_d2h(gpu, st->res, d_results, sizeof(la_bz2_result) * n) != LA_OK ||
	    la_gpu_memcpy_d2h(gpu, &ms, d_state, sizeof(ms)) != LA_OK || la_gpu_sync(gpu) != LA_OK)
		return la_window_fail(self, &rd->w, "la_gpu_memcpy_d2h");
	/* the prefix of confirmed blocks that fits the decoded-bytes budget; one block always goes (at most 46 MB) */
	uint32_t n_emit = ms.n_taken;
	uint64_t dst_bytes = 0;
	for (uint32_t i = 0; i < ms.n_taken; i++) {
		const la_bz2_result *q = &st->res[i];
		if (q->status != LA_ST_OK || q->out_len == 0)
			continue;
		if (dst_bytes && rd->w.out_budget && dst_bytes + q->out_len > rd->w.out_budget) {
			n_emit = i;
			break;
		}
		dst_bytes += q->out_len;
	}
	if (la_buf_dev(gpu, &rd->d_dst, (size_t)dst_bytes + 64) < 0) return la_window_fail(self, &rd->w, "la_gpu_malloc");
	if (la_buf_pinned(gpu, &rd->hb.out, (size_t)dst_bytes + 64, 0) < 0) return la_window_fail(self, &rd->w, "la_gpu_malloc_host");
	bt.phase = LA_BZ2_EMIT;
	bt.d_dst = rd->d_dst.p; bt.dst_cap = dst_bytes; bt.n_emit = n_emit;
	if (la_gpu_bzip2_decode(gpu, &bt) != LA_OK) return la_window_fail(self, &rd->w, "la_gpu_bzip2_decode");
	if (la_gpu_memcpy_d2h(gpu, &es, d_state, sizeof(es)) != LA_OK ||
	    la_gpu_memcpy_d2h(gpu, st->res, d_results, sizeof(la_bz2_result) * n) != LA_OK ||
	    la_gpu_memcpy_d2h(gpu, rd->hb.out.p, rd->d_dst.p, dst_bytes) != LA_OK || la_gpu_sync(gpu) != LA_OK)
		return la_window_fail(self, &rd->w, "la_gpu_memcpy_d2h");
	rd->hb.out_len = (size_t)es.total_out;	/* (through a block with a wrong CRC: libbz2 emits it before it compares) */
	rd->hb.total += es.total_out;
	const uint64_t stop_bit = es.start_bit;
	const size_t used = (size_t)(stop_bit >> 3) < len ? (size_t)(stop_bit >> 3) : len;
	int more = 0;	/* the unit at stop_bit needs bytes the window does not hold */
	if (es.first_bad != 0xFFFFFFFFu) {
		bz_end_data(st);
	} else if (es.n_taken < ms.n_taken || es.stop == LA_BZ2_STOP_LEVEL) {
		;	/* the budget, or a stream of a higher level, ends the window: on from there */
	} else if (es.stop == LA_BZ2_STOP_ENTRY) {
		if (st->res[es.stop_entry].status != LA_ST_BZ2_TRUNCATED)
			bz_end_data(st);	/* LA_ST_BZ2_DATA, LA_ST_BZ2_RANDOMISED */
		else if (rd->w.upstream_eof)
			bz_end_truncated(st);
		else
			more = 1;
	} else if (es.stop == LA_BZ2_STOP_TABLE) {
		const int m = bz_magic_at(src, len, stop_bit);
		if (m < 0)
			bz_end_data(st);
		else if (m == 0) {
			if (rd->w.upstream_eof)
				bz_end_truncated(st);
			else
				more = 1;
		}
		/* m == 1: a candidate the table had no room for */
	} else if (es.stop == LA_BZ2_STOP_BID) {
		bz_end_clean(st);	/* bzip2.c:236-241: what follows the stream fails the bid */
	} else {	/* LA_BZ2_STOP_SHORT: fewer than 14 bytes behind a stream */
		if (rd->w.upstream_eof)
			bz_end_clean(st);
		else
			more = 1;
	}
	if (!rd->hb.ended && !more && used == 0 && es.total_out == 0) {
		/* (cannot be: a window that neither ends the stream nor asks for more input has passed at least one unit) */
		archive_set_error(&self->archive->archive, ARCHIVE_ERRNO_MISC, "bzip2 GPU data plane: a window made no progress");
		return ARCHIVE_FATAL;
	}
	if ((r = la_reader_finish(self, rd, used, more, "block")) != ARCHIVE_OK || rd->hb.ended)
		return r;
	st->st.open = es.open; st->st.level = es.level; st->st.crc = es.crc;
	st->st.start_bit = stop_bit - (uint64_t)used * 8;
	return ARCHIVE_OK;
}

static ssize_t bzip2_filter_read(struct archive_read_filter *self, const void **p)
{
	return la_reader_read(self, &((struct bzip2_private *)self->data)->r, p, bz_window);
}

static int bzip2_filter_close(struct archive_read_filter *self)
{
	struct bzip2_private *st = (struct bzip2_private *)self->data;
	if (st == NULL)
		return ARCHIVE_OK;
	la_reader_close(&st->r);
	free(st);
	self->data = NULL;
	return ARCHIVE_OK;
}
