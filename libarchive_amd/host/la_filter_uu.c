/*
 * la_filter_uu.c -- the uu read filter (uuencode and base64) on the MI355X data plane.
 *
 * Mirrors libarchive/archive_read_support_filter_uu.c: the same bidder (uu.c:211-359: the line-wise look-ahead with its
 * 128 KiB cap, firstline + 30 / + 40, the check of the first data line), filter code and name (ARCHIVE_FILTER_UU, "uu",
 * uu.c:375-376), vtable shape (read / close / read_header, uu.c:361-366), the header line's mode and name
 * (uu.c:572-601, handed to the entry as uu.c:444-457 does) and the strings and errno classes of uudecode_filter_read
 * (uu.c:459-723).  Where the reference decodes line after line into a 64 KiB buffer, this filter gathers a window of
 * the stream and hands ALL of its lines to the device in ONE la_gpu_uu_decode call (csrc/la_uu.hip; the per-line rules
 * are csrc/la_uu_dev.h's).  The call takes whole lines; the untaken tail line opens the next window, and nothing else
 * is kept between windows but the two words of la_uu_state.  No stream shape is one serial unit, so the bidder never
 * consults la_bid_declines.  No CPU fallback.
 *
 * Verdicts.  "Insufficient compressed data" (ARCHIVE_ERRNO_MISC): a bad byte in a data or `end` state, a bad byte while
 * looking for a head with nothing decoded yet, a bad data line, a wrong `end` line.  "Missing format data"
 * (ARCHIVE_ERRNO_FILE_FORMAT): the stream ends inside a line in any state but wait-for-`end`.  "Invalid format data"
 * (ARCHIVE_ERRNO_FILE_FORMAT): the length limits below.  A bad byte while looking for a head behind decoded bytes ends
 * the stream without an error and the rest is ignored (ST_IGNORE); so does a stream that ends at a line boundary, in
 * any state.
 *
 * Where the reference's answer depends on how its input happens to be buffered, this filter decides:
 *   - Bytes in front of an error.  The reference loses what the failing read call had decoded, up to 64 KiB, depending
 *     on upstream's block sizes.  This filter hands out every byte of the lines in front of the failing line, then the
 *     error (la_holdback_rebase behind every window, LA_HB_ALL).
 *   - Line length.  The reference fails a line in FIND_HEAD when total + len >= 128 KiB and a carried partial line over
 *     34 KiB (which arises only where a line straddles its buffers), and ends the stream silently at a data line with
 *     len * 2 > 64 KiB.  Here a line of 128 KiB or more, line end included, while looking for a head, and a data line
 *     of more than 32 768 bytes are "Invalid format data"; nothing else is limited.
 *   - A '\r' that ends one upstream block with '\n' first in the next is the "\r\n" the stream holds, not a line end
 *     and an empty line.
 *   - An `end` split across buffers is accepted, unless the stream itself ends inside it.
 *   - The bidder's look-ahead.  Over the client it is the reference's; over another filter (a .uu inside a .gz) it
 *     looks only at what that filter has already decoded, its first window, and asks for no more (struct uu_look).
 *   - A line is judged when its line end, or the stream's end, is in the window: one that does not end inside a window
 *     of 256 MiB (UU_MAX_WINDOW, or LA_GPU_MAX_BATCH_MIB where that is less) is refused as "uu line too large for the
 *     GPU data plane", not as the "Invalid format data" its length would earn: a bad byte further on in the line would
 *     change that verdict, and it is not known until the line has been read.
 *   - With windows larger than the reference's 64 KiB reads, read_header may report the name of a later section of a
 *     multi-section stream than the reference would.  Single-section streams agree.
 */
#include "la_read_private.h"
#include "la_host.h"
#include "../csrc/la_uu_dev.h"	/* the byte classes and the header line, as the device states them */
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

struct uu_private {
	la_reader r;		/* stage: from the first byte of the untaken tail line on; d_tabs: the result record */
	la_uu_state st;		/* the state in front of the next window */
	/* the most recent header line (uu.c:62-64) */
	unsigned mode;
	int mode_set;
	char *name;
	/* our own verdict, for the errno class la_holdback's report does not carry */
	int end_errno;
	char end_msg[48];
};

static int uudecode_bidder_bid(struct archive_read_filter_bidder *, struct archive_read_filter *);
static int uudecode_bidder_init(struct archive_read_filter *);
static int uudecode_read_header(struct archive_read_filter *, struct archive_entry *);
static ssize_t uudecode_filter_read(struct archive_read_filter *, const void **);
static int uudecode_filter_close(struct archive_read_filter *);

static const struct archive_read_filter_bidder_vtable uudecode_bidder_vtable = {
	.bid = uudecode_bidder_bid,
	.init = uudecode_bidder_init,
};
static const struct archive_read_filter_vtable uudecode_reader_vtable = {
	.read = uudecode_filter_read,
	.close = uudecode_filter_close,
	.read_header = uudecode_read_header,
};

int archive_read_support_filter_uu(struct archive *_a)
{
	struct archive_read *a = (struct archive_read *)_a;
	return __archive_read_register_bidder(a, NULL, "uu", &uudecode_bidder_vtable);
}

/* Deprecated; uu.c:77-84 */
int archive_read_support_compression_uu(struct archive *a)
{
	return archive_read_support_filter_uu(a);
}

/*
 * The bidder.  What it answers is the reference's (uu.c:211-359), stated here over one look-ahead buffer:
 *   - lines are taken from the start of the stream; a bad byte in front of the verdict, or a line that does not end
 *     inside the look-ahead, is 0;
 *   - the first header line (la_uu_header_kind) ends the search; 20 points if it is the stream's first line; behind a
 *     line that is no header, a look-ahead that has reached UU_BID_CAP bytes gives up;
 *   - the line behind the header must be complete and pass a check of its own, and what stands behind THAT decides:
 *     uuencode  a length character in uuchar[] that counts at most 45 and no more than the characters behind it, that
 *               many CHARACTERS in uuchar[] (the reference counts characters off with a byte count); if exactly one
 *               more character follows and it is a checksum (uuchar[]) or MINIX padding (a-z) it is passed over; then
 *               the byte one line end further on must be in uuchar[] -- which is inside the same line whenever more
 *               characters were left, and the next line's first byte otherwise: + 30;
 *     base64    every character in base64[]; then "====" and its line end: + 40, or a character of base64[]: + 30.
 * Over the client the look-ahead grows as lines ask for it.  Over another FILTER it is what that filter has handed out
 * already and no more: asking for more can turn a late error of that stream into a failed open, and the bytes in front
 * of that error, which every such stream delivered before this filter existed, would be lost.
 */
#define UU_MAX_WINDOW ((size_t)256 << 20)
#define UU_BID_CAP  (128u * 1024u)	/* UUENCODE_BID_MAX_READ, uu.c:44 */
#define UU_BID_STEP 4096u

struct uu_look {
	struct archive_read_filter *filter;
	const unsigned char *p;
	size_t have;
	int done;	/* nothing more is to be had: upstream ended, failed, or is a filter */
};

/* at least `want` bytes in the look-ahead if upstream has them; 0 when upstream failed */
static int uu_look_grow(struct uu_look *lk, size_t want)
{
	while (!lk->done && lk->have < want) {
		ssize_t avail;
		const unsigned char *p = __archive_read_filter_ahead(lk->filter, lk->have + UU_BID_STEP > want ? lk->have + UU_BID_STEP : want, &avail);
		if (p == NULL) {
			if (avail < 0)
				return 0;
			lk->done = 1;	/* the stream is shorter: take what there is */
			if (avail > 0 && (p = __archive_read_filter_ahead(lk->filter, (size_t)avail, &avail)) == NULL)
				return 0;
			if (avail <= 0)
				break;
		}
		lk->p = p;
		lk->have = (size_t)avail;
	}
	return 1;
}

/* The line at `at`: 1 and its length and line end, 0 when it holds a bad byte, does not end inside the cap, or upstream
 * failed.  A '\r' is judged with the byte behind it when there is one. */
static int uu_look_line(struct uu_look *lk, size_t at, size_t *len, size_t *nl)
{
	size_t i = at;
	for (;;) {
		for (; i < lk->have; i++) {
			const unsigned c = lk->p[i];
			if (c == '\n' || c == '\r')
				break;
			if (la_uu_is_bad(c))
				return 0;
		}
		if (i < lk->have && (lk->p[i] == '\n' || i + 1 < lk->have || lk->done))
			break;
		if (lk->done || lk->have >= UU_BID_CAP)
			return 0;
		if (!uu_look_grow(lk, lk->have + 1))
			return 0;
	}
	*nl = lk->p[i] == '\r' && i + 1 < lk->have && lk->p[i + 1] == '\n' ? 2 : 1;
	*len = i - at + *nl;
	return 1;
}

static int uudecode_bidder_bid(struct archive_read_filter_bidder *self, struct archive_read_filter *filter)
{
	struct uu_look lk = { filter, NULL, 0, filter->upstream != NULL };
	ssize_t avail;
	size_t at = 0, len, nl;
	uint32_t kind;
	int bid = 20;

	(void)self;
	lk.p = __archive_read_filter_ahead(filter, 1, &avail);
	if (lk.p == NULL)
		return 0;
	lk.have = (size_t)avail;
	for (;;) {
		if (!uu_look_line(&lk, at, &len, &nl))
			return 0;
		kind = la_uu_header_kind(lk.p + at, (uint32_t)(len - nl));
		at += len;
		if (kind)
			break;
		bid = 0;
		if (lk.have >= UU_BID_CAP)
			return 0;
	}
	/* the line behind the header, and up to six bytes behind it ("====\r\n") */
	if (at == lk.have && (!uu_look_grow(&lk, at + 1) || at == lk.have))
		return 0;
	if (!uu_look_line(&lk, at, &len, &nl) || !uu_look_grow(&lk, at + len + 6))
		return 0;
	const unsigned char *b = lk.p + at;
	const size_t body = len - nl, behind = lk.have - (at + len);
	if (kind == 6) {
		if (body == 0 || !la_uu_is_uuchar(b[0]))
			return 0;
		const size_t l = la_uu_dec(b[0]);
		if (l > 45 || l > body - 1)
			return 0;
		for (size_t i = 1; i <= l; i++)
			if (!la_uu_is_uuchar(b[i]))
				return 0;
		size_t look = 1 + l;
		if (body - look == 1 && (la_uu_is_uuchar(b[look]) || (b[look] >= 'a' && b[look] <= 'z')))
			look++;
		look += nl;	/* (at most len: inside the look-ahead when anything stands behind the line) */
		return behind && la_uu_is_uuchar(b[look]) ? bid + 30 : 0;
	}
	for (size_t i = 0; i < body; i++)
		if (!la_uu_is_b64(b[i]))
			return 0;
	b += len;
	if ((behind >= 5 && memcmp(b, "====\n", 5) == 0) || (behind >= 6 && memcmp(b, "====\r\n", 6) == 0))
		return bid + 40;
	return behind && la_uu_is_b64(b[0]) ? bid + 30 : 0;
}

static int uudecode_bidder_init(struct archive_read_filter *self)
{
	self->code = ARCHIVE_FILTER_UU;
	self->name = "uu";
	struct uu_private *st = calloc(1, sizeof(*st));
	if (la_reader_open(self, st ? &st->r : NULL, "uu", sizeof(la_uu_result), 0, "Can't allocate data for uudecode") != ARCHIVE_OK) {	/* uu.c:382-383 */
		free(st);
		return ARCHIVE_FATAL;
	}
	/* the device's line table takes 12 bytes per byte of the window (la_gpu_uu_workspace_bytes): a window grows no
	 * further than UU_MAX_WINDOW, 3 GiB of workspace, whatever LA_GPU_MAX_BATCH_MIB allows */
	if (st->r.w.max_batch_bytes > UU_MAX_WINDOW)
		st->r.w.max_batch_bytes = UU_MAX_WINDOW;
	if (st->r.w.target_bytes > UU_MAX_WINDOW)
		st->r.w.target_bytes = UU_MAX_WINDOW;
	if (st->r.w.batch_bytes > UU_MAX_WINDOW)
		st->r.w.batch_bytes = UU_MAX_WINDOW;
	st->st.state = LA_UU_FIND_HEAD;
	self->data = st;
	self->vtable = &uudecode_reader_vtable;
	return ARCHIVE_OK;
}

/* uu.c:444-457 */
static int uudecode_read_header(struct archive_read_filter *self, struct archive_entry *entry)
{
	struct uu_private *st = (struct uu_private *)self->data;
	if (st->mode_set != 0)
		archive_entry_set_mode(entry, AE_IFREG | st->mode);
	if (st->name != NULL)
		archive_entry_set_pathname(entry, st->name);
	return ARCHIVE_OK;
}

/* uu.c:572-601 over the header line b[0, len) the device accepted: mode, and the name when it is longer than one character */
static int uu_take_header(struct archive_read_filter *self, struct uu_private *st, const uint8_t *b, size_t len)
{
	const size_t nl = len >= 2 && b[len - 2] == '\r' ? 2 : 1;
	const size_t l = b[5] == ' ' ? 6 : 13;
	if (len < nl + l + 4)
		return ARCHIVE_OK;	/* (not a line the rules accept) */
	st->mode = (unsigned)(b[l] - '0') * 64 + (unsigned)(b[l + 1] - '0') * 8 + (unsigned)(b[l + 2] - '0');
	st->mode_set = 1;
	const size_t namelen = len - nl - 4 - l;
	if (namelen > 1) {
		char *name = malloc(namelen + 1);
		if (name == NULL) {
			archive_set_error(&self->archive->archive, ENOMEM, "Can't allocate data for uudecode");
			return ARCHIVE_FATAL;
		}
		memcpy(name, b + l + 4, namelen);
		name[namelen] = '\0';
		free(st->name);
		st->name = name;
	}
	return ARCHIVE_OK;
}

static void uu_end(struct uu_private *st, int errno_class, const char *msg)
{
	st->end_errno = errno_class;
	snprintf(st->end_msg, sizeof(st->end_msg), "%s", msg);
	la_holdback_end(&st->r.hb, ARCHIVE_FATAL, msg, LA_HB_ALL);
}

/* One window: gather, upload, one call, the bytes, the verdict if this window shows one.
 * ARCHIVE_OK, or a fatal code with the error set. */
static int uu_window(struct archive_read_filter *self)
{
	struct uu_private *st = (struct uu_private *)self->data;
	la_reader *r = &st->r;
	la_gpu_ctx *gpu = r->w.gpu;
	int rc = la_reader_gather(self, r);
	if (rc != ARCHIVE_OK)
		return rc;
	const size_t len = r->stage_len;
	const int eof = r->w.upstream_eof;
	la_uu_result *res = (la_uu_result *)r->h_tabs.p;
	memset(res, 0, sizeof(*res));
	res->state = st->st.state;
	res->decoded = st->st.decoded;
	if (len) {
		if (la_buf_dev(gpu, &r->d_dst, len + 64) < 0 || la_buf_dev(gpu, &r->d_tabs, sizeof(la_uu_result)) < 0)
			return la_window_fail(self, &r->w, "la_gpu_malloc");
		la_uu_batch bt;
		memset(&bt, 0, sizeof(bt));
		bt.d_src = r->d_src.p; bt.src_bytes = len;
		bt.final = eof ? 1u : 0u;
		bt.in = st->st;
		bt.d_dst = r->d_dst.p; bt.dst_cap = r->d_dst.cap;
		bt.d_result = (la_uu_result *)r->d_tabs.p;
		if (la_gpu_uu_decode(gpu, &bt) != LA_OK) return la_window_fail(self, &r->w, "la_gpu_uu_decode");
		if (la_gpu_memcpy_d2h(gpu, res, bt.d_result, sizeof(*res)) != LA_OK || la_gpu_sync(gpu) != LA_OK)
			return la_window_fail(self, &r->w, "la_gpu_memcpy_d2h");
		if (res->n_headers && res->head_off + res->head_len <= len &&
		    (rc = uu_take_header(self, st, r->stage.p + res->head_off, res->head_len)) != ARCHIVE_OK)
			return rc;
		if ((rc = la_reader_take(self, r, res->out_len)) != ARCHIVE_OK)
			return rc;
		la_holdback_rebase(&r->hb);	/* every line in front of a failing one is out before the error */
	}
	st->st.state = res->state;
	st->st.decoded = res->decoded;
	switch (res->status) {
	case LA_ST_OK:
		if (eof)	/* the stream ended at a line boundary, in whatever state */
			la_holdback_end(&r->hb, ARCHIVE_OK, NULL, LA_HB_ALL);
		break;
	case LA_ST_UU_IGNORED:	/* ST_IGNORE: the rest is consumed and dropped, uu.c:484-487 */
		la_holdback_end(&r->hb, ARCHIVE_OK, NULL, LA_HB_ALL);
		break;
	case LA_ST_UU_TOO_LONG:
		uu_end(st, ARCHIVE_ERRNO_FILE_FORMAT, "Invalid format data");
		break;
	case LA_ST_UU_UNTERMINATED:
		uu_end(st, ARCHIVE_ERRNO_FILE_FORMAT, "Missing format data");
		break;
	default:
		uu_end(st, ARCHIVE_ERRNO_MISC, "Insufficient compressed data");
		break;
	}
	return la_reader_finish(self, r, (size_t)res->consumed, !eof, "line");
}

static ssize_t uudecode_filter_read(struct archive_read_filter *self, const void **p)
{
	struct uu_private *st = (struct uu_private *)self->data;
	const int was_finished = st->r.hb.finished;
	const ssize_t n = la_reader_read(self, &st->r, p, uu_window);
	/* the verdict la_holdback reported is ours: give it the reference's errno class */
	if (n == ARCHIVE_FATAL && !was_finished && st->r.hb.ended && st->end_msg[0])
		archive_set_error(&self->archive->archive, st->end_errno, "%s", st->end_msg);
	return n;
}

static int uudecode_filter_close(struct archive_read_filter *self)
{
	struct uu_private *st = (struct uu_private *)self->data;
	if (st == NULL)
		return ARCHIVE_OK;
	la_reader_close(&st->r);
	free(st->name);
	free(st);
	self->data = NULL;
	return ARCHIVE_OK;
}
