/*
 * la_filter_gzip.c -- the gzip read filter with an MI355X data plane.
 *
 * Drop-in for libarchive/archive_read_support_filter_gzip.c: same public entry
 * points (archive_read_support_filter_gzip and the deprecated
 * archive_read_support_compression_gzip, gzip.c:85-117), same bidder
 * (gzip.c:244-255), same filter name/code, same vtable shape
 * {read, close, read_header} (gzip.c:298-305), same return codes and error
 * strings.  read() gathers a window of the compressed stream, finds the
 * member boundaries on the host (la_gzip_index.c), inflates all members of
 * the window on the GPU (la_gpu_gzip_decode) and returns the decoded slab.
 *
 * Parity details kept on purpose:
 *   - the trailer CRC32/ISIZE is computed on the device but, like the reference
 *     (gzip.c:423), NOT enforced unless LA_GZIP_STRICT=1;
 *   - on an error the reference has delivered whole 64 KiB output blocks only
 *     (gzip.c:314, :446): this filter never hands out the last partial 64 KiB
 *     of what it has decoded until the bytes after it are known to be fine, so
 *     the bytes delivered before an error are exactly the reference's;
 *   - entry name / mtime come from the last member header parsed while the
 *     first 64 KiB were produced (gzip.c:160-163, :196-201, :280-296).
 * There is no CPU decode path: without a usable GPU, init() fails the open.
 *
 * Environment: LA_GPU_DEVICE, LA_GPU_BATCH_MIB (as for lz4), LA_GZIP_STRICT, LA_GZIP_FLUSH_POINTS, LA_GZIP_BLOCK_STARTS.
 */
#include "la_read_private.h"
#include "../../include/la_gpu.h"
#include "../../include/la_host.h"
#include <errno.h>
#include <stdio.h>
#include <time.h>

/* LA_GPU_TRACE=1: per-window phase times on stderr (diagnostic) */
static double gz_now(void)
{
	struct timespec ts;
	clock_gettime(CLOCK_MONOTONIC, &ts);
	return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
}

#define OUT_BLOCK 65536u	/* gzip.c:314 */
#define LA_GZ_HIST 32768u	/* the deflate window: as far as a distance reaches */
#define LA_GZ_BLOCKS_SPAN_MAX (((size_t)1 << 29) - 65536)	/* LA_GZ_OPT_BLOCK_STARTS: a source below 2^29 bytes, header included */

/* What a walk asks of the next window's first unit, because a decode refuted the table: pass over `skip` candidate
 * boundaries (1f 8b 08 guesses, 00 00 FF FF markers) and give it an output slot of `cap` bytes at least. */
struct gz_hint { uint32_t skip, cap; };

/* which table the window in flight was queued from */
enum gz_inflight { GZ_NONE = 0, GZ_MEMBERS, GZ_PIECES, GZ_BLOCKS };

struct gzip_private {
	la_window w;
	la_buf stage;		/* pinned */
	size_t stage_len;
	la_buf d_src, d_dst, d_tabs;
	la_buf slab;		/* [carry | this batch's bytes] (pinned) */
	/* The second slab: while the caller holds `slab`, the NEXT window's decoded bytes are already on their way into this
	 * one (queued behind the decode by gz_prepare, at the offset the carry will take).  When the window turns out as
	 * its index promised -- every member exactly as long as its ISIZE said, nothing refused -- the bytes are in place
	 * when the next read() looks, the carry is put in front and the two slabs change roles; otherwise the copy is done
	 * again the ordinary way.  (The lz4 and zstd filters have two whole slots; here one slab more is what was missing.) */
	la_buf slab2;
	int no_ahead;		/* LA_GZ_NO_COPY_AHEAD=1 (measurements: the single-slab behaviour of round 2) */
	int ahead_ok;		/* a copy into slab2 is queued ... */
	size_t ahead_rem;	/* ... behind this many carry bytes ... */
	size_t ahead_len;	/* ... this long */
	size_t carry_len;	/* decoded but not yet delivered (< 64 KiB) */
	size_t last_ret;	/* bytes handed out by the previous read() */
	la_buf h_res;
	uint64_t total_out;	/* bytes decoded so far (delivered + carry) */
	struct gz_hint hint;	/* for the first member of the next window, and for that one only */
	int strict;
	uint32_t slot_limit;	/* an output slot cannot pass 2 GiB (32-bit positions on the device); LA_GZ_TEST_SLOT_LIMIT lowers it for tests */
	uint64_t span_limit;	/* a member's compressed span cannot pass 4 GiB - 1 (32-bit table); LA_GZ_TEST_SPAN_LIMIT lowers it */
	int trace;
	int loose;		/* the stream's headers carry unusual XFL / OS bytes: index without LA_GZ_INDEX_STRICT */
	/* header metadata (gzip.c:280-296) */
	uint32_t mtime;
	char *name;
	/* the window whose device work is queued but not yet looked at (decode-ahead: it was gathered,
	 * uploaded, indexed and launched BEFORE the previous read() returned, so the device works on it
	 * while the caller consumes the slab it was given): st->idx or st->pcs, as `inflight` says */
	la_gz_index idx;
	enum gz_inflight inflight;
	size_t o_res;		/* where its results are in d_tabs */
	la_verdict verdict;	/* what the next read() reports once the bytes in front of it are out */
	int eof;
	/* Piece mode (LA_GZIP_FLUSH_POINTS=1 or =chain): ONE member decoded from its flush points, a piece per lane or wave
	 * (la_gz_pieces_build, LA_GZ_OPT_PIECES).  The member may span any number of windows; what is carried from one
	 * to the next is {in the member, CRC32 so far, bytes so far}. */
	int fp_on;
	struct { int in_member; uint32_t crc; uint64_t bytes; } pm;
	int pm_declined;	/* the member at the head of the window is decoded the ordinary way (its pieces depend on each other) */
	struct gz_hint pm_hint;	/* skip: for the first piece of the next window; cap: from that piece on, for the rest of the member */
	size_t pm_from;		/* where the pieces of the window in flight start: behind the header in a member's first window, else 0 */
	la_gz_pieces pcs;
	/* LA_GZIP_FLUSH_POINTS=chain: the pieces are decoded as one stream (LA_GZ_OPT_CHAIN), so a member in piece mode carries
	 * one thing more from window to window: the last min(32768, bytes so far) bytes of its output, which go in front of
	 * the next window's packed range on the device.  They are kept HERE, on the host, and uploaded with each window, not
	 * copied from the previous window's output on the device: the bytes pass through the host slab anyway; a window that
	 * gave fewer than 32 KiB needs bytes of the windows before it, which on the device would be a copy onto itself; the
	 * output buffer may be reallocated when a window needs a larger one; and after a retry (merged pieces, larger slots)
	 * only the host knows which of the device's bytes were confirmed.  32 KiB per window of megabytes is not measurable. */
	int fp_chain;
	la_buf hist;		/* pinned, LA_GZ_HIST bytes */
	size_t hist_len;
	/* Block-start mode (LA_GZIP_BLOCK_STARTS=1): the FIRST member of the stream, when it carries no BGZF size, is decoded
	 * from the block starts the device finds in it (LA_GZ_OPT_BLOCK_STARTS): one span per window, from a true block
	 * boundary -- behind the header, or where the window before stopped -- to the end of the window.  What is carried
	 * from window to window is what the chain of pieces carries (st->pm, st->hist) and one thing more: the bit of the
	 * span's first byte the boundary lies at.  Members behind the first go the ordinary way. */
	int bs_on;
	int bs_done;		/* the first member is behind us, or it left this mode before anything of it was out */
	uint32_t bs_bit;	/* 0..7 */
	uint32_t bs_cap;	/* a larger output capacity asked for by a window that could not place one piece */
	size_t bs_span_limit;	/* bytes of the window given to one call: below 2^29 (32-bit bit offsets on the device); grows when
				 * a span confirms nothing; LA_GZ_TEST_BLOCKS_WINDOW lowers where it starts, for tests */
	size_t bs_from, bs_len;	/* the span of the window in flight */
	la_gz_member bs_span;
};

static int gzip_bidder_bid(struct archive_read_filter_bidder *, struct archive_read_filter *);
static int gzip_bidder_init(struct archive_read_filter *);
static ssize_t gzip_filter_read(struct archive_read_filter *, const void **);
static int gzip_filter_close(struct archive_read_filter *);
static int gzip_read_header(struct archive_read_filter *, struct archive_entry *);

static const struct archive_read_filter_bidder_vtable gzip_bidder_vtable = {
	.bid = gzip_bidder_bid,
	.init = gzip_bidder_init,
};

static const struct archive_read_filter_vtable gzip_reader_vtable = {
	.read = gzip_filter_read,
	.close = gzip_filter_close,
	.read_header = gzip_read_header,
};

int archive_read_support_filter_gzip(struct archive *_a)
{
	struct archive_read *a = (struct archive_read *)_a;
	if (__archive_read_register_bidder(a, NULL, "gzip", &gzip_bidder_vtable) != ARCHIVE_OK)
		return ARCHIVE_FATAL;
	return ARCHIVE_OK;
}

int archive_read_support_compression_gzip(struct archive *a)
{
	return archive_read_support_filter_gzip(a);
}

/*
 * gzip.c:128-239 through the peek interface: the fixed 10 bytes first, then as
 * much as the optional fields need (file names are limited to what upstream
 * can expose in one peek, as in the reference).
 */
static int gzip_bidder_bid(struct archive_read_filter_bidder *self, struct archive_read_filter *filter)
{
	ssize_t avail;
	(void)self;
	const unsigned char *p = __archive_read_filter_ahead(filter, 10, &avail);
	if (p == NULL || avail == 0)
		return 0;
	if (p[0] != 0x1f || p[1] != 0x8b || p[2] != 0x08 || (p[3] & 0xE0))
		return 0;
	/* optional fields: like the reference's parser (gzip.c:183-194), extend the peek one
	 * byte at a time until the header parses or upstream cannot supply another byte */
	for (;;) {
		la_gz_header h;
		if (la_gz_header_parse(p, (size_t)avail, &h)) {
			/* Deployment switch: with LA_GZIP_BID_ONLY_INDEXED=1 this bidder takes only
			 * streams whose first member carries the BGZF "BC" size subfield -- the many-member shape the
			 * device path is built for -- and bids 0 on anything else, so that the reference's own gzip
			 * bidder, registered beside it, wins ordinary single-member .gz files (one serial deflate
			 * chain decodes faster on a host core than on one GPU wave). */
			const char *only = getenv("LA_GZIP_BID_ONLY_INDEXED");
			if (only && only[0] == '1' && h.bgzf_size == 0)
				return 0;
			/* Default policy (la_bid_policy.c): ONE large member is a single serial deflate chain -- one wave on the
			 * device, far slower than zlib on a host core -- so a stream whose first member carries no size subfield and
			 * shows no second member header inside the look-ahead is not bid for (LA_GPU_BID=all takes everything). */
			if (h.bgzf_size == 0 && !la_bid_take_all()) {
				const size_t la = la_bid_lookahead(256);
				size_t got = 0;
				const unsigned char *w = la_bid_peek(filter, la, &got);
				if (w != NULL && !la_bid_gzip_parallel(w, got, h.len, la))
					return 0;
			}
			return 27;
		}
		p = __archive_read_filter_ahead(filter, (size_t)avail + 1, &avail);
		if (p == NULL)
			return 0;
	}
}

static int gzip_bidder_init(struct archive_read_filter *self)
{
	self->code = ARCHIVE_FILTER_GZIP;
	self->name = "gzip";
	struct gzip_private *st = calloc(1, sizeof(*st));
	if (st == NULL) {
		archive_set_error(&self->archive->archive, ENOMEM, "Can't allocate data for gzip decompression");
		return ARCHIVE_FATAL;
	}
	const char *sv = getenv("LA_GZIP_STRICT");
	st->strict = sv && atoi(sv) != 0;
	st->slot_limit = 0x80000000u;
	{
		const char *sl = getenv("LA_GZ_TEST_SLOT_LIMIT");
		if (sl != NULL && strtoul(sl, NULL, 10) >= 65536 && strtoul(sl, NULL, 10) < st->slot_limit)
			st->slot_limit = (uint32_t)strtoul(sl, NULL, 10);
	}
	st->span_limit = LA_GZ_SPAN_LIMIT;
	{
		const char *v = getenv("LA_GZ_TEST_SPAN_LIMIT");
		if (v != NULL && strtoull(v, NULL, 10) > 0 && strtoull(v, NULL, 10) < st->span_limit)
			st->span_limit = strtoull(v, NULL, 10);
	}
	st->fp_on = la_gz_flush_points_enabled();
	st->fp_chain = la_gz_flush_points_chain();
	st->bs_on = la_gz_block_starts_enabled();
	st->bs_span_limit = LA_GZ_BLOCKS_SPAN_MAX;
	{
		const char *v = getenv("LA_GZ_TEST_BLOCKS_WINDOW");
		if (v != NULL && strtoull(v, NULL, 10) >= 1024 && strtoull(v, NULL, 10) < st->bs_span_limit)
			st->bs_span_limit = (size_t)strtoull(v, NULL, 10);
	}
	st->trace = getenv("LA_GPU_TRACE") != NULL && atoi(getenv("LA_GPU_TRACE")) != 0;
	st->no_ahead = getenv("LA_GZ_NO_COPY_AHEAD") != NULL && atoi(getenv("LA_GZ_NO_COPY_AHEAD")) != 0;
	if (la_window_open(self, &st->w, "gzip") != ARCHIVE_OK) {
		free(st);
		return ARCHIVE_FATAL;
	}
	self->data = st;
	self->vtable = &gzip_reader_vtable;
	return ARCHIVE_OK;
}

static int gzip_read_header(struct archive_read_filter *self, struct archive_entry *entry)
{
	struct gzip_private *st = (struct gzip_private *)self->data;
	if (st->mtime != 0)	/* a mtime of 0 is considered invalid/missing */
		archive_entry_set_mtime(entry, st->mtime, 0);
	if (st->name)
		archive_entry_set_pathname(entry, st->name);
	return ARCHIVE_OK;
}

#define ALIGN256(x) (((x) + 255) & ~(size_t)255)

/* The units in flight, members of st->idx or pieces of st->pcs: what the launch, the result fetch and the slab need of
 * either table. */
struct gz_units {
	enum gz_inflight kind;
	const la_gz_member *tab;
	uint32_t n;
	uint32_t n_res;		/* results the device writes: one per unit, three for the one span of block-start mode */
	uint64_t consumed;	/* bytes of the window the table covers */
	uint64_t max_out;	/* sum of the slots */
	int end_kind;		/* LA_END_*: what follows the last unit */
	size_t lead;		/* room in front of unit 0's output on the device: chain keeps the history there */
	int packed;		/* the units' bytes lie back to back from unit 0's, whatever their slots say (LA_GZ_OPT_CHAIN) */
};

static struct gz_units gz_units_of(const struct gzip_private *st, enum gz_inflight kind)
{
	const la_gz_pieces *p = &st->pcs;
	const la_gz_index *x = &st->idx;
	if (kind == GZ_PIECES)
		return (struct gz_units){ kind, p->pieces, p->n, p->n, p->consumed, p->max_out, p->end_kind,
		    st->fp_chain ? LA_GZ_HIST : 0, st->fp_chain };
	if (kind == GZ_BLOCKS)
		return (struct gz_units){ kind, &st->bs_span, 1, 3, st->bs_from + st->bs_len, st->bs_span.dst_cap, LA_END_NEED_MORE,
		    LA_GZ_HIST, 1 };
	return (struct gz_units){ kind, x->members, x->n, x->n, x->consumed, x->max_out, x->end_kind, 0, 0 };
}

/* the window's table is done with (the one that is not in use is empty: freeing it changes nothing) */
static void gz_free_tables(struct gzip_private *st)
{
	la_gz_pieces_free(&st->pcs);
	la_gz_index_free(&st->idx);
}

/* One window's stream-order walk: what gzip_walk_members and gzip_walk_pieces work out and gz_slab acts on. */
struct gz_walk {
	uint64_t total;		/* stream offset behind the units taken whole */
	uint64_t cutoff;	/* deliver only up to here (UINT64_MAX: no error follows) */
	uint32_t take;		/* units whose bytes join the slab */
	uint32_t last_out;	/* bytes of a failing last unit that still count as produced */
	int contiguous;		/* every unit taken filled its slot: their bytes are one range on the device */
	size_t used;		/* compressed bytes of the window that are done with (all the table covers, unless a unit comes again) */
	int again;		/* the walk asked for the same bytes again on other terms (merged units, larger slots, the ordinary way) */
	double b0, b1;		/* trace stamps: in front of and behind the wait for the results */
};

/* ---- the delivery rules of the reference, each stated once ---- */

/* gzip.c:314, :446: on an error the reference has delivered whole 64 KiB blocks only */
static uint64_t gz_floor(uint64_t off)
{
	return (off / OUT_BLOCK) * OUT_BLOCK;
}

/* an error stands in front of the next unit: whole blocks of what is confirmed, then the message */
static void gz_refuse(struct gzip_private *st, struct gz_walk *w, const char *msg)
{
	la_verdict_set(&st->verdict, ARCHIVE_FATAL, "%s", msg);
	w->cutoff = gz_floor(w->total);
}

static void gz_too_large(struct gzip_private *st, struct gz_walk *w)
{
	gz_refuse(st, w, la_end_message(LA_END_GZ_TOO_LARGE, 1));
}

/* a trailer that does not match under LA_GZIP_STRICT=1 (new behaviour: the reference never looks, gzip.c:423), or an
 * answer the walk does not know: EVERYTHING in front of the unit that shows it, then the message */
static void gz_fail_in_front(struct gzip_private *st, struct gz_walk *w, const char *msg)
{
	la_verdict_set(&st->verdict, ARCHIVE_FATAL, "%s", msg);
	w->cutoff = w->total;
}

/* inflate() failed after out_len bytes of the last unit taken: the block that holds the last of them is not out yet.
 * GZ_DATA_ERROR (gzip.c:494-499), or GZ_NO_TRAILER -- the body is complete, the trailer is short: ARCHIVE_FATAL
 * without a message (gzip.c:419-421). */
#define GZ_DATA_ERROR "gzip decompression failed"
#define GZ_NO_TRAILER NULL
static void gz_failed_after(struct gzip_private *st, struct gz_walk *w, uint32_t take, uint32_t out_len, const char *msg)
{
	la_verdict_set(&st->verdict, ARCHIVE_FATAL, msg ? "%s" : NULL, msg);
	w->cutoff = out_len == 0 ? gz_floor(w->total) : gz_floor(w->total + out_len - 1);
	w->last_out = out_len;
	w->take = take;
}

/* the input ended after out_len bytes (gzip.c:464-469): the reference has flushed the block they complete */
static void gz_truncated(struct gzip_private *st, struct gz_walk *w, uint32_t take, uint32_t out_len)
{
	la_verdict_set(&st->verdict, ARCHIVE_FATAL, "truncated gzip input");
	w->cutoff = gz_floor(w->total + out_len);
	w->last_out = out_len;
	w->take = take;
}

/*
 * LA_ST_GZ_OUT_FULL: unit i comes again with twice the slot, up to st->slot_limit; a slot that cannot grow any further
 * (32-bit positions on the device) is said by name instead of retrying for ever or delivering a wrapped slot.
 * `prev`: the hint this window was built with, `h`: the one for the next.  small_to_64k: a slot below 32 KiB goes
 * straight to 64 KiB -- the member walk's rule (an ISIZE claim may be anything); a piece's slot is never that small
 * unless it is all its span can produce (piece_slot, la_gzip_index.c), so the piece walk has no such step.
 */
static void gz_grow_slot(struct gzip_private *st, struct gz_walk *w, struct gz_hint *h, struct gz_hint prev, uint32_t i,
    uint32_t dst_cap, int small_to_64k)
{
	const uint32_t base = dst_cap > prev.cap ? dst_cap : prev.cap;
	if (base >= st->slot_limit) { gz_too_large(st, w); return; }
	h->cap = small_to_64k && base < 32768 ? 65536 : (base > st->slot_limit / 2 ? st->slot_limit : base * 2);
	h->skip = i == 0 ? prev.skip : 0;
	w->again = 1;
}

/* header metadata: what the reference has parsed while the first 64 KiB were produced (gzip.c:160-163, :196-201) */
static void gz_take_metadata(struct gzip_private *st, const struct gz_walk *w, const la_gz_header *h)
{
	if (w->total >= OUT_BLOCK)
		return;
	st->mtime = h->mtime;
	if (h->name_off) {
		free(st->name);
		st->name = strdup((const char *)st->stage.p + h->off + h->name_off);
	}
}

/*
 * Queue the device work of one window (its compressed bytes are already on their way: gz_prepare): table layout,
 * device buffers, table upload, under chain the history in front of the output, and the decode.  Nothing is waited for.
 */
static int gz_launch(struct archive_read_filter *self, struct gzip_private *st, const struct gz_units *u)
{
	la_gpu_ctx *gpu = st->w.gpu;
	const int blocks = u->kind == GZ_BLOCKS;
	const int pieces = u->kind == GZ_PIECES || blocks;
	size_t o = 0;
	const size_t o_mem = o; o += ALIGN256((size_t)u->n * sizeof(la_gz_member));
	const size_t o_res = o; o += ALIGN256((size_t)u->n_res * sizeof(la_gz_result));	/* (st->o_res once the window is in flight) */
	const size_t o_sum = o; o += 256;
	if (la_buf_dev(gpu, &st->d_dst, u->lead + (size_t)u->max_out + 64) < 0 || la_buf_dev(gpu, &st->d_tabs, o) < 0)
		return la_window_fail(self, &st->w, "device allocation");
	uint8_t *T = st->d_tabs.p;
	if (la_gpu_memcpy_h2d(gpu, T + o_mem, u->tab, (size_t)u->n * sizeof(la_gz_member)) != LA_OK)
		return la_window_fail(self, &st->w, "host to device copy");
	la_gz_batch bt = {
		.d_src = st->d_src.p, .src_bytes = blocks ? (size_t)u->consumed : pieces ? st->stage_len : (size_t)u->consumed,
		.d_members = (const la_gz_member *)(T + o_mem), .n_members = u->n,
		.d_dst = st->d_dst.p + u->lead, .dst_cap = u->max_out, .d_results = (la_gz_result *)(T + o_res),
		.d_summary = pieces ? NULL : (la_batch_summary *)(T + o_sum), .options = pieces ? LA_GZ_OPT_PIECES : 0,
	};
	if (u->packed) {
		if (la_buf_pinned(gpu, &st->hist, LA_GZ_HIST, st->hist_len) < 0)
			return la_window_fail(self, &st->w, "pinned history allocation");
		if (!st->pm.in_member)
			st->hist_len = 0;
		if (st->hist_len &&
		    la_gpu_memcpy_h2d(gpu, st->d_dst.p + u->lead - st->hist_len, st->hist.p, st->hist_len) != LA_OK)
			return la_window_fail(self, &st->w, "host to device copy");
		bt.options |= LA_GZ_OPT_CHAIN;
		bt.hist_len = (uint32_t)st->hist_len;
	}
	if (blocks)
		bt.options |= LA_GZ_OPT_BLOCK_STARTS | st->bs_bit << LA_GZ_OPT_START_BIT_SHIFT;
	if (la_gpu_gzip_decode(gpu, &bt) != LA_OK)
		return la_window_fail(self, &st->w, "la_gpu_gzip_decode");
	st->o_res = o_res;
	st->inflight = u->kind;
	return 0;
}

/*
 * The end of a window's stream-order walk, for members and pieces alike: bring the bytes of units [0, w->take) behind
 * the carry and decide how much of [carry | new bytes] may go out now.
 */
static int gz_slab(struct archive_read_filter *self, struct gzip_private *st, const struct gz_units *u,
    const la_gz_result *res, const struct gz_walk *w)
{
	la_gpu_ctx *gpu = st->w.gpu;
	const uint8_t *d_out = st->d_dst.p + u->lead;	/* where unit 0's bytes are on the device */
	const uint32_t take = w->take, last_out = w->last_out;
	uint64_t new_bytes = (w->total - st->total_out) + last_out;
	const int ahead = st->ahead_ok && take && w->contiguous && last_out == 0 && st->carry_len == st->ahead_rem &&
	    new_bytes <= st->ahead_len;
	st->ahead_ok = 0;
	if (ahead) {
		/* they came over while the caller was busy (the sync above covered the copy): carry in front, change slabs */
		if (st->carry_len)
			memcpy(st->slab2.p, st->slab.p, st->carry_len);
		const la_buf tb = st->slab; st->slab = st->slab2; st->slab2 = tb;
	} else if (la_buf_pinned(gpu, &st->slab, st->carry_len + (size_t)new_bytes + 16, st->carry_len) < 0)
		return la_window_fail(self, &st->w, "pinned slab allocation");
	uint8_t *dstp = st->slab.p + st->carry_len;
	const double b2 = st->trace ? gz_now() : 0;
	if (take && !ahead) {
		if (u->packed || (w->contiguous && last_out == 0)) {	/* one copy brings them all */
			if (new_bytes && la_gpu_memcpy_d2h(gpu, dstp, d_out, (size_t)new_bytes) != LA_OK)
				return la_window_fail(self, &st->w, "device to host copy");
		} else {
			size_t at = 0;
			for (uint32_t i = 0; i < take; i++) {
				size_t len = res[i].out_len;
				if (len && la_gpu_memcpy_d2h(gpu, dstp + at, d_out + u->tab[i].dst_off, len) != LA_OK)
					return la_window_fail(self, &st->w, "device to host copy");
				at += len;
			}
		}
		if (la_gpu_sync(gpu) != LA_OK)
			return la_window_fail(self, &st->w, "device to host copy");
	}
	if (st->trace)
		fprintf(stderr, "la_gzip:   h2d+decode %.1f ms, walk+grow %.1f ms, d2h %.1f ms (%llu bytes, contiguous %d, copied ahead %d)\n",
		    w->b1 - w->b0, b2 - w->b1, gz_now() - b2, (unsigned long long)new_bytes, w->contiguous, ahead);
	if (u->packed && st->pm.in_member) {
		/* the member goes on: the last LA_GZ_HIST bytes of [history | confirmed bytes of this window] are the next
		 * window's history */
		const size_t nb = (size_t)(w->total - st->total_out);
		if (nb >= LA_GZ_HIST) {
			memcpy(st->hist.p, dstp + nb - LA_GZ_HIST, LA_GZ_HIST);
			st->hist_len = LA_GZ_HIST;
		} else {
			const size_t keep = st->hist_len < LA_GZ_HIST - nb ? st->hist_len : LA_GZ_HIST - nb;
			memmove(st->hist.p, st->hist.p + st->hist_len - keep, keep);
			memcpy(st->hist.p + keep, dstp, nb);
			st->hist_len = keep + nb;
		}
	} else if (u->packed)
		st->hist_len = 0;
	st->total_out = w->total + last_out;
	st->carry_len += (size_t)new_bytes;

	/* how much of [carry | new bytes] may go out now */
	uint64_t slab_start = st->total_out - st->carry_len;	/* stream offset of slab[0] */
	uint64_t lim;
	if (w->cutoff != UINT64_MAX)
		lim = w->cutoff;			/* an error follows: the reference's count */
	else if (st->eof)
		lim = st->total_out;			/* clean end: everything */
	else
		lim = gz_floor(st->total_out);		/* keep the partial last block back */
	if (lim < slab_start)
		lim = slab_start;
	st->last_ret = (size_t)(lim - slab_start);
	return 0;
}

/*
 * The stream-order walk over the members of st->idx: each one is judged by its own trailer.  On return w->used =
 * compressed bytes of the window that are done with, w->cutoff = stream offset up to which bytes may be delivered
 * (everything, unless an error follows).
 */
static void gzip_walk_members(struct gzip_private *st, const la_gz_result *res, struct gz_walk *w)
{
	const la_gz_index *x = &st->idx;
	const struct gz_hint prev = st->hint;
	st->hint.skip = st->hint.cap = 0;
	for (uint32_t i = 0; i < x->n; i++) {
		const la_gz_result *r = &res[i];
		const la_gz_member *m = &x->members[i];
		const la_gz_header *h = &x->headers[i];
		const uint64_t member_start = h->off;

		/* The deflate stream ran into the end of its span although more input exists:
		 * the boundary (a 1f 8b 08 guess, or a wrong BGZF size) was not the member's
		 * end.  Decode this member again with the span extended past it. */
		if ((r->status == LA_ST_GZ_TRUNCATED &&
		    (m->src_off + m->src_len < st->stage_len || !st->w.upstream_eof)) ||
		    /* ... or it ended with fewer than 8 bytes left in a span that a BGZF size field or a
		     * boundary guess cut short while the window holds more bytes: same cure */
		    (r->status == LA_ST_GZ_NO_TRAILER && m->src_off + m->src_len < st->stage_len)) {
			w->used = (size_t)member_start;
			st->hint.skip = (i == 0 ? prev.skip : 0) + 1;
			st->hint.cap = i == 0 ? prev.cap : 0;
			w->again = 1;
			return;
		}
		if (r->status == LA_ST_GZ_OUT_FULL) {
			/* the ISIZE claim was too small for what the member really holds */
			w->used = (size_t)member_start;
			gz_grow_slot(st, w, &st->hint, prev, i, m->dst_cap, 1);
			return;
		}
		if (r->status == LA_ST_GZ_NO_TRAILER && !st->w.upstream_eof) {
			/* the trailer lies beyond this window */
			w->used = (size_t)member_start;
			return;
		}
		gz_take_metadata(st, w, h);
		switch (r->status) {
		case LA_ST_OK:
		case LA_ST_GZ_BAD_CRC:
		case LA_ST_GZ_BAD_ISIZE:
			if (st->strict && r->status != LA_ST_OK) {
				gz_fail_in_front(st, w, la_status_message(r->status));
				break;
			}
			if (r->out_len != m->dst_cap)
				w->contiguous = 0;
			w->take = i + 1;
			w->total += r->out_len;
			if (h->bgzf_size && (uint64_t)r->consumed + 8 < m->src_len) {
				/* the member ended before the place its BGZF size field points at: the field is
				 * only a hint (the reference never reads FEXTRA, gzip.c:185-199) and it was wrong.
				 * The stream goes on right behind this member's trailer: index again from there. */
				w->used = (size_t)(m->src_off + (uint64_t)r->consumed + 8);
				break;
			}
			if (x->speculative && !h->bgzf_size && (uint64_t)r->consumed + 8 < m->src_len) {
				const uint64_t p = m->src_off + (uint64_t)r->consumed + 8;
				const uint8_t *q = st->stage.p + p;
				const uint64_t rem = st->stage_len - p;
				if (!st->loose && rem >= 4 && q[0] == 0x1f && q[1] == 0x8b && q[2] == 0x08 && (q[3] & 0xE0) == 0) {
					/* a header the strict boundary search passed over (unusual XFL / OS): the
					 * stream goes on here; from now on every 1f 8b 08 is a candidate */
					st->loose = 1;
					w->used = (size_t)p;
					break;
				}
				/* bytes after the trailer are not a member header: silent end (gzip.c:351-353) */
				st->eof = 1;
				break;
			}
			continue;	/* the member is fine: on to the next */
		case LA_ST_GZ_DATA:
			gz_failed_after(st, w, i + 1, r->out_len, GZ_DATA_ERROR);
			break;
		case LA_ST_GZ_TRUNCATED:
			gz_truncated(st, w, i + 1, r->out_len);
			break;
		case LA_ST_GZ_NO_TRAILER:
			gz_failed_after(st, w, i + 1, r->out_len, GZ_NO_TRAILER);
			break;
		default:
			gz_fail_in_front(st, w, GZ_DATA_ERROR);
			break;
		}
		return;		/* the walk ends at member i */
	}
	/* every member of the window is fine: what comes after it? */
	if (x->end_kind == LA_END_EOF)
		st->eof = 1;
	else if (x->end_kind == LA_END_TRUNCATED)
		gz_truncated(st, w, w->take, 0);
	else if (x->end_kind == LA_END_GZ_TOO_LARGE)
		gz_too_large(st, w);
}

/*
 * The stream-order walk over the pieces of st->pcs.  Piece k is confirmed only by LA_ST_GZ_PIECE_END with consumed ==
 * src_len (la_host.h: the chain is then correct by induction); what the first unconfirmed piece answers decides how the
 * walk ends, and whatever the pieces behind it decoded is discarded.
 */
static void gzip_walk_pieces(struct gzip_private *st, const la_gz_result *res, struct gz_walk *w)
{
	const la_gz_pieces *x = &st->pcs;
	const struct gz_hint prev = st->pm_hint;
	st->pm_hint.skip = 0;		/* (pm_hint.cap stays for the rest of the member: "from that piece on") */
	/* A retry that the member walk asked for and a window of pieces overtook (the member at the head of that window
	 * shows a flush point) is still on record in st->hint, and has always counted as "asked again" for this window
	 * too: kept as it is (open point). */
	w->again = st->hint.skip != 0 || st->hint.cap != 0;
	if (!st->pm.in_member) {
		/* (dropped again should the member leave piece mode: it is then parsed a second time) */
		la_gz_header h;
		la_gz_header_parse(st->stage.p, st->stage_len, &h);
		gz_take_metadata(st, w, &h);
	}
	for (uint32_t i = 0; i < x->n; i++) {
		const la_gz_result *r = &res[i];
		const la_gz_member *m = &x->pieces[i];
		/* where the next window starts when piece i has to be decoded again (piece 0 of a member's first
		 * window: at the header) */
		const size_t again_at = i == 0 ? 0 : (size_t)m->src_off;
		const int more_behind = m->src_off + m->src_len < st->stage_len || !st->w.upstream_eof;
		switch (r->status) {
		case LA_ST_GZ_PIECE_END:
			if (r->consumed != m->src_len) {	/* (a span the image cut short: not a boundary we can vouch for) */
				gz_refuse(st, w, GZ_DATA_ERROR);
				break;
			}
			st->pm.crc = la_crc32_combine(st->pm.crc, r->crc32, r->out_len);
			st->pm.bytes += r->out_len;
			st->pm.in_member = 1;
			if (i + 1 < x->n && (r->out_len != m->dst_cap || (m->dst_cap & 15)))
				w->contiguous = 0;
			w->take = i + 1;
			w->total += r->out_len;
			continue;	/* confirmed: on to the next */
		case LA_ST_OK: {
			/* the stream's final block ended inside this piece: the member's trailer follows */
			const uint64_t tr = m->src_off + (uint64_t)r->consumed;
			if (tr + 8 > st->stage_len && !st->w.upstream_eof) {
				w->used = again_at;	/* the trailer lies beyond this window */
				break;
			}
			if (tr + 8 > st->stage_len) {	/* short trailer at the end of input */
				gz_failed_after(st, w, i + 1, r->out_len, GZ_NO_TRAILER);
				break;
			}
			const uint8_t *t = st->stage.p + tr;
			const uint32_t crc = la_crc32_combine(st->pm.crc, r->crc32, r->out_len);
			const uint32_t isize = (uint32_t)(st->pm.bytes + r->out_len);
			const uint32_t t_crc = (uint32_t)t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24;
			const uint32_t t_len = (uint32_t)t[4] | (uint32_t)t[5] << 8 | (uint32_t)t[6] << 16 | (uint32_t)t[7] << 24;
			if (st->strict && (t_crc != crc || t_len != isize)) {
				/* as a many-member mismatch: everything in front of the unit that shows it (the pieces confirmed so far) */
				gz_fail_in_front(st, w, la_status_message(t_crc != crc ? LA_ST_GZ_BAD_CRC : LA_ST_GZ_BAD_ISIZE));
				break;
			}
			w->take = i + 1;
			w->total += r->out_len;
			/* the member is over: indexing resumes the ordinary way behind its trailer */
			memset(&st->pm, 0, sizeof(st->pm));
			st->pm_hint.cap = 0;
			w->used = (size_t)(tr + 8);
			break;
		}
		case LA_ST_GZ_NEEDS_HISTORY:
			/* the blocks behind this flush point reach back into the piece before (Z_SYNC_FLUSH) */
			if (st->pm_from) {
				/* the member's header is still at the head of the window, so nothing of the member has left
				 * a walk: piece mode is left, the pieces confirmed above are dropped, and the member is
				 * indexed again from its header the ordinary way */
				memset(&st->pm, 0, sizeof(st->pm));
				st->pm_hint.cap = 0;
				st->pm_declined = w->again = 1;
				w->total = st->total_out;
				w->take = 0;
				w->contiguous = 1;
				w->used = 0;
				break;
			}
			/* a member that changes its nature after pieces of it are out: refused by name (deliberate
			 * divergences) -- the device has no window of the bytes in front to go on from */
			gz_refuse(st, w,
			    "gzip member stops being independent pieces: blocks behind a flush point depend on earlier output (read it without LA_GZIP_FLUSH_POINTS)");
			break;
		case LA_ST_GZ_TRUNCATED:
			if (more_behind) {
				/* the marker this piece ends in is not a block boundary (00 00 FF FF inside stored data or
				 * Huffman bits): merge the piece with the next one and decode again from here */
				w->used = again_at;
				st->pm_hint.skip = (i == 0 ? prev.skip : 0) + 1;
				w->again = 1;
				break;
			}
			gz_truncated(st, w, i + 1, r->out_len);
			break;
		case LA_ST_GZ_OUT_FULL:
			w->used = again_at;
			gz_grow_slot(st, w, &st->pm_hint, prev, i, m->dst_cap, 0);
			break;
		case LA_ST_GZ_DATA:
		default:
			gz_failed_after(st, w, i + 1, r->out_len, GZ_DATA_ERROR);
			break;
		}
		return;		/* the walk ends at piece i */
	}
	if (st->w.upstream_eof && x->consumed >= st->stage_len)
		/* every piece confirmed, no final block, no byte left: the member was cut behind a flush point */
		gz_truncated(st, w, w->take, 0);
	else if (x->end_kind == LA_END_GZ_TOO_LARGE)
		gz_too_large(st, w);
}

/*
 * Block-start mode: the one span of the window, judged by the three results of LA_GZ_OPT_BLOCK_STARTS (la_gpu.h).  The
 * device has confirmed the chain itself; what is left to the host is where the chain stands on a block boundary (res[2]),
 * whether more input lies behind the span, and the member's trailer.
 */
static void gzip_walk_blocks(struct gzip_private *st, const la_gz_result *res, struct gz_walk *w)
{
	const la_gz_result *r = &res[0], *b = &res[2];
	const size_t from = st->bs_from, span_end = from + st->bs_len;
	const int more_behind = span_end < st->stage_len || !st->w.upstream_eof;
	const uint32_t start_bit = st->bs_bit;
	if (!st->pm.in_member) {
		la_gz_header h;
		la_gz_header_parse(st->stage.p, st->stage_len, &h);
		gz_take_metadata(st, w, &h);
	}
	w->used = 0;
	if (r->status == LA_ST_OK) {
		/* the final block ended: the member's trailer follows on the next byte boundary */
		const uint64_t tr = from + (((uint64_t)r->consumed + 7) >> 3);
		if (tr + 8 > st->stage_len && !st->w.upstream_eof) {
			/* the trailer lies beyond this window: the same bytes again once more of them are here (a span that was
			 * cut short of the window reaches further next time) */
			if (span_end < st->stage_len) {
				st->bs_span_limit *= 2;
				w->again = 1;
			}
			return;
		}
		if (tr + 8 > st->stage_len) {
			gz_failed_after(st, w, 1, r->out_len, GZ_NO_TRAILER);
			return;
		}
		const uint8_t *t = st->stage.p + tr;
		const uint32_t crc = la_crc32_combine(st->pm.crc, r->crc32, r->out_len);
		const uint32_t isize = (uint32_t)(st->pm.bytes + r->out_len);
		const uint32_t t_crc = (uint32_t)t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24;
		const uint32_t t_len = (uint32_t)t[4] | (uint32_t)t[5] << 8 | (uint32_t)t[6] << 16 | (uint32_t)t[7] << 24;
		if (st->strict && (t_crc != crc || t_len != isize)) {
			gz_fail_in_front(st, w, la_status_message(t_crc != crc ? LA_ST_GZ_BAD_CRC : LA_ST_GZ_BAD_ISIZE));
			return;
		}
		w->take = 1;
		w->total += r->out_len;
		/* the member is over: what follows is indexed the ordinary way */
		memset(&st->pm, 0, sizeof(st->pm));
		st->bs_done = 1;
		st->bs_bit = 0;
		w->used = (size_t)(tr + 8);
		return;
	}
	if (r->status == LA_ST_GZ_DATA) {
		/* (the failing piece starts on a confirmed boundary and read nothing but the stream's own bits: the error is the
		 * stream's) */
		gz_failed_after(st, w, 1, r->out_len, GZ_DATA_ERROR);
		return;
	}
	if (r->status == LA_ST_GZ_TRUNCATED && !more_behind) {
		gz_truncated(st, w, 1, r->out_len);
		return;
	}
	if (r->status != LA_ST_GZ_TRUNCATED && r->status != LA_ST_GZ_PIECE_END && r->status != LA_ST_GZ_OUT_FULL) {
		gz_fail_in_front(st, w, GZ_DATA_ERROR);
		return;
	}
	/* the member goes on behind what stands on a block boundary */
	if (b->status == LA_ST_GZ_PIECE_END && (uint64_t)b->consumed > start_bit) {
		st->pm.crc = la_crc32_combine(st->pm.crc, b->crc32, b->out_len);
		st->pm.bytes += b->out_len;
		st->pm.in_member = 1;
		w->take = 1;
		w->total += b->out_len;
		w->used = from + (size_t)(b->consumed >> 3);
		st->bs_bit = b->consumed & 7u;
		if (!more_behind && w->used >= st->stage_len)
			/* a non-final block ended on the last bit of the input */
			gz_truncated(st, w, 1, 0);
		return;
	}
	/* nothing confirmed: not one piece of the span ended on a block boundary inside it */
	if (r->status == LA_ST_GZ_OUT_FULL) {
		/* ... because the first piece does not fit */
		const struct gz_hint prev = { 0, st->bs_cap };
		struct gz_hint h = prev;
		gz_grow_slot(st, w, &h, prev, 0, st->bs_span.dst_cap, 0);
		st->bs_cap = h.cap;
		return;
	}
	if (span_end < st->stage_len) {		/* the span was cut short of the window: a longer one */
		st->bs_span_limit = st->bs_span_limit * 2 < LA_GZ_BLOCKS_SPAN_MAX ? st->bs_span_limit * 2 : LA_GZ_BLOCKS_SPAN_MAX;
		if (st->bs_len < LA_GZ_BLOCKS_SPAN_MAX - from) {
			w->again = 1;
			return;
		}
	}
	if (st->stage_len < st->w.max_batch_bytes && st->bs_len < LA_GZ_BLOCKS_SPAN_MAX - from)
		return;		/* (no progress and nothing asked again: the window grows, gzip_filter_read) */
	/* one run of fixed and stored blocks as long as the window may get */
	if (!st->pm.in_member) {
		st->bs_done = 1;	/* nothing of the member is out: it goes the ordinary way, on one wave */
		w->again = 1;
		return;
	}
	gz_refuse(st, w, "gzip member holds no dynamic block start within LA_GPU_MAX_BATCH_MIB (read it without LA_GZIP_BLOCK_STARTS)");
}

/*
 * The window in flight: results, stream-order walk, slab.  On return the slab holds carry + newly decoded bytes
 * (st->carry_len updated to the total now waiting) and st->last_ret says how many of them go out now.
 */
static int gz_finish(struct archive_read_filter *self, struct gzip_private *st, struct gz_walk *w)
{
	const struct gz_units u = gz_units_of(st, st->inflight);
	*w = (struct gz_walk){ .total = st->total_out, .cutoff = UINT64_MAX, .contiguous = 1, .used = (size_t)u.consumed,
	    .b0 = st->trace ? gz_now() : 0 };
	if (la_buf_host(&st->h_res, (size_t)u.n_res * sizeof(la_gz_result)) < 0) {
		archive_set_error(&self->archive->archive, ENOMEM, "Can't allocate data for gzip decompression");
		return ARCHIVE_FATAL;
	}
	const la_gz_result *res = (const la_gz_result *)st->h_res.p;
	if (la_gpu_memcpy_d2h(st->w.gpu, st->h_res.p, st->d_tabs.p + st->o_res, (size_t)u.n_res * sizeof(la_gz_result)) != LA_OK ||
	    la_gpu_sync(st->w.gpu) != LA_OK)
		return la_window_fail(self, &st->w, "result copy");
	w->b1 = st->trace ? gz_now() : 0;
	if (u.kind == GZ_PIECES) {
		gzip_walk_pieces(st, res, w);
		st->ahead_ok = 0;
	} else if (u.kind == GZ_BLOCKS) {
		gzip_walk_blocks(st, res, w);
		st->ahead_ok = 0;
	} else
		gzip_walk_members(st, res, w);
	return gz_slab(self, st, &u, res, w);
}

/*
 * A window in which the walker found no unit to queue, for either table: free it, let the window move, and say what
 * the next look at the state will find.
 */
static int gz_nothing_queued(struct archive_read_filter *self, struct gzip_private *st, enum gz_inflight kind)
{
	const int pieces = kind == GZ_PIECES;
	const int end_kind = gz_units_of(st, kind).end_kind;
	gz_free_tables(st);
	if (la_gpu_sync(st->w.gpu) != LA_OK)	/* the upload: the window may move now */
		return la_window_fail(self, &st->w, "host to device copy");
	if (end_kind == LA_END_GZ_TOO_LARGE)
		la_verdict_set(&st->verdict, ARCHIVE_FATAL, "%s", la_end_message(LA_END_GZ_TOO_LARGE, 1));
	else if (pieces ? st->w.upstream_eof : end_kind == LA_END_TRUNCATED)
		la_verdict_set(&st->verdict, ARCHIVE_FATAL, "truncated gzip input");	/* (pieces: in a member, no byte left) */
	else if (!pieces && (end_kind != LA_END_NEED_MORE || st->w.upstream_eof))
		st->eof = 1;
	else if (!pieces && !st->loose)
		/* no trusted boundary in the whole window: before widening it, look
		 * with every 1f 8b 08 as a candidate (and keep doing so) */
		st->loose = 1;
	else if (!pieces || st->w.batch_bytes < st->w.max_batch_bytes)
		st->w.batch_bytes *= 2;		/* one member larger than the window / no marker behind the current position */
	else if (st->pm_from) {	/* the member's header is at the head of the window */
		st->pm_hint.skip = st->pm_hint.cap = 0;
		st->pm_declined = 1;		/* (the LA_ST_GZ_NEEDS_HISTORY route, before anything of the member is out) */
	} else
		la_verdict_set(&st->verdict, ARCHIVE_FATAL,
		    "gzip member stops being independent pieces: no flush point within LA_GPU_MAX_BATCH_MIB (read it without LA_GZIP_FLUSH_POINTS)");
	return 0;
}

/* The table just built goes to the device.  1: in flight; 0: it is empty, the state changed instead; < 0: error. */
static int gz_queue(struct archive_read_filter *self, struct gzip_private *st, enum gz_inflight kind)
{
	const struct gz_units u = gz_units_of(st, kind);
	if (u.n == 0)
		return gz_nothing_queued(self, st, kind);
	const int rc = gz_launch(self, st, &u);
	if (rc < 0)
		gz_free_tables(st);
	return rc < 0 ? rc : 1;
}

/*
 * gz_prepare's piece-mode branch, behind the gather and the upload.  2: the window is not one for piece mode (go on
 * the ordinary way); otherwise as gz_prepare.
 */
static int gz_prepare_pieces(struct archive_read_filter *self, struct gzip_private *st)
{
	size_t from = 0;
	if (!st->pm.in_member) {
		/* a member without a BGZF size enters piece mode if the window shows a marker inside its body */
		la_gz_header h;
		const size_t hlen = la_gz_header_parse(st->stage.p, st->stage_len, &h);
		if (hlen == 0 || h.bgzf_size || hlen >= st->stage_len ||
		    la_gz_next_marker(st->stage.p, st->stage_len, hlen) >= st->stage_len)
			return 2;
		from = hlen;
	}
	if (la_gz_pieces_build(st->stage.p, st->stage_len, from, st->w.upstream_eof, st->pm_hint.skip, st->pm_hint.cap,
	    st->w.out_budget, st->span_limit, &st->pcs) != 0) {
		archive_set_error(&self->archive->archive, ENOMEM, "Can't allocate data for gzip decompression");
		return ARCHIVE_FATAL;
	}
	st->pm_from = from;
	const int rc = gz_queue(self, st, GZ_PIECES);
	if (rc <= 0)
		return rc;
	st->ahead_ok = 0;
	la_window_ramp(&st->w);
	if (st->trace)
		fprintf(stderr, "la_gzip: window %zu bytes, %u pieces queued from %zu\n", st->stage_len, st->pcs.n, from);
	return 1;
}

/*
 * gz_prepare's block-start branch, behind the gather and the upload.  2: the window is not one for this mode (go on the
 * ordinary way); otherwise as gz_prepare.
 */
static int gz_prepare_blocks(struct archive_read_filter *self, struct gzip_private *st)
{
	size_t from = 0;
	if (!st->pm.in_member) {
		/* the stream's first member, when its header carries no BGZF size */
		la_gz_header h;
		const size_t hlen = la_gz_header_parse(st->stage.p, st->stage_len, &h);
		if (hlen == 0 || h.bgzf_size || hlen >= st->stage_len) {
			/* (a header that is not all here yet is looked at again with the next window) */
			if ((hlen != 0 && h.bgzf_size) || st->w.upstream_eof)
				st->bs_done = 1;
			return 2;
		}
		from = hlen;
		st->bs_bit = 0;
	}
	size_t len = st->stage_len - from;
	if (len > st->bs_span_limit)
		len = st->bs_span_limit;
	if (len > LA_GZ_BLOCKS_SPAN_MAX - from)
		len = LA_GZ_BLOCKS_SPAN_MAX - from;
	/* the capacity: eight times the span (as the piece walker's slots), more when a window asked for it */
	uint64_t cap = (uint64_t)len * 8 < 65536 ? 65536 : (uint64_t)len * 8;
	if (cap < st->bs_cap)
		cap = st->bs_cap;
	if (cap > st->slot_limit)
		cap = st->slot_limit;
	st->bs_from = from;
	st->bs_len = len;
	st->bs_span = (la_gz_member){ .src_off = from, .src_len = (uint32_t)len, .dst_cap = (uint32_t)cap, .dst_off = 0 };
	const int rc = gz_queue(self, st, GZ_BLOCKS);
	if (rc <= 0)
		return rc;
	st->ahead_ok = 0;
	la_window_ramp(&st->w);
	if (st->trace)
		fprintf(stderr, "la_gzip: window %zu bytes, block starts of %zu bytes from %zu, bit %u\n", st->stage_len, len, from, st->bs_bit);
	return 1;
}

/*
 * Gather one window, start its upload, find the member boundaries and queue the decode: nothing is
 * waited for.  Returns 1 when a window is in flight (st->inflight), 0 when the state changed
 * instead (end of stream, pending error, wider window, looser boundary search: the caller looks again),
 * ARCHIVE_FATAL on error.
 */
static int gz_prepare(struct archive_read_filter *self, struct gzip_private *st)
{
	const double t0 = st->trace ? gz_now() : 0;
	if (la_window_gather(self, &st->w, &st->stage, &st->stage_len) != ARCHIVE_OK)
		return ARCHIVE_FATAL;
	const double t1 = st->trace ? gz_now() : 0;
	/* the window goes to the device while the host looks for the member boundaries in it
	 * (stream-ordered copy from the pinned window; nothing writes to [0, stage_len)
	 * before the batch has been waited for) */
	if (st->stage_len &&
	    (la_buf_dev(st->w.gpu, &st->d_src, st->stage_len + 64) < 0 ||
	     la_gpu_memcpy_h2d(st->w.gpu, st->d_src.p, st->stage.p, st->stage_len) != LA_OK))
		return la_window_fail(self, &st->w, "host to device copy");
	if (st->fp_on && !st->pm_declined) {
		const int pr = gz_prepare_pieces(self, st);
		if (pr != 2)
			return pr;
	}
	if (st->bs_on && !st->bs_done && !st->fp_on) {
		const int pr = gz_prepare_blocks(self, st);
		if (pr != 2)
			return pr;
	}
	if (la_gz_index_build_ex(st->stage.p, st->stage_len, st->w.upstream_eof, st->hint.skip, st->hint.cap,
	    st->loose ? 0 : LA_GZ_INDEX_STRICT, st->w.out_budget, st->span_limit, &st->idx) != 0) {
		archive_set_error(&self->archive->archive, ENOMEM, "Can't allocate data for gzip decompression");
		return ARCHIVE_FATAL;
	}
	const int rc = gz_queue(self, st, GZ_MEMBERS);
	if (rc <= 0)
		return rc;
	/* decoded bytes of this window towards the OTHER slab, behind the place of what will be left of the carry: only for a
	 * window whose boundaries and sizes are the index's own (no guessed boundary, no retry hints) and of ordinary size */
	st->ahead_ok = 0;
	/* (not before the window ramp has reached its target: a second pinned slab costs about half a millisecond per MiB, and one
	 * that has to grow three times costs a short stream more than the copies it hides) */
	if (!st->no_ahead && st->w.batch_bytes >= st->w.target_bytes && !st->idx.speculative && st->hint.skip == 0 && st->hint.cap == 0 && st->idx.max_out != 0 &&
	    st->idx.max_out <= ((uint64_t)1 << 30) && st->carry_len >= st->last_ret) {
		const size_t rem = st->carry_len - st->last_ret;
		if (la_buf_pinned(st->w.gpu, &st->slab2, rem + (size_t)st->idx.max_out + 16, 0) == 0 &&
		    la_gpu_memcpy_d2h(st->w.gpu, st->slab2.p + rem, st->d_dst.p, (size_t)st->idx.max_out) == LA_OK) {
			st->ahead_ok = 1;
			st->ahead_rem = rem;
			st->ahead_len = (size_t)st->idx.max_out;
		}
	}
	la_window_ramp(&st->w);
	if (st->trace)
		fprintf(stderr, "la_gzip: window %zu bytes, %u members queued: gather %.1f ms, index + launch %.1f ms\n",
		    st->stage_len, st->idx.n, t1 - t0, gz_now() - t1);
	return 1;
}

static ssize_t gzip_filter_read(struct archive_read_filter *self, const void **p)
{
	struct gzip_private *st = (struct gzip_private *)self->data;
	*p = NULL;

	/* the bytes handed out last time are released now: close the gap */
	if (st->last_ret) {
		memmove(st->slab.p, st->slab.p + st->last_ret, st->carry_len - st->last_ret);
		st->carry_len -= st->last_ret;
		st->last_ret = 0;
	}
	for (;;) {
		if (st->verdict.rc)
			return la_verdict_report(self, &st->verdict);
		if (st->eof) {
			if (st->carry_len) {	/* the held-back tail of a clean stream */
				st->last_ret = st->carry_len;
				*p = st->slab.p;
				return (ssize_t)st->carry_len;
			}
			return 0;
		}
		if (st->inflight == GZ_NONE) {
			int pr = gz_prepare(self, st);
			if (pr < 0)
				return pr;
			if (pr == 0)
				continue;
		}
		/* the window in flight: results, stream-order walk, slab */
		struct gz_walk w;
		const double t2 = st->trace ? gz_now() : 0;
		const int members = st->inflight == GZ_MEMBERS;
		int rc = gz_finish(self, st, &w);
		const size_t used = w.used;
		const int made_progress = used > 0;
		gz_free_tables(st);
		st->inflight = GZ_NONE;
		if (members && made_progress)
			st->pm_declined = 0;	/* (the member that left piece mode is behind us, or will be found declined again) */
		if (st->trace)
			fprintf(stderr, "la_gzip:   finished in %.1f ms, used %zu of %zu, out %zu\n", gz_now() - t2, used, st->stage_len, st->last_ret);
		if (rc < 0)
			return rc;
		if (used < st->stage_len)
			memmove(st->stage.p, st->stage.p + used, st->stage_len - used);
		st->stage_len -= used;
		if (!made_progress && !st->verdict.rc && !st->eof && !w.again) {
			/* nothing could be finished in this window and nothing asked for the same bytes again: it has to grow */
			if (st->w.upstream_eof) { st->eof = 1; continue; }
			st->w.batch_bytes *= 2;
		}
		if (st->last_ret) {
			/* Decode ahead: gather, upload, index and launch the NEXT window before handing this
			 * slab out, so that the device works while the caller consumes it (the slab is not
			 * touched until the next read()).  An outcome other than "in flight" is simply met
			 * again by the next read(). */
			if (!st->verdict.rc && !st->eof) {
				int pr = gz_prepare(self, st);
				if (pr < 0)	/* reported by the next read(), after these bytes (the error is set) */
					la_verdict_set(&st->verdict, pr, NULL);
			}
			*p = st->slab.p;
			return (ssize_t)st->last_ret;
		}
	}
}

static int gzip_filter_close(struct archive_read_filter *self)
{
	struct gzip_private *st = (struct gzip_private *)self->data;
	if (st == NULL)
		return ARCHIVE_OK;
	la_gpu_ctx *gpu = st->w.gpu;
	la_gpu_sync(gpu);
	gz_free_tables(st);
	la_buf_release(gpu, &st->stage);
	la_buf_release(gpu, &st->slab);
	la_buf_release(gpu, &st->slab2);
	la_buf_release(gpu, &st->d_src);
	la_buf_release(gpu, &st->d_dst);
	la_buf_release(gpu, &st->d_tabs);
	la_buf_release(gpu, &st->h_res);
	la_buf_release(gpu, &st->hist);
	la_gpu_close(gpu);
	free(st->name);
	free(st);
	self->data = NULL;
	return ARCHIVE_OK;
}
