/*
 * la_filter_xz.c -- the xz read filter on the MI355X data plane.
 *
 * Mirrors libarchive/archive_read_support_filter_xz.c: the same bidder (xz.c:201-221: 6 magic bytes, 48 bits), filter
 * code and name (ARCHIVE_FILTER_XZ, "xz", xz.c:393-394), vtable shape (read / close, xz.c:462-466) and the strings of
 * set_error (xz.c:420-458).  Where the reference feeds lzma_code (a stream decoder opened with LZMA_CONCATENATED,
 * xz.c:512-515) whatever __archive_read_filter_ahead returns (xz.c:651-735), this filter gathers a window of the stream
 * and walks the container on the host: stream header, block headers, index, footer, stream padding, in liblzma's order
 * of checks (stream_decoder.c, block_header_decoder.c, index_hash.c, stream_flags_decoder.c of liblzma 5.2).  Blocks
 * whose header carries both sizes are hopped over without decoding; all of them in a window go to the device in ONE
 * la_gpu_xz_decode call, output offsets from a prefix sum.  A block without a compressed size is a serial unit of
 * unknown extent: it is decoded alone, its end is learnt from the result, then the walk goes on.  What the window did
 * not finish opens the next window at that unit's first byte.  No CPU fallback.
 *
 * The index is checked as liblzma checks it, by a running comparison (count, sums of padded sizes, uncompressed sizes
 * and record lengths, and a hash chain over the pairs), not against a stored list.
 *
 * Departures from liblzma.  (1) By default only a single LZMA2 filter is decoded: a block that lists delta or a BCJ
 * filter (IDs 0x03 .. 0x0B) ends the read with "xz GPU data plane: unsupported filter <name> in a block's filter chain";
 * liblzma decodes such chains.  With LA_XZ_CHAINS=1 in the environment (read once in xz_reader_init; off by default
 * because two tests pin the refusal -- making it the default is a follow-up that touches them) up to three of delta,
 * x86, PowerPC, IA-64, ARM, ARM-Thumb and SPARC in front of LZMA2 are judged as liblzma judges them and undone on the
 * device (csrc/la_xz_filters.hip, the chain table behind the block table, LA_XZ_BATCH_CHAINS); ARM64 (0x0A) and RISC-V
 * (0x0B) stay refused by name either way.  With a BCJ filter in the chain, liblzma holds back the tail bytes its coder
 * cannot decide yet (a branch may reach over them: up to 4 for x86, less than a unit otherwise), so at an error inside
 * a block its T lies up to that much below the LZMA2 level's.  This filter takes the most that could be held off its
 * own T (xz_chain_hold): where the error falls within those few bytes behind a multiple of 64 KiB, the bytes handed out
 * are still a prefix of the plain data, with the reference's code and message, but may be one 64 KiB block fewer than
 * the reference's; everywhere else they are the reference's.
 * (2) A block has to fit a window: more than LA_GPU_MAX_BATCH_MIB (2048) compressed MiB, or more
 * than min(LA_GPU_OUT_BUDGET_MIB, 4095) decoded MiB (default 4095), is refused by name.  (3) Verdicts inside a block
 * are the device's (csrc/la_xz_dev.h), where liblzma's reading is pinned: dictionary sizes rounded up to 4096 and to a
 * multiple of 16, a non-zero first byte of a chunk's range-coder data refused.
 *
 * Bytes in front of an error.  The reference hands out its 64 KiB block when lzma_code has filled it (avail_out == 0,
 * xz.c:669) and, at the end of the stream, the partial block; on an error it returns ARCHIVE_FATAL and the partial block
 * is lost (xz.c:702-705).  lzma_code goes on reading input when the output block is full -- behind a block's last byte
 * it takes the end marker, padding, check, the next header, the index -- but it does not decode another LZMA symbol.
 * With T the bytes liblzma has emitted when it reports:
 *   - an error of the container or at a chunk boundary (every status but LA_ST_XZ_LZMA) arrives in the call that
 *     emitted byte T, so that byte's block is not handed out (LA_HB_EARLY);
 *   - an error inside an LZMA chunk (LA_ST_XZ_LZMA), and LZMA_BUF_ERROR for input that ends inside a stream (the
 *     reference calls lzma_code twice more without input: "No progress is possible", not "truncated input"), arrive
 *     in a call of their own, after a full block has been returned (LA_HB_LATE);
 *   - a clean end (LZMA_STREAM_END at the end of input, the stream padding a multiple of four) hands out all T (LA_HB_ALL).
 * What each kind lets out, and the holding back until the next window says which it is, is la_holdback's (la_host.h,
 * la_bid_policy.c).  (tests/xz_support.py restates the reference's loop over the real liblzma; the rule above is what
 * that emulator gives.  For T a multiple of 64 KiB the first case assumes that upstream hands the reference the damaged
 * bytes together with byte T's block, as a memory reader does.)
 */
#include "la_read_private.h"
#include "la_host.h"
#include "../csrc/la_xz_dev.h"	/* la_xz_check_size: the rules header is plain C too */
#include "../csrc/la_xz_filters_dev.h"	/* la_xz_filter_valid */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define XZ_TAB_CAP    4096u		/* blocks one launch takes; a window with more is taken in parts */
#define XZ_VLI_MAX    (~(uint64_t)0 >> 1)

/* liblzma's return codes, as far as set_error (xz.c:420-458) words them */
enum { XZ_E_FORMAT, XZ_E_OPTIONS, XZ_E_DATA, XZ_E_BUF };
static const char *const xz_msg[] = {
	"Lzma library error: format not recognized", "Lzma library error: Invalid options",
	"Lzma library error: Corrupted input data", "Lzma library error:  No progress is possible",
};

enum { SEQ_HEADER, SEQ_BLOCK, SEQ_INDEX, SEQ_FOOTER, SEQ_PADDING };

/* one side of the index comparison (index_hash.c: lzma_index_hash_info) */
typedef struct xz_sums {
	uint64_t count, blocks_size, uncomp, list_size, hash;
} xz_sums;

struct xz_private {
	la_reader r;			/* stage: from the first byte of the next unit on; d_tabs: block table, results */
	la_xz_block *tab;		/* host copies of the tables, in r.h_tabs (XZ_TAB_CAP entries; room for the chains of a launch behind its blocks) */
	la_xz_chain *chains;		/* tab[i]'s delta / BCJ filters (LA_XZ_CHAINS=1; otherwise all empty) */
	la_xz_result *res;
	int chains_on;			/* LA_XZ_CHAINS=1: delta and BCJ filters in front of LZMA2 are run, not refused */
	/* where the container stands at stage[0] */
	int seq, first_stream;
	uint32_t check_id;		/* of the stream header: the footer's has to be the same */
	unsigned pad_mod;		/* stream padding bytes so far, mod 4 */
	xz_sums blocks, records;
	uint64_t solo_cap;		/* output budget of the next size-less block (grows on LA_ST_XZ_OUT_FULL) */
};

static int xz_reader_bid(struct archive_read_filter_bidder *, struct archive_read_filter *);
static int xz_reader_init(struct archive_read_filter *);
static ssize_t xz_filter_read(struct archive_read_filter *, const void **);
static int xz_filter_close(struct archive_read_filter *);

static const struct archive_read_filter_bidder_vtable xz_bidder_vtable = {
	.bid = xz_reader_bid,
	.init = xz_reader_init,
};
static const struct archive_read_filter_vtable xz_reader_vtable = {
	.read = xz_filter_read,
	.close = xz_filter_close,
};

int archive_read_support_filter_xz(struct archive *_a)
{
	struct archive_read *a = (struct archive_read *)_a;
	if (__archive_read_register_bidder(a, NULL, "xz", &xz_bidder_vtable) != ARCHIVE_OK)
		return ARCHIVE_FATAL;
	return ARCHIVE_OK;
}

/* xz.c:201-221 */
static int xz_reader_bid(struct archive_read_filter_bidder *self, struct archive_read_filter *filter)
{
	ssize_t avail;
	(void)self;
	const unsigned char *p = __archive_read_filter_ahead(filter, 6, &avail);
	if (p == NULL)
		return 0;
	if (memcmp(p, "\xFD\x37\x7A\x58\x5A\x00", 6) != 0)
		return 0;
	/* Default policy (la_bid_policy.c): a block without a compressed size is one serial chain of unknown extent; a
	 * stream that opens with one and does not end inside the look-ahead is left to liblzma on a host core. */
	if (la_bid_declines(filter, la_bid_xz_parallel))
		return 0;
	return 48;
}

static int xz_reader_init(struct archive_read_filter *self)
{
	self->code = ARCHIVE_FILTER_XZ;
	self->name = "xz";
	struct xz_private *st = calloc(1, sizeof(*st));
	/* (a block's dst_cap is at most LA_XZ_DST_CAP_MAX: 4095 MiB) */
	if (la_reader_open(self, st ? &st->r : NULL, "xz", (sizeof(la_xz_block) + 2 * sizeof(la_xz_chain) + sizeof(la_xz_result)) * XZ_TAB_CAP,
	    (uint64_t)4095 << 20, "Can't allocate data for xz decompression") != ARCHIVE_OK) {	/* xz.c:482-483 */
		free(st);
		return ARCHIVE_FATAL;
	}
	st->tab = (la_xz_block *)st->r.h_tabs.p;
	st->chains = (la_xz_chain *)((uint8_t *)st->tab + (sizeof(la_xz_block) + sizeof(la_xz_chain)) * XZ_TAB_CAP);	/* (zeroed) */
	st->res = (la_xz_result *)(st->chains + XZ_TAB_CAP);
	const char *v = getenv("LA_XZ_CHAINS");	/* read once, here */
	st->chains_on = v != NULL && v[0] == '1';
	st->seq = SEQ_HEADER;
	st->first_stream = 1;
	self->data = st;
	self->vtable = &xz_reader_vtable;
	return ARCHIVE_OK;
}

/* the stream ends here, T being hb.total: an error reported in the call that emitted byte T ... */
static void xz_end_early(struct xz_private *st, int e)
{
	la_holdback_end(&st->r.hb, ARCHIVE_FATAL, xz_msg[e], LA_HB_EARLY);
}
/* ... or in a call of its own */
static void xz_end_late(struct xz_private *st, int e)
{
	la_holdback_end(&st->r.hb, ARCHIVE_FATAL, xz_msg[e], LA_HB_LATE);
}

/* vli.c, single-call mode: 0 and *pos advanced, or -1 (LZMA_DATA_ERROR: no byte left, a zero byte that is not the first,
 * a tenth byte).  -2: the bytes end inside the number (multi-call mode asks for more there; single-call mode is -1 too). */
static int xz_vli(const uint8_t *p, size_t n, size_t *pos, uint64_t *v)
{
	uint64_t r = 0;
	for (unsigned k = 0; k < 9; k++) {
		if (*pos >= n)
			return -2;
		const uint8_t b = p[(*pos)++];
		r |= (uint64_t)(b & 0x7F) << (7 * k);
		if (!(b & 0x80)) {
			if (b == 0 && k > 0)
				return -1;
			*v = r;
			return 0;
		}
	}
	return -1;
}
static unsigned xz_vli_size(uint64_t v)
{
	unsigned k = 1;
	while (v >>= 7)
		k++;
	return k;
}
static uint64_t ceil4(uint64_t v) { return (v + 3) & ~(uint64_t)3; }

static void sums_append(xz_sums *s, uint64_t unpadded, uint64_t uncomp)
{
	s->count++;
	s->blocks_size += ceil4(unpadded);
	s->uncomp += uncomp;
	s->list_size += xz_vli_size(unpadded) + xz_vli_size(uncomp);
	const uint64_t v[2] = { unpadded, uncomp };
	for (unsigned i = 0; i < 16; i++)	/* FNV-1a over the pair, chained */
		s->hash = (s->hash ^ ((v[i >> 3] >> (8 * (i & 7))) & 0xFF)) * 1099511628211ull;
}

static const char *xz_filter_name(uint64_t id)
{
	static const char *const names[] = { "delta", "x86 BCJ", "PowerPC BCJ", "IA-64 BCJ", "ARM BCJ", "ARM-Thumb BCJ", "SPARC BCJ",
		"ARM64 BCJ", "RISC-V BCJ" };	/* (0x0A and 0x0B: xz 5.4 and 5.6; a liblzma from before them answers LZMA_OPTIONS_ERROR) */
	return id >= 3 && id <= 0x0B ? names[id - 3] : NULL;
}

typedef struct xz_block_header {
	uint64_t comp, uncomp;	/* LA_XZ_UNKNOWN when absent */
	uint32_t dict_size;
	const char *unsupported;	/* a filter this data plane does not run */
	la_xz_chain chain;		/* the filters in front of LZMA2 (chains_on) */
} xz_block_header;

/* block_header_decoder.c over the whole header h[0, size), then what lzma_raw_decoder_init says about the chain:
 * -1 or an XZ_E_*.  With chains_on, delta and the BCJ filters 0x04 .. 0x09 are taken into bh->chain, their properties
 * judged as liblzma's decoders judge them (delta_decoder.c, simple_decoder.c: sizes in lzma_properties_decode, the
 * offset's alignment and the chain's shape in the init, all LZMA_OPTIONS_ERROR); ARM64 and RISC-V stay unsupported. */
static int xz_block_header_parse(const uint8_t *h, size_t size, uint32_t check_id, int chains_on, xz_block_header *bh)
{
	const size_t n = size - 4;
	if ((uint32_t)la_crc32(0, h, n) != archive_le32dec(h + n))
		return XZ_E_DATA;
	if (h[1] & 0x3C)
		return XZ_E_OPTIONS;
	size_t pos = 2;
	bh->comp = bh->uncomp = LA_XZ_UNKNOWN;
	bh->unsupported = NULL;
	bh->dict_size = 0;
	memset(&bh->chain, 0, sizeof(bh->chain));
	if (h[1] & 0x40) {
		if (xz_vli(h, n, &pos, &bh->comp) != 0)
			return XZ_E_DATA;
		/* lzma_block_unpadded_size: no compressed size of 0, no unpadded size above LZMA_VLI_MAX & ~3 */
		if (bh->comp == 0 || bh->comp > (XZ_VLI_MAX & ~(uint64_t)3) - size - la_xz_check_size(check_id))
			return XZ_E_DATA;
	}
	if ((h[1] & 0x80) && xz_vli(h, n, &pos, &bh->uncomp) != 0)
		return XZ_E_DATA;
	const unsigned nf = (h[1] & 3u) + 1u;
	int lzma2_last = 0, others = 0, bad_offset = 0;
	for (unsigned f = 0; f < nf; f++) {
		uint64_t id, psize;
		if (xz_vli(h, n, &pos, &id) != 0 || id >= ((uint64_t)1 << 62))
			return XZ_E_DATA;
		if (xz_vli(h, n, &pos, &psize) != 0 || n - pos < psize)
			return XZ_E_DATA;
		if (id == 0x21) {
			if (psize != 1 || (h[pos] & 0xC0) || h[pos] > 40)
				return XZ_E_OPTIONS;
			bh->dict_size = h[pos] == 40 ? 0xFFFFFFFFu : (2u | (h[pos] & 1u)) << (h[pos] / 2 + 11);
			lzma2_last = f == nf - 1;
			others += f != nf - 1;
		} else if (chains_on && id >= LA_XZF_DELTA && id <= LA_XZF_SPARC) {
			uint32_t prop;
			if (id == LA_XZF_DELTA) {
				if (psize != 1)
					return XZ_E_OPTIONS;
				prop = (uint32_t)h[pos] + 1u;
			} else {
				if (psize != 0 && psize != 4)
					return XZ_E_OPTIONS;
				prop = psize ? archive_le32dec(h + pos) : 0u;
			}
			bad_offset |= !la_xz_filter_valid((uint32_t)id, prop);
			if (f < LA_XZ_CHAIN_MAX) {	/* (a fourth one stands in LZMA2's place: refused below) */
				bh->chain.id[f] = (uint32_t)id;
				bh->chain.prop[f] = prop;
				bh->chain.count = f + 1u;
			}
		} else if (xz_filter_name(id)) {
			if (bh->unsupported == NULL)
				bh->unsupported = xz_filter_name(id);
		} else {
			return XZ_E_OPTIONS;	/* lzma_properties_decode: no such filter */
		}
		pos += (size_t)psize;
	}
	while (pos < n)
		if (h[pos++] != 0)
			return XZ_E_OPTIONS;
	if (bh->unsupported)
		return -1;
	if (!lzma2_last || others || bad_offset)
		return XZ_E_OPTIONS;	/* lzma_raw_decoder_init: the chain has to end in LZMA2 and hold it once; a BCJ offset has to be aligned */
	return -1;
}

/* index_hash.c over what is there of the index, p[0] the indicator.  Returns the index's size when it is complete and
 * sound (the records side is then committed), 0 when the bytes end first, -1 for LZMA_DATA_ERROR. */
static int64_t xz_index_parse(struct xz_private *st, const uint8_t *p, size_t n)
{
	xz_sums rec;
	memset(&rec, 0, sizeof(rec));
	size_t pos = 1;
	uint64_t count;
	int r = xz_vli(p, n, &pos, &count);
	if (r != 0)
		return r == -2 ? 0 : -1;
	if (count != st->blocks.count)
		return -1;
	for (uint64_t i = 0; i < count; i++) {
		uint64_t unpadded, uncomp;
		if ((r = xz_vli(p, n, &pos, &unpadded)) != 0)
			return r == -2 ? 0 : -1;
		if (unpadded < 5 || unpadded > (XZ_VLI_MAX & ~(uint64_t)3))
			return -1;
		if ((r = xz_vli(p, n, &pos, &uncomp)) != 0)
			return r == -2 ? 0 : -1;
		sums_append(&rec, unpadded, uncomp);
		if (st->blocks.blocks_size < rec.blocks_size || st->blocks.uncomp < rec.uncomp || st->blocks.list_size < rec.list_size)
			return -1;
	}
	while (pos & 3) {
		if (pos >= n)
			return 0;
		if (p[pos++] != 0)
			return -1;
	}
	if (pos >= n)
		return 0;	/* (index_hash.c compares when the first byte behind the padding is there) */
	if (st->blocks.blocks_size != rec.blocks_size || st->blocks.uncomp != rec.uncomp || st->blocks.list_size != rec.list_size ||
	    st->blocks.hash != rec.hash)
		return -1;
	const uint32_t crc = (uint32_t)la_crc32(0, p, pos);
	for (unsigned k = 0; k < 4; k++) {
		if (pos >= n)
			return 0;
		if (p[pos++] != ((crc >> (8 * k)) & 0xFF))
			return -1;
	}
	st->records = rec;
	return (int64_t)pos;
}

/* Decode tab[0, n) in one call and append the bytes to the window's output; the results are in st->res. */
static int xz_launch(struct archive_read_filter *self, struct xz_private *st, uint32_t n, uint64_t dst_bytes)
{
	la_reader *r = &st->r;
	la_gpu_ctx *gpu = r->w.gpu;
	const size_t o_res = (sizeof(la_xz_block) + sizeof(la_xz_chain)) * XZ_TAB_CAP;
	size_t tab_bytes = sizeof(la_xz_block) * n;
	int chained = 0;
	for (uint32_t i = 0; i < n; i++)
		chained |= st->chains[i].count != 0;
	if (la_buf_dev(gpu, &r->d_tabs, o_res + sizeof(la_xz_result) * XZ_TAB_CAP) < 0 || la_buf_dev(gpu, &r->d_dst, (size_t)dst_bytes + 64) < 0)
		return la_window_fail(self, &r->w, "la_gpu_malloc");
	la_xz_batch bt;
	memset(&bt, 0, sizeof(bt));
	bt.d_src = r->d_src.p; bt.src_bytes = r->stage_len;
	bt.d_blocks = (const la_xz_block *)r->d_tabs.p; bt.n = n;
	bt.d_dst = r->d_dst.p; bt.dst_cap = dst_bytes;
	bt.d_results = (la_xz_result *)(r->d_tabs.p + o_res);
	if (chained) {	/* the chain table rides behind the blocks, and only then */
		memcpy(st->tab + n, st->chains, sizeof(la_xz_chain) * n);
		tab_bytes += sizeof(la_xz_chain) * n;
		bt.reserved = LA_XZ_BATCH_CHAINS;
	}
	if (la_gpu_memcpy_h2d(gpu, r->d_tabs.p, st->tab, tab_bytes) != LA_OK) return la_window_fail(self, &r->w, "la_gpu_memcpy_h2d");
	if (la_gpu_xz_decode(gpu, &bt) != LA_OK) return la_window_fail(self, &r->w, "la_gpu_xz_decode");
	if (la_gpu_memcpy_d2h(gpu, st->res, bt.d_results, sizeof(la_xz_result) * n) != LA_OK || la_gpu_sync(gpu) != LA_OK)
		return la_window_fail(self, &r->w, "la_gpu_memcpy_d2h");
	return ARCHIVE_OK;
}

/* The verdict on a failed block: T counts its valid bytes. */
static void xz_block_failed(struct xz_private *st, uint32_t status)
{
	if (status == LA_ST_XZ_LZMA)
		xz_end_late(st, XZ_E_DATA);
	else
		xz_end_early(st, XZ_E_DATA);
}

/* the most bytes at the end of unfinished data that the chain's BCJ filters leave undecided: less than a unit each,
 * 4 for x86 (liblzma's simple coder holds them back until more data or the end of the LZMA2 data arrives) */
static uint64_t xz_chain_hold(const la_xz_chain *ch)
{
	uint64_t hold = 0;
	for (uint32_t k = 0; k < ch->count; k++)
		hold += ch->id[k] == LA_XZF_X86 ? 4u : la_xz_unit_bytes(ch->id[k]) ? la_xz_unit_bytes(ch->id[k]) - 1u : 0u;
	return hold;
}

/* Walk the results of tab[0, n) in stream order; the bytes of the blocks in front of the first failure, and the valid
 * bytes of that one, come back from the device. */
static int xz_take_results(struct archive_read_filter *self, struct xz_private *st, uint32_t n)
{
	uint64_t bytes = 0;
	uint32_t bad = n;
	for (uint32_t i = 0; i < n && bad == n; i++) {
		if (st->res[i].status != LA_ST_OK)
			bad = i;
		bytes = st->tab[i].dst_off + st->res[i].out_len;	/* (the table is packed: no gaps in front of a failure) */
	}
	if (bad < n && st->res[bad].status != LA_ST_XZ_BAD_CHECK && st->res[bad].status != LA_ST_XZ_PADDING) {
		/* the data ends inside the block: a BCJ filter could not decide the last bytes (a branch may reach over the end),
		 * and liblzma's coder keeps such bytes back; they do not count */
		const uint64_t hold = xz_chain_hold(&st->chains[bad]);
		bytes -= hold < st->res[bad].out_len ? hold : st->res[bad].out_len;
	}
	const int rc = la_reader_take(self, &st->r, bytes);
	if (rc == ARCHIVE_OK && bad < n)
		xz_block_failed(st, st->res[bad].status);
	return rc;
}

/* One window: gather, upload, walk; updates T, and says how the stream ends if this window shows it.
 * ARCHIVE_OK, or a fatal code with the error set. */
static int xz_window(struct archive_read_filter *self)
{
	struct xz_private *st = (struct xz_private *)self->data;
	const la_window *w = &st->r.w;
	int r = la_reader_gather(self, &st->r);
	if (r != ARCHIVE_OK)
		return r;
	const uint8_t *src = st->r.stage.p;
	const size_t len = st->r.stage_len;
	const int eof = w->upstream_eof;
	size_t pos = 0;		/* the first byte of the unit the walk stands at */
	int more = 0;		/* that unit needs bytes the window does not hold */
	uint32_t n = 0;		/* sized blocks collected for one launch */
	uint64_t dst_bytes = 0;
	while (!st->r.hb.ended && !more) {
		/* the block header at pos, when the walk stands at one and all of it is here: parsed once per turn */
		xz_block_header bh;
		size_t hsize = 0;
		int hdr = -2;	/* -2: no whole block header at pos; -1: a sound one; otherwise its XZ_E_* */
		const uint32_t cs = la_xz_check_size(st->check_id);
		memset(&bh, 0, sizeof(bh));
		if (st->seq == SEQ_BLOCK && len - pos >= 1 && src[pos] != 0 && len - pos >= (hsize = ((size_t)src[pos] + 1) * 4))
			hdr = xz_block_header_parse(src + pos, hsize, st->check_id, st->chains_on, &bh);
		const int sound = hdr == -1 && !bh.unsupported;
		const int too_large = sound && ((bh.comp != LA_XZ_UNKNOWN && bh.comp > w->max_batch_bytes) ||
		    (bh.uncomp != LA_XZ_UNKNOWN && bh.uncomp > w->out_budget));
		/* both sizes in the header and the whole block in the window: hopped over, decoded with its neighbours */
		const int whole = sound && !too_large && bh.comp != LA_XZ_UNKNOWN && bh.uncomp != LA_XZ_UNKNOWN &&
		    len - pos - hsize >= ceil4(bh.comp) + cs;
		if (whole && n < XZ_TAB_CAP && !(n && dst_bytes + bh.uncomp > w->out_budget)) {
			st->chains[n] = bh.chain;
			la_xz_block *b = &st->tab[n++];
			b->src_off = pos + hsize; b->comp_size = bh.comp; b->uncomp_size = bh.uncomp;
			b->dst_off = dst_bytes; b->dst_cap = bh.uncomp;
			b->check_off = pos + hsize + ceil4(bh.comp);
			b->dict_size = bh.dict_size; b->check_id = st->check_id;
			dst_bytes += bh.uncomp;
			sums_append(&st->blocks, hsize + bh.comp + cs, bh.uncomp);
			pos += hsize + (size_t)ceil4(bh.comp) + cs;
			continue;
		}
		if (n) {	/* anything else ends the run of sized blocks: their bytes count in front of what follows */
			if ((r = xz_launch(self, st, n, dst_bytes)) != ARCHIVE_OK || (r = xz_take_results(self, st, n)) != ARCHIVE_OK)
				return r;
			n = 0;
			dst_bytes = 0;
			continue;	/* (the unit at pos is looked at again, now with nothing collected) */
		}
		switch (st->seq) {
		case SEQ_HEADER: {
			if (len - pos < 12) {
				if (eof) xz_end_late(st, XZ_E_BUF); else more = 1;
				break;
			}
			const uint8_t *h = src + pos;
			if (memcmp(h, "\xFD\x37\x7A\x58\x5A\x00", 6) != 0)	/* stream_decoder.c: FORMAT_ERROR behind the first stream is DATA_ERROR */
				xz_end_early(st, st->first_stream ? XZ_E_FORMAT : XZ_E_DATA);
			else if ((uint32_t)la_crc32(0, h + 6, 2) != archive_le32dec(h + 8))
				xz_end_early(st, XZ_E_DATA);
			else if (h[6] != 0 || (h[7] & 0xF0))
				xz_end_early(st, XZ_E_OPTIONS);
			else {
				st->check_id = h[7] & 0x0F;
				memset(&st->blocks, 0, sizeof(st->blocks));
				memset(&st->records, 0, sizeof(st->records));
				st->seq = SEQ_BLOCK;
				pos += 12;
			}
			break;
		}
		case SEQ_BLOCK: {
			if (len - pos >= 1 && src[pos] == 0) {
				st->seq = SEQ_INDEX;
				break;
			}
			if (hdr == -2) {	/* not one byte, or not the whole header */
				if (eof) xz_end_late(st, XZ_E_BUF); else more = 1;
				break;
			}
			if (hdr >= 0) {
				xz_end_early(st, hdr);
				break;
			}
			if (bh.unsupported) {
				archive_set_error(&self->archive->archive, ARCHIVE_ERRNO_MISC,
				    "xz GPU data plane: unsupported filter %s in a block's filter chain (only LZMA2 is decoded)", bh.unsupported);
				return ARCHIVE_FATAL;
			}
			if (too_large) {
				archive_set_error(&self->archive->archive, ARCHIVE_ERRNO_MISC,
				    "xz block too large for the GPU data plane (more than %llu compressed or %llu decoded bytes; LA_GPU_MAX_BATCH_MIB, LA_GPU_OUT_BUDGET_MIB)",
				    (unsigned long long)w->max_batch_bytes, (unsigned long long)w->out_budget);
				return ARCHIVE_FATAL;
			}
			/* a size is missing, or the block is not all here: alone, bounded by the window's end and by a budget that grows
			 * when it proves too small */
			const uint64_t have = len - pos - hsize;
			if (!eof && bh.comp != LA_XZ_UNKNOWN && have < ceil4(bh.comp) + cs) {
				more = 1;	/* the header says how much is missing */
				break;
			}
			const uint64_t cap = bh.uncomp != LA_XZ_UNKNOWN ? bh.uncomp : la_reader_solo_cap(&st->r, &st->solo_cap, have);
			st->chains[0] = bh.chain;
			la_xz_block *b = &st->tab[0];
			b->src_off = pos + hsize; b->comp_size = bh.comp; b->uncomp_size = bh.uncomp;
			b->dst_off = 0; b->dst_cap = cap; b->check_off = LA_XZ_UNKNOWN;
			b->dict_size = bh.dict_size; b->check_id = st->check_id;
			if ((r = xz_launch(self, st, 1, cap)) != ARCHIVE_OK)
				return r;
			const la_xz_result q = st->res[0];
			if (q.status == LA_ST_XZ_OUT_FULL) {
				if ((r = la_reader_solo_full(self, &st->r, &st->solo_cap, cap, "block")) != ARCHIVE_OK)
					return r;
				break;	/* again, with twice the room */
			}
			if (q.status == LA_ST_XZ_TRUNCATED && !eof) {
				more = 1;
				break;
			}
			st->solo_cap = 0;
			if ((r = xz_take_results(self, st, 1)) != ARCHIVE_OK)
				return r;
			if (q.status == LA_ST_XZ_TRUNCATED) {
				xz_end_late(st, XZ_E_BUF);	/* (replaces xz_take_results' data error: the input ends inside the block) */
			} else if (q.status == LA_ST_OK) {
				sums_append(&st->blocks, hsize + q.consumed + cs, q.out_len);
				pos += hsize + (size_t)ceil4(q.consumed) + cs;
			}
			break;
		}
		case SEQ_INDEX: {
			const int64_t k = xz_index_parse(st, src + pos, len - pos);
			if (k < 0)
				xz_end_early(st, XZ_E_DATA);
			else if (k == 0) {
				if (eof) xz_end_late(st, XZ_E_BUF); else more = 1;
			} else {
				pos += (size_t)k;
				st->seq = SEQ_FOOTER;
			}
			break;
		}
		case SEQ_FOOTER: {
			if (len - pos < 12) {
				if (eof) xz_end_late(st, XZ_E_BUF); else more = 1;
				break;
			}
			const uint8_t *f = src + pos;
			const uint64_t index_size = ceil4(1 + xz_vli_size(st->records.count) + st->records.list_size) + 4;
			if (f[10] != 'Y' || f[11] != 'Z')	/* (FORMAT_ERROR, which the stream decoder turns into DATA_ERROR) */
				xz_end_early(st, XZ_E_DATA);
			else if ((uint32_t)la_crc32(0, f + 4, 6) != archive_le32dec(f))
				xz_end_early(st, XZ_E_DATA);
			else if (f[8] != 0 || (f[9] & 0xF0))
				xz_end_early(st, XZ_E_OPTIONS);
			else if (((uint64_t)archive_le32dec(f + 4) + 1) * 4 != index_size || (f[9] & 0x0F) != st->check_id)
				xz_end_early(st, XZ_E_DATA);
			else {
				pos += 12;
				st->seq = SEQ_PADDING;
				st->pad_mod = 0;
				st->first_stream = 0;
			}
			break;
		}
		default: {	/* SEQ_PADDING */
			while (pos < len && src[pos] == 0) {
				pos++;
				st->pad_mod = (st->pad_mod + 1) & 3;
			}
			if (pos < len) {
				if (st->pad_mod)
					xz_end_early(st, XZ_E_DATA);
				else
					st->seq = SEQ_HEADER;
			} else if (eof) {
				if (st->pad_mod)
					xz_end_early(st, XZ_E_DATA);
				else
					la_holdback_end(&st->r.hb, ARCHIVE_OK, NULL, LA_HB_ALL);
			} else {
				more = 1;
			}
			break;
		}
		}
	}
	return la_reader_finish(self, &st->r, pos, more, "block");
}

static ssize_t xz_filter_read(struct archive_read_filter *self, const void **p)
{
	return la_reader_read(self, &((struct xz_private *)self->data)->r, p, xz_window);
}

static int xz_filter_close(struct archive_read_filter *self)
{
	struct xz_private *st = (struct xz_private *)self->data;
	if (st == NULL)
		return ARCHIVE_OK;
	la_reader_close(&st->r);
	free(st);
	self->data = NULL;
	return ARCHIVE_OK;
}
