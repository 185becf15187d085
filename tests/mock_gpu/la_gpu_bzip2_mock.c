/*
 * la_gpu_bzip2_mock.c -- TEST INFRASTRUCTURE: a CPU stand-in for la_gpu_bzip2_scan / la_gpu_bzip2_decode as
 * include/la_gpu.h words them, over the image's real libbz2, so that the host side (la_filter_bzip2.c: windows, carry,
 * budget, held-back bytes, verdicts) is tested without a GPU.  Linked beside la_gpu_mock.c.
 *
 * The walk is the ABI's (confirm candidates in stream order from state_in).  A block the walk reaches is decoded by
 * libbz2: its bits are re-aligned behind a "BZh<level>" header and fed to BZ2_bzDecompress one byte at a time.  libbz2
 * takes input bytes only when it needs bits, decodes a block completely before it emits a byte and emits the whole
 * block in one call when there is room, so the first call that produces output has just taken the byte that holds the
 * last bit of the end-of-block symbol: the block ends in that byte, and out_len is what that call produced.  The CRCs
 * are this file's own (MSB-first 0x04C11DB7).  libbz2 is on the image, bzlib.h is not: the prototypes are local.
 */
#include "../../include/la_gpu.h"
#include <stdlib.h>
#include <string.h>

typedef struct {
	char *next_in; unsigned int avail_in, total_in_lo32, total_in_hi32;
	char *next_out; unsigned int avail_out, total_out_lo32, total_out_hi32;
	void *state; void *(*bzalloc)(void *, int, int); void (*bzfree)(void *, void *); void *opaque;
} bz_stream;
int BZ2_bzDecompressInit(bz_stream *, int, int);
int BZ2_bzDecompress(bz_stream *);
int BZ2_bzDecompressEnd(bz_stream *);
#define BZ_OK 0

#define MAGIC_BLOCK 0x314159265359ull
#define MAGIC_END   0x177245385090ull
#define OUT_MAX     ((size_t)47 << 20)	/* 900 000 bytes of run-length data expand to about 46 MB */

static unsigned bit_at(const uint8_t *p, uint64_t nbits, uint64_t bit)
{
	return bit < nbits ? (p[bit >> 3] >> (7 - (bit & 7))) & 1u : 0u;
}
static uint64_t bits_at(const uint8_t *p, uint64_t nbits, uint64_t bit, unsigned n)
{
	uint64_t v = 0;
	for (unsigned i = 0; i < n; i++)
		v = v << 1 | bit_at(p, nbits, bit + i);
	return v;
}

static uint32_t crc_tab[256];
static uint32_t bz_crc(const uint8_t *p, size_t n)
{
	if (!crc_tab[1])
		for (uint32_t i = 0; i < 256; i++) {
			uint32_t c = i << 24;
			for (int k = 0; k < 8; k++)
				c = (c << 1) ^ ((c >> 31) ? 0x04C11DB7u : 0u);
			crc_tab[i] = c;
		}
	uint32_t c = 0xFFFFFFFFu;
	for (size_t i = 0; i < n; i++)
		c = (c << 8) ^ crc_tab[(c >> 24) ^ p[i]];
	return ~c;
}

uint32_t la_gpu_bzip2_max_blocks(uint32_t slot_level) { return slot_level >= 1 && slot_level <= 9 ? 4096u : 0u; }
uint64_t la_gpu_bzip2_workspace_bytes(uint32_t n, uint32_t slot_level) { (void)n; (void)slot_level; return 0; }

int la_gpu_bzip2_scan(la_gpu_ctx *c, const uint8_t *src, uint64_t src_bytes, la_bz2_cand *cands, uint32_t cap, uint32_t *count)
{
	(void)c;
	const uint64_t nbits = src_bytes * 8;
	uint64_t w = 0, found = 0;
	for (uint64_t bit = 0; bit < nbits; bit++) {
		w = (w << 1 | bit_at(src, nbits, bit)) & 0xFFFFFFFFFFFFull;
		if (bit < 47 || (w != MAGIC_BLOCK && w != MAGIC_END))
			continue;
		if (found < cap) {
			cands[found].bit_off = bit - 47;
			cands[found].kind = w == MAGIC_BLOCK ? LA_BZ2_KIND_BLOCK : LA_BZ2_KIND_END;
			cands[found].reserved = 0;
		}
		found++;
	}
	*count = found > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)found;
	return LA_OK;
}

/* what MEASURE keeps for EMIT (one window at a time, as the ABI asks) */
static struct {
	uint8_t **bytes;	/* [n] decoded blocks */
	uint8_t *after;		/* [n] libbz2 failed the block behind its bytes: a wrong CRC, or the missing count */
	uint32_t n;
	la_bz2_state walk, in;
} M;

static void m_free(void)
{
	for (uint32_t i = 0; i < M.n; i++)
		free(M.bytes[i]);
	free(M.bytes);
	free(M.after);
	M.bytes = NULL;
	M.after = NULL;
	M.n = 0;
}

/* how many leading bits at `bit` agree with one of the two magics (of those the source still holds, at most 48) */
static unsigned magic_prefix(const uint8_t *p, uint64_t nbits, uint64_t bit)
{
	unsigned a = 0, b = 0;
	while (a < 48 && bit + a < nbits && bit_at(p, nbits, bit + a) == ((MAGIC_BLOCK >> (47 - a)) & 1u)) a++;
	while (b < 48 && bit + b < nbits && bit_at(p, nbits, bit + b) == ((MAGIC_END >> (47 - b)) & 1u)) b++;
	return a > b ? a : b;
}

/* Feeds in[0, n) to a fresh libbz2 stream one byte at a time until it produces output, fails or the bytes run out, then
 * lets it emit the block ONE BYTE per call until a call emits nothing (libbz2 wants the next header) or fails.  One
 * byte per call, because libbz2 does not count the bytes of a call that ends in BZ_DATA_ERROR (a wrong CRC is found
 * behind the block's last byte; a block that ends on four equal bytes without their count is found out only behind the
 * run libbz2 makes up for it): this way every byte written is a byte counted.  *after = the error came behind output. */
static size_t feed_bytes(uint8_t *in, size_t n, uint8_t *buf, size_t *fed, int *ret, int *after)
{
	bz_stream s;
	memset(&s, 0, sizeof(s));
	*fed = 0;
	*after = 0;
	*ret = BZ2_bzDecompressInit(&s, 0, 0);
	if (*ret != BZ_OK)
		return 0;
	size_t got = 0;
	while (*fed < n && *ret == BZ_OK && got == 0) {
		s.next_in = (char *)in + *fed; s.avail_in = 1;
		s.next_out = (char *)buf; s.avail_out = 1;
		*ret = BZ2_bzDecompress(&s);
		(*fed)++;
		got = 1 - s.avail_out;
	}
	while (got && *ret == BZ_OK && got < OUT_MAX) {
		s.avail_in = 0;
		s.next_out = (char *)buf + got; s.avail_out = 1;
		*ret = BZ2_bzDecompress(&s);
		if (s.avail_out)
			break;
		got++;
	}
	if (got && *ret != BZ_OK)
		*after = 1;
	BZ2_bzDecompressEnd(&s);
	return got;
}

/* one block through libbz2; fills status, out_len, end_bit, stored_crc of r, *out = malloc'ed bytes */
static void decode_block(const uint8_t *src, uint64_t src_bytes, uint64_t bit_off, uint32_t level, la_bz2_result *r, uint8_t **out, int *after)
{
	const uint64_t nbits = src_bytes * 8;
	*out = NULL;
	r->end_bit = bit_off;
	if (bit_off + 48 + 32 + 1 > nbits) { r->status = LA_ST_BZ2_TRUNCATED; return; }
	r->stored_crc = (uint32_t)bits_at(src, nbits, bit_off + 48, 32);
	if (bit_at(src, nbits, bit_off + 80)) { r->status = LA_ST_BZ2_RANDOMISED; return; }
	const size_t body = (size_t)((nbits - bit_off + 7) / 8);
	uint8_t *in = malloc(4 + body), *buf = malloc(OUT_MAX);
	if (!in || !buf) { free(in); free(buf); r->status = LA_ST_BZ2_DATA; return; }
	memcpy(in, "BZh", 3);
	in[3] = (uint8_t)('0' + level);
	for (size_t i = 0; i < body; i++)
		in[4 + i] = (uint8_t)bits_at(src, nbits, bit_off + 8 * (uint64_t)i, 8);
	/* A source that ends inside a byte of the re-aligned stream leaves up to 7 bits in a last, partial byte.  It is fed
	 * padded with zeros; a block that ends in that byte counts only if it ends the same way padded with ones (a prefix
	 * code cannot give the same symbol for both values of a bit it reads, so then it read none of the padding). */
	const unsigned tail_bits = (unsigned)((nbits - bit_off) % 8);
	size_t fed = 0;
	int ret = BZ_OK;
	size_t got = feed_bytes(in, 4 + body, buf, &fed, &ret, after);
	if (got && tail_bits && fed == 4 + body) {
		size_t fed1 = 0;
		int ret1 = BZ_OK, after1 = 0;
		in[4 + body - 1] |= (uint8_t)(0xFFu >> tail_bits);
		uint8_t *buf1 = malloc(OUT_MAX);
		const size_t got1 = buf1 ? feed_bytes(in, 4 + body, buf1, &fed1, &ret1, &after1) : 0;
		free(buf1);
		if (got1 != got) { got = 0; ret = BZ_OK; *after = 0; }
	}
	if (got == 0 || (ret != BZ_OK && !*after)) {
		r->status = ret != BZ_OK ? LA_ST_BZ2_DATA : LA_ST_BZ2_TRUNCATED;
		free(in); free(buf);
		return;
	}
	{
		const size_t produced = got;
		/* the end-of-block symbol's last bit lies in byte `fed - 1` of the re-aligned stream, whose bit 32 is bit_off */
		const uint64_t lo = bit_off + 8 * (uint64_t)(fed - 1) - 32 + 1, hi = bit_off + 8 * (uint64_t)fed - 32;
		uint64_t best = hi < nbits ? hi : nbits;
		unsigned best_m = 0;
		for (uint64_t x = lo; x <= hi && x <= nbits; x++) {
			const unsigned m = magic_prefix(src, nbits, x);
			if (m > best_m || (m == best_m && x == nbits)) { best_m = m; best = x; }
		}
		r->status = LA_ST_OK;
		r->out_len = produced;
		r->end_bit = best;
		*out = realloc(buf, produced ? produced : 1);
		free(in);
	}
}

static int walk(const la_bz2_batch *bt)
{
	const uint8_t *src = bt->d_src;
	const uint64_t src_bytes = bt->src_bytes;
	const la_bz2_cand *cands = bt->d_cands;
	const uint32_t n = bt->n;
	la_bz2_result *results = bt->d_results;
	m_free();
	M.bytes = calloc(n ? n : 1, sizeof(uint8_t *));
	M.after = calloc(n ? n : 1, 1);
	if (!M.bytes || !M.after) return LA_ERR_NOMEM;
	M.n = n;
	for (uint32_t i = 0; i < n; i++) {
		memset(&results[i], 0, sizeof(results[i]));
		results[i].status = LA_ST_BZ2_REFUTED;
	}
	la_bz2_state st = *bt->state_in;
	uint32_t open = st.open, level = st.level, i = 0;
	uint64_t pos = st.start_bit, total = 0;
	st.stop = LA_BZ2_STOP_TABLE; st.stop_entry = 0xFFFFFFFFu; st.first_bad = 0xFFFFFFFFu; st.reserved = 0;
	for (;;) {
		if (!open) {
			pos = (pos + 7) & ~7ull;
			const uint64_t by = pos >> 3;
			if (by + 14 > src_bytes) { st.stop = LA_BZ2_STOP_SHORT; break; }
			const uint8_t *h = src + by;
			while (i < n && cands[i].bit_off < pos + 32) i++;
			if (memcmp(h, "BZh", 3) != 0 || h[3] < '1' || h[3] > '9' || i >= n || cands[i].bit_off != pos + 32) { st.stop = LA_BZ2_STOP_BID; break; }
			if ((uint32_t)(h[3] - '0') > bt->slot_level) { st.stop = LA_BZ2_STOP_LEVEL; break; }
			open = 1; level = (uint32_t)(h[3] - '0'); st.crc = 0;
			pos += 32;
		}
		while (i < n && cands[i].bit_off < pos) i++;
		if (i >= n || cands[i].bit_off != pos) { st.stop = LA_BZ2_STOP_TABLE; break; }
		la_bz2_result r;
		memset(&r, 0, sizeof(r));
		r.level = level; r.dst_off = total;
		if (cands[i].kind == LA_BZ2_KIND_BLOCK) {
			int after = 0;
			decode_block(src, src_bytes, pos, level, &r, &M.bytes[i], &after);
			M.after[i] = (uint8_t)after;
			if (r.status != LA_ST_OK) {
				r.out_len = 0;
				results[i] = r;
				st.stop = LA_BZ2_STOP_ENTRY; st.stop_entry = i;
				break;
			}
			total += r.out_len;
		} else {
			if (pos + 80 > src_bytes * 8) {
				r.status = LA_ST_BZ2_TRUNCATED; r.end_bit = pos;
				results[i] = r;
				st.stop = LA_BZ2_STOP_ENTRY; st.stop_entry = i;
				break;
			}
			r.stored_crc = (uint32_t)bits_at(src, src_bytes * 8, pos + 48, 32);
			r.end_bit = (pos + 80 + 7) & ~7ull;
			open = 0;
		}
		results[i] = r;
		pos = r.end_bit;
		i++;
	}
	st.open = open; st.level = level; st.start_bit = pos; st.total_out = total; st.n_taken = i;
	M.walk = st;
	M.in = *bt->state_in;
	*bt->d_state_out = st;
	return LA_OK;
}

static int emit(const la_bz2_batch *bt)
{
	if (bt->n != M.n) return LA_ERR_ARG;
	la_bz2_result *results = bt->d_results;
	const la_bz2_state w = M.walk;
	la_bz2_state st = M.in;
	st.stop = LA_BZ2_STOP_TABLE; st.stop_entry = 0xFFFFFFFFu; st.first_bad = 0xFFFFFFFFu; st.total_out = 0; st.reserved = 0;
	const uint32_t ne = bt->n_emit < bt->n ? bt->n_emit : bt->n, lim = ne < w.n_taken ? ne : w.n_taken;
	uint32_t i = 0;
	for (; i < lim; i++) {
		la_bz2_result r = results[i];
		if (r.status == LA_ST_BZ2_REFUTED)
			continue;
		if (!st.open) { st.open = 1; st.level = r.level; st.crc = 0; }
		if (bt->d_cands[i].kind == LA_BZ2_KIND_BLOCK) {
			if (r.dst_off > bt->dst_cap || r.out_len > bt->dst_cap - r.dst_off)
				break;
			memcpy(bt->d_dst + r.dst_off, M.bytes[i], (size_t)r.out_len);
			const uint32_t crc = bz_crc(M.bytes[i], (size_t)r.out_len);
			results[i].crc = crc;
			st.total_out += r.out_len;
			st.start_bit = r.end_bit;
			if (M.after[i] || crc != r.stored_crc) {
				/* (a missing count whose bytes also miss the CRC is reported as the wrong CRC here) */
				results[i].status = crc != r.stored_crc ? LA_ST_BZ2_BAD_CRC : LA_ST_BZ2_DATA;
				st.first_bad = i++;
				break;
			}
			st.crc = ((st.crc << 1) | (st.crc >> 31)) ^ crc;
		} else {
			results[i].crc = st.crc;
			st.start_bit = r.end_bit;
			if (st.crc != r.stored_crc) {
				results[i].status = LA_ST_BZ2_BAD_CRC;
				st.first_bad = i++;
				break;
			}
			st.open = 0; st.crc = 0;
		}
	}
	st.n_taken = i;
	if (st.first_bad == 0xFFFFFFFFu && i == w.n_taken) {
		st.stop = w.stop; st.stop_entry = w.stop_entry; st.start_bit = w.start_bit; st.open = w.open; st.level = w.level;
	}
	*bt->d_state_out = st;
	return LA_OK;
}

int la_gpu_bzip2_decode(la_gpu_ctx *c, const la_bz2_batch *bt)
{
	(void)c;
	if (!bt || !bt->state_in || !bt->d_state_out || bt->slot_level < 1 || bt->slot_level > 9 || bt->n > 4096)
		return LA_ERR_ARG;
	return bt->phase == LA_BZ2_MEASURE ? walk(bt) : bt->phase == LA_BZ2_EMIT ? emit(bt) : LA_ERR_ARG;
}

/* for a program that wants to end with nothing allocated (the sanitizer build) */
void la_gpu_bzip2_mock_release(void) { m_free(); }
