/*
 * la_xz_enc_dev.h -- the xz ENCODER's rules, stated ONCE: the chunk kernel and the pack kernels (la_xz_comp.hip), the CPU
 * stand-in of the tests (tests/mock_xz_write) and its sanitizer program all compile this file, as la_xz_dev.h is compiled
 * by everything that decodes.  It is the common subset of C and C++.  The including file defines, before it:
 *   LA_XZ_FN                  the function qualifiers (static inline on the host, __host__ __device__ in the kernel)
 *   LA_XZC_LANE_LOOP(l)       optional: the loop head of a step's 64 lanes.  The default walks them one after the other; the
 *                             kernel runs the body once, l = its lane
 *   LA_XZC_SYNC()             optional: what separates "all lanes have read" from "any lane writes" (nothing for the loop)
 *   LA_XZC_TAB_MAX(p, v)      optional: *p = max(*p, v) on the match table.  Positions only grow, so the maximum is what the
 *                             last lane of a loop would have left; the kernel uses an LDS atomic and gets the same table
 *   LA_XZC_PUT(p, v)          optional: one byte store of the serial part (the kernel stores from one lane)
 *   LA_XZC_EVENT(kind)        optional: a test's counter hook, LA_XZC_EV_* below
 * With the defaults the stand-in therefore writes the device's bytes, not just an equivalent stream.
 *
 * The stream shape.  Blocks of LA_XZC_BLOCK_BYTES of input, each with a 16-byte header that carries both
 * sizes (zero padding up to the declared size keeps the header's length fixed), one LZMA2 filter, dictionary 1 MiB.  The
 * body is chunks of LA_XZC_CHUNK_BYTES of input, the end marker, zero padding to four bytes, CRC64.
 *
 * One chunk (la_xzc_chunk: la_xzc_chain_init, la_xzc_chain_steps, then LZMA2's own tail), three phases per step of 64
 * positions:
 *   MATCH    every lane hashes the four bytes at its position, reads the table's candidate, then (behind LA_XZC_SYNC)
 *            enters its own position and extends the candidate.  Matches end at or before the chunk's end.  Levels 0..3
 *            start from an empty table; levels 4..9 first enter the up to 64 KiB of the same block in front of the chunk,
 *            so distances reach back across the chunk border but never in front of the block (the dictionary reset).
 *   SYMBOLS  the positions of the step in order, greedily: a match is taken when it is longer than five bytes, or five
 *            below distance 16 384, or four below distance 512 (shorter ones further away are dearer than their literals), as rep0..rep3 when its distance is one of them, split into pieces of at most 273 (the later pieces are
 *            rep0; no piece of one byte is left over).  In front of a literal rep0 is tried: two bytes and more are a rep0
 *            match, one byte is a short rep.  A literal behind a match is coded in the matched form (state >= 7).
 *   CODE     the range coder, lc 3, lp 0, pb 2, model reset per chunk.  pos_state and the literal's previous byte come
 *            from the position inside the BLOCK.  64-bit low, cache, cache_size, carry propagation, five flush bytes; the
 *            chunk's first byte is the initial cache, 0.  Bytes are counted beyond the slot's end but not stored there.
 * Every chunk resets state and properties (control 0xE0 for the block's first chunk, 0xC0 otherwise), so a chunk is valid
 * behind any neighbour and is coded without knowing it.  A chunk whose payload is not smaller than its input is stored
 * (0x01 for the block's first chunk, 0x02 otherwise): a chunk takes at most its input + 5 bytes.
 */
#ifndef LA_XZ_ENC_DEV_H
#define LA_XZ_ENC_DEV_H

#include "la_xz_dev.h"

#define LA_XZC_PROBS      (LA_XZ_P_LITERAL + (768u << 3))	/* lc 3, lp 0: 7990 entries */
#define LA_XZC_PROPS      93u					/* (pb 2 * 5 + lp 0) * 9 + lc 3 */
#define LA_XZC_HASH_BITS  12u
#define LA_XZC_TAB        (1u << LA_XZC_HASH_BITS)
#define LA_XZC_BLOCK_HDR  16u
#define LA_XZC_DICT_PROP  16u					/* 1 MiB, the smallest dictionary that covers a block */
#define LA_XZC_SLOT_BYTES (LA_XZC_CHUNK_BYTES + 16u)		/* a coded chunk: 6 header bytes, at most input - 1 of payload */
#define LA_XZC_WARM_LEVEL 4u
#define LA_XZC_LEN4_DIST  (1u << 9)				/* a match of four bytes is taken below this distance, */
#define LA_XZC_LEN5_DIST  (1u << 14)				/* one of five below this one, longer ones anywhere */

enum {
	LA_XZC_EV_CARRY_LONG, LA_XZC_EV_STORED, LA_XZC_EV_REP0, LA_XZC_EV_REP1, LA_XZC_EV_REP2, LA_XZC_EV_REP3, LA_XZC_EV_SHORT_REP,
	LA_XZC_EV_LEN_LOW, LA_XZC_EV_LEN_MID, LA_XZC_EV_LEN_HIGH, LA_XZC_EV_SPLIT, LA_XZC_EV_DIST_SLOT, LA_XZC_EV_DIST_SPECIAL,
	LA_XZC_EV_DIST_ALIGN, LA_XZC_EV_MATCHED_LITERAL, LA_XZC_EV_ACROSS_CHUNKS, LA_XZC_EV_COUNT
};

#ifndef LA_XZC_LANE_LOOP
#define LA_XZC_LANE_LOOP(l) for (uint32_t l = 0; l < 64u; l++)
#endif
#ifndef LA_XZC_SYNC
#define LA_XZC_SYNC() do { } while (0)
#endif
#ifndef LA_XZC_TAB_MAX
#define LA_XZC_TAB_MAX(p, v) do { if (*(p) < (v)) *(p) = (v); } while (0)
#endif
#ifndef LA_XZC_PUT
#define LA_XZC_PUT(p, v) (*(p) = (v))
#endif
#ifndef LA_XZC_EVENT
#define LA_XZC_EVENT(kind) do { } while (0)
#endif

/* ---- framing ---- */

LA_XZ_FN uint32_t la_xzc_crc32(const uint8_t *p, uint32_t n)
{
	uint32_t c = 0xFFFFFFFFu;
	for (uint32_t i = 0; i < n; i++) {
		c ^= p[i];
		for (int k = 0; k < 8; k++)
			c = (c & 1u) ? (c >> 1) ^ 0xEDB88320u : c >> 1;
	}
	return ~c;
}

/* the 12 bytes in front of the first block: magic, flags (check CRC64), their CRC32 */
LA_XZ_FN void la_xzc_stream_header(uint8_t *h)
{
	const uint8_t magic[8] = { 0xFD, '7', 'z', 'X', 'Z', 0x00, 0x00, 0x04 };
	for (uint32_t i = 0; i < 8u; i++)
		h[i] = magic[i];
	const uint32_t c = la_xzc_crc32(h + 6, 2);
	for (uint32_t i = 0; i < 4u; i++)
		h[8u + i] = (uint8_t)(c >> (8u * i));
}

/* h[LA_XZC_BLOCK_HDR]: size byte, flags (both sizes, one filter), the sizes, LZMA2 with its dictionary byte, zero padding, CRC32 */
LA_XZ_FN void la_xzc_block_header(uint8_t *h, uint64_t comp, uint64_t uncomp)
{
	uint32_t n = 0;
	h[n++] = (uint8_t)(LA_XZC_BLOCK_HDR / 4u - 1u);
	h[n++] = 0xC0;
	for (int k = 0; k < 2; k++) {
		uint64_t v = k ? uncomp : comp;
		while (v >= 0x80u) {
			h[n++] = (uint8_t)(v | 0x80u);
			v >>= 7;
		}
		h[n++] = (uint8_t)v;
	}
	h[n++] = 0x21;
	h[n++] = 1;
	h[n++] = (uint8_t)LA_XZC_DICT_PROP;
	while (n < LA_XZC_BLOCK_HDR - 4u)
		h[n++] = 0;
	const uint32_t c = la_xzc_crc32(h, n);
	for (uint32_t i = 0; i < 4u; i++)
		h[n + i] = (uint8_t)(c >> (8u * i));
}

/* bytes of a chunk of n input bytes in the block body; payload = 0: stored */
LA_XZ_FN uint32_t la_xzc_chunk_bytes(uint32_t n, uint32_t payload)
{
	return payload ? 6u + payload : 3u + n;
}

/* a block of `comp` body bytes (chunks and end marker) in the stream: header, body, padding, CRC64 */
LA_XZ_FN uint64_t la_xzc_block_bytes(uint64_t comp)
{
	return LA_XZC_BLOCK_HDR + ((comp + 3u) & ~(uint64_t)3u) + 8u;
}

/* the most a block of n input bytes takes: every chunk at its input + 5 */
LA_XZ_FN uint64_t la_xzc_block_bound(uint64_t n)
{
	const uint64_t chunks = (n + LA_XZC_CHUNK_BYTES - 1u) / LA_XZC_CHUNK_BYTES;
	return la_xzc_block_bytes(n + 5u * chunks + 1u);
}

LA_XZ_FN uint64_t la_xzc_bound(uint64_t src_bytes)
{
	const uint64_t full = src_bytes / LA_XZC_BLOCK_BYTES, rest = src_bytes % LA_XZC_BLOCK_BYTES;
	return 12u + full * la_xzc_block_bound(LA_XZC_BLOCK_BYTES) + (rest ? la_xzc_block_bound(rest) : 0u);
}

/* the three bytes in front of a stored chunk of n bytes */
LA_XZ_FN void la_xzc_stored_header(uint8_t *h, uint32_t n, int first_of_block)
{
	h[0] = first_of_block ? 0x01 : 0x02;
	h[1] = (uint8_t)((n - 1u) >> 8);
	h[2] = (uint8_t)(n - 1u);
}

/* ---- the range coder ---- */

typedef struct la_xzc_rc {
	uint64_t low;
	uint32_t range, cache, cache_size;
	uint32_t pos, lim;	/* bytes produced (counted beyond lim, stored below it only) */
	uint8_t *out;
} la_xzc_rc;

LA_XZ_FN void la_xzc_rc_byte(la_xzc_rc *rc, uint32_t b)
{
	if (rc->pos < rc->lim)
		LA_XZC_PUT(rc->out + rc->pos, (uint8_t)b);
	rc->pos++;
}

LA_XZ_FN void la_xzc_rc_shift(la_xzc_rc *rc)
{
	if ((uint32_t)rc->low < 0xFF000000u || (uint32_t)(rc->low >> 32) != 0u) {
		const uint32_t carry = (uint32_t)(rc->low >> 32);
		if (carry && rc->cache_size >= 2u)
			LA_XZC_EVENT(LA_XZC_EV_CARRY_LONG);
		la_xzc_rc_byte(rc, rc->cache + carry);
		/* the 0xFF bytes held back behind it; cache_size - 1 of them, at most the chunk's bytes so far */
		for (uint32_t k = 1; k < rc->cache_size; k++)
			la_xzc_rc_byte(rc, 0xFFu + carry);
		rc->cache_size = 0;
		rc->cache = (uint32_t)(rc->low >> 24) & 0xFFu;
	}
	rc->cache_size++;
	rc->low = (rc->low & 0x00FFFFFFu) << 8;
}

LA_XZ_FN void la_xzc_bit(la_xzc_rc *rc, uint16_t *probs, uint32_t idx, uint32_t bit)
{
	const uint32_t pr = probs[idx];
	const uint32_t bound = (rc->range >> 11) * pr;
	if (bit == 0) {
		rc->range = bound;
		probs[idx] = (uint16_t)(pr + ((2048u - pr) >> 5));
	} else {
		rc->low += bound;
		rc->range -= bound;
		probs[idx] = (uint16_t)(pr - (pr >> 5));
	}
	if (rc->range < (1u << 24)) {
		rc->range <<= 8;
		la_xzc_rc_shift(rc);
	}
}

/* nb bits of v, most significant first, down the tree at base */
LA_XZ_FN void la_xzc_tree(la_xzc_rc *rc, uint16_t *probs, uint32_t base, uint32_t nb, uint32_t v)
{
	uint32_t m = 1;
	for (uint32_t i = nb; i-- > 0u;) {
		const uint32_t b = (v >> i) & 1u;
		la_xzc_bit(rc, probs, base + m, b);
		m = (m << 1) | b;
	}
}

/* nb bits of v, least significant first */
LA_XZ_FN void la_xzc_tree_reverse(la_xzc_rc *rc, uint16_t *probs, uint32_t base, uint32_t nb, uint32_t v)
{
	uint32_t m = 1;
	for (uint32_t i = 0; i < nb; i++) {
		const uint32_t b = (v >> i) & 1u;
		la_xzc_bit(rc, probs, base + m, b);
		m = (m << 1) | b;
	}
}

/* ---- the symbol coder: state, reps and the model indices, as la_xz_lzma_chunk reads them ---- */

typedef struct la_xzc_enc {
	la_xzc_rc rc;
	uint32_t state, rep0, rep1, rep2, rep3;
} la_xzc_enc;

LA_XZ_FN void la_xzc_literal(la_xzc_enc *e, uint16_t *probs, const uint8_t *blk, uint32_t pos)
{
	const uint32_t cur = blk[pos], prev = pos ? blk[pos - 1u] : 0u;
	const uint32_t lit = LA_XZ_P_LITERAL + 768u * (prev >> 5);	/* lc 3, lp 0 */
	la_xzc_bit(&e->rc, probs, LA_XZ_P_IS_MATCH + e->state * 16u + (pos & 3u), 0);
	if (e->state < 7u) {
		la_xzc_tree(&e->rc, probs, lit, 8, cur);
	} else {
		uint32_t mb = (uint32_t)blk[pos - e->rep0 - 1u] << 1, offset = 0x100u, sym = 1;
		LA_XZC_EVENT(LA_XZC_EV_MATCHED_LITERAL);
		for (uint32_t i = 8; i-- > 0u;) {
			const uint32_t bit = (cur >> i) & 1u, match_bit = mb & offset;
			la_xzc_bit(&e->rc, probs, lit + offset + match_bit + sym, bit);
			sym = (sym << 1) | bit;
			if (bit) offset &= match_bit; else offset &= ~match_bit;
			mb <<= 1;
		}
	}
	e->state = e->state < 4u ? 0u : e->state < 10u ? e->state - 3u : e->state - 6u;
}

LA_XZ_FN void la_xzc_len(la_xzc_enc *e, uint16_t *probs, uint32_t lenp, uint32_t len, uint32_t pos_state)
{
	const uint32_t l = len - 2u;
	if (l < 8u) {
		LA_XZC_EVENT(LA_XZC_EV_LEN_LOW);
		la_xzc_bit(&e->rc, probs, lenp, 0);
		la_xzc_tree(&e->rc, probs, lenp + LA_XZ_LEN_LOW + pos_state * 8u, 3, l);
	} else if (l < 16u) {
		LA_XZC_EVENT(LA_XZC_EV_LEN_MID);
		la_xzc_bit(&e->rc, probs, lenp, 1);
		la_xzc_bit(&e->rc, probs, lenp + 1u, 0);
		la_xzc_tree(&e->rc, probs, lenp + LA_XZ_LEN_MID + pos_state * 8u, 3, l - 8u);
	} else {
		LA_XZC_EVENT(LA_XZC_EV_LEN_HIGH);
		la_xzc_bit(&e->rc, probs, lenp, 1);
		la_xzc_bit(&e->rc, probs, lenp + 1u, 1);
		la_xzc_tree(&e->rc, probs, lenp + LA_XZ_LEN_HIGH, 8, l - 16u);
	}
}

/* a match with a new distance; dist = distance - 1, len 2 .. 273 */
LA_XZ_FN void la_xzc_match(la_xzc_enc *e, uint16_t *probs, uint32_t pos, uint32_t len, uint32_t dist)
{
	const uint32_t pos_state = pos & 3u;
	la_xzc_bit(&e->rc, probs, LA_XZ_P_IS_MATCH + e->state * 16u + pos_state, 1);
	la_xzc_bit(&e->rc, probs, LA_XZ_P_IS_REP + e->state, 0);
	la_xzc_len(e, probs, LA_XZ_P_LEN, len, pos_state);
	uint32_t slot = dist;
	if (dist >= 4u) {
		const uint32_t n = 31u - (uint32_t)__builtin_clz(dist);
		slot = 2u * n + ((dist >> (n - 1u)) & 1u);
	}
	la_xzc_tree(&e->rc, probs, LA_XZ_P_DIST_SLOT + (len < 6u ? len - 2u : 3u) * 64u, 6, slot);
	if (slot < 4u) {
		LA_XZC_EVENT(LA_XZC_EV_DIST_SLOT);
	} else {
		const uint32_t nb = (slot >> 1) - 1u, base = (2u | (slot & 1u)) << nb, rest = dist - base;
		if (slot < 14u) {
			LA_XZC_EVENT(LA_XZC_EV_DIST_SPECIAL);
			la_xzc_tree_reverse(&e->rc, probs, LA_XZ_P_DIST_SPECIAL + base - slot - 1u, nb, rest);
		} else {
			LA_XZC_EVENT(LA_XZC_EV_DIST_ALIGN);
			for (uint32_t i = nb; i-- > 4u;) {	/* direct bits, most significant first */
				e->rc.range >>= 1;
				if ((rest >> i) & 1u)
					e->rc.low += e->rc.range;
				if (e->rc.range < (1u << 24)) {
					e->rc.range <<= 8;
					la_xzc_rc_shift(&e->rc);
				}
			}
			la_xzc_tree_reverse(&e->rc, probs, LA_XZ_P_DIST_ALIGN, 4, rest & 15u);
		}
	}
	e->rep3 = e->rep2; e->rep2 = e->rep1; e->rep1 = e->rep0; e->rep0 = dist;
	e->state = e->state < 7u ? 7u : 10u;
}

/* a match at rep `r` (0 .. 3), len 2 .. 273 */
LA_XZ_FN void la_xzc_rep(la_xzc_enc *e, uint16_t *probs, uint32_t pos, uint32_t len, uint32_t r)
{
	const uint32_t pos_state = pos & 3u;
	LA_XZC_EVENT(LA_XZC_EV_REP0 + (int)r);
	la_xzc_bit(&e->rc, probs, LA_XZ_P_IS_MATCH + e->state * 16u + pos_state, 1);
	la_xzc_bit(&e->rc, probs, LA_XZ_P_IS_REP + e->state, 1);
	if (r == 0u) {
		la_xzc_bit(&e->rc, probs, LA_XZ_P_IS_REP0 + e->state, 0);
		la_xzc_bit(&e->rc, probs, LA_XZ_P_IS_REP0_LONG + e->state * 16u + pos_state, 1);
	} else {
		uint32_t d;
		la_xzc_bit(&e->rc, probs, LA_XZ_P_IS_REP0 + e->state, 1);
		if (r == 1u) {
			la_xzc_bit(&e->rc, probs, LA_XZ_P_IS_REP1 + e->state, 0);
			d = e->rep1;
		} else {
			la_xzc_bit(&e->rc, probs, LA_XZ_P_IS_REP1 + e->state, 1);
			la_xzc_bit(&e->rc, probs, LA_XZ_P_IS_REP2 + e->state, r - 2u);
			if (r == 2u) {
				d = e->rep2;
			} else {
				d = e->rep3;
				e->rep3 = e->rep2;
			}
			e->rep2 = e->rep1;
		}
		e->rep1 = e->rep0;
		e->rep0 = d;
	}
	la_xzc_len(e, probs, LA_XZ_P_REP_LEN, len, pos_state);
	e->state = e->state < 7u ? 8u : 11u;
}

LA_XZ_FN void la_xzc_short_rep(la_xzc_enc *e, uint16_t *probs, uint32_t pos)
{
	const uint32_t pos_state = pos & 3u;
	LA_XZC_EVENT(LA_XZC_EV_SHORT_REP);
	la_xzc_bit(&e->rc, probs, LA_XZ_P_IS_MATCH + e->state * 16u + pos_state, 1);
	la_xzc_bit(&e->rc, probs, LA_XZ_P_IS_REP + e->state, 1);
	la_xzc_bit(&e->rc, probs, LA_XZ_P_IS_REP0 + e->state, 0);
	la_xzc_bit(&e->rc, probs, LA_XZ_P_IS_REP0_LONG + e->state * 16u + pos_state, 0);
	e->state = e->state < 7u ? 9u : 11u;
}

/* a match of len >= 2 at distance dist + 1: a rep when the distance is one, in pieces of at most 273, none of one byte */
LA_XZ_FN void la_xzc_match_any(la_xzc_enc *e, uint16_t *probs, uint32_t pos, uint32_t len, uint32_t dist)
{
	int first = 1;
	while (len) {
		uint32_t n = len > 273u ? 273u : len;
		if (len - n == 1u)
			n--;
		if (!first) {
			LA_XZC_EVENT(LA_XZC_EV_SPLIT);
			la_xzc_rep(e, probs, pos, n, 0);
		} else if (dist == e->rep0) {
			la_xzc_rep(e, probs, pos, n, 0);
		} else if (dist == e->rep1) {
			la_xzc_rep(e, probs, pos, n, 1);
		} else if (dist == e->rep2) {
			la_xzc_rep(e, probs, pos, n, 2);
		} else if (dist == e->rep3) {
			la_xzc_rep(e, probs, pos, n, 3);
		} else {
			la_xzc_match(e, probs, pos, n, dist);
		}
		first = 0;
		pos += n;
		len -= n;
	}
}

/* ---- the matcher ---- */

LA_XZ_FN uint32_t la_xzc_ld4(const uint8_t *p)
{
	return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}

LA_XZ_FN uint32_t la_xzc_hash(uint32_t v)
{
	return (v * 2654435761u) >> (32u - LA_XZC_HASH_BITS);
}

/* ---- one chain: la_xzc_chunk below and la_lzc_member (la_lzip_enc_dev.h) are callers of the same two pieces ---- */

/* The chain's start: a fresh range coder that stores into out[0, lim) and counts beyond, state and reps, the model and
 * the match table reset; then the table is warmed with blk[lo, cs), nothing emitted (lo == cs: no warm-up).  The table
 * holds position + 1, 0 for none. */
LA_XZ_FN void la_xzc_chain_init(la_xzc_enc *e, const uint8_t *blk, uint32_t lo, uint32_t cs, uint32_t ce, uint16_t *probs, uint32_t *tab,
    uint8_t *out, uint32_t lim)
{
	e->rc.low = 0; e->rc.range = 0xFFFFFFFFu; e->rc.cache = 0; e->rc.cache_size = 1;
	e->rc.pos = 0; e->rc.lim = lim; e->rc.out = out;
	e->state = 0; e->rep0 = e->rep1 = e->rep2 = e->rep3 = 0;
	LA_XZC_LANE_LOOP(l) {
		for (uint32_t i = l; i < LA_XZC_PROBS; i += 64u)
			probs[i] = 1024;
		for (uint32_t i = l; i < LA_XZC_TAB; i += 64u)
			tab[i] = 0;
	}
	LA_XZC_SYNC();
	LA_XZC_LANE_LOOP(l) {
		for (uint32_t p = lo + l; p < cs && p + 4u <= ce; p += 64u)
			LA_XZC_TAB_MAX(&tab[la_xzc_hash(la_xzc_ld4(blk + p))], p + 1u);
	}
}

/* The steps of 64 positions over blk[cs, ce): MATCH, SYMBOLS, CODE.  lo is the lowest position a distance may reach;
 * pos_state and the literal's previous byte come from the position behind blk.  The walk ends early once more than
 * `stop` bytes are out (a caller with a stored form gives up there; 0xFFFFFFFF: never). */
LA_XZ_FN void la_xzc_chain_steps(la_xzc_enc *e, const uint8_t *blk, uint32_t lo, uint32_t cs, uint32_t ce, uint32_t stop, uint16_t *probs,
    uint32_t *tab, uint32_t *m_len, uint32_t *m_cand)
{
	uint32_t base = cs, anchor = cs;
	while (base < ce && e->rc.pos <= stop) {
		/* MATCH: all reads of the table, then all writes */
		LA_XZC_SYNC();
		LA_XZC_LANE_LOOP(l) {
			const uint32_t p = base + l;
			m_cand[l] = p + 4u <= ce ? tab[la_xzc_hash(la_xzc_ld4(blk + p))] : 0u;
		}
		LA_XZC_SYNC();
		LA_XZC_LANE_LOOP(l) {
			const uint32_t p = base + l;
			uint32_t len = 0;
			if (p + 4u <= ce) {
				const uint32_t v = la_xzc_ld4(blk + p), c = m_cand[l];
				LA_XZC_TAB_MAX(&tab[la_xzc_hash(v)], p + 1u);
				if (c != 0u && la_xzc_ld4(blk + c - 1u) == v) {
					const uint8_t *q = blk + c - 1u;
					len = 4;
					while (p + len < ce && q[len] == blk[p + len])
						len++;
				}
			}
			m_len[l] = len;
		}
		LA_XZC_SYNC();
		/* SYMBOLS and CODE: the step's positions in order, the same values in every lane */
		const uint32_t end = base + 64u < ce ? base + 64u : ce;
		uint32_t p = anchor > base ? anchor : base;
		while (p < end && e->rc.pos <= stop) {
			const uint32_t f = p - base;
			uint32_t len = m_len[f];
			const uint32_t dist = len ? p - m_cand[f] : 0u;	/* distance - 1: the table holds position + 1 */
			if ((len == 4u && dist >= LA_XZC_LEN4_DIST) || (len == 5u && dist >= LA_XZC_LEN5_DIST))
				len = 0;	/* dearer than its literals */
			if (len) {
				if (m_cand[f] <= cs)
					LA_XZC_EVENT(LA_XZC_EV_ACROSS_CHUNKS);
				la_xzc_match_any(e, probs, p, len, dist);
				p += len;
			} else if (p - lo > e->rep0 && blk[p - e->rep0 - 1u] == blk[p]) {
				const uint8_t *q = blk + p - e->rep0 - 1u;
				uint32_t rl = 1;
				while (rl < 273u && p + rl < ce && q[rl] == blk[p + rl])
					rl++;
				if (rl >= 2u)
					la_xzc_rep(e, probs, p, rl, 0);
				else
					la_xzc_short_rep(e, probs, p);
				p += rl;
			} else {
				la_xzc_literal(e, probs, blk, p);
				p++;
			}
		}
		anchor = p;
		base = base + 64u > anchor ? base + 64u : anchor;
	}
}

/* One chunk: blk[cs, ce) of the block that starts at blk (ce - cs <= LA_XZC_CHUNK_BYTES, ce <= the block's bytes) into
 * slot[0, LA_XZC_SLOT_BYTES): the six header bytes and the payload.  probs holds LA_XZC_PROBS entries, tab LA_XZC_TAB,
 * m_len and m_cand 64 each (the kernel keeps all four in LDS).  Returns the payload's bytes, or 0: the chunk is stored
 * and the slot's content means nothing.  What is LZMA2's own is here: five flush bytes, the stored decision, the header. */
LA_XZ_FN uint32_t la_xzc_chunk(const uint8_t *blk, uint32_t cs, uint32_t ce, uint32_t level, uint16_t *probs, uint32_t *tab, uint32_t *m_len,
    uint32_t *m_cand, uint8_t *slot)
{
	const uint32_t n = ce - cs;
	/* the lowest position a distance may reach */
	const uint32_t lo = level < LA_XZC_WARM_LEVEL ? cs : cs > LA_XZC_CHUNK_BYTES ? cs - LA_XZC_CHUNK_BYTES : 0u;
	la_xzc_enc e;
	la_xzc_chain_init(&e, blk, lo, cs, ce, probs, tab, slot + 6, n - 1u);
	la_xzc_chain_steps(&e, blk, lo, cs, ce, e.rc.lim, probs, tab, m_len, m_cand);
	for (int i = 0; i < 5; i++)
		la_xzc_rc_shift(&e.rc);
	if (e.rc.pos > e.rc.lim) {
		LA_XZC_EVENT(LA_XZC_EV_STORED);
		return 0;
	}
	LA_XZC_PUT(slot + 0, (uint8_t)(cs == 0u ? 0xE0 : 0xC0));
	LA_XZC_PUT(slot + 1, (uint8_t)((n - 1u) >> 8));
	LA_XZC_PUT(slot + 2, (uint8_t)(n - 1u));
	LA_XZC_PUT(slot + 3, (uint8_t)((e.rc.pos - 1u) >> 8));
	LA_XZC_PUT(slot + 4, (uint8_t)(e.rc.pos - 1u));
	LA_XZC_PUT(slot + 5, (uint8_t)LA_XZC_PROPS);
	return e.rc.pos;
}

#endif
