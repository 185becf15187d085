/*
 * la_xz_dev.h -- what the .xz file format (version 1.0.4) and liblzma 5.2 say about an LZMA2 block, stated ONCE: the
 * kernel (la_xz.hip), the CPU stand-in of the tests (tests/mock_xz) and its sanitizer program all compile this file.
 * It is the common subset of C and C++; nothing in it is device-only.  The including file defines, before it:
 *   LA_XZ_FN                 the function qualifiers (static inline on the host, __host__ __device__ in the kernel)
 *   LA_XZ_COPY(d, s, n)      optional: copy n bytes of an uncompressed chunk, source to destination (never overlapping);
 *                            the kernel spreads it over the workgroup, the default is a byte loop
 *
 * The rules, in liblzma's order (lzma2_decoder.c, lzma_decoder.c; where the format text and liblzma differ, liblzma is
 * pinned, because the filter has to give liblzma's bytes and verdicts):
 *   control  0x00 ends the block.  0x01 and 0xE0 .. 0xFF reset the dictionary and ask for new properties; any other
 *            control while a dictionary reset is still owed (the block's first chunk) is LA_ST_XZ_DATA.  0x03 .. 0x7F
 *            are LA_ST_XZ_DATA.  An LZMA chunk below 0xC0 while properties are owed is LA_ST_XZ_DATA (owed at the
 *            block's start and again behind every 0x01 chunk).  0xA0 and above reset state, reps and the model.
 *   props    a byte above 224, or lc + lp > 4, is LA_ST_XZ_DATA.
 *   chunk    the range decoder reads 5 bytes (the first has to be 0, else LA_ST_XZ_DATA), normalises BEFORE every bit
 *            and once more behind the chunk's last symbol; then its code has to be 0 and its cursor on the chunk's last
 *            compressed byte, else LA_ST_XZ_DATA.  A match that runs over the chunk's uncompressed size is copied up to
 *            it and is LA_ST_XZ_DATA.  A normalisation that asks for a byte behind the chunk's compressed size is
 *            LA_ST_XZ_LZMA (liblzma notices it behind the call, not at the byte).
 *   distance a match, rep or short rep whose distance is not below min(bytes since the last dictionary reset,
 *            dictionary size as liblzma rounds it: at least 4096, up to a multiple of 16) is LA_ST_XZ_LZMA.  The
 *            end-of-payload marker (distance 0xFFFFFFFF) is such a distance: LZMA2 has no use for it.
 *   limits   the source ends at min(compressed size of the header, bytes there are); asking for more is
 *            LA_ST_XZ_SIZE for the first and LA_ST_XZ_TRUNCATED for the second.  The output ends at the header's
 *            uncompressed size (more: LA_ST_XZ_SIZE) or at the caller's budget (more: LA_ST_XZ_OUT_FULL).
 * A symbol is written only when all of it could be decoded, so on every failure out_len is the count of valid bytes:
 * exactly what liblzma has emitted when it runs out of input in the same place.
 *
 * Below the decoder: CRC64 (ECMA-182, reflected, table entry and combine arithmetic) and SHA-256, for the block checks.
 */
#ifndef LA_XZ_DEV_H
#define LA_XZ_DEV_H

#include "../../include/la_gpu.h"

#ifndef LA_XZ_FN
#define LA_XZ_FN static inline
#endif

/* the probability model: 1846 entries and the literal coders, 768 << (lc + lp), lc + lp <= 4 */
#define LA_XZ_P_IS_MATCH      0u	/* [12][16] */
#define LA_XZ_P_IS_REP        192u	/* [12] */
#define LA_XZ_P_IS_REP0       204u
#define LA_XZ_P_IS_REP1       216u
#define LA_XZ_P_IS_REP2       228u
#define LA_XZ_P_IS_REP0_LONG  240u	/* [12][16] */
#define LA_XZ_P_DIST_SLOT     432u	/* [4][64] */
#define LA_XZ_P_DIST_SPECIAL  688u	/* [114] */
#define LA_XZ_P_DIST_ALIGN    802u	/* [16] */
#define LA_XZ_P_LEN           818u	/* choice, choice2, low[16][8], mid[16][8], high[256] */
#define LA_XZ_P_REP_LEN       1332u
#define LA_XZ_P_LITERAL       1846u
#define LA_XZ_PROBS_MAX       (1846u + (768u << 4))
#define LA_XZ_LEN_LOW         2u
#define LA_XZ_LEN_MID         130u
#define LA_XZ_LEN_HIGH        258u

typedef struct la_xz_lzma {
	uint32_t state, rep0, rep1, rep2, rep3;
	uint32_t lc, lp, pb;
} la_xz_lzma;

LA_XZ_FN uint32_t la_xz_dict_cap(uint32_t dict_size)
{
	uint64_t d = dict_size < 4096u ? 4096u : dict_size;
	d = (d + 15u) & ~(uint64_t)15u;
	return d > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)d;
}

LA_XZ_FN void la_xz_lzma_reset(la_xz_lzma *s, uint16_t *probs)
{
	s->state = 0;
	s->rep0 = s->rep1 = s->rep2 = s->rep3 = 0;
	const uint32_t n = LA_XZ_P_LITERAL + (768u << (s->lc + s->lp));
	for (uint32_t i = 0; i < n; i++)
		probs[i] = 1024;
}

/* 0, or LA_ST_XZ_DATA */
LA_XZ_FN uint32_t la_xz_props(la_xz_lzma *s, uint32_t byte)
{
	if (byte > 224u)
		return LA_ST_XZ_DATA;
	const uint32_t pb = byte / 45u;
	byte -= pb * 45u;
	const uint32_t lp = byte / 9u, lc = byte - lp * 9u;
	if (lc + lp > 4u)
		return LA_ST_XZ_DATA;
	s->lc = lc; s->lp = lp; s->pb = pb;
	return LA_ST_OK;
}

#define LA_XZ_NORM() do { if (range < (1u << 24)) { if (p >= lim) { st = lim_status; goto out; } \
		range <<= 8; code = (code << 8) | src[p]; p++; } } while (0)
#define LA_XZ_BIT(idx, bit) do { LA_XZ_NORM(); { const uint32_t i_ = (idx); const uint32_t pr_ = probs[i_]; \
		const uint32_t bd_ = (range >> 11) * pr_; \
		if (code < bd_) { range = bd_; probs[i_] = (uint16_t)(pr_ + ((2048u - pr_) >> 5)); bit = 0; } \
		else { range -= bd_; code -= bd_; probs[i_] = (uint16_t)(pr_ - (pr_ >> 5)); bit = 1; } } } while (0)

/* The LZMA symbol loop, stated once for its two callers: an LZMA2 chunk (la_xz_lzma_chunk below, marker == 0) and an
 * lzip member (la_lzip_dev.h, marker == 1).  src[*pp, lim) into dst[*ppos, stop); lim_status is what asking for src[lim]
 * means.  The last dictionary reset lies at dst[dict_start].
 *   marker == 0: the chunk's ends are known.  stop <= chunk_out_end; chunk_end is the chunk's last compressed byte + 1.
 * Returns LA_ST_OK with *ppos == stop: the chunk is complete and checked when stop == chunk_out_end, otherwise the output
 * limit cut it.  The end-of-payload marker is refused as the distance it is.
 *   marker == 1: neither end is known (chunk_end and chunk_out_end are not read).  The stream goes on until the
 * end-of-payload marker: behind it liblzma normalises once more and asks for code == 0 (else LA_ST_XZ_DATA); then
 * *ended = 1 and *pp stands behind the marker.  A symbol that does not fit in front of `stop` is over_status (a match is
 * copied up to stop first); nothing is decoded behind the marker. */
LA_XZ_FN uint32_t la_xz_lzma_run(la_xz_lzma *s, uint16_t *probs, const uint8_t *src, uint64_t *pp, uint64_t lim, uint64_t chunk_end,
    uint32_t lim_status, uint8_t *dst, uint64_t *ppos, uint64_t stop, uint64_t chunk_out_end, uint64_t dict_start, uint32_t dict_cap,
    const int marker, uint32_t over_status, uint32_t *ended)
{
	uint64_t p = *pp, pos = *ppos;
	uint32_t range = 0xFFFFFFFFu, code = 0, st = LA_ST_OK;
	uint32_t state = s->state, rep0 = s->rep0, rep1 = s->rep1, rep2 = s->rep2, rep3 = s->rep3;
	const uint32_t lc = s->lc, lp_mask = (1u << s->lp) - 1u, pb_mask = (1u << s->pb) - 1u;
	for (int i = 0; i < 5; i++) {
		if (p >= lim) { st = lim_status; goto out; }
		if (i == 0 && src[p] != 0) { st = LA_ST_XZ_DATA; goto out; }
		code = (code << 8) | src[p];
		p++;
	}
	while (marker || pos < stop) {
		const uint32_t pos_state = (uint32_t)pos & pb_mask;
		uint32_t bit;
		LA_XZ_BIT(LA_XZ_P_IS_MATCH + state * 16u + pos_state, bit);
		if (bit == 0) {
			if (marker && pos >= stop) { st = over_status; goto out; }
			const uint32_t prev = pos == dict_start ? 0u : dst[pos - 1];
			const uint32_t lit = LA_XZ_P_LITERAL + 768u * ((((uint32_t)pos & lp_mask) << lc) + (prev >> (8u - lc)));
			uint32_t sym = 1;
			if (state < 7u) {
				do {
					LA_XZ_BIT(lit + sym, bit);
					sym = (sym << 1) | bit;
				} while (sym < 0x100u);
			} else {
				uint32_t mb = (uint32_t)dst[pos - rep0 - 1] << 1, offset = 0x100u;
				do {
					const uint32_t match_bit = mb & offset;
					LA_XZ_BIT(lit + offset + match_bit + sym, bit);
					sym = (sym << 1) | bit;
					if (bit) offset &= match_bit; else offset &= ~match_bit;
					mb <<= 1;
				} while (sym < 0x100u);
			}
			dst[pos++] = (uint8_t)sym;
			state = state < 4u ? 0u : state < 10u ? state - 3u : state - 6u;
			continue;
		}
		uint32_t len, lenp;
		const uint64_t avail = pos - dict_start < dict_cap ? pos - dict_start : dict_cap;
		LA_XZ_BIT(LA_XZ_P_IS_REP + state, bit);
		if (bit == 0) {
			rep3 = rep2; rep2 = rep1; rep1 = rep0;
			lenp = LA_XZ_P_LEN;
			state = state < 7u ? 7u : 10u;
		} else {
			if (avail == 0) { st = LA_ST_XZ_LZMA; goto out; }
			LA_XZ_BIT(LA_XZ_P_IS_REP0 + state, bit);
			if (bit == 0) {
				LA_XZ_BIT(LA_XZ_P_IS_REP0_LONG + state * 16u + pos_state, bit);
				if (bit == 0) {
					if (rep0 >= avail) { st = LA_ST_XZ_LZMA; goto out; }
					if (marker && pos >= stop) { st = over_status; goto out; }
					dst[pos] = dst[pos - rep0 - 1];
					pos++;
					state = state < 7u ? 9u : 11u;
					continue;
				}
			} else {
				uint32_t d;
				LA_XZ_BIT(LA_XZ_P_IS_REP1 + state, bit);
				if (bit == 0) {
					d = rep1;
				} else {
					LA_XZ_BIT(LA_XZ_P_IS_REP2 + state, bit);
					if (bit == 0) {
						d = rep2;
					} else {
						d = rep3;
						rep3 = rep2;
					}
					rep2 = rep1;
				}
				rep1 = rep0;
				rep0 = d;
			}
			lenp = LA_XZ_P_REP_LEN;
			state = state < 7u ? 8u : 11u;
		}
		{	/* the length: 2 .. 9, 10 .. 17, 18 .. 273 */
			uint32_t base, nb, add, sym = 1;
			LA_XZ_BIT(lenp, bit);
			if (bit == 0) {
				base = lenp + LA_XZ_LEN_LOW + pos_state * 8u; nb = 3; add = 2;
			} else {
				LA_XZ_BIT(lenp + 1u, bit);
				if (bit == 0) { base = lenp + LA_XZ_LEN_MID + pos_state * 8u; nb = 3; add = 10; }
				else { base = lenp + LA_XZ_LEN_HIGH; nb = 8; add = 18; }
			}
			for (uint32_t i = 0; i < nb; i++) {
				LA_XZ_BIT(base + sym, bit);
				sym = (sym << 1) | bit;
			}
			len = sym - (1u << nb) + add;
		}
		if (lenp == LA_XZ_P_LEN) {	/* a new distance: slots 0 .. 3, 4 .. 13 (reverse tree), 14 .. 63 (direct bits and align) */
			const uint32_t ds = LA_XZ_P_DIST_SLOT + (len < 6u ? len - 2u : 3u) * 64u;
			uint32_t slot = 1;
			for (int i = 0; i < 6; i++) {
				LA_XZ_BIT(ds + slot, bit);
				slot = (slot << 1) | bit;
			}
			slot -= 64u;
			if (slot < 4u) {
				rep0 = slot;
			} else {
				uint32_t nb = (slot >> 1) - 1u;
				rep0 = 2u | (slot & 1u);
				if (slot < 14u) {
					rep0 <<= nb;
					const uint32_t base = LA_XZ_P_DIST_SPECIAL + rep0 - slot - 1u;
					uint32_t sym = 1;
					for (uint32_t i = 0; i < nb; i++) {
						LA_XZ_BIT(base + sym, bit);
						sym = (sym << 1) | bit;
						rep0 += bit << i;
					}
				} else {
					nb -= 4u;
					for (uint32_t i = 0; i < nb; i++) {
						LA_XZ_NORM();
						range >>= 1;
						code -= range;
						const uint32_t t = 0u - (code >> 31);
						code += range & t;
						rep0 = (rep0 << 1) + (t + 1u);
					}
					rep0 <<= 4;
					uint32_t sym = 1;
					for (uint32_t i = 0; i < 4u; i++) {
						LA_XZ_BIT(LA_XZ_P_DIST_ALIGN + sym, bit);
						sym = (sym << 1) | bit;
						rep0 += bit << i;
					}
				}
			}
		}
		if (marker && lenp == LA_XZ_P_LEN && rep0 == 0xFFFFFFFFu) {	/* the end-of-payload marker, whatever its length */
			LA_XZ_NORM();
			if (code != 0)
				st = LA_ST_XZ_DATA;
			else
				*ended = 1;
			goto out;
		}
		if (rep0 >= avail) { st = LA_ST_XZ_LZMA; goto out; }
		{
			const uint64_t room = stop - pos;
			const uint32_t n = len < room ? len : (uint32_t)room;
			const uint64_t from = pos - rep0 - 1u;
			for (uint32_t i = 0; i < n; i++)
				dst[pos + i] = dst[from + i];
			pos += n;
			if (n < len) {	/* the output ends inside the match */
				if (marker)
					st = over_status;
				else if (stop == chunk_out_end)
					st = LA_ST_XZ_DATA;
				goto out;
			}
		}
	}
	if (!marker && pos == chunk_out_end) {
		LA_XZ_NORM();
		if (code != 0 || p != chunk_end)
			st = LA_ST_XZ_DATA;
	}
out:
	s->state = state; s->rep0 = rep0; s->rep1 = rep1; s->rep2 = rep2; s->rep3 = rep3;
	*pp = p; *ppos = pos;
	return st;
}

/* One LZMA chunk of an LZMA2 block: see la_xz_lzma_run, marker == 0 */
LA_XZ_FN uint32_t la_xz_lzma_chunk(la_xz_lzma *s, uint16_t *probs, const uint8_t *src, uint64_t *pp, uint64_t lim, uint64_t chunk_end,
    uint32_t lim_status, uint8_t *dst, uint64_t *ppos, uint64_t stop, uint64_t chunk_out_end, uint64_t dict_start, uint32_t dict_cap)
{
	return la_xz_lzma_run(s, probs, src, pp, lim, chunk_end, lim_status, dst, ppos, stop, chunk_out_end, dict_start, dict_cap, 0, LA_ST_OK,
	    (uint32_t *)0);
}

#ifndef LA_XZ_COPY
#define LA_XZ_COPY(d, s, n) do { for (uint64_t i_ = 0; i_ < (n); i_++) (d)[i_] = (s)[i_]; } while (0)
#endif

/* One block: LZMA2 data at src[src_off ...) into dst[0, cap).  src_lim = min(src_off + compressed size of the header,
 * bytes of the source) and lim_status says which of the two it is (LA_ST_XZ_SIZE, LA_ST_XZ_TRUNCATED); cap_status the
 * same for the output (LA_ST_XZ_SIZE, LA_ST_XZ_OUT_FULL).  probs holds LA_XZ_PROBS_MAX entries.  Fills status, out_len
 * and consumed (the bytes through the end marker; what was read so far on a failure). */
LA_XZ_FN void la_xz_block_decode(const uint8_t *src, uint64_t src_off, uint64_t src_lim, uint32_t lim_status, uint8_t *dst, uint64_t cap,
    uint32_t cap_status, uint32_t dict_size, uint16_t *probs, la_xz_lzma *lz, la_xz_result *res)
{
	const uint32_t dict_cap = la_xz_dict_cap(dict_size);
	uint64_t p = src_off, pos = 0, dict_start = 0;
	uint32_t st = LA_ST_OK;
	int need_props = 1, need_reset = 1;
	lz->lc = lz->lp = lz->pb = 0;
	lz->state = lz->rep0 = lz->rep1 = lz->rep2 = lz->rep3 = 0;
	for (;;) {
		if (p >= src_lim) { st = lim_status; break; }
		const uint32_t c = src[p++];
		if (c == 0)
			break;
		if (c >= 0xE0u || c == 1u) {
			need_props = 1;
			need_reset = 1;
		} else if (need_reset) {
			st = LA_ST_XZ_DATA;
			break;
		}
		if (c >= 0x80u) {
			if (c < 0xC0u && need_props) { st = LA_ST_XZ_DATA; break; }
			const uint32_t hdr = c >= 0xC0u ? 5u : 4u;
			if (src_lim - p < hdr) { st = lim_status; p = src_lim; break; }
			const uint64_t usize = (((uint64_t)(c & 0x1Fu) << 16) | ((uint64_t)src[p] << 8) | src[p + 1]) + 1u;
			const uint64_t csize = (((uint64_t)src[p + 2] << 8) | src[p + 3]) + 1u;
			p += 4;
			if (c >= 0xC0u) {
				if ((st = la_xz_props(lz, src[p++])) != LA_ST_OK)
					break;
				need_props = 0;
				la_xz_lzma_reset(lz, probs);
			} else if (c >= 0xA0u) {
				la_xz_lzma_reset(lz, probs);
			}
			if (need_reset) {
				need_reset = 0;
				dict_start = pos;
			}
			const uint64_t chunk_end = p + csize, out_end = pos + usize;
			const uint64_t lim = chunk_end <= src_lim ? chunk_end : src_lim;
			st = la_xz_lzma_chunk(lz, probs, src, &p, lim, chunk_end, chunk_end <= src_lim ? (uint32_t)LA_ST_XZ_LZMA : lim_status, dst, &pos,
			    out_end <= cap ? out_end : cap, out_end, dict_start, dict_cap);
			if (st != LA_ST_OK)
				break;
			if (pos < out_end) { st = cap_status; break; }
		} else {
			if (c > 2u) { st = LA_ST_XZ_DATA; break; }
			if (src_lim - p < 2u) { st = lim_status; p = src_lim; break; }
			const uint64_t n = (((uint64_t)src[p] << 8) | src[p + 1]) + 1u;
			p += 2;
			if (need_reset) {
				need_reset = 0;
				dict_start = pos;
			}
			const uint64_t have = src_lim - p, room = cap - pos;
			uint64_t k = n < have ? n : have;
			if (k > room) k = room;
			LA_XZ_COPY(dst + pos, src + p, k);
			pos += k;
			p += k;
			if (k < n) { st = (have < n && have <= room) ? lim_status : cap_status; break; }
		}
	}
	res->status = st;
	res->reserved = 0;
	res->out_len = pos;
	res->consumed = p - src_off;
	res->valid = pos;
}

/* behind a complete decode: do the sizes of the block header (and the check offset worked out from them) hold? */
LA_XZ_FN int la_xz_sizes_agree(const la_xz_block *blk, const la_xz_result *r)
{
	if (blk->comp_size != LA_XZ_UNKNOWN && r->consumed != blk->comp_size)
		return 0;
	if (blk->uncomp_size != LA_XZ_UNKNOWN && r->out_len != blk->uncomp_size)
		return 0;
	if (blk->check_off != LA_XZ_UNKNOWN && blk->check_off != blk->src_off + r->consumed + ((4u - (r->consumed & 3u)) & 3u))
		return 0;
	return 1;
}

/* ---- the block checks ---- */

/* check field bytes by check ID (the format's table 2.1.1.2) */
LA_XZ_FN uint32_t la_xz_check_size(uint32_t id)
{
	return id == 0u ? 0u : id <= 3u ? 4u : id <= 6u ? 8u : id <= 9u ? 16u : id <= 12u ? 32u : 64u;
}

#define LA_XZ_CRC64_POLY 0xC96C5795D7870F42ull	/* ECMA-182, reflected */

LA_XZ_FN uint64_t la_xz_crc64_entry(uint32_t i)
{
	uint64_t r = i;
	for (int k = 0; k < 8; k++)
		r = (r & 1u) ? (r >> 1) ^ LA_XZ_CRC64_POLY : r >> 1;
	return r;
}

/* CRC64 of p[0, n) continued from crc (0 for a fresh one), table of 256 la_xz_crc64_entry values */
LA_XZ_FN uint64_t la_xz_crc64(const uint64_t *table, const uint8_t *p, uint64_t n, uint64_t crc)
{
	crc = ~crc;
	for (uint64_t i = 0; i < n; i++)
		crc = table[(uint8_t)crc ^ p[i]] ^ (crc >> 8);
	return ~crc;
}

/* a * b mod P, polynomials over GF(2) in the reflected form: bit 63 is x^0 */
LA_XZ_FN uint64_t la_xz_crc64_mul(uint64_t a, uint64_t b)
{
	uint64_t m = (uint64_t)1 << 63, r = 0;
	for (int i = 0; i < 64; i++) {
		if (a & m)
			r ^= b;
		m >>= 1;
		b = (b & 1u) ? (b >> 1) ^ LA_XZ_CRC64_POLY : b >> 1;
	}
	return r;
}

/* x^(8 n) mod P: crc(A B) = la_xz_crc64_mul(la_xz_crc64_shift(|B|), crc(A)) ^ crc(B) */
LA_XZ_FN uint64_t la_xz_crc64_shift(uint64_t n)
{
	uint64_t r = (uint64_t)1 << 63, b = (uint64_t)1 << 55;
	while (n) {
		if (n & 1u)
			r = la_xz_crc64_mul(b, r);
		b = la_xz_crc64_mul(b, b);
		n >>= 1;
	}
	return r;
}

typedef struct la_xz_sha256 {
	uint32_t h[8];
} la_xz_sha256;

LA_XZ_FN uint32_t la_xz_sha_k(uint32_t i)
{
	/* the first 32 bits of the fractional parts of the cube roots of the first 64 primes (FIPS 180-4, 4.2.2) */
	const uint32_t k[64] = {
		0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u,
		0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u,
		0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau,
		0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u,
		0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,
		0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u,
		0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u,
		0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u };
	return k[i];
}

#define LA_XZ_ROR(x, n) (((x) >> (n)) | ((x) << (32 - (n))))

LA_XZ_FN void la_xz_sha256_block(la_xz_sha256 *s, const uint8_t *b)
{
	uint32_t w[16], v[8];
	for (int i = 0; i < 16; i++)
		w[i] = (uint32_t)b[4 * i] << 24 | (uint32_t)b[4 * i + 1] << 16 | (uint32_t)b[4 * i + 2] << 8 | b[4 * i + 3];
	for (int i = 0; i < 8; i++)
		v[i] = s->h[i];
	for (uint32_t i = 0; i < 64; i++) {
		if (i >= 16) {
			const uint32_t w15 = w[(i + 1) & 15], w2 = w[(i + 14) & 15];
			w[i & 15] += (LA_XZ_ROR(w15, 7) ^ LA_XZ_ROR(w15, 18) ^ (w15 >> 3)) + w[(i + 9) & 15] +
			    (LA_XZ_ROR(w2, 17) ^ LA_XZ_ROR(w2, 19) ^ (w2 >> 10));
		}
		const uint32_t e = v[4], a = v[0];
		const uint32_t t1 = v[7] + (LA_XZ_ROR(e, 6) ^ LA_XZ_ROR(e, 11) ^ LA_XZ_ROR(e, 25)) + ((e & v[5]) ^ (~e & v[6])) + la_xz_sha_k(i) + w[i & 15];
		const uint32_t t2 = (LA_XZ_ROR(a, 2) ^ LA_XZ_ROR(a, 13) ^ LA_XZ_ROR(a, 22)) + ((a & v[1]) ^ (a & v[2]) ^ (v[1] & v[2]));
		v[7] = v[6]; v[6] = v[5]; v[5] = v[4]; v[4] = v[3] + t1;
		v[3] = v[2]; v[2] = v[1]; v[1] = v[0]; v[0] = t1 + t2;
	}
	for (int i = 0; i < 8; i++)
		s->h[i] += v[i];
}

/* SHA-256 of p[0, n): one chain; out[32] big-endian, as the check field stores it */
LA_XZ_FN void la_xz_sha256_all(const uint8_t *p, uint64_t n, uint8_t *out)
{
	la_xz_sha256 s = { { 0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au, 0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u } };
	uint64_t i = 0;
	for (; i + 64 <= n; i += 64)
		la_xz_sha256_block(&s, p + i);
	uint8_t last[128];
	uint32_t k = 0;
	for (; i < n; i++)
		last[k++] = p[i];
	last[k++] = 0x80;
	const uint32_t total = k <= 56u ? 64u : 128u;
	while (k < total - 8u)
		last[k++] = 0;
	const uint64_t bits = n * 8u;
	for (int j = 7; j >= 0; j--)
		last[k++] = (uint8_t)(bits >> (8 * j));
	la_xz_sha256_block(&s, last);
	if (total == 128u)
		la_xz_sha256_block(&s, last + 64);
	for (int j = 0; j < 8; j++) {
		out[4 * j] = (uint8_t)(s.h[j] >> 24); out[4 * j + 1] = (uint8_t)(s.h[j] >> 16);
		out[4 * j + 2] = (uint8_t)(s.h[j] >> 8); out[4 * j + 3] = (uint8_t)s.h[j];
	}
}

/* Behind the end marker: the zero padding up to a multiple of four, then the check field.  Reads src below src_bytes
 * only.  `have` is the check value computed over the block's bytes (la_xz_check_size(check_id) bytes, as stored);
 * supported says whether there is one (IDs 0, 1, 4, 10: the others are passed over unverified, as liblzma does without
 * LZMA_TELL_UNSUPPORTED_CHECK).  LA_ST_OK, LA_ST_XZ_TRUNCATED, LA_ST_XZ_PADDING or LA_ST_XZ_BAD_CHECK. */
LA_XZ_FN uint32_t la_xz_block_tail(const uint8_t *src, uint64_t src_bytes, uint64_t src_off, uint64_t consumed, uint32_t check_id,
    const uint8_t *have, int supported)
{
	uint64_t p = src_off + consumed;
	const uint32_t pad = (uint32_t)((4u - (consumed & 3u)) & 3u), cs = la_xz_check_size(check_id);
	for (uint32_t i = 0; i < pad; i++, p++) {
		if (p >= src_bytes)
			return LA_ST_XZ_TRUNCATED;
		if (src[p] != 0)
			return LA_ST_XZ_PADDING;
	}
	if (src_bytes - p < cs)
		return LA_ST_XZ_TRUNCATED;
	if (supported)
		for (uint32_t i = 0; i < cs; i++)
			if (src[p + i] != have[i])
				return LA_ST_XZ_BAD_CHECK;
	return LA_ST_OK;
}

#endif
