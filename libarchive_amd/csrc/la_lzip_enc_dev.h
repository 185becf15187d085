/*
 * la_lzip_enc_dev.h -- the lzip ENCODER's rules, stated ONCE: the member kernel and the pack kernel (la_lzip_comp.hip),
 * the CPU stand-in of the tests (tests/mock_lzip_write) and its sanitizer program all compile this file.  It is the common
 * subset of C and C++ and sits on la_xz_enc_dev.h, whose hook macros (LA_XZ_FN, LA_XZC_LANE_LOOP, LA_XZC_SYNC,
 * LA_XZC_TAB_MAX, LA_XZC_PUT, LA_XZC_EVENT) the including file defines before it, as for the xz encoder: lzip carries the
 * same LZMA bit stream (lc 3, lp 0, pb 2), so matcher, symbol choice and range coder are that header's, used unchanged.
 *
 * The stream shape.  The input is cut every la_lzc_member_bytes(level) bytes; every cut is one complete
 * MEMBER: 6 header bytes ("LZIP", version 1, the dictionary byte), one raw LZMA1 stream that ends with the end marker,
 * and 20 trailer bytes (CRC32 of the data, data size, member size, little-endian).  A stream is members back to back,
 * as plzip writes them; no input at all is one member of no data.  Members know nothing of each other.
 *
 * One member (la_lzc_member) is one chain of la_xz_enc_dev.h with lo = cs = 0: positions, pos_state and the literal's
 * previous byte come from the offset inside the member, and distances stay inside it.  Behind the last byte comes the
 * end marker, a match of length 2 with distance 0xFFFFFFFF (distance slot 63, 26 direct bits set, four align bits set),
 * then the coder's five flush bytes.  lzip has no uncompressed member, so there is no stored form and no early exit.
 *
 * THE BOUND, which therefore has to hold by arithmetic and not by a fallback:
 *   - a probability starts at 1024 of 2048 and moves by p += (2048 - p) >> 5 or p -= p >> 5: upwards it stops at 2017
 *     (31 >> 5 == 0), downwards at 31, so either bit of a decision has a probability of at least 31 / 2048;
 *   - the coder gives a 0 bit (range >> 11) * p and a 1 bit the rest; range >= 2^24, so the truncation takes less than
 *     2^-13 of it: a decision costs at most log2(2048 / 31) + log2(1 / (1 - 2^-13)) < 6.0461 bits, a direct bit exactly 1;
 *   - the range is renormalised by whole bytes, so a stream of B bits of decisions takes at most ceil(B / 8) shifts, the
 *     five flush shifts behind them, and the bytes put out never outnumber the shifts (a shift holds its byte back or
 *     releases the ones held; the first is the initial cache byte);
 *   - per input byte, with distances below 2^18 (slot <= 35: 12 direct bits, 4 align bits):
 *       literal            1 + 8 decisions                          over 1 byte    6.81 bytes per byte   <- the dearest
 *       short rep          4 decisions                              over 1 byte    3.03
 *       rep match          5 + 10 decisions                         over >= 2      5.67
 *       match              2 + 10 + 6 + 4 decisions + 12 direct     over >= 4      4.54
 *     (10 is the longest length code: two choices and the 8-bit high tree, which only lengths of 18 and more take);
 *   - the marker is 2 + 4 + 6 + 4 decisions and 26 direct bits: under 16 bytes; with the flush and the rounding, under 24.
 * A member of m input bytes is therefore below 6.81 m + 24 stream bytes; la_lzc_slot_bytes(m) = 7 m + 64 is what every
 * buffer is sized by, and la_lzc_bound adds the 26 bytes of framing per member.  (Measured expansion on noise is about
 * 1.4 %; nothing is sized by that.)  The price: workspace and output buffers are about SEVEN times the
 * window, 448 MiB each for a 64 MiB window (la_gpu_bzip2_compress takes 2.9 GiB of workspace for the same window).
 *
 * Below the encoder: CRC32 (IEEE 802.3, reflected) as table entry, running value and combine arithmetic, the 32-bit
 * twin of la_xz_dev.h's CRC64.
 */
#ifndef LA_LZIP_ENC_DEV_H
#define LA_LZIP_ENC_DEV_H

#include "la_xz_enc_dev.h"

#define LA_LZC_HEADER_BYTES  6u
#define LA_LZC_TRAILER_BYTES 20u
#define LA_LZC_BIG_LEVEL     7u			/* from here on members of 256 KiB */
#define LA_LZC_EV_MARKER     LA_XZC_EV_COUNT	/* the event hook's one kind more than the xz encoder's */
#define LA_LZC_EV_COUNT      (LA_XZC_EV_COUNT + 1)

/* input bytes per member; 0 for a level above 9.  The larger member resets the model a quarter as often and reaches
 * distances up to 256 KiB, and gives a window a quarter of the chains; the default level keeps the fast shape. */
LA_XZ_FN uint32_t la_lzc_member_bytes(uint32_t level)
{
	return level > 9u ? 0u : level < LA_LZC_BIG_LEVEL ? 1u << 16 : 1u << 18;
}

/* the header's dictionary byte: the smallest dictionary that covers a member (2^16, 2^18) */
LA_XZ_FN uint32_t la_lzc_dict_byte(uint32_t level)
{
	return level < LA_LZC_BIG_LEVEL ? 0x10u : 0x12u;
}

/* the most the raw stream of a member of m input bytes takes (THE BOUND above), and what a member's slot holds */
LA_XZ_FN uint64_t la_lzc_slot_bytes(uint64_t m)
{
	return 7u * m + 64u;
}

LA_XZ_FN uint64_t la_lzc_members(uint64_t src_bytes, uint32_t level)
{
	const uint64_t m = la_lzc_member_bytes(level);
	return src_bytes ? (src_bytes + m - 1u) / m : 1u;
}

/* the most src_bytes take at `level` (0 .. 9): every member at its slot plus header and trailer */
LA_XZ_FN uint64_t la_lzc_bound(uint64_t src_bytes, uint32_t level)
{
	const uint64_t m = la_lzc_member_bytes(level), frame = LA_LZC_HEADER_BYTES + LA_LZC_TRAILER_BYTES;
	const uint64_t full = src_bytes / m, rest = src_bytes % m;
	return full * (la_lzc_slot_bytes(m) + frame) + (rest || !src_bytes ? la_lzc_slot_bytes(rest) + frame : 0u);
}

LA_XZ_FN void la_lzc_header(uint8_t *h, uint32_t level)
{
	h[0] = 'L'; h[1] = 'Z'; h[2] = 'I'; h[3] = 'P';
	h[4] = 1;
	h[5] = (uint8_t)la_lzc_dict_byte(level);
}

/* t[LA_LZC_TRAILER_BYTES] behind a stream of `stream` bytes that codes `data` bytes of CRC32 `crc` */
LA_XZ_FN void la_lzc_trailer(uint8_t *t, uint32_t crc, uint64_t data, uint64_t stream)
{
	const uint64_t member = LA_LZC_HEADER_BYTES + stream + LA_LZC_TRAILER_BYTES;
	for (uint32_t i = 0; i < 4u; i++)
		t[i] = (uint8_t)(crc >> (8u * i));
	for (uint32_t i = 0; i < 8u; i++) {
		t[4u + i] = (uint8_t)(data >> (8u * i));
		t[12u + i] = (uint8_t)(member >> (8u * i));
	}
}

/* One member: src[0, n) as one raw LZMA1 stream into slot[0, lim), counted beyond lim and stored below it only.  probs
 * holds LA_XZC_PROBS entries, tab LA_XZC_TAB, m_len and m_cand 64 each.  Returns the stream's bytes. */
LA_XZ_FN uint32_t la_lzc_member(const uint8_t *src, uint32_t n, uint16_t *probs, uint32_t *tab, uint32_t *m_len, uint32_t *m_cand, uint8_t *slot,
    uint32_t lim)
{
	la_xzc_enc e;
	la_xzc_chain_init(&e, src, 0, 0, n, probs, tab, slot, lim);
	la_xzc_chain_steps(&e, src, 0, 0, n, 0xFFFFFFFFu, probs, tab, m_len, m_cand);
	LA_XZC_EVENT(LA_LZC_EV_MARKER);
	la_xzc_match(&e, probs, n, 2, 0xFFFFFFFFu);
	for (int i = 0; i < 5; i++)
		la_xzc_rc_shift(&e.rc);
	return e.rc.pos;
}

/* ---- CRC32 ---- */

#define LA_LZC_CRC32_POLY 0xEDB88320u	/* IEEE 802.3, reflected */

LA_XZ_FN uint32_t la_lzc_crc32_entry(uint32_t i)
{
	uint32_t r = i;
	for (int k = 0; k < 8; k++)
		r = (r & 1u) ? (r >> 1) ^ LA_LZC_CRC32_POLY : r >> 1;
	return r;
}

/* CRC32 of p[0, n) continued from crc (0 for a fresh one), table of 256 la_lzc_crc32_entry values */
LA_XZ_FN uint32_t la_lzc_crc32(const uint32_t *table, const uint8_t *p, uint32_t n, uint32_t crc)
{
	crc = ~crc;
	for (uint32_t i = 0; i < n; i++)
		crc = table[(uint8_t)crc ^ p[i]] ^ (crc >> 8);
	return ~crc;
}

/* a * b mod P, polynomials over GF(2) in the reflected form: bit 31 is x^0 */
LA_XZ_FN uint32_t la_lzc_crc32_mul(uint32_t a, uint32_t b)
{
	uint32_t m = 1u << 31, r = 0;
	for (int i = 0; i < 32; i++) {
		if (a & m)
			r ^= b;
		m >>= 1;
		b = (b & 1u) ? (b >> 1) ^ LA_LZC_CRC32_POLY : b >> 1;
	}
	return r;
}

/* x^(8 n) mod P: crc(A B) = la_lzc_crc32_mul(la_lzc_crc32_shift(|B|), crc(A)) ^ crc(B) */
LA_XZ_FN uint32_t la_lzc_crc32_shift(uint32_t n)
{
	uint32_t r = 1u << 31, b = 1u << 23;
	while (n) {
		if (n & 1u)
			r = la_lzc_crc32_mul(b, r);
		b = la_lzc_crc32_mul(b, b);
		n >>= 1;
	}
	return r;
}

#endif
