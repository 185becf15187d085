/*
 * la_lzo_dev.h -- the LZO1X instruction rules of one lzop block, stated ONCE: the kernel (la_lzo.hip), the CPU stand-in
 * of the tests (tests/mock_lzop) and its sanitizer program all compile this file.  Common subset of C and C++.
 *
 * No liblzo2 stands behind this file: the rules are written from the format description (DESIGN.md names what that
 * leaves unverified).  tests/lzop_support.py holds the same rules in Python, and the Adler-32 that every block of the
 * reference's lzop fixtures carries pins both.
 *
 * The decoder below is the instruction chain only.  It moves bytes through three hooks, so that the host runs them as
 * plain loops and the kernel as wave-wide copies fed from a register window:
 *   la_lzo_byte(io, ip)               the source byte at ip
 *   la_lzo_literals(io, op, ip, n)    dst[op, op + n) = src[ip, ip + n)
 *   la_lzo_match(io, op, dist, n)     dst[op + i] = dst[op + i - dist] for i = 0 .. n - 1, in that order (dist <= op)
 * A translation unit that defines LA_LZO_HOOKS brings its own la_lzo_io and hooks; otherwise the plain ones below hold.
 *
 * The rules.  t is an instruction's first byte; state is the number of literals the previous instruction copied (0 at
 * the start, 4 after a literal run of 4 or more); a zero-run length is base + 255 * (number of 0x00 bytes) + (the first
 * non-zero byte).
 *   first byte of the block only: t > 17 copies t - 17 literals, state = min(t - 17, 4); anything else is ordinary.
 *   t 0..15,  state 0      literal run of t + 3 (t == 0: zero-run base 15, plus 3); state = 4
 *   t 0..15,  state 1..3   M1, 2 bytes: length 2, distance (next << 2) + (t >> 2) + 1
 *   t 0..15,  state 4      M1, 3 bytes: length 3, distance (next << 2) + (t >> 2) + 2049
 *   t 64..255              M2: length (t >> 5) + 1, distance (next << 3) + ((t >> 2) & 7) + 1
 *   t 32..63               M3: length (t & 31) + 2 (0: zero-run base 31, plus 2); LE16 w: distance (w >> 2) + 1
 *   t 16..31               M4: length (t & 7) + 2 (0: zero-run base 7, plus 2); LE16 w: d = ((t & 8) << 11) + (w >> 2);
 *                          d == 0 is the END of the stream whatever the length field and w's low bits say, else the
 *                          distance is d + 16384
 *   every match is followed by n literals, n the low two bits of t (M1, M2) or of w (M3, M4); state = n.
 * Verdicts: a match that starts in front of the first output byte is LA_ST_LZOP_LOOKBEHIND, tested before the output
 * room; a literal run or match that passes dst_len is LA_ST_LZOP_OUTPUT_OVERRUN, tested (for literals) before the input;
 * whatever asks for a byte at or behind src_len is LA_ST_LZOP_INPUT_OVERRUN; the end in front of src_len is
 * LA_ST_LZOP_NOT_CONSUMED; the end at src_len with fewer than dst_len bytes is LA_ST_LZOP_SHORT_OUTPUT.  An instruction
 * is carried out only when all of it fits, so on every failure out_len counts valid bytes.
 */
#ifndef LA_LZO_DEV_H
#define LA_LZO_DEV_H

#include "../../include/la_gpu.h"

#ifndef LA_LZO_FN
#define LA_LZO_FN static inline
#endif

#ifndef LA_LZO_HOOKS
typedef struct la_lzo_io {
	const uint8_t *src;
	uint8_t *dst;
} la_lzo_io;

LA_LZO_FN uint32_t la_lzo_byte(la_lzo_io *io, uint32_t ip)
{
	return io->src[ip];
}

LA_LZO_FN void la_lzo_literals(la_lzo_io *io, uint32_t op, uint32_t ip, uint32_t n)
{
	for (uint32_t i = 0; i < n; i++)
		io->dst[op + i] = io->src[ip + i];
}

LA_LZO_FN void la_lzo_match(la_lzo_io *io, uint32_t op, uint32_t dist, uint32_t n)
{
	for (uint32_t i = 0; i < n; i++)
		io->dst[op + i] = io->dst[op + i - dist];
}
#endif

/* 1: the entry may be touched: it points inside both buffers and its sizes are ones the format allows */
LA_LZO_FN int la_lzop_entry_ok(const la_lzop_block *b, uint64_t src_bytes, uint64_t dst_total)
{
	if (b->src_off > src_bytes || b->src_len > src_bytes - b->src_off || b->dst_off > dst_total || b->dst_len > dst_total - b->dst_off)
		return 0;
	return b->src_len <= b->dst_len && b->dst_len <= LA_LZOP_MAX_BLOCK;
}

/* a zero-run length from `base`; 0: the run asks for a byte behind src_len */
LA_LZO_FN int la_lzo_run(la_lzo_io *io, uint32_t src_len, uint32_t *ip, uint32_t base, uint64_t *len)
{
	uint64_t n = base;
	for (;;) {
		if (*ip >= src_len)
			return 0;
		const uint32_t b = la_lzo_byte(io, (*ip)++);
		if (b) {
			*len = n + b;
			return 1;
		}
		n += 255u;
	}
}

/* One block's stream: src[0, src_len) into dst[0, dst_len).  Returns LA_ST_OK or LA_ST_LZOP_*; *out_len = valid bytes,
 * *consumed = source bytes read (through the end marker when one was found). */
LA_LZO_FN uint32_t la_lzo1x_decode(la_lzo_io *io, uint32_t src_len, uint32_t dst_len, uint32_t *out_len, uint32_t *consumed)
{
	uint32_t ip = 0, op = 0, state = 0, st = LA_ST_OK;
	if (src_len > 0 && la_lzo_byte(io, 0) > 17u) {
		const uint32_t n = la_lzo_byte(io, 0) - 17u;
		ip = 1;
		if (n > dst_len - op)
			st = LA_ST_LZOP_OUTPUT_OVERRUN;
		else if (n > src_len - ip)
			st = LA_ST_LZOP_INPUT_OVERRUN;
		else {
			la_lzo_literals(io, op, ip, n);
			ip += n; op += n;
			state = n < 4u ? n : 4u;
		}
	}
	while (st == LA_ST_OK) {
		uint64_t mlen = 0;
		uint32_t dist, trail;
		if (ip >= src_len) { st = LA_ST_LZOP_INPUT_OVERRUN; break; }
		const uint32_t t = la_lzo_byte(io, ip++);
		if (t < 16u && state == 0) {
			/* a literal run */
			uint64_t n = t;
			if (n == 0 && !la_lzo_run(io, src_len, &ip, 15u, &n)) { st = LA_ST_LZOP_INPUT_OVERRUN; break; }
			n += 3u;
			if (n > dst_len - op) { st = LA_ST_LZOP_OUTPUT_OVERRUN; break; }
			if (n > src_len - ip) { st = LA_ST_LZOP_INPUT_OVERRUN; break; }
			la_lzo_literals(io, op, ip, (uint32_t)n);
			ip += (uint32_t)n; op += (uint32_t)n;
			state = 4;
			continue;
		}
		if (t < 16u) {
			/* M1: two bytes behind 1..3 literals, three bytes behind a literal run */
			if (ip >= src_len) { st = LA_ST_LZOP_INPUT_OVERRUN; break; }
			dist = (la_lzo_byte(io, ip++) << 2) + (t >> 2) + (state == 4u ? 2049u : 1u);
			mlen = state == 4u ? 3u : 2u;
			trail = t & 3u;
		} else if (t >= 64u) {
			/* M2 */
			if (ip >= src_len) { st = LA_ST_LZOP_INPUT_OVERRUN; break; }
			dist = (la_lzo_byte(io, ip++) << 3) + ((t >> 2) & 7u) + 1u;
			mlen = (t >> 5) + 1u;
			trail = t & 3u;
		} else {
			/* M3 (t >= 32) and M4 */
			const uint32_t m3 = t >= 32u;
			mlen = t & (m3 ? 31u : 7u);
			if (mlen == 0 && !la_lzo_run(io, src_len, &ip, m3 ? 31u : 7u, &mlen)) { st = LA_ST_LZOP_INPUT_OVERRUN; break; }
			mlen += 2u;
			if (src_len - ip < 2u) { st = LA_ST_LZOP_INPUT_OVERRUN; break; }
			const uint32_t w = la_lzo_byte(io, ip) | (la_lzo_byte(io, ip + 1) << 8);
			ip += 2;
			trail = w & 3u;
			if (m3)
				dist = (w >> 2) + 1u;
			else {
				const uint32_t d = ((t & 8u) << 11) + (w >> 2);
				if (d == 0) {
					/* the end of the stream */
					st = ip != src_len ? (uint32_t)LA_ST_LZOP_NOT_CONSUMED : op != dst_len ? (uint32_t)LA_ST_LZOP_SHORT_OUTPUT : (uint32_t)LA_ST_OK;
					*out_len = op;
					*consumed = ip;
					return st;
				}
				dist = d + 16384u;
			}
		}
		if (dist > op) { st = LA_ST_LZOP_LOOKBEHIND; break; }
		if (mlen > dst_len - op) { st = LA_ST_LZOP_OUTPUT_OVERRUN; break; }
		la_lzo_match(io, op, dist, (uint32_t)mlen);
		op += (uint32_t)mlen;
		if (trail) {
			if (trail > dst_len - op) { st = LA_ST_LZOP_OUTPUT_OVERRUN; break; }
			if (trail > src_len - ip) { st = LA_ST_LZOP_INPUT_OVERRUN; break; }
			la_lzo_literals(io, op, ip, trail);
			ip += trail; op += trail;
		}
		state = trail;
	}
	*out_len = op;
	*consumed = ip;
	return st;
}

/* which sum a block's flags ask for over its compressed (shift 0) or uncompressed (shift 2) bytes: CRC32 wins over
 * Adler-32 (lzop.c:419-424, :465-472) */
#define LA_LZOP_SUM_NONE  0u
#define LA_LZOP_SUM_ADLER 1u
#define LA_LZOP_SUM_CRC   2u
LA_LZO_FN uint32_t la_lzop_sum_kind(uint32_t flags, uint32_t uncompressed)
{
	const uint32_t f = uncompressed ? flags >> 2 : flags;
	return (f & LA_LZOP_C_CRC32) ? LA_LZOP_SUM_CRC : (f & LA_LZOP_C_ADLER32) ? LA_LZOP_SUM_ADLER : LA_LZOP_SUM_NONE;
}

#endif
