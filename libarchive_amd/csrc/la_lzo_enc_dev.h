/*
 * la_lzo_enc_dev.h -- how a sequence (literal count, match distance, match length) becomes LZO1X bytes, stated ONCE: the
 * kernel (la_lzo_comp.hip), the CPU stand-in of the tests (tests/mock_gpu/la_gpu_lzop_comp_mock.c) and its sanitizer
 * program all compile this file.  Common subset of C and C++.  It says nothing about how matches are found.
 *
 * No liblzo2 stands behind this file: the forms are those la_lzo_dev.h decodes, written from the format description.
 *
 * The emitter moves bytes through four hooks, so that the host runs them as plain loops and the kernel wave-wide.  Every
 * argument is the same on all lanes of a wave.  A hook stores nothing at or behind the stream's room (io->cap): the
 * emitter goes on COUNTING there, so a block that will be stored anyway needs no more room than its own bytes.
 *   la_lzoe_put(io, at, b)            stream[at] = b                              (the kernel: lane 0)
 *   la_lzoe_or(io, at, bits)          stream[at] |= bits, the trail patch         (the kernel: lane 0)
 *   la_lzoe_zeros(io, at, n)          stream[at, at + n) = 0                      (the kernel: a byte per lane and step)
 *   la_lzoe_literals(io, at, ip, n)   stream[at, at + n) = plain[ip, ip + n)      (the kernel: 64 bytes per step)
 * A translation unit that defines LA_LZOE_HOOKS brings its own la_lzoe_io and hooks; otherwise the plain ones below hold.
 *
 * The rules.
 *   form by distance and length   M2 (2 bytes) for length 3..8 and distance <= 2048: t = ((len - 1) << 5) | (((dist - 1) & 7) << 2),
 *                                 then (dist - 1) >> 3.
 *                                 M3 for distance <= 16384: t = 32 | (len - 2), or 32 and a zero-run for len - 2 > 31 (base 31);
 *                                 then LE16 w = (dist - 1) << 2.
 *                                 M4 for 16385 .. 49151: d = dist - 16384 (never 0, which is the end marker), t = 16 |
 *                                 ((d >> 14) << 3) | (len - 2), or a zero-run for len - 2 > 7 (base 7); then LE16 w = (d & 0x3FFF) << 2.
 *                                 No M1.  A distance above LA_LZOE_MAX_DIST cannot be coded and must never reach the emitter.
 *   a zero-run that adds v >= 1   (v - 1) / 255 bytes 0x00, then the byte v - 255 * that count (1 .. 255)
 *   literals in front of a match  (or of the end): 1..3 go into the low two bits of the instruction in front of them, t (M2) or
 *                                 w's low byte (M3, M4), and follow it; 4 or more are a literal run: t = n - 3 for n <= 18, else
 *                                 0x00 and a zero-run of n - 18 (base 15, plus 3)
 *   start of a block              up to 238 literals: the first byte 17 + n; more: an ordinary run (0x00 is no first-byte form)
 *   end                           11 00 00
 * A match is at least 3 bytes long; the device matcher's are at least 4.
 *
 * WORST CASE.  la_lzoe_worst(n) = n + n / 7 + 4 bounds the stream of ANY sequence list over a block of n bytes.  Proof: a
 * match never costs more than the bytes it stands for (M2: 2 <= 3; M3: 3 for len <= 33, 4 + (len - 34) / 255 behind;
 * M4: 3 for len <= 9, 4 + (len - 10) / 255 behind; all <= len for len >= 3).  Literals cost themselves, 1..3 of them
 * nothing more.  Only the prefix of a run of L >= 4 adds: p(L) = 1 for L <= 18, 2 + (L - 19) / 255 above, and
 * p(L) <= (L + 3) / 7 for every L >= 4 (7 <= L + 3 below 19; at 19, 2 <= 22 / 7, and the slope 1 / 255 is below 1 / 7).
 * Charge the + 3 to the match in front of the run, which is at least 3 bytes and in front of no other run; the run at
 * the block's start has no match in front but is either the first-byte form (1 byte, counted apart) or longer than 238,
 * where p(L) <= L / 7.  So all prefixes together are at most n / 7 + 1, and the marker adds 3.
 * A block whose stream reaches n bytes is stored (archive_write_add_filter_lzop.c:364-381), and la_lzoe_worst(n) > n, so
 * the scratch slot of a block is la_lzoe_slot_bytes(n): the block's own size, with the hooks counting behind it.
 */
#ifndef LA_LZO_ENC_DEV_H
#define LA_LZO_ENC_DEV_H

#include <stdint.h>

#ifndef LA_LZO_FN
#define LA_LZO_FN static inline
#endif

#define LA_LZOE_MAX_DIST    49151u
#define LA_LZOE_FIRST_MAX   238u
#define LA_LZOE_NO_PATCH    0xFFFFFFFFu

#ifndef LA_LZOE_HOOKS
typedef struct la_lzoe_io {
	const uint8_t *plain;
	uint8_t *out;
	uint32_t cap;
} la_lzoe_io;

LA_LZO_FN void la_lzoe_put(la_lzoe_io *io, uint32_t at, uint32_t b)
{
	if (at < io->cap)
		io->out[at] = (uint8_t)b;
}

LA_LZO_FN void la_lzoe_or(la_lzoe_io *io, uint32_t at, uint32_t bits)
{
	if (at < io->cap)
		io->out[at] = (uint8_t)(io->out[at] | bits);
}

LA_LZO_FN void la_lzoe_zeros(la_lzoe_io *io, uint32_t at, uint32_t n)
{
	for (uint32_t i = 0; i < n && at + i < io->cap; i++)
		io->out[at + i] = 0;
}

LA_LZO_FN void la_lzoe_literals(la_lzoe_io *io, uint32_t at, uint32_t ip, uint32_t n)
{
	for (uint32_t i = 0; i < n && at + i < io->cap; i++)
		io->out[at + i] = io->plain[ip + i];
}
#endif

typedef struct la_lzoe_state {
	uint32_t op;		/* stream bytes so far, those counted behind the room included */
	uint32_t patch;		/* where the next 1..3 literals put their count; LA_LZOE_NO_PATCH in front of the first match */
} la_lzoe_state;

LA_LZO_FN uint32_t la_lzoe_worst(uint32_t n)
{
	return n + n / 7u + 4u;
}

LA_LZO_FN uint32_t la_lzoe_slot_bytes(uint32_t n)
{
	return (n + 15u) & ~15u;	/* la_lzoe_worst(n) > n, and what reaches n is stored: the first n stream bytes are all that is read */
}

LA_LZO_FN void la_lzoe_begin(la_lzoe_state *st)
{
	st->op = 0;
	st->patch = LA_LZOE_NO_PATCH;
}

/* a zero-run that adds v >= 1 to its base */
LA_LZO_FN void la_lzoe_run(la_lzoe_io *io, la_lzoe_state *st, uint32_t v)
{
	const uint32_t zeros = (v - 1u) / 255u;
	la_lzoe_zeros(io, st->op, zeros);
	st->op += zeros;
	la_lzoe_put(io, st->op++, v - 255u * zeros);
}

/* plain[ip, ip + n) in front of a match or of the end */
LA_LZO_FN void la_lzoe_lits(la_lzoe_io *io, la_lzoe_state *st, uint32_t ip, uint32_t n)
{
	if (n == 0)
		return;
	if (st->patch == LA_LZOE_NO_PATCH && n <= LA_LZOE_FIRST_MAX)
		la_lzoe_put(io, st->op++, 17u + n);
	else if (n <= 3u)
		la_lzoe_or(io, st->patch, n);
	else if (n <= 18u)
		la_lzoe_put(io, st->op++, n - 3u);
	else {
		la_lzoe_put(io, st->op++, 0);
		la_lzoe_run(io, st, n - 18u);
	}
	la_lzoe_literals(io, st->op, ip, n);
	st->op += n;
}

/* one sequence: `lit` literals from plain[ip], then a match of `len` bytes (>= 3) at distance 1 .. LA_LZOE_MAX_DIST */
LA_LZO_FN void la_lzoe_seq(la_lzoe_io *io, la_lzoe_state *st, uint32_t ip, uint32_t lit, uint32_t dist, uint32_t len)
{
	la_lzoe_lits(io, st, ip, lit);
	if (dist <= 2048u && len <= 8u) {
		st->patch = st->op;
		la_lzoe_put(io, st->op++, ((len - 1u) << 5) | (((dist - 1u) & 7u) << 2));
		la_lzoe_put(io, st->op++, (dist - 1u) >> 3);
		return;
	}
	const uint32_t m3 = dist <= 16384u;
	const uint32_t d = m3 ? dist - 1u : dist - 16384u;
	const uint32_t t = m3 ? 32u : 16u | ((d >> 14) << 3), short_max = m3 ? 31u : 7u;
	if (len - 2u <= short_max)
		la_lzoe_put(io, st->op++, t | (len - 2u));
	else {
		la_lzoe_put(io, st->op++, t);
		la_lzoe_run(io, st, len - 2u - short_max);
	}
	const uint32_t w = (d & 0x3FFFu) << 2;
	st->patch = st->op;
	la_lzoe_put(io, st->op++, w & 255u);
	la_lzoe_put(io, st->op++, w >> 8);
}

/* the block's last `lit` literals from plain[ip] and the end marker; returns the stream's size */
LA_LZO_FN uint32_t la_lzoe_end(la_lzoe_io *io, la_lzoe_state *st, uint32_t ip, uint32_t lit)
{
	la_lzoe_lits(io, st, ip, lit);
	la_lzoe_put(io, st->op++, 0x11);
	la_lzoe_put(io, st->op++, 0);
	la_lzoe_put(io, st->op++, 0);
	return st->op;
}

#endif
