/*
 * la_xz_filters_dev.h -- the inverse transforms of the .xz filters that may stand in front of LZMA2 in a block's chain
 * (delta 0x03, and the BCJ filters x86 0x04, PowerPC 0x05, IA-64 0x06, ARM 0x07, ARM-Thumb 0x08, SPARC 0x09), as
 * liblzma 5.2 runs them (delta_decoder.c, simple/x86.c and its siblings), stated ONCE: the kernels (la_xz_filters.hip),
 * the CPU stand-in of the tests (tests/mock_xz_chains), its sanitizer program and the rules test
 * (tests/test_xz_unfilter_rules.py) all compile this file.  The common subset of C and C++; nothing device-only.
 * The including file may define LA_XZ_FN (the function qualifiers) before it.
 *
 * Every transform runs in place over the n bytes of ONE block; state restarts at every block.
 *   delta   prop = the distance, 1 .. 256.  out[i] = in[i] + out[i - dist] mod 256, bytes in front of the block are 0:
 *           out[i] is the sum of the column in[i], in[i - dist], in[i - 2 dist], ...  Per tile: the sum of every column
 *           (la_xz_delta_col_sum), an exclusive scan of those sums over the tiles, then la_xz_delta_col_apply with the
 *           scanned value as carry.  A column is i mod dist over the block, so a tile need not be a multiple of dist.
 *   BCJ     prop = start_offset; the position of byte i is start_offset + i in 32-bit arithmetic.  start_offset has to
 *           be a multiple of la_xz_bcj_align(id) (x86 1, Thumb 2, ARM / PowerPC / SPARC 4, IA-64 16).  The decoder
 *           takes the position (plus the architecture's bias) off the branch target.  Bytes that cannot hold a whole
 *           unit at the end of the block pass unchanged.
 *   unit    ARM, PowerPC, SPARC (4 bytes at a multiple of 4) and IA-64 (16 bytes at a multiple of 16) touch nothing
 *           outside their unit: a map.  ARM-Thumb looks at 4 bytes at every multiple of 2; a unit that converts has
 *           (b[1] & 0xF8) == 0xF0 and (b[3] & 0xF8) == 0xF8 and keeps those five bits, so neither neighbour (which
 *           would need 0xF8 at b[1], or 0xF0 at b[3]) converts: liblzma's extra i += 2 skips nothing, and the units
 *           are a map as well.
 *   x86     serial state: prev_mask (the last visited opcode bytes that did not convert) and prev_pos.  An E8 / E9
 *           byte with no E8 / E9 byte among the 5 bytes in front of it (a HEAD) is always visited -- what liblzma
 *           skips lies within 4 bytes behind a converted opcode -- and always sees prev_mask == 0, so heads cut the
 *           block into independent segments.  la_xz_x86_walk runs the serial step from a head (or from 0) and stops
 *           at the first head at or behind stop_from; a converted opcode at q rewrites q + 1 .. q + 4 and the next
 *           head is at q + 6 or later, so walks that start at different heads never touch each other's bytes.
 *           la_xz_x86_first_head finds heads from the bytes as they are BEFORE any walk.
 */
#ifndef LA_XZ_FILTERS_DEV_H
#define LA_XZ_FILTERS_DEV_H

#include "../../include/la_gpu.h"

#ifndef LA_XZ_FN
#define LA_XZ_FN static inline
#endif

#define LA_XZF_DELTA    0x03u
#define LA_XZF_X86      0x04u
#define LA_XZF_POWERPC  0x05u
#define LA_XZF_IA64     0x06u
#define LA_XZF_ARM      0x07u
#define LA_XZF_ARMTHUMB 0x08u
#define LA_XZF_SPARC    0x09u

/* start_offset's alignment; 0: not a BCJ filter of this file */
LA_XZ_FN uint32_t la_xz_bcj_align(uint32_t id)
{
	return id == LA_XZF_X86 ? 1u : id == LA_XZF_ARMTHUMB ? 2u : id == LA_XZF_IA64 ? 16u :
	    (id == LA_XZF_POWERPC || id == LA_XZF_ARM || id == LA_XZF_SPARC) ? 4u : 0u;
}

/* a chain entry the transforms below can run */
LA_XZ_FN int la_xz_filter_valid(uint32_t id, uint32_t prop)
{
	if (id == LA_XZF_DELTA)
		return prop >= 1u && prop <= 256u;
	const uint32_t a = la_xz_bcj_align(id);
	return a != 0u && (prop & (a - 1u)) == 0u;
}

LA_XZ_FN int la_xz_chain_valid(const la_xz_chain *ch)
{
	if (ch->count > LA_XZ_CHAIN_MAX)
		return 0;
	for (uint32_t k = 0; k < ch->count; k++)
		if (!la_xz_filter_valid(ch->id[k], ch->prop[k]))
			return 0;
	return 1;
}

/* ---- delta: the column c (= i mod dist) of the bytes [lo, hi), rows r0 .. r1 - 1 counted from lo rounded down to a
 * multiple of dist.  t holds the block's bytes from `base` on: byte i is t[i - base]. */
LA_XZ_FN uint32_t la_xz_delta_col_sum(const uint8_t *t, uint64_t base, uint64_t lo, uint64_t hi, uint32_t dist, uint32_t c, uint64_t r0, uint64_t r1)
{
	const uint64_t al = lo - lo % dist;
	uint32_t acc = 0;
	for (uint64_t r = r0; r < r1; r++) {
		const uint64_t i = al + r * dist + c;
		if (i >= lo && i < hi)
			acc += t[i - base];
	}
	return acc & 0xFFu;
}
LA_XZ_FN void la_xz_delta_col_apply(uint8_t *t, uint64_t base, uint64_t lo, uint64_t hi, uint32_t dist, uint32_t c, uint64_t r0, uint64_t r1, uint32_t carry)
{
	const uint64_t al = lo - lo % dist;
	uint32_t acc = carry;
	for (uint64_t r = r0; r < r1; r++) {
		const uint64_t i = al + r * dist + c;
		if (i >= lo && i < hi) {
			acc = (acc + t[i - base]) & 0xFFu;
			t[i - base] = (uint8_t)acc;
		}
	}
}
/* rows of the tile [lo, hi) */
LA_XZ_FN uint64_t la_xz_delta_rows(uint64_t lo, uint64_t hi, uint32_t dist)
{
	return hi > lo ? (hi - (lo - lo % dist) + dist - 1u) / dist : 0u;
}

/* ---- the units of the map filters: u points at the unit's first byte, pos is its position */
LA_XZ_FN void la_xz_unit_arm(uint8_t *u, uint32_t pos)
{
	if (u[3] != 0xEBu)
		return;
	uint32_t v = ((uint32_t)u[2] << 16) | ((uint32_t)u[1] << 8) | u[0];
	v = ((v << 2) - (pos + 8u)) >> 2;
	u[0] = (uint8_t)v; u[1] = (uint8_t)(v >> 8); u[2] = (uint8_t)(v >> 16);
}
LA_XZ_FN void la_xz_unit_powerpc(uint8_t *u, uint32_t pos)
{
	if ((u[0] >> 2) != 0x12u || (u[3] & 3u) != 1u)
		return;
	const uint32_t src = (((uint32_t)u[0] & 3u) << 24) | ((uint32_t)u[1] << 16) | ((uint32_t)u[2] << 8) | ((uint32_t)u[3] & ~3u);
	const uint32_t v = src - pos;
	u[0] = (uint8_t)(0x48u | ((v >> 24) & 3u)); u[1] = (uint8_t)(v >> 16); u[2] = (uint8_t)(v >> 8);
	u[3] = (uint8_t)((u[3] & 3u) | (v & 0xFCu));
}
LA_XZ_FN void la_xz_unit_sparc(uint8_t *u, uint32_t pos)
{
	if (!((u[0] == 0x40u && (u[1] & 0xC0u) == 0x00u) || (u[0] == 0x7Fu && (u[1] & 0xC0u) == 0xC0u)))
		return;
	uint32_t v = ((uint32_t)u[0] << 24) | ((uint32_t)u[1] << 16) | ((uint32_t)u[2] << 8) | u[3];
	v = ((v << 2) - pos) >> 2;
	v = (((0u - ((v >> 22) & 1u)) << 22) & 0x3FFFFFFFu) | (v & 0x3FFFFFu) | 0x40000000u;
	u[0] = (uint8_t)(v >> 24); u[1] = (uint8_t)(v >> 16); u[2] = (uint8_t)(v >> 8); u[3] = (uint8_t)v;
}
LA_XZ_FN void la_xz_unit_armthumb(uint8_t *u, uint32_t pos)
{
	if ((u[1] & 0xF8u) != 0xF0u || (u[3] & 0xF8u) != 0xF8u)
		return;
	uint32_t v = (((uint32_t)u[1] & 7u) << 19) | ((uint32_t)u[0] << 11) | (((uint32_t)u[3] & 7u) << 8) | u[2];
	v = ((v << 1) - (pos + 4u)) >> 1;
	u[1] = (uint8_t)(0xF0u | ((v >> 19) & 7u)); u[0] = (uint8_t)(v >> 11);
	u[3] = (uint8_t)(0xF8u | ((v >> 8) & 7u)); u[2] = (uint8_t)v;
}
LA_XZ_FN void la_xz_unit_ia64(uint8_t *u, uint32_t pos)
{
	/* which of the bundle's three 41-bit slots may hold a branch, by template: 0 below 16, then 4 4 6 6 0 0 7 7 4 4 0 0 4 4 0 0 */
	const uint32_t tmpl = u[0] & 0x1Fu;
	const uint32_t mask = tmpl < 16u ? 0u : (uint32_t)((0x0044004477006644ull >> ((tmpl - 16u) * 4u)) & 0xFu);
	uint32_t bit_pos = 5;
	for (uint32_t slot = 0; slot < 3u; slot++, bit_pos += 41u) {
		if (((mask >> slot) & 1u) == 0u)
			continue;
		const uint32_t byte_pos = bit_pos >> 3, bit_res = bit_pos & 7u;
		uint64_t ins = 0;
		for (uint32_t j = 0; j < 6u; j++)
			ins |= (uint64_t)u[byte_pos + j] << (8u * j);
		uint64_t norm = ins >> bit_res;
		if (((norm >> 37) & 0xFu) != 0x5u || ((norm >> 9) & 0x7u) != 0u)
			continue;
		uint32_t v = (uint32_t)((norm >> 13) & 0xFFFFFu);
		v |= (uint32_t)((norm >> 36) & 1u) << 20;
		v = ((v << 4) - pos) >> 4;
		norm &= ~((uint64_t)0x8FFFFFu << 13);
		norm |= (uint64_t)(v & 0xFFFFFu) << 13;
		norm |= (uint64_t)(v & 0x100000u) << (36 - 20);
		ins &= ((uint64_t)1 << bit_res) - 1u;
		ins |= norm << bit_res;
		for (uint32_t j = 0; j < 6u; j++)
			u[byte_pos + j] = (uint8_t)(ins >> (8u * j));
	}
}

/* size and stride of a map filter's units; 0: not a map filter */
LA_XZ_FN uint32_t la_xz_unit_bytes(uint32_t id)
{
	return id == LA_XZF_IA64 ? 16u : (id == LA_XZF_POWERPC || id == LA_XZF_ARM || id == LA_XZF_SPARC || id == LA_XZF_ARMTHUMB) ? 4u : 0u;
}
LA_XZ_FN uint32_t la_xz_unit_stride(uint32_t id)
{
	return id == LA_XZF_ARMTHUMB ? 2u : la_xz_unit_bytes(id);
}
/* the unit at byte i of the block (i a multiple of the stride, i + la_xz_unit_bytes(id) <= n) */
LA_XZ_FN void la_xz_unit(uint32_t id, uint8_t *buf, uint64_t i, uint32_t start_offset)
{
	const uint32_t pos = start_offset + (uint32_t)i;
	if (id == LA_XZF_ARM) la_xz_unit_arm(buf + i, pos);
	else if (id == LA_XZF_POWERPC) la_xz_unit_powerpc(buf + i, pos);
	else if (id == LA_XZF_SPARC) la_xz_unit_sparc(buf + i, pos);
	else if (id == LA_XZF_ARMTHUMB) la_xz_unit_armthumb(buf + i, pos);
	else if (id == LA_XZF_IA64) la_xz_unit_ia64(buf + i, pos);
}

/* ---- x86 */
LA_XZ_FN int la_xz_x86_op(uint32_t b) { return (b & 0xFEu) == 0xE8u; }
LA_XZ_FN int la_xz_x86_msb(uint32_t b) { return b == 0x00u || b == 0xFFu; }

/* The first head in [lo, hi): an opcode byte at i, i + 4 < n, with no opcode byte in [i - 5, i - 1].  n when there is
 * none.  Reads buf[lo - 5, hi) as the decoder left it. */
LA_XZ_FN uint64_t la_xz_x86_first_head(const uint8_t *buf, uint64_t n, uint64_t lo, uint64_t hi)
{
	if (n < 5u)
		return n;
	if (hi > n - 4u)
		hi = n - 4u;
	uint32_t clear = 5;	/* bytes without an opcode in front of i, capped at 5 */
	for (uint64_t k = lo < 5u ? lo : 5u; k > 0u; k--)
		clear = la_xz_x86_op(buf[lo - k]) ? 0u : (clear < 5u ? clear + 1u : 5u);
	for (uint64_t i = lo; i < hi; i++) {
		if (la_xz_x86_op(buf[i])) {
			if (clear >= 5u)
				return i;
			clear = 0u;
		} else if (clear < 5u) {
			clear++;
		}
	}
	return n;
}

/* liblzma's x86_code (decoder) from byte `from` -- 0 or a head -- to the first head at or behind stop_from, or the end */
LA_XZ_FN void la_xz_x86_walk(uint8_t *buf, uint64_t n, uint32_t start_offset, uint64_t from, uint64_t stop_from)
{
	if (n < 5u)
		return;
	const uint64_t limit = n - 5u;
	uint32_t prev_mask = 0u;
	uint32_t prev_pos = start_offset + (uint32_t)from - 5u;
	uint64_t i = from;
	uint64_t last_op = 0;	/* one behind the last opcode byte of the undecoded data in front of i; 0: none since `from` */
	while (i <= limit) {
		if (!la_xz_x86_op(buf[i])) {
			i++;
			continue;
		}
		if (i >= stop_from && (last_op == 0u || i - (last_op - 1u) > 5u) && i != from)
			return;		/* a head: another walk's */
		const uint32_t p = start_offset + (uint32_t)i;
		const uint32_t off = p - prev_pos;
		prev_pos = p;
		if (off > 5u)
			prev_mask = 0u;
		else
			for (uint32_t k = 0; k < off; k++)
				prev_mask = (prev_mask & 0x77u) << 1;
		last_op = i + 1u;
		const uint32_t b1 = buf[i + 1], b2 = buf[i + 2], b3 = buf[i + 3], b4 = buf[i + 4];
		if (la_xz_x86_msb(b4) && ((0x17u >> ((prev_mask >> 1) & 7u)) & 1u) && (prev_mask >> 1) < 0x10u) {
			uint32_t src = (b4 << 24) | (b3 << 16) | (b2 << 8) | b1, dest;
			for (;;) {
				dest = src - (p + 5u);
				if (prev_mask == 0u)
					break;
				const uint32_t k = (0xFFA4u >> (2u * ((prev_mask >> 1) & 7u))) & 3u;	/* 0 1 2 2 3 3 3 3 */
				if (!la_xz_x86_msb((dest >> (24u - k * 8u)) & 0xFFu))
					break;
				src = dest ^ (uint32_t)(((uint64_t)1 << (32u - k * 8u)) - 1u);
			}
			if (la_xz_x86_op(b4)) last_op = i + 5u;
			else if (la_xz_x86_op(b3)) last_op = i + 4u;
			else if (la_xz_x86_op(b2)) last_op = i + 3u;
			else if (la_xz_x86_op(b1)) last_op = i + 2u;
			buf[i + 4] = (uint8_t)(0u - ((dest >> 24) & 1u));
			buf[i + 3] = (uint8_t)(dest >> 16);
			buf[i + 2] = (uint8_t)(dest >> 8);
			buf[i + 1] = (uint8_t)dest;
			i += 5u;
			prev_mask = 0u;
		} else {
			i++;
			prev_mask |= 1u;
			if (la_xz_x86_msb(b4))
				prev_mask |= 0x10u;
		}
	}
}

/* ---- one filter over a whole block, serially */
LA_XZ_FN void la_xz_unfilter_serial(uint32_t id, uint32_t prop, uint8_t *buf, uint64_t n)
{
	if (id == LA_XZF_DELTA) {
		for (uint64_t i = prop; i < n; i++)
			buf[i] = (uint8_t)(buf[i] + buf[i - prop]);
	} else if (id == LA_XZF_X86) {
		la_xz_x86_walk(buf, n, prop, 0u, n);
	} else {
		const uint32_t ub = la_xz_unit_bytes(id), us = la_xz_unit_stride(id);
		if (ub == 0u)
			return;
		for (uint64_t i = 0; i + ub <= n; i += us)
			la_xz_unit(id, buf, i, prop);
	}
}

/* a whole chain over a block: the filters in reverse chain order */
LA_XZ_FN void la_xz_unchain_serial(const la_xz_chain *ch, uint8_t *buf, uint64_t n)
{
	for (uint32_t k = ch->count; k > 0u; k--)
		la_xz_unfilter_serial(ch->id[k - 1u], ch->prop[k - 1u], buf, n);
}

#endif
