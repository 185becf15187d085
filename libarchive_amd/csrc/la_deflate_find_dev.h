/*
 * la_deflate_find_dev.h -- which bit positions of a raw-deflate stream are CANDIDATES for the start of a block,
 * stated ONCE: the finder kernels (la_inflate_find.hip), the rules test (tests/test_deflate_find_rules.py) and its
 * sanitizer program (tests/deflate_find/) all compile this file.  It compiles for the device (hipcc, after la_dev.h) and
 * for the host (any C++ compiler: the qualifiers of la_deflate_dev.h are defined away below).
 *
 * The rule.  Bit position p of a span of `end` bits is a candidate when the bits from p on read as the header of a
 * NON-FINAL DYNAMIC block that zlib 1.2.11 would accept, every bit of that header inside the span:
 *   BFINAL 0, BTYPE 10;
 *   dfl_dynamic_header (la_deflate_dev.h) answers LA_ST_OK: HLIT <= 29, HDIST <= 29, a complete code-length code, the
 *   HLIT + 257 + HDIST + 1 code lengths read without an unassigned code, a repeat with nothing before it or a repeat
 *   past the end, and lens[256] != 0;
 *   dfl_code_verdict accepts the literal/length code and the distance code.
 * Stored and fixed blocks are never candidates (their headers are 3 bits, or 3 bits and a 32-bit word that is right by
 * chance once in 65 536 positions -- no evidence): a piece runs over them.  A final block is never a candidate: the
 * piece in front of it decodes it, and nothing starts behind it.
 *
 * The rule never misses a true non-final dynamic block start whose header lies inside the span: the decoder reads that
 * header through the same dfl_dynamic_header and dfl_code_verdict, so a header the decoder accepts is a candidate.
 * It is NOT trusted the other way: a position inside a block, or inside stored data, may read as a perfect header.
 * Only the confirming walk (la_inflate_find.hip) decides, by whether a confirmed piece ended exactly there.
 *
 * Two forms.  dfl_find_quick is the part that needs no loop over the stream: the 17 bits BFINAL .. HCLEN and the up to
 * 57 bits of code-length-code lengths (Kraft sum of a complete code: exactly 1).  It is necessary, not sufficient; one
 * position in about 2 200 of random bits passes it.  dfl_find_full is the rule, over a bounded byte reader that keeps
 * no table: the code-length code lives in three 64-bit words, and of the two codes it reads only what their verdicts
 * need -- the Kraft sum, the longest length, and lens[256].  (A code of lengths l_i is over-subscribed exactly when
 * sum 2^(15 - l_i) > 2^15 and incomplete exactly when it is smaller: the builders' `left`, scaled.)
 */
#ifndef LA_DEFLATE_FIND_DEV_H
#define LA_DEFLATE_FIND_DEV_H

#include <stdint.h>
#include "../../include/la_gpu.h"

#ifndef __HIPCC__
#ifndef __device__
#define __device__
#endif
#ifndef __constant__
#define __constant__ const
#endif
#ifndef __forceinline__
#define __forceinline__ inline
#endif
#endif
#include "la_deflate_dev.h"

#define DFL_FIND_QUICK_BITS 74u		/* 17 + 3 * 19: what dfl_find_quick may look at behind a position */

/* hdr: the 17 bits at the position (first bit lowest); clc: the 57 bits behind them.  Returns the bits the quick part
 * of the header occupies (17 + 3 * ncode, at most DFL_FIND_QUICK_BITS) when it passes, 0 when the position is out. */
__device__ __forceinline__ uint32_t dfl_find_quick(uint32_t hdr, uint64_t clc)
{
	if ((hdr & 7u) != 4u)		/* BFINAL 0, BTYPE 10 (first bit lowest: 0, then 0 1) */
		return 0;
	if (((hdr >> 3) & 31u) > 29u || ((hdr >> 8) & 31u) > 29u)
		return 0;
	const uint32_t ncode = ((hdr >> 13) & 15u) + 4u;
	uint32_t kraft = 0;
	for (uint32_t i = 0; i < ncode; i++) {
		const uint32_t l = (uint32_t)(clc >> (3u * i)) & 7u;
		kraft += l ? 128u >> l : 0u;
	}
	return kraft == 128u ? 17u + 3u * ncode : 0u;
}

/* the reader of la_deflate_dev.h over bytes base[0 .. (end + 7) / 8), bit cursor pos, no bit at or behind `end` read */
struct dfl_find_reader {
	const uint8_t *base;
	uint64_t pos, end;
	int *nlen;		/* dfl_dynamic_header's: set before the first code length is stored */
	uint64_t clens;		/* code-length-code lengths, 3 bits per symbol */
	uint64_t counts;	/* codes per length 1..7, 8 bits each */
	uint64_t sym_lo, sym_hi;	/* the symbols sorted by (length, symbol), 5 bits each: 12 and 7 */
	uint32_t clmax;
	int built;
	uint32_t ll_kraft, d_kraft, ll_max, d_max, len256;

	__device__ __forceinline__ bool take(uint32_t n, uint32_t &v)
	{
		if (pos + n > end)
			return false;
		/* (n <= 32 bits from bit pos & 7 on: at most five bytes, none behind the byte of the last bit asked for) */
		const uint64_t first = pos >> 3, last = (pos + n - 1) >> 3;
		uint64_t acc = 0;
		for (uint64_t k = first; k <= last && n != 0; k++)
			acc |= (uint64_t)base[k] << (8u * (uint32_t)(k - first));
		v = n == 0 ? 0u : (uint32_t)((acc >> (pos & 7u)) & ((1ull << n) - 1ull));
		pos += n;
		return true;
	}
	__device__ __forceinline__ void to_byte() { pos = (pos + 7u) & ~(uint64_t)7u; }
	__device__ __forceinline__ void store(uint32_t idx, uint32_t val, uint32_t rep)
	{
		if (!built) {
			for (uint32_t k = idx; k < idx + rep && k < 19u; k++)
				clens = (clens & ~(7ull << (3u * k))) | ((uint64_t)(val & 7u) << (3u * k));
			return;
		}
		const uint32_t nl = (uint32_t)*nlen;
		const uint32_t in_ll = idx >= nl ? 0u : (idx + rep <= nl ? rep : nl - idx);
		const uint32_t in_d = rep - in_ll;
		if (val != 0 && in_ll != 0) {
			ll_kraft += in_ll << (15u - val);
			if (val > ll_max) ll_max = val;
		}
		if (val != 0 && in_d != 0) {
			d_kraft += in_d << (15u - val);
			if (val > d_max) d_max = val;
		}
		if (idx <= 256u && 256u < idx + rep)
			len256 = val;
	}
	__device__ __forceinline__ uint32_t len_at(uint32_t idx) { return idx == 256u ? len256 : 0u; }
	__device__ __forceinline__ int clc_build(uint32_t &maxlen)
	{
		uint32_t kraft = 0, nsym = 0;
		counts = 0; sym_lo = 0; sym_hi = 0; clmax = 0;
		for (uint32_t l = 1; l <= 7u; l++)
			for (uint32_t s = 0; s < 19u; s++) {
				if (((uint32_t)(clens >> (3u * s)) & 7u) != l)
					continue;
				kraft += 128u >> l;
				counts += 1ull << (8u * l);
				clmax = l;
				if (nsym < 12u) sym_lo |= (uint64_t)s << (5u * nsym);
				else sym_hi |= (uint64_t)s << (5u * (nsym - 12u));
				nsym++;
			}
		built = 1;
		maxlen = clmax;
		return 128 - (int)kraft;
	}
	__device__ __forceinline__ int clc_sym()
	{
		uint32_t code = 0, first = 0, index = 0;
		const uint32_t ml = clmax ? clmax : 1u;
		for (uint32_t k = 1; k <= ml; k++) {
			uint32_t bit;
			if (!take(1, bit))
				return -1;
			code |= bit;
			const uint32_t cn = (uint32_t)(counts >> (8u * k)) & 255u;
			if (code < first + cn) {
				const uint32_t at = index + (code - first);
				return (int)((at < 12u ? sym_lo >> (5u * at) : sym_hi >> (5u * (at - 12u))) & 31u);
			}
			index += cn;
			first = (first + cn) << 1;
			code <<= 1;
		}
		return -2;
	}
};

/* the rule: is bit position p of the span base[0 .. (end_bits + 7) / 8) a candidate */
__device__ __forceinline__ bool dfl_find_full(const uint8_t *base, uint64_t p, uint64_t end_bits)
{
	int nlen = 0, ndist = 0;
	dfl_find_reader r = { base, p, end_bits, &nlen, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 };
	uint32_t v;
	if (!r.take(3, v) || v != 4u)
		return false;
	if (dfl_dynamic_header(r, nlen, ndist) != LA_ST_OK)
		return false;
	if (dfl_code_verdict(32768 - (int)r.ll_kraft, r.ll_max, DFL_CODE_LITLEN) != LA_ST_OK)
		return false;
	return dfl_code_verdict(32768 - (int)r.d_kraft, r.d_max, DFL_CODE_DIST) == LA_ST_OK;
}

#endif
