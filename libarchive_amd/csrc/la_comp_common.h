/*
 * la_comp_common.h -- device code the compressors share (la_lz4_comp.hip, la_deflate_comp.hip, la_zstd_comp.hip,
 * la_lzo_comp.hip): small load / copy / store helpers, wave reductions, the LZ77 window matcher of the lz4, zstd and lzop block kernels,
 * the wave bit-stream appender of the deflate and Huffman encoders and the per-frame checksum kernel.  (The launchers'
 * workspace carver, la_carve, comes with la_dev.h.)
 */
#ifndef LA_COMP_COMMON_H
#define LA_COMP_COMMON_H

#include "la_dev.h"

#define LZ77_HASH_BITS 12	/* 4096-entry match tables */

__device__ __forceinline__ uint64_t ld_u64(const uint8_t *p)
{
	uint64_t v;
	__builtin_memcpy(&v, p, 8);
	return v;
}

/* wave-cooperative byte copy, n uniform */
__device__ __forceinline__ void wave_copy(uint8_t *d, const uint8_t *s, uint32_t n, uint32_t lane)
{
	for (uint32_t i = lane; i < n; i += 64)
		d[i] = s[i];
}

__device__ __forceinline__ void st_le32(uint8_t *p, uint32_t v)
{
	p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24);
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
#pragma unroll
	for (int d = 1; d < 64; d <<= 1)
		v += (uint32_t)__shfl_xor((int)v, d, 64);
	return v;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v)
{
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
		const uint32_t o = (uint32_t)__shfl_xor((int)v, d, 64);
		v = o > v ? o : v;
	}
	return v;
}

/* LZ77 matching of one block by one wave.  The wave looks at 64 consecutive positions at a time: every lane hashes
 * the four bytes at its position, takes the table's candidate (from an earlier window), replaces it, verifies the
 * candidate and extends the match eight bytes at a time, then byte by byte.  The wave then takes the matches in
 * position order (ballot + first set bit), skipping the ones an earlier match has covered, and calls
 * emit(pf, mf, cf, anchor) for each: match position, length, candidate position and the first position not yet
 * emitted.  Matches start at or before `plast` and end at or before `mend`; a candidate further back than `max_dist`
 * (the format's longest distance, where a block is longer than that) is not taken.  `tab` holds 2^LZ77_HASH_BITS
 * positions (T: uint16_t or uint32_t), zeroed.  Returns the first position no match covers. */
template <typename T, typename Emit>
__device__ __forceinline__ uint32_t lz77_match(T *tab, const uint8_t *in, uint32_t plast, uint32_t mend, uint32_t lane,
    Emit emit, uint32_t max_dist = 0xFFFFFFFFu)
{
	uint32_t anchor = 0, base = 0;	/* wave-uniform */
	while (base <= plast) {
		const uint32_t p = base + lane;
		const bool valid = p <= plast;
		uint32_t v = 0, cand = 0, mlen = 0;
		bool ok = false;
		if (valid) {
			v = ld_u32(in + p);
			const uint32_t h = (v * 2654435761u) >> (32 - LZ77_HASH_BITS);
			cand = tab[h];		/* every lane reads before any lane of this window writes */
		}
		__builtin_amdgcn_wave_barrier();
		if (valid) {
			const uint32_t h = (v * 2654435761u) >> (32 - LZ77_HASH_BITS);
			tab[h] = (T)p;
			/* (position 0 doubles as "empty": a candidate is only taken if its bytes match) */
			ok = cand < p && p - cand <= max_dist && ld_u32(in + cand) == v;
			if (ok) {
				mlen = 4;
				while (p + mlen + 8u <= mend && ld_u64(in + p + mlen) == ld_u64(in + cand + mlen))
					mlen += 8;
				while (p + mlen < mend && in[p + mlen] == in[cand + mlen])
					mlen++;
			}
		}
		uint64_t mask = __ballot(ok);
		while (mask != 0) {
			const uint32_t f = (uint32_t)__builtin_ctzll(mask);
			mask &= mask - 1;
			const uint32_t pf = base + f;
			if (pf < anchor)
				continue;	/* an earlier match of this window already covers it */
			const uint32_t mf = (uint32_t)__builtin_amdgcn_readlane((int)mlen, (int)f);
			const uint32_t cf = (uint32_t)__builtin_amdgcn_readlane((int)cand, (int)f);
			emit(pf, mf, cf, anchor);
			anchor = pf + mf;
		}
		base = (base + 64 > anchor) ? base + 64 : anchor;
	}
	return anchor;
}

/* Appends one token per lane -- `nb` bits of `bits`, nb = 0 for none -- to an LSB-first bit stream at the
 * wave-uniform bit position bp, in lane order.  A wave prefix sum of the bit counts gives every token its place,
 * lanes OR their bits into the LDS stage (whose dword 0 holds the stream's partial last dword, the rest zero), and
 * whole dwords leave through store(i, dword), i = the dword's index in the stream; the new partial one stays in
 * stage[0].  The stage holds at least one dword more than 64 tokens can fill.  Returns the bits appended. */
template <uint32_t N, typename Store>
__device__ __forceinline__ uint32_t wave_bits_append(uint64_t bp, uint32_t bits, uint32_t nb, uint32_t (&stage)[N],
    uint32_t lane, Store store)
{
	uint32_t inc = nb;
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
		const uint32_t t = __shfl_up(inc, d, 64);
		if ((int)lane >= d) inc += t;
	}
	const uint32_t total = __shfl(inc, 63, 64);
	const uint32_t at = (uint32_t)(bp & 31u) + inc - nb;	/* bit offset inside the stage */
	if (nb) {
		const uint64_t w = (uint64_t)bits << (at & 31u);
		atomicOr(&stage[at >> 5], (uint32_t)w);
		if ((uint32_t)(w >> 32))
			atomicOr(&stage[(at >> 5) + 1], (uint32_t)(w >> 32));
	}
	__builtin_amdgcn_wave_barrier();
	/* whole dwords leave; the partial last one stays as the next step's first */
	const uint32_t nd = ((uint32_t)(bp & 31u) + total) >> 5;
	const uint32_t g0 = (uint32_t)(bp >> 5);
	uint32_t mine = 0;
	const uint32_t carry = stage[nd];
	if (lane < nd)
		mine = stage[lane];
	__builtin_amdgcn_wave_barrier();
	if (lane < nd)
		store(g0 + lane, mine);
	if (lane <= nd && lane < N)
		stage[lane] = 0;
	if (N > 64 && nd >= 64 && lane == 0)	/* (at most 64 * 31 + 31 bits: dword 64 can only be the partial one) */
		stage[64] = 0;
	__builtin_amdgcn_wave_barrier();
	if (lane == 0)
		stage[0] = carry;
	__builtin_amdgcn_wave_barrier();
	return total;
}

/* content checksum of every frame (frame_bytes of input each, the last one shorter), four lanes per frame;
 * QuadHash()(p, len, j) is a hash computed by the four lanes j = 0..3 of a quad, valid in lane 0 */
template <typename QuadHash>
__global__ __launch_bounds__(64) void frame_sums_kernel(const uint8_t *__restrict__ src, uint64_t src_bytes,
    uint64_t frame_bytes, uint32_t n_frames, uint32_t *__restrict__ frame_sum)
{
	const uint32_t q = (blockIdx.x * 64 + threadIdx.x) >> 2, j = threadIdx.x & 3u;
	const bool have = q < n_frames;
	const uint64_t fo = have ? (uint64_t)q * frame_bytes : 0;
	const uint64_t fl = have && src_bytes > fo ? (src_bytes - fo < frame_bytes ? src_bytes - fo : frame_bytes) : 0;
	const uint32_t h = QuadHash()(src + fo, fl, j);
	if (have && j == 0)
		frame_sum[q] = h;
}

#endif /* LA_COMP_COMMON_H */
