/*
 * la_bzip2_comp.hip -- bzip2 compression on the device (la_gpu_bzip2_compress), written from the format.
 *
 * The input is cut every block_bytes(level) = 4 * ((100000 * level - 19) / 5) bytes.  The first run-length stage
 * (RLE1) turns four equal bytes into five at worst, so a cut of that size always fits the format's limit of
 * 100000 * level - 19 symbols per block: no cut depends on the data and every block starts at a known offset.  libbz2
 * fills each block up to the limit instead, so on input that RLE1 does not expand its blocks are up to a quarter
 * longer and its ratio a little better: that is the price of the fixed cut.  RLE1 restarts at every cut.
 *
 * Stages, all window-wide (every block of the call at once):
 *   rle1      one workgroup per block: run starts by a max-scan over thread chunks, counts, then bytes; block CRC by
 *             per-thread CRCs combined in GF(2); the 256 "byte in use" flags (of the RLE1 bytes, counts included).  The RLE1 bytes of all blocks lie back
 *             to back (offs[b]).
 *   sort      Burrows-Wheeler sort of all blocks in ONE segmented sort over the whole window: prefix doubling over
 *             (rank[i], rank[(i + h) mod n]) pairs, the rank being global (block base + rank inside the block), so one
 *             stable LSD radix sort per round (8-bit digits, one wave per 2048-key tile, ballot ranking) orders every
 *             block at once and keeps every CU busy at any level.  Round 0 sorts by (block, byte); round r compares
 *             2^r bytes; a round in which all ranks come out distinct ends the sort (the later launches return at
 *             once), so there are at most ceil(log2 n) + 1 rounds whatever the data.  Equal rotations stay tied;
 *             origPtr is the row of rotation 0 itself.
 *   mtf       one workgroup per block: 1024-byte chunks; a chunk's effect on the recency list is its distinct bytes
 *             latest first; one wave composes them in order (the scan), then every chunk is re-run from its true
 *             start list.  Zero runs become RUNA / RUNB (bijective base 2), a run open at the end is flushed, then
 *             the end-of-block symbol.
 *   code      one workgroup per block: 2..6 tables by symbol count, groups of 50, four refinement passes; Huffman
 *             code lengths, one wave per table, rebuilt from halved counts while deeper than 17 (the count halving of
 *             la_deflate_comp.hip's and bzip2's own limiters; every symbol of the alphabet gets a length); selectors
 *             move-to-front coded in unary; the exact size is then known, and a block whose fitted coding would pass
 *             the flat one's bound is written with two flat tables (lengths ceil(log2 alphabet) and one less): the
 *             bound of bz2c_block_bits() holds by construction.
 *             Bits go through wave_bits_append (LSB-first dwords, codes bit-reversed; the pack turns the bytes round).
 *   link      one thread: bit offsets of the pieces (pending bits of *d_state or the stream header, the blocks, the
 *             trailer), the combined CRC, the new *d_state.
 *   pack      output driven: one thread per 16 bytes of d_out finds its source pieces in the offset table and
 *             funnel-shifts; no byte has two writers.
 */
#include "la_comp_common.h"

#define BZC_TPB       256u
#define BZC_TILE      2048u	/* keys per wave in the radix passes */
#define BZC_SCAN_TILE 2048u	/* keys per workgroup in the head scan */
#define BZC_CHUNK     1024u	/* BWT bytes per MTF chunk */
#define BZC_MTF_TPB   128u
#define BZC_CODE_TPB  1024u
#define BZC_GROUP     50u
#define BZC_MAXSEL    18002u
#define BZC_MAXLEN    17u
#define BZC_ALPHA_MAX 258u
#define BZC_ROUNDS    32u

struct bz2c_ctl {
	uint32_t nd[BZC_ROUNDS];	/* round r left equal keys behind */
	uint64_t total_bits;
	uint64_t out_bytes;
};

/* ---- sizes, shared by host and device ---- */
__host__ __device__ __forceinline__ uint32_t bz2c_block_bytes(uint32_t level) { return 4u * ((100000u * level - 19u) / 5u); }
__host__ __device__ __forceinline__ uint32_t bz2c_rle_max(uint32_t len) { return len + len / 4u; }
/* Most bits a block of `len` input bytes takes.  48 magic + 32 CRC + 1 + 24 origPtr + 16 + 256 map = 377; 3 + 15 for
 * the table and selector counts.  The flat fallback has two tables and every selector 0: one bit per selector (one per
 * 50 symbols, at most 18002); a flat table is 5 bits, one bit per symbol and one two-bit step where the length drops
 * (at most 258 + 2 + 5 = 265 each); the symbols, at most bz2c_rle_max(len) + 1 with the end-of-block, take at most
 * ceil(log2 258) = 9 bits each.  A fitted coding is written only if it is no longer than this. */
__host__ __device__ __forceinline__ uint64_t bz2c_block_bits(uint32_t len)
{
	const uint64_t nsym = (uint64_t)bz2c_rle_max(len) + 1u;
	return 377u + 18u + (nsym + BZC_GROUP - 1u) / BZC_GROUP + 2u * 265u + 9u * nsym;
}
__host__ __device__ __forceinline__ uint32_t bz2c_stride_words(uint32_t level)
{
	return (uint32_t)((bz2c_block_bits(bz2c_block_bytes(level)) + 31u) / 32u) + 4u;
}

/* ---- small helpers ---- */
__device__ __forceinline__ uint32_t bz2c_rev(uint32_t v, uint32_t n) { return n ? __builtin_bitreverse32(v) >> (32u - n) : 0u; }

/* block-wide inclusive scans of one value per thread (TPB threads, `tmp` holds TPB words) */
template <uint32_t TPB, bool MAX>
__device__ __forceinline__ uint32_t bz2c_block_scan(uint32_t v, uint32_t *tmp, uint32_t *total)
{
	const uint32_t t = threadIdx.x;
	tmp[t] = v;
	__syncthreads();
	for (uint32_t d = 1; d < TPB; d <<= 1) {
		const uint32_t o = t >= d ? tmp[t - d] : 0u;
		__syncthreads();
		if (t >= d)
			tmp[t] = MAX ? (o > tmp[t] ? o : tmp[t]) : tmp[t] + o;
		__syncthreads();
	}
	const uint32_t r = tmp[t];
	*total = tmp[TPB - 1];
	__syncthreads();
	return r;
}

/* block that holds element i of the back-to-back layout: offs[b] <= i < offs[b + 1] (empty blocks are skipped) */
__device__ __forceinline__ uint32_t bz2c_find_block(const uint32_t *offs, uint32_t nb, uint32_t i)
{
	uint32_t lo = 0, hi = nb;	/* answer in [lo, hi) */
	while (hi - lo > 1u) {
		const uint32_t mid = (lo + hi) >> 1;
		if (offs[mid] <= i) lo = mid; else hi = mid;
	}
	return lo;
}

/* CRC: MSB-first polynomial 0x04C11DB7, as la_bzip2.hip has it */
__device__ __forceinline__ uint32_t bz2c_mulmod(uint32_t a, uint32_t b)
{
	uint32_t r = 0;
	for (int i = 31; i >= 0; i--) {
		r = (r << 1) ^ ((r & 0x80000000u) ? 0x04C11DB7u : 0u);
		if ((b >> i) & 1u) r ^= a;
	}
	return r;
}
__device__ __forceinline__ uint32_t bz2c_shift_bytes(uint32_t a, uint32_t bytes, const uint32_t *pw)
{
	for (uint32_t k = 0; bytes; k++, bytes >>= 1)
		if (bytes & 1u) a = bz2c_mulmod(a, pw[k]);
	return a;
}

/* ------------------------------------------------------------------ RLE1 */

/* one workgroup per block.  WRITE = false: n_rle[b], crc[b], used[b]; WRITE = true: the bytes at rle + offs[b] */
template <bool WRITE>
__global__ __launch_bounds__(BZC_TPB) void bz2c_rle1_kernel(const uint8_t *__restrict__ src, uint64_t src_bytes, uint32_t bb,
    uint32_t *__restrict__ n_rle, uint32_t *__restrict__ crc_out, uint32_t *__restrict__ used, const uint32_t *__restrict__ offs,
    uint8_t *__restrict__ rle)
{
	__shared__ uint32_t tmp[BZC_TPB], tab[256], pw[32], uflag[8], r_crc[BZC_TPB], r_len[BZC_TPB];
	const uint32_t b = blockIdx.x, t = threadIdx.x;
	const uint64_t so = (uint64_t)b * bb;
	const uint32_t L = (uint32_t)(src_bytes - so < bb ? src_bytes - so : bb);
	const uint8_t *in = src + so;
	const uint32_t per = (L + BZC_TPB - 1u) / BZC_TPB;
	const uint32_t c0 = t * per < L ? t * per : L, c1 = c0 + per < L ? c0 + per : L;
	if (!WRITE) {
		uint32_t c = t << 24;
		for (int k = 0; k < 8; k++)
			c = (c << 1) ^ ((c & 0x80000000u) ? 0x04C11DB7u : 0u);
		tab[t] = c;
		if (t < 8) uflag[t] = 0;
		if (t == 0) {
			pw[0] = 0x100u;
			for (int k = 1; k < 32; k++)
				pw[k] = bz2c_mulmod(pw[k - 1], pw[k - 1]);
		}
	}
	/* the last run start of every chunk (index + 1, 0 = none), then the one in front of every chunk */
	uint32_t ls = 0;
	for (uint32_t i = c1; i > c0; i--)
		if (i - 1u == 0 || in[i - 1u] != in[i - 2u]) { ls = i; break; }
	uint32_t tot;
	/* run start of the byte at c0: exclusive maximum, unless c0 starts a run itself */
	__shared__ uint32_t lsv[BZC_TPB];
	lsv[t] = ls;
	__syncthreads();
	uint32_t rs = 0;
	{	/* (exclusive max by a second scan of the shifted values) */
		const uint32_t prev = t ? lsv[t - 1] : 0u;
		const uint32_t ex = bz2c_block_scan<BZC_TPB, true>(prev, tmp, &tot);
		rs = ex ? ex - 1u : 0u;
	}
	/* count (and take the CRC), or write */
	uint32_t cnt = 0, crc = 0, j = 0;
	for (int pass = 0; pass < (WRITE ? 2 : 1); pass++) {
		uint32_t out = 0;
		if (WRITE && pass == 1) {
			const uint32_t inc = bz2c_block_scan<BZC_TPB, false>(cnt, tmp, &tot);
			out = offs[b] + inc - cnt;
		}
		uint32_t n = 0;
		if (c0 < c1)
			j = (c0 - rs) % 255u;
		for (uint32_t i = c0; i < c1; i++) {
			const uint32_t ch = in[i];
			if (i == 0 || in[i - 1u] != ch)
				j = 0;
			const bool last = j == 254u || i + 1u == L || in[i + 1u] != ch;
			if (j < 4u) {
				if (WRITE && pass == 1) rle[out++] = (uint8_t)ch;
				n++;
			}
			if (last && j >= 3u) {
				if (WRITE && pass == 1) rle[out++] = (uint8_t)(j - 3u);
				if (!WRITE) atomicOr(&uflag[(j - 3u) >> 5], 1u << ((j - 3u) & 31u));	/* a count is a byte of the block too */
				n++;
			}
			if (!WRITE) {
				crc = (crc << 8) ^ tab[(crc >> 24) ^ ch];
				atomicOr(&uflag[ch >> 5], 1u << (ch & 31u));
			}
			j = j == 254u ? 0u : j + 1u;
		}
		cnt = n;
	}
	if (WRITE)
		return;
	const uint32_t inc = bz2c_block_scan<BZC_TPB, false>(cnt, tmp, &tot);
	(void)inc;
	r_crc[t] = crc; r_len[t] = c1 - c0;
	__syncthreads();
	for (uint32_t d = 1; d < BZC_TPB; d <<= 1) {
		if ((t & (2u * d - 1u)) == 0) {
			const uint32_t lb = r_len[t + d];
			r_crc[t] = bz2c_shift_bytes(r_crc[t], lb, pw) ^ r_crc[t + d];
			r_len[t] += lb;
		}
		__syncthreads();
	}
	if (t == 0) {
		n_rle[b] = tot;
		crc_out[b] = ~(r_crc[0] ^ bz2c_shift_bytes(0xFFFFFFFFu, L, pw));
	}
	if (t < 8)
		used[b * 8u + t] = uflag[t];
}

__global__ void bz2c_offsets_kernel(const uint32_t *__restrict__ n_rle, uint32_t nb, uint32_t *__restrict__ offs)
{
	uint32_t o = 0;
	for (uint32_t b = 0; b < nb; b++) {
		offs[b] = o;
		o += n_rle[b];
	}
	offs[nb] = o;
}

/* ------------------------------------------------------------------ the sort */

/* round 0: keys (block, byte); rounds r >= 1: (rank[i], rank[(i + h) mod n]) of the order the last round left in
 * sa_in.  Keys and order go to key_out / sa_out (the same buffers as sa_in when the parity says so). */
__global__ __launch_bounds__(BZC_TPB) void bz2c_keys_kernel(const bz2c_ctl *__restrict__ ctl, uint32_t round, uint32_t h, uint32_t B,
    const uint32_t *__restrict__ offs, const uint32_t *__restrict__ n_rle, uint32_t nb, const uint8_t *__restrict__ rle,
    const uint32_t *__restrict__ rank, const uint32_t *sa_in, uint32_t *sa_out, uint64_t *__restrict__ key_out)
{
	if (round && ctl->nd[round - 1u] == 0)
		return;
	const uint32_t N = offs[nb];
	const uint32_t jdx = blockIdx.x * BZC_TPB + threadIdx.x;
	if (jdx >= N)
		return;
	if (round == 0) {
		const uint32_t b = bz2c_find_block(offs, nb, jdx);
		sa_out[jdx] = jdx;
		key_out[jdx] = ((uint64_t)b << 8) | rle[jdx];
		return;
	}
	const uint32_t i = sa_in[jdx];
	const uint32_t b = bz2c_find_block(offs, nb, i);
	const uint32_t o = offs[b], n = n_rle[b];
	const uint32_t i2 = o + (uint32_t)(((uint64_t)(i - o) + h) % n);
	sa_out[jdx] = i;
	key_out[jdx] = ((uint64_t)rank[i] << B) | rank[i2];
}

/* radix pass, first half: digit counts of every tile, hist[digit * tiles + tile] */
__global__ __launch_bounds__(BZC_TPB) void bz2c_hist_kernel(const bz2c_ctl *__restrict__ ctl, uint32_t round, const uint32_t *__restrict__ offs,
    uint32_t nb, const uint64_t *__restrict__ key, uint32_t shift, uint32_t tiles, uint32_t *__restrict__ hist)
{
	__shared__ uint32_t cnt[BZC_TPB / 64u][256];
	if (round && ctl->nd[round - 1u] == 0)
		return;
	const uint32_t N = offs[nb];
	const uint32_t w = threadIdx.x >> 6, lane = threadIdx.x & 63u;
	const uint32_t tile = blockIdx.x * (BZC_TPB / 64u) + w;
	for (uint32_t d = lane; d < 256u; d += 64u)
		cnt[w][d] = 0;
	__syncthreads();
	if (tile < tiles) {
		const uint32_t base = tile * BZC_TILE;
		for (uint32_t it = 0; it < BZC_TILE / 64u; it++) {
			const uint32_t idx = base + it * 64u + lane;
			if (idx < N)
				atomicAdd(&cnt[w][(uint32_t)(key[idx] >> shift) & 255u], 1u);
		}
	}
	__syncthreads();
	if (tile < tiles)
		for (uint32_t d = lane; d < 256u; d += 64u)
			hist[d * tiles + tile] = cnt[w][d];
}

/* radix pass, second half: stable scatter.  The wave ranks its 64 keys by digit with ballots, in index order. */
__global__ __launch_bounds__(BZC_TPB) void bz2c_scatter_kernel(const bz2c_ctl *__restrict__ ctl, uint32_t round, const uint32_t *__restrict__ offs,
    uint32_t nb, const uint64_t *__restrict__ key, const uint32_t *__restrict__ sa, uint32_t shift, uint32_t tiles,
    const uint64_t *__restrict__ hscan, uint64_t *__restrict__ key_out, uint32_t *__restrict__ sa_out)
{
	__shared__ uint32_t base[BZC_TPB / 64u][256];
	if (round && ctl->nd[round - 1u] == 0)
		return;
	const uint32_t N = offs[nb];
	const uint32_t w = threadIdx.x >> 6, lane = threadIdx.x & 63u;
	const uint32_t tile = blockIdx.x * (BZC_TPB / 64u) + w;
	const bool have = tile < tiles;
	if (have)
		for (uint32_t d = lane; d < 256u; d += 64u)
			base[w][d] = (uint32_t)hscan[d * tiles + tile];
	__syncthreads();
	const uint64_t below = ((uint64_t)1 << lane) - 1u;
	for (uint32_t it = 0; it < BZC_TILE / 64u; it++) {
		const uint32_t idx = tile * BZC_TILE + it * 64u + lane;
		const bool valid = have && idx < N;
		uint64_t k = 0;
		uint32_t v = 0, d = 0;
		if (valid) {
			k = key[idx]; v = sa[idx];
			d = (uint32_t)(k >> shift) & 255u;
		}
		uint64_t m = __ballot(valid);
#pragma unroll
		for (uint32_t bit = 0; bit < 8u; bit++) {
			const bool one = (d >> bit) & 1u;
			const uint64_t bl = __ballot(one);
			m &= one ? bl : ~bl;
		}
		const uint32_t r = (uint32_t)__builtin_popcountll(m & below);
		uint32_t pos = 0;
		if (valid)
			pos = base[w][d] + r;
		__syncthreads();
		if (valid) {
			if (pos < N) {	/* (always: the counts are of the same keys) */
				key_out[pos] = k;
				sa_out[pos] = v;
			}
			if (r == 0)
				base[w][d] += (uint32_t)__builtin_popcountll(m);
		}
		__syncthreads();
	}
}

/* heads of the groups of equal keys: the last head of every scan tile (index + 1), and whether any key is no head */
__global__ __launch_bounds__(BZC_TPB) void bz2c_heads_kernel(bz2c_ctl *__restrict__ ctl, uint32_t round, const uint32_t *__restrict__ offs,
    uint32_t nb, const uint64_t *__restrict__ key, uint32_t *__restrict__ tile_last)
{
	__shared__ uint32_t tmp[BZC_TPB];
	if (round && ctl->nd[round - 1u] == 0)
		return;
	const uint32_t N = offs[nb];
	const uint32_t j0 = blockIdx.x * BZC_SCAN_TILE + threadIdx.x * 8u;
	uint32_t last = 0;
	bool tie = false;
	for (uint32_t k = 0; k < 8u; k++) {
		const uint32_t jdx = j0 + k;
		if (jdx < N) {
			if (jdx == 0 || key[jdx] != key[jdx - 1u]) last = jdx + 1u;
			else tie = true;
		}
	}
	uint32_t tot;
	bz2c_block_scan<BZC_TPB, true>(last, tmp, &tot);
	if (threadIdx.x == 0)
		tile_last[blockIdx.x] = tot;
	if (tie)
		atomicOr(&ctl->nd[round], 1u);
}

/* exclusive max-scan over the tiles' last heads, one workgroup */
__global__ __launch_bounds__(BZC_TPB) void bz2c_head_carry_kernel(const bz2c_ctl *__restrict__ ctl, uint32_t round, uint32_t *tile_last, uint32_t ntiles)
{
	__shared__ uint32_t tmp[BZC_TPB];
	if (round && ctl->nd[round - 1u] == 0)
		return;
	uint32_t carry = 0;
	for (uint32_t t0 = 0; t0 < ntiles; t0 += BZC_TPB) {
		const uint32_t i = t0 + threadIdx.x;
		const uint32_t v = i < ntiles ? tile_last[i] : 0u;
		uint32_t tot;
		const uint32_t inc = bz2c_block_scan<BZC_TPB, true>(v, tmp, &tot);
		/* exclusive: the inclusive value of the thread before */
		__shared__ uint32_t incs[BZC_TPB];
		incs[threadIdx.x] = inc;
		__syncthreads();
		const uint32_t ex = threadIdx.x ? incs[threadIdx.x - 1u] : 0u;
		if (i < ntiles)
			tile_last[i] = ex > carry ? ex : carry;
		carry = tot > carry ? tot : carry;
		__syncthreads();
	}
}

/* rank[sa[j]] = index of the head of j's group */
__global__ __launch_bounds__(BZC_TPB) void bz2c_ranks_kernel(const bz2c_ctl *__restrict__ ctl, uint32_t round, const uint32_t *__restrict__ offs,
    uint32_t nb, const uint64_t *__restrict__ key, const uint32_t *__restrict__ sa, const uint32_t *__restrict__ tile_carry,
    uint32_t *__restrict__ rank)
{
	__shared__ uint32_t tmp[BZC_TPB], incs[BZC_TPB];
	if (round && ctl->nd[round - 1u] == 0)
		return;
	const uint32_t N = offs[nb];
	const uint32_t j0 = blockIdx.x * BZC_SCAN_TILE + threadIdx.x * 8u;
	uint32_t hd[8], last = 0;
	for (uint32_t k = 0; k < 8u; k++) {
		const uint32_t jdx = j0 + k;
		hd[k] = 0;
		if (jdx < N && (jdx == 0 || key[jdx] != key[jdx - 1u]))
			hd[k] = last = jdx + 1u;
	}
	uint32_t tot;
	incs[threadIdx.x] = bz2c_block_scan<BZC_TPB, true>(last, tmp, &tot);
	__syncthreads();
	uint32_t cur = threadIdx.x ? incs[threadIdx.x - 1u] : 0u;
	const uint32_t carry = tile_carry[blockIdx.x];
	cur = cur > carry ? cur : carry;
	for (uint32_t k = 0; k < 8u; k++) {
		const uint32_t jdx = j0 + k;
		if (jdx < N) {
			if (hd[k]) cur = hd[k];
			rank[sa[jdx]] = cur - 1u;
		}
	}
}

/* last column of the sorted rotations, and origPtr */
__global__ __launch_bounds__(BZC_TPB) void bz2c_bwt_kernel(const uint32_t *__restrict__ offs, const uint32_t *__restrict__ n_rle, uint32_t nb,
    const uint8_t *__restrict__ rle, const uint32_t *__restrict__ sa, uint8_t *__restrict__ bwt, uint32_t *__restrict__ origptr)
{
	const uint32_t N = offs[nb];
	const uint32_t jdx = blockIdx.x * BZC_TPB + threadIdx.x;
	if (jdx >= N)
		return;
	const uint32_t i = sa[jdx];
	const uint32_t b = bz2c_find_block(offs, nb, i);
	const uint32_t o = offs[b], n = n_rle[b];
	bwt[jdx] = rle[i == o ? o + n - 1u : i - 1u];
	if (i == o)
		origptr[b] = jdx - o;
}

/* ------------------------------------------------------------------ MTF + RLE2 */

/* symbols of chunk [i0, i1) of one block's MTF values, the zero run in front of it starting at zrs */
template <typename Emit>
__device__ __forceinline__ void bz2c_rle2_chunk(const uint8_t *mtf, uint32_t i0, uint32_t i1, uint32_t n, uint32_t zrs, Emit emit)
{
	for (uint32_t i = i0; i < i1; i++) {
		const uint32_t v = mtf[i];
		if (v) {
			emit(v + 1u);
			zrs = i + 1u;
		} else if (i + 1u == n || mtf[i + 1u] != 0) {
			uint32_t r = i - zrs + 1u;
			while (r) {
				if (r & 1u) { emit(0u); r = (r - 1u) >> 1; }
				else { emit(1u); r = (r - 2u) >> 1; }
			}
		}
	}
}

__global__ __launch_bounds__(BZC_MTF_TPB) void bz2c_mtf_kernel(const uint32_t *__restrict__ offs, const uint32_t *__restrict__ n_rle,
    const uint32_t *__restrict__ used, const uint8_t *__restrict__ bwt, uint8_t *__restrict__ mtf, uint8_t *__restrict__ csum,
    uint32_t *__restrict__ ccnt, uint8_t *__restrict__ cstart, uint32_t *__restrict__ clastnz, uint32_t *__restrict__ czrs,
    uint32_t *__restrict__ csyms, uint16_t *__restrict__ sym, uint32_t *__restrict__ nsym, uint32_t *__restrict__ freq)
{
	__shared__ uint8_t lst[256u * BZC_MTF_TPB];
	__shared__ uint32_t seen[8][BZC_MTF_TPB];
	__shared__ uint8_t cur[2][256], inset[256];
	__shared__ uint32_t fr[BZC_ALPHA_MAX + 2u];
	const uint32_t b = blockIdx.x, t = threadIdx.x;
	const uint32_t o = offs[b], n = n_rle[b];
	const uint32_t nch = (n + BZC_CHUNK - 1u) / BZC_CHUNK;
	const uint32_t cb = o / BZC_CHUNK + b;	/* this block's first chunk slot */
	const uint8_t *in = bwt + o;
	uint8_t *mv = mtf + o;
	uint32_t nused = 0;
	for (uint32_t k = 0; k < 8u; k++)
		nused += (uint32_t)__builtin_popcount(used[b * 8u + k]);
	for (uint32_t k = t; k < BZC_ALPHA_MAX + 2u; k += BZC_MTF_TPB)
		fr[k] = 0;
	/* 1: every chunk's distinct bytes, latest first */
	for (uint32_t c = t; c < nch; c += BZC_MTF_TPB) {
		for (uint32_t k = 0; k < 8u; k++)
			seen[k][t] = 0;
		const uint32_t i0 = c * BZC_CHUNK, i1 = i0 + BZC_CHUNK < n ? i0 + BZC_CHUNK : n;
		uint8_t *s = csum + (uint64_t)(cb + c) * 256u;
		uint32_t cnt = 0;
		for (uint32_t i = i1; i > i0; i--) {
			const uint32_t ch = in[i - 1u];
			const uint32_t wv = seen[ch >> 5][t];
			if (!((wv >> (ch & 31u)) & 1u)) {
				seen[ch >> 5][t] = wv | (1u << (ch & 31u));
				s[cnt++] = (uint8_t)ch;
			}
		}
		ccnt[cb + c] = cnt;
	}
	__threadfence_block();
	__syncthreads();
	/* 2: the scan, by one wave: start list of every chunk.  The list begins with the bytes in use in ascending order
	 * (so a value's position is its position among the bytes in use), the others behind them never move forward. */
	if (t < 64u) {
		if (t == 0) {
			uint32_t k = 0;
			for (uint32_t c = 0; c < 256u; c++)
				if ((used[b * 8u + (c >> 5)] >> (c & 31u)) & 1u) cur[0][k++] = (uint8_t)c;
			for (uint32_t c = 0; c < 256u; c++)
				if (!((used[b * 8u + (c >> 5)] >> (c & 31u)) & 1u)) cur[0][k++] = (uint8_t)c;
		}
		for (uint32_t k = t; k < 256u; k += 64u)
			inset[k] = 0;
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
		__builtin_amdgcn_wave_barrier();
		__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
		uint32_t p = 0;
		for (uint32_t c = 0; c < nch; c++) {
			const uint8_t *s = csum + (uint64_t)(cb + c) * 256u;
			uint8_t *st = cstart + (uint64_t)(cb + c) * 256u;
			const uint32_t cnt = ccnt[cb + c];
			for (uint32_t k = t; k < 256u; k += 64u)
				st[k] = cur[p][k];
			for (uint32_t k = t; k < cnt; k += 64u)
				inset[s[k]] = 1;
			__builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
			__builtin_amdgcn_wave_barrier();
			__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
			uint32_t at = cnt;
			for (uint32_t k0 = 0; k0 < 256u; k0 += 64u) {
				const uint32_t e = cur[p][k0 + t];
				const bool keep = !inset[e];
				const uint64_t m = __ballot(keep);
				if (keep)
					cur[p ^ 1u][at + (uint32_t)__builtin_popcountll(m & (((uint64_t)1 << t) - 1u))] = (uint8_t)e;
				at += (uint32_t)__builtin_popcountll(m);
			}
			for (uint32_t k = t; k < cnt; k += 64u)
				cur[p ^ 1u][k] = s[k];
			__builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
			__builtin_amdgcn_wave_barrier();
			__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
			for (uint32_t k = t; k < cnt; k += 64u)
				inset[s[k]] = 0;
			p ^= 1u;
		}
	}
	__threadfence_block();
	__syncthreads();
	/* 3: every chunk again, from its true start list */
	for (uint32_t c = t; c < nch; c += BZC_MTF_TPB) {
		const uint8_t *st = cstart + (uint64_t)(cb + c) * 256u;
		for (uint32_t k = 0; k < 256u; k++)
			lst[k * BZC_MTF_TPB + t] = st[k];
		const uint32_t i0 = c * BZC_CHUNK, i1 = i0 + BZC_CHUNK < n ? i0 + BZC_CHUNK : n;
		uint32_t lastnz = 0;
		for (uint32_t i = i0; i < i1; i++) {
			const uint8_t ch = in[i];
			uint32_t p = 0;
			uint8_t prev = lst[t];
			while (prev != ch && p < 255u) {	/* (ch is in the list: the bound is for the compiler's sake) */
				p++;
				const uint8_t x = lst[p * BZC_MTF_TPB + t];
				lst[p * BZC_MTF_TPB + t] = prev;
				prev = x;
			}
			lst[t] = ch;
			mv[i] = (uint8_t)p;
			if (p) lastnz = i + 1u;
		}
		clastnz[cb + c] = lastnz;
	}
	__threadfence_block();
	__syncthreads();
	/* 4: where the zero run in front of every chunk starts */
	if (t == 0) {
		uint32_t z = 0;
		for (uint32_t c = 0; c < nch; c++) {
			czrs[cb + c] = z;
			const uint32_t l = clastnz[cb + c];
			z = l ? l : z;
		}
	}
	__threadfence_block();
	__syncthreads();
	/* 5: symbols per chunk; 6: their places; 7: the symbols and their counts */
	for (uint32_t c = t; c < nch; c += BZC_MTF_TPB) {
		const uint32_t i0 = c * BZC_CHUNK, i1 = i0 + BZC_CHUNK < n ? i0 + BZC_CHUNK : n;
		uint32_t cnt = 0;
		bz2c_rle2_chunk(mv, i0, i1, n, czrs[cb + c], [&](uint32_t) { cnt++; });
		csyms[cb + c] = cnt;
	}
	__threadfence_block();
	__syncthreads();
	if (t == 0) {
		uint32_t z = 0;
		for (uint32_t c = 0; c < nch; c++) {
			const uint32_t v = csyms[cb + c];
			csyms[cb + c] = z;
			z += v;
		}
		sym[(uint64_t)o + b + z] = (uint16_t)(nused + 1u);	/* end of block */
		nsym[b] = z + 1u;
		fr[nused + 1u] = 1;
	}
	__threadfence_block();
	__syncthreads();
	for (uint32_t c = t; c < nch; c += BZC_MTF_TPB) {
		const uint32_t i0 = c * BZC_CHUNK, i1 = i0 + BZC_CHUNK < n ? i0 + BZC_CHUNK : n;
		uint16_t *out = sym + (uint64_t)o + b + csyms[cb + c];
		bz2c_rle2_chunk(mv, i0, i1, n, czrs[cb + c], [&](uint32_t s) {
			*out++ = (uint16_t)s;
			atomicAdd(&fr[s], 1u);
		});
	}
	__syncthreads();
	for (uint32_t k = t; k < BZC_ALPHA_MAX + 2u; k += BZC_MTF_TPB)
		freq[b * (BZC_ALPHA_MAX + 2u) + k] = fr[k];
}

/* ------------------------------------------------------------------ tables and bits */

#define BZC_SLOTS 5	/* 258 symbols over 64 lanes */

/* Huffman code lengths 1..17 for ALL `alpha` symbols (the format gives every symbol of the alphabet a length), one wave
 * per table.  Counts of 0 count as 1.  The lanes rank the symbols by count; lane 0 merges the sorted leaves with the
 * two-queue method (internal nodes come out in ascending weight, so the two smallest are always at a queue's head) and
 * walks the parents down from the root for the depths.  A code deeper than 17 halves the counts (1 + f / 2) and builds
 * again, as bzip2 itself does.  1 + f / 2 has the fixed points 1 and 2, so after at most 20 halvings every count is 1 or
 * 2 and the code is no deeper than ceil(log2 258) + 1 = 10: the loop always ends by its break, well inside its 24 tries.
 * `fs` = L_out doubles as the counts by symbol while building; wt holds 2 * alpha words, par 2 * alpha and ord alpha
 * halfwords. */
__device__ __forceinline__ void bz2c_code_lengths(const uint32_t *F_in, uint32_t alpha, uint32_t *L_out, uint32_t lane, uint32_t *wt,
    uint16_t *par, uint16_t *ord)
{
	uint32_t *fs = L_out;
	for (uint32_t s = lane; s < alpha; s += 64u)
		fs[s] = F_in[s] ? F_in[s] : 1u;
	for (uint32_t tries = 0; tries < 24u; tries++) {
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
		__builtin_amdgcn_wave_barrier();
		__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
		for (uint32_t s = lane; s < alpha; s += 64u) {
			const uint32_t f = fs[s];
			uint32_t r = 0;
			for (uint32_t j = 0; j < alpha; j++) {
				const uint32_t g = fs[j];
				r += (g < f || (g == f && j < s)) ? 1u : 0u;
			}
			ord[r] = (uint16_t)s;
			wt[r] = f;
		}
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
		__builtin_amdgcn_wave_barrier();
		__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
		uint32_t deepest = 0;
		if (lane == 0) {
			uint32_t qa = 0, qb = alpha, next = alpha;
			for (uint32_t m = 0; m + 1u < alpha; m++) {
				uint32_t sum = 0;
				for (int two = 0; two < 2; two++) {
					const bool leaf = qa < alpha && (qb >= next || wt[qa] <= wt[qb]);
					const uint32_t pick = leaf ? qa++ : qb++;
					sum += wt[pick];
					par[pick] = (uint16_t)next;
				}
				wt[next++] = sum;
			}
			wt[next - 1u] = 0;	/* the root's depth; a node's parent has a higher index */
			for (uint32_t i = next - 1u; i > 0; i--) {
				const uint32_t d = wt[par[i - 1u]] + 1u;
				wt[i - 1u] = d;
				if (i - 1u < alpha && d > deepest) deepest = d;
			}
		}
		deepest = (uint32_t)__shfl((int)deepest, 0, 64);
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
		__builtin_amdgcn_wave_barrier();
		__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
		if (deepest <= BZC_MAXLEN)
			break;
		for (uint32_t s = lane; s < alpha; s += 64u)
			fs[s] = 1u + fs[s] / 2u;
	}
	/* (ord and the depths are read before fs = L_out is overwritten: every lane reads its own entries only) */
	for (uint32_t i = lane; i < alpha; i += 64u) {
		const uint32_t d = wt[i];
		/* (1 <= d <= 17 here: at least three leaves, and the loop above left by its break.  The clamp cannot be reached;
		 * it only keeps a length inside the 5-bit field should that reasoning ever be broken, where the code would no
		 * longer be a prefix code and every reader would refuse the block.) */
		L_out[ord[i]] = d < 1u ? 1u : (d > BZC_MAXLEN ? BZC_MAXLEN : d);
	}
}

/* canonical codes, shortest first, by symbol inside a length; stored bit-reversed | length << 24 */
__device__ __forceinline__ void bz2c_assign_codes(const uint32_t *L, uint32_t alpha, uint32_t *code, uint32_t lane)
{
	const uint64_t below = ((uint64_t)1 << lane) - 1u;
	uint32_t next = 0;
	for (uint32_t len = 1; len <= BZC_MAXLEN; len++) {
		next <<= 1;
#pragma unroll
		for (int k = 0; k < BZC_SLOTS; k++) {
			const uint32_t s = lane + 64u * k;
			const bool m = s < alpha && L[s] == len;
			const uint64_t bl = __ballot(m);
			if (m)
				code[s] = bz2c_rev(next + (uint32_t)__builtin_popcountll(bl & below), len) | (len << 24);
			next += (uint32_t)__builtin_popcountll(bl);
		}
	}
}

/* the bits a table's lengths take: 5 for the first, then per symbol two per step and one to end */
__device__ __forceinline__ uint32_t bz2c_delta_token(uint32_t from, uint32_t to, uint32_t *nbits)
{
	const uint32_t d = to > from ? to - from : from - to;
	*nbits = 2u * d;
	if (d == 0)
		return 0;
	const uint32_t mask = d >= 16u ? 0xFFFFFFFFu : (1u << (2u * d)) - 1u;
	return (to > from ? 0x55555555u : 0xFFFFFFFFu) & mask;	/* "10" up, "11" down, first bit lowest */
}

__global__ __launch_bounds__(BZC_CODE_TPB) void bz2c_code_kernel(const uint8_t *__restrict__ src, uint64_t src_bytes, uint32_t bb,
    const uint32_t *__restrict__ offs, const uint32_t *__restrict__ used, const uint32_t *__restrict__ crc, const uint32_t *__restrict__ origptr,
    const uint16_t *__restrict__ sym, const uint32_t *__restrict__ nsym_v, const uint32_t *__restrict__ freq, uint8_t *__restrict__ sel_g,
    uint32_t *__restrict__ gbits_g, uint32_t *__restrict__ bitbuf, uint32_t stride, uint32_t *__restrict__ blk_bits)
{
	__shared__ uint32_t len[6][BZC_ALPHA_MAX + 2u], fave[6][BZC_ALPHA_MAX + 2u], code[6][BZC_ALPHA_MAX + 2u];
	__shared__ uint32_t stage[BZC_CODE_TPB / 64u][68];
	__shared__ uint32_t tmp[BZC_CODE_TPB];
	/* the code builders' scratch while the tables are fitted, the move-to-front coded selectors afterwards */
	__shared__ uint32_t scratch[6u * (2u * (BZC_ALPHA_MAX + 2u) + (BZC_ALPHA_MAX + 2u) + (BZC_ALPHA_MAX + 2u) / 2u)];
	uint8_t *selm = (uint8_t *)scratch;
	__shared__ uint32_t sh_selbits, sh_tabbits[6], sh_flat;
	const uint32_t b = blockIdx.x, t = threadIdx.x, w = t >> 6, lane = t & 63u;
	const uint64_t so = (uint64_t)b * bb;
	const uint32_t L = (uint32_t)(src_bytes - so < bb ? src_bytes - so : bb);
	const uint32_t nsym = nsym_v[b];
	const uint16_t *sy = sym + (uint64_t)offs[b] + b;
	uint8_t *sel = sel_g + (uint64_t)b * BZC_MAXSEL;
	uint32_t *gbits = gbits_g + (uint64_t)b * (BZC_MAXSEL + 1u);
	const uint32_t *fr = freq + b * (BZC_ALPHA_MAX + 2u);
	uint32_t *out = bitbuf + (uint64_t)b * stride;
	uint32_t nused = 0;
	for (uint32_t k = 0; k < 8u; k++)
		nused += (uint32_t)__builtin_popcount(used[b * 8u + k]);
	const uint32_t alpha = nused + 2u;
	const uint32_t ng = (nsym + BZC_GROUP - 1u) / BZC_GROUP;
	uint32_t nt = nsym < 200u ? 2u : nsym < 600u ? 3u : nsym < 1200u ? 4u : nsym < 2400u ? 5u : 6u;

	/* first tables: the alphabet cut into nt ranges of about equal count; cheap inside a table's range, dear outside */
	if (t == 0) {
		uint32_t rem = nsym, gs = 0;
		for (uint32_t part = nt; part > 0; part--) {
			const uint32_t want = rem / part;
			uint32_t ge = gs, acc = 0;
			while (ge < alpha && (acc < want || ge == gs)) acc += fr[ge++];
			if (part == 1u) ge = alpha;
			for (uint32_t v = 0; v < alpha; v++)
				len[part - 1u][v] = (v >= gs && v < ge) ? 0u : 15u;
			gs = ge; rem -= acc < rem ? acc : rem;
		}
	}
	__syncthreads();
	for (uint32_t iter = 0; iter < 4u; iter++) {
		for (uint32_t k = t; k < 6u * (BZC_ALPHA_MAX + 2u); k += BZC_CODE_TPB)
			(&fave[0][0])[k] = 0;
		__syncthreads();
		for (uint32_t g = t; g < ng; g += BZC_CODE_TPB) {
			const uint32_t i0 = g * BZC_GROUP, i1 = i0 + BZC_GROUP < nsym ? i0 + BZC_GROUP : nsym;
			uint32_t cost[6] = { 0, 0, 0, 0, 0, 0 };
			for (uint32_t i = i0; i < i1; i++) {
				const uint32_t s = sy[i];
#pragma unroll
				for (uint32_t k = 0; k < 6u; k++)
					cost[k] += len[k][s];
			}
			uint32_t best = 0;
#pragma unroll
			for (uint32_t k = 1; k < 6u; k++)
				if (k < nt && cost[k] < cost[best]) best = k;
			sel[g] = (uint8_t)best;
			for (uint32_t i = i0; i < i1; i++)
				atomicAdd(&fave[best][sy[i]], 1u);
		}
		__syncthreads();
		if (w < nt) {
			uint32_t *wk = scratch + w * (2u * (BZC_ALPHA_MAX + 2u) + (BZC_ALPHA_MAX + 2u) + (BZC_ALPHA_MAX + 2u) / 2u);
			uint16_t *hp = (uint16_t *)(wk + 2u * (BZC_ALPHA_MAX + 2u));
			bz2c_code_lengths(fave[w], alpha, len[w], lane, wk, hp, hp + 2u * (BZC_ALPHA_MAX + 2u));
		}
		__syncthreads();
	}

	/* the exact size, fitted first; the flat coding if that passes the bound */
	uint32_t hdr_bits = 0, total = 0;
	for (uint32_t attempt = 0; attempt < 2u; attempt++) {
		if (attempt == 1u) {
			/* two flat tables: 2^bits - alpha symbols one bit shorter, every selector 0 */
			uint32_t bits = 1;
			while ((1u << bits) < alpha) bits++;
			const uint32_t shorter = (1u << bits) - alpha;
			nt = 2;
			for (uint32_t v = t; v < alpha; v += BZC_CODE_TPB)
				len[0][v] = len[1][v] = v < shorter ? bits - 1u : bits;
			for (uint32_t g = t; g < ng; g += BZC_CODE_TPB)
				sel[g] = 0;
			__syncthreads();
		}
		for (uint32_t g = t; g < ng; g += BZC_CODE_TPB) {
			const uint32_t i0 = g * BZC_GROUP, i1 = i0 + BZC_GROUP < nsym ? i0 + BZC_GROUP : nsym;
			const uint32_t k = sel[g];
			uint32_t c = 0;
			for (uint32_t i = i0; i < i1; i++)
				c += len[k][sy[i]];
			gbits[g] = c;
		}
		__threadfence_block();
		__syncthreads();
		{	/* exclusive scan of the groups' bits, a run of groups per thread */
			const uint32_t per = (ng + BZC_CODE_TPB - 1u) / BZC_CODE_TPB;
			const uint32_t g0 = t * per < ng ? t * per : ng, g1 = g0 + per < ng ? g0 + per : ng;
			uint32_t s = 0;
			for (uint32_t g = g0; g < g1; g++) s += gbits[g];
			uint32_t tot;
			uint32_t ex = bz2c_block_scan<BZC_CODE_TPB, false>(s, tmp, &tot) - s;
			for (uint32_t g = g0; g < g1; g++) {
				const uint32_t v = gbits[g];
				gbits[g] = ex;
				ex += v;
			}
			if (t == 0) gbits[ng] = tot;
			total = tot;
		}
		/* selectors, move-to-front, by one thread; table bits by one wave per table */
		if (t == 0) {
			uint32_t pos[6] = { 0, 1, 2, 3, 4, 5 }, bits = 0;
			for (uint32_t g = 0; g < ng; g++) {
				const uint32_t v = sel[g];
				uint32_t jx = 0, prev = pos[0];
				while (prev != v && jx < 5u) {
					jx++;
					const uint32_t x = pos[jx];
					pos[jx] = prev;
					prev = x;
				}
				pos[0] = v;
				selm[g] = (uint8_t)jx;
				bits += jx + 1u;
			}
			sh_selbits = bits;
		}
		if (w < nt) {
			uint32_t bits = 0;
			for (uint32_t v = lane; v < alpha; v += 64u)
				bits += 1u + 2u * (v ? (len[w][v] > len[w][v - 1u] ? len[w][v] - len[w][v - 1u] : len[w][v - 1u] - len[w][v]) : 0u);
			bits = wave_sum(bits);
			if (lane == 0) sh_tabbits[w] = bits + 5u;
		}
		__threadfence_block();
		__syncthreads();
		uint32_t nranges = 0;
		for (uint32_t r = 0; r < 16u; r++)
			nranges += ((used[b * 8u + (r >> 1)] >> ((r & 1u) * 16u)) & 0xFFFFu) != 0;
		hdr_bits = 48u + 32u + 1u + 24u + 16u + 16u * nranges + 3u + 15u + sh_selbits;
		for (uint32_t k = 0; k < nt; k++)
			hdr_bits += sh_tabbits[k];
		if (t == 0)
			sh_flat = (uint64_t)hdr_bits + total > bz2c_block_bits(L);
		__syncthreads();
		const bool over = sh_flat != 0;
		__syncthreads();
		if (!over)
			break;
	}
	if (w < nt)
		bz2c_assign_codes(len[w], alpha, code[w], lane);
	for (uint32_t k = lane; k < 68u; k += 64u)
		stage[w][k] = 0;
	__syncthreads();

	uint64_t bp = 0;
	uint32_t first = 0;	/* a wave's first dword may be the wave before's last: it is OR-ed in, as the last one is */
	auto store = [&](uint32_t i, uint32_t v) {
		if (i == first) atomicOr(&out[i], v);
		else out[i] = v;
	};
	if (w == 0) {
		/* the block header */
		uint32_t bits = 0, nbv = 0;
		const uint32_t r = lane - 6u;
		if (lane == 0) { bits = 0x314159u; nbv = 24; }
		else if (lane == 1) { bits = 0x265359u; nbv = 24; }
		else if (lane == 2) { bits = crc[b]; nbv = 32; }
		else if (lane == 3) { bits = 0; nbv = 1; }
		else if (lane == 4) { bits = origptr[b]; nbv = 24; }
		else if (lane == 22) { bits = nt; nbv = 3; }
		else if (lane == 23) { bits = ng; nbv = 15; }
		bits = bz2c_rev(bits, nbv);
		if (lane == 5) {	/* bit r = range r in use: already first-bit-lowest */
			for (uint32_t q = 0; q < 16u; q++)
				bits |= (uint32_t)(((used[b * 8u + (q >> 1)] >> ((q & 1u) * 16u)) & 0xFFFFu) != 0) << q;
			nbv = 16;
		} else if (lane >= 6 && lane < 22) {
			bits = (used[b * 8u + (r >> 1)] >> ((r & 1u) * 16u)) & 0xFFFFu;
			nbv = bits ? 16u : 0u;
		}
		bp += wave_bits_append(bp, bits, nbv, stage[0], lane, store);
		for (uint32_t g0 = 0; g0 < ng; g0 += 64u) {
			const uint32_t g = g0 + lane;
			const uint32_t v = g < ng ? selm[g] : 0u;
			bp += wave_bits_append(bp, (1u << v) - 1u, g < ng ? v + 1u : 0u, stage[0], lane, store);
		}
		for (uint32_t k = 0; k < nt; k++) {
			bp += wave_bits_append(bp, bz2c_rev(len[k][0], 5), lane == 0 ? 5u : 0u, stage[0], lane, store);
			for (uint32_t x0 = 0; x0 < 2u * alpha; x0 += 64u) {
				const uint32_t x = x0 + lane, v = x >> 1;
				uint32_t nbt = 0, tk = 0;
				if (x < 2u * alpha) {
					if (x & 1u) { tk = 0; nbt = 1; }
					else if (v) tk = bz2c_delta_token(len[k][v - 1u], len[k][v], &nbt);
				}
				bp += wave_bits_append(bp, tk, nbt, stage[0], lane, store);
			}
		}
	}
	/* the symbols: a run of groups per wave, from the scanned bit offsets */
	{
		const uint32_t nw = BZC_CODE_TPB / 64u;
		const uint32_t per = (ng + nw - 1u) / nw;
		const uint32_t g0 = w * per < ng ? w * per : ng, g1 = g0 + per < ng ? g0 + per : ng;
		if (w != 0) {
			bp = (uint64_t)hdr_bits + gbits[g0];
			first = (uint32_t)(bp >> 5);
		}
		const uint32_t i0 = g0 * BZC_GROUP, i1 = g1 * BZC_GROUP < nsym ? g1 * BZC_GROUP : nsym;
		for (uint32_t x0 = i0; x0 < i1; x0 += 64u) {
			const uint32_t x = x0 + lane;
			uint32_t c = 0;
			if (x < i1)
				c = code[sel[x / BZC_GROUP]][sy[x]];
			bp += wave_bits_append(bp, c & 0xFFFFFFu, c >> 24, stage[w], lane, store);
		}
		if (lane == 0 && (bp & 31u) && stage[w][0])
			atomicOr(&out[bp >> 5], stage[w][0]);
	}
	if (t == 0)
		blk_bits[b] = hdr_bits + total;
}

/* ------------------------------------------------------------------ link and pack */

struct bz2c_segs {
	const uint64_t *off;	/* [nseg + 1] bit offsets */
	const uint32_t *pend, *bitbuf, *trail;
	uint32_t nb, stride;
};
__device__ __forceinline__ const uint32_t *bz2c_seg_buf(const bz2c_segs &S, uint32_t s)
{
	return s == 0 ? S.pend : s <= S.nb ? S.bitbuf + (uint64_t)(s - 1u) * S.stride : S.trail;
}
/* up to 32 bits of the stream at bit q (first bit lowest), zeros behind `total`; *seg is the piece q lies in or before */
__device__ __forceinline__ uint32_t bz2c_gather32(const bz2c_segs &S, uint32_t nseg, uint64_t total, uint64_t q, uint32_t *seg)
{
	uint32_t got = 0, v = 0, s = *seg;
	while (got < 32u && q < total) {
		while (s + 1u < nseg && S.off[s + 1u] <= q) s++;
		const uint64_t lo = q - S.off[s], left = S.off[s + 1u] - q;
		const uint32_t c = left < 32u - got ? (uint32_t)left : 32u - got;
		const uint32_t *buf = bz2c_seg_buf(S, s);
		const uint64_t two = (uint64_t)buf[lo >> 5] | ((uint64_t)buf[(lo >> 5) + 1u] << 32);
		const uint32_t piece = (uint32_t)(two >> (lo & 31u)) & (c == 32u ? 0xFFFFFFFFu : (1u << c) - 1u);
		v |= piece << got;
		got += c; q += c;
	}
	*seg = s;
	return v;
}

/* one thread: the pieces' offsets, the combined CRC, the trailer, the new state */
__global__ void bz2c_link_kernel(bz2c_ctl *__restrict__ ctl, la_bz2c_state *state, uint32_t level, uint32_t flags, uint32_t nb,
    const uint32_t *__restrict__ blk_bits, const uint32_t *__restrict__ crc, uint64_t *__restrict__ seg_off, uint32_t *__restrict__ pend,
    uint32_t *__restrict__ trail, const uint32_t *__restrict__ bitbuf, uint32_t stride, uint64_t *__restrict__ out_bytes, uint64_t out_cap)
{
	la_bz2c_state st = *state;
	if (flags & LA_BZ2C_FIRST) { st.crc = 0; st.nbits = 0; st.bits = 0; }
	st.nbits &= 7u;
	uint32_t pbits = st.nbits;
	/* pending bits: most significant first in the low byte -> first bit lowest */
	pend[0] = __builtin_bitreverse32(st.bits & 0xFFu) >> 24;
	pend[0] &= (1u << pbits) - 1u;
	pend[1] = pend[2] = pend[3] = 0;
	if (flags & LA_BZ2C_FIRST) {
		const uint32_t hdr = ('B' << 24) | ('Z' << 16) | ('h' << 8) | ('0' + level);
		pend[0] = __builtin_bitreverse32(hdr);
		pbits = 32;
	}
	uint64_t o = 0;
	seg_off[0] = 0; o = pbits;
	for (uint32_t b = 0; b < nb; b++) {
		seg_off[b + 1u] = o;
		o += blk_bits[b];
		st.crc = ((st.crc << 1) | (st.crc >> 31)) ^ crc[b];
	}
	seg_off[nb + 1u] = o;
	trail[0] = trail[1] = trail[2] = trail[3] = 0;
	if (flags & LA_BZ2C_LAST) {
		/* 0x177245385090 then the combined CRC, 80 bits, first bit lowest */
		trail[0] = __builtin_bitreverse32(0x17724538u);
		trail[1] = (__builtin_bitreverse32(0x5090u) >> 16) | ((__builtin_bitreverse32(st.crc) & 0xFFFFu) << 16);
		trail[2] = __builtin_bitreverse32(st.crc) >> 16;
		o += 80u;
	}
	seg_off[nb + 2u] = o;
	ctl->total_bits = o;
	const uint64_t nbytes = (flags & LA_BZ2C_LAST) ? (o + 7u) >> 3 : o >> 3;
	ctl->out_bytes = nbytes;
	*out_bytes = nbytes;
	if (flags & LA_BZ2C_LAST) {
		st.crc = 0; st.nbits = 0; st.bits = 0;
	} else {
		bz2c_segs S = { seg_off, pend, bitbuf, trail, nb, stride };
		uint32_t seg = 0;
		st.nbits = (uint32_t)(o & 7u);
		const uint32_t v = bz2c_gather32(S, nb + 2u, o, o & ~(uint64_t)7u, &seg);
		st.bits = (__builtin_bitreverse32(v) >> 24) & 0xFFu;
	}
	st.reserved = 0;
	if (nbytes <= out_cap)	/* a piece that did not fit was not written whole: the caller repeats the call with more room */
		*state = st;
}

__global__ __launch_bounds__(BZC_TPB) void bz2c_pack_kernel(const bz2c_ctl *__restrict__ ctl, uint32_t nb, const uint64_t *__restrict__ seg_off,
    const uint32_t *__restrict__ pend, const uint32_t *__restrict__ trail, const uint32_t *__restrict__ bitbuf, uint32_t stride,
    uint8_t *__restrict__ d_out, uint64_t out_cap)
{
	const uint64_t nbytes = ctl->out_bytes < out_cap ? ctl->out_bytes : out_cap;
	const uint64_t total = ctl->total_bits;
	const uint64_t p = ((uint64_t)blockIdx.x * BZC_TPB + threadIdx.x) * 16u;
	if (p >= nbytes)
		return;
	bz2c_segs S = { seg_off, pend, bitbuf, trail, nb, stride };
	const uint32_t nseg = nb + 2u;
	/* the piece that holds bit 8p */
	uint32_t lo = 0, hi = nseg;
	while (hi - lo > 1u) {
		const uint32_t mid = (lo + hi) >> 1;
		if (seg_off[mid] <= p * 8u) lo = mid; else hi = mid;
	}
	uint32_t seg = lo, v[4];
	for (uint32_t k = 0; k < 4u; k++) {
		const uint32_t x = bz2c_gather32(S, nseg, total, p * 8u + 32u * k, &seg);
		v[k] = __builtin_bswap32(__builtin_bitreverse32(x));	/* every byte turned round, the bytes in place */
	}
	if (p + 16u <= nbytes) {
		const uint4 q = make_uint4(v[0], v[1], v[2], v[3]);
		__builtin_memcpy(d_out + p, &q, 16);
	} else {
		for (uint32_t k = 0; p + k < nbytes; k++)
			d_out[p + k] = (uint8_t)(v[k >> 2] >> ((k & 3u) * 8u));
	}
}

/* ------------------------------------------------------------------ workspace and launch */

struct bz2c_ws {
	bz2c_ctl *ctl;
	uint32_t *n_rle, *offs, *crc, *used, *origptr, *nsym, *freq, *blk_bits;
	uint64_t *seg_off;
	uint32_t *pend, *trail;
	uint8_t *rle, *bwt, *mtf;
	uint32_t *sa[2], *rank;
	uint64_t *key[2];
	uint32_t *hist;
	uint64_t *hscan;
	uint8_t *scan_scratch;
	uint32_t *tile_last;
	uint8_t *csum, *cstart;
	uint32_t *ccnt, *clastnz, *czrs, *csyms;
	uint16_t *sym;
	uint8_t *sel;
	uint32_t *gbits, *bitbuf;
	uint64_t bitbuf_words;
};

static uint32_t bz2c_nblocks(uint64_t src_bytes, uint32_t level)
{
	const uint32_t bb = bz2c_block_bytes(level);
	return (uint32_t)((src_bytes + bb - 1u) / bb);
}
static uint64_t bz2c_nmax(uint64_t src_bytes, uint32_t nb) { return src_bytes + src_bytes / 4u + nb; }

static uint64_t bz2c_carve(bz2c_ws *W, uint8_t *base, uint64_t src_bytes, uint32_t level)
{
	la_carve cv = { base, 0 };
	const uint32_t nb = bz2c_nblocks(src_bytes, level);
	const uint64_t nmax = bz2c_nmax(src_bytes, nb);
	const uint64_t tiles = (nmax + BZC_TILE - 1u) / BZC_TILE;
	const uint64_t stiles = (nmax + BZC_SCAN_TILE - 1u) / BZC_SCAN_TILE;
	const uint64_t chunks = nmax / BZC_CHUNK + nb + 1u;
	W->ctl = cv.take<bz2c_ctl>(1, 16);
	W->n_rle = cv.take<uint32_t>(nb + 1u);
	W->offs = cv.take<uint32_t>(nb + 1u);
	W->crc = cv.take<uint32_t>(nb + 1u);
	W->used = cv.take<uint32_t>(8u * (uint64_t)nb + 8u);
	W->origptr = cv.take<uint32_t>(nb + 1u);
	W->nsym = cv.take<uint32_t>(nb + 1u);
	W->freq = cv.take<uint32_t>((uint64_t)(BZC_ALPHA_MAX + 2u) * nb + 1u);
	W->blk_bits = cv.take<uint32_t>(nb + 1u);
	W->seg_off = cv.take<uint64_t>(nb + 4u);
	W->pend = cv.take<uint32_t>(4);
	W->trail = cv.take<uint32_t>(4);
	W->rle = cv.take<uint8_t>(nmax + 16u, 16);
	W->bwt = cv.take<uint8_t>(nmax + 16u, 16);
	W->mtf = cv.take<uint8_t>(nmax + 16u, 16);
	W->sa[0] = cv.take<uint32_t>(nmax + 1u, 16);
	W->sa[1] = cv.take<uint32_t>(nmax + 1u, 16);
	W->rank = cv.take<uint32_t>(nmax + 1u, 16);
	W->key[0] = cv.take<uint64_t>(nmax + 1u, 16);
	W->key[1] = cv.take<uint64_t>(nmax + 1u, 16);
	W->hist = cv.take<uint32_t>(256u * tiles + 1u, 16);
	W->hscan = cv.take<uint64_t>(256u * tiles + 2u, 16);
	W->scan_scratch = cv.take<uint8_t>(la_scan_scratch_bytes((uint32_t)(256u * tiles)) + 16u, 16);
	W->tile_last = cv.take<uint32_t>(stiles + 1u);
	W->csum = cv.take<uint8_t>(chunks * 256u, 16);
	W->cstart = cv.take<uint8_t>(chunks * 256u, 16);
	W->ccnt = cv.take<uint32_t>(chunks);
	W->clastnz = cv.take<uint32_t>(chunks);
	W->czrs = cv.take<uint32_t>(chunks);
	W->csyms = cv.take<uint32_t>(chunks);
	W->sym = cv.take<uint16_t>(nmax + nb + 2u, 16);
	W->sel = cv.take<uint8_t>((uint64_t)BZC_MAXSEL * nb + 16u, 16);
	W->gbits = cv.take<uint32_t>((uint64_t)(BZC_MAXSEL + 1u) * nb + 1u);
	W->bitbuf_words = (uint64_t)bz2c_stride_words(level) * nb + 4u;
	W->bitbuf = cv.take<uint32_t>(W->bitbuf_words, 16);
	return cv.off;
}

uint64_t la_bzip2_compress_ws_bytes(uint64_t src_bytes, uint32_t level)
{
	bz2c_ws W;
	return bz2c_carve(&W, nullptr, src_bytes, level);
}

uint32_t la_bzip2_compress_block_bytes(uint32_t level) { return bz2c_block_bytes(level); }

/* sort rounds the call that last used `ws` ran before all ranks were distinct (or the round limit): the control block
 * is the first thing carved, nd[r] says that round r left ties, so round r + 1 ran */
uint32_t la_bzip2_compress_rounds(hipStream_t s, const uint8_t *ws)
{
	bz2c_ctl ctl;
	if (hipMemcpyAsync(&ctl, ws, sizeof(ctl), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
		return 0;
	uint32_t r = 1;
	while (r < BZC_ROUNDS && ctl.nd[r - 1u])
		r++;
	return r;
}

/* header 32 bits + the blocks + trailer 80 bits + up to 7 pending bits in front and 7 of padding behind */
uint64_t la_bzip2_compress_bound(uint64_t src_bytes, uint32_t level)
{
	const uint32_t bb = bz2c_block_bytes(level);
	const uint64_t full = src_bytes / bb;
	const uint32_t rest = (uint32_t)(src_bytes % bb);
	const uint64_t bits = 32u + 80u + 14u + full * bz2c_block_bits(bb) + (rest ? bz2c_block_bits(rest) : 0u);
	return (bits + 7u) / 8u;
}

static uint32_t bz2c_bits_of(uint64_t v)	/* bits that hold every value below v */
{
	uint32_t b = 1;
	while (b < 63u && ((uint64_t)1 << b) < v) b++;
	return b;
}

void la_launch_bzip2_compress(hipStream_t s, const la_bz2c_batch *bt, uint8_t *ws, const la_stage_hook *hook)
{
	auto stage = [&](const char *name) { if (hook) hook->mark(hook->cx, name); };
	bz2c_ws W;
	const uint32_t level = bt->level, bb = bz2c_block_bytes(level);
	const uint32_t nb = bz2c_nblocks(bt->src_bytes, level);
	bz2c_carve(&W, ws, bt->src_bytes, level);
	const uint32_t stride = bz2c_stride_words(level);
	(void)hipMemsetAsync(W.ctl, 0, sizeof(bz2c_ctl), s);
	if (nb) {
		const uint64_t nmax = bz2c_nmax(bt->src_bytes, nb);
		const uint32_t tiles = (uint32_t)((nmax + BZC_TILE - 1u) / BZC_TILE);
		const uint32_t stiles = (uint32_t)((nmax + BZC_SCAN_TILE - 1u) / BZC_SCAN_TILE);
		const uint32_t egrid = (uint32_t)((nmax + BZC_TPB - 1u) / BZC_TPB);
		const uint32_t tgrid = (tiles + BZC_TPB / 64u - 1u) / (BZC_TPB / 64u);
		stage("bz2c_rle1");
		(void)hipMemsetAsync(W.bitbuf, 0, W.bitbuf_words * 4u, s);
		hipLaunchKernelGGL(bz2c_rle1_kernel<false>, dim3(nb), dim3(BZC_TPB), 0, s, bt->d_src, bt->src_bytes, bb, W.n_rle, W.crc, W.used,
		    W.offs, W.rle);
		hipLaunchKernelGGL(bz2c_offsets_kernel, dim3(1), dim3(1), 0, s, W.n_rle, nb, W.offs);
		hipLaunchKernelGGL(bz2c_rle1_kernel<true>, dim3(nb), dim3(BZC_TPB), 0, s, bt->d_src, bt->src_bytes, bb, W.n_rle, W.crc, W.used,
		    W.offs, W.rle);
		/* the sort: every round's order ends in buffer `fin` */
		stage("bz2c_sort");
		const uint32_t B = bz2c_bits_of(nmax);
		const uint32_t passes = (2u * B + 7u) / 8u, passes0 = (8u + bz2c_bits_of(nb) + 7u) / 8u;
		const uint32_t fin = passes & 1u;
		const uint32_t nblk_max = bz2c_rle_max(bb) < nmax ? bz2c_rle_max(bb) : (uint32_t)nmax;
		uint32_t round = 0;
		for (uint32_t h = 0; round < BZC_ROUNDS; round++) {
			const uint32_t np = round ? passes : passes0;
			uint32_t cur = (fin + np) & 1u;	/* start here so that np passes end in fin */
			hipLaunchKernelGGL(bz2c_keys_kernel, dim3(egrid), dim3(BZC_TPB), 0, s, W.ctl, round, h, B, W.offs, W.n_rle, nb, W.rle, W.rank,
			    W.sa[fin], W.sa[cur], W.key[cur]);
			for (uint32_t p = 0; p < np; p++, cur ^= 1u) {
				hipLaunchKernelGGL(bz2c_hist_kernel, dim3(tgrid), dim3(BZC_TPB), 0, s, W.ctl, round, W.offs, nb, W.key[cur], 8u * p, tiles,
				    W.hist);
				la_launch_scan_u32(s, W.hist, 256u * tiles, W.hscan, W.scan_scratch);
				hipLaunchKernelGGL(bz2c_scatter_kernel, dim3(tgrid), dim3(BZC_TPB), 0, s, W.ctl, round, W.offs, nb, W.key[cur], W.sa[cur],
				    8u * p, tiles, W.hscan, W.key[cur ^ 1u], W.sa[cur ^ 1u]);
			}
			hipLaunchKernelGGL(bz2c_heads_kernel, dim3(stiles), dim3(BZC_TPB), 0, s, W.ctl, round, W.offs, nb, W.key[fin], W.tile_last);
			hipLaunchKernelGGL(bz2c_head_carry_kernel, dim3(1), dim3(BZC_TPB), 0, s, W.ctl, round, W.tile_last, stiles);
			hipLaunchKernelGGL(bz2c_ranks_kernel, dim3(stiles), dim3(BZC_TPB), 0, s, W.ctl, round, W.offs, nb, W.key[fin], W.sa[fin],
			    W.tile_last, W.rank);
			/* round r has compared 2^r bytes: enough once that reaches the longest block */
			const uint32_t cmp = round ? 2u * h : 1u;
			if (cmp >= nblk_max)
				break;
			h = cmp;
		}
		stage("bz2c_bwt");
		hipLaunchKernelGGL(bz2c_bwt_kernel, dim3(egrid), dim3(BZC_TPB), 0, s, W.offs, W.n_rle, nb, W.rle, W.sa[fin], W.bwt, W.origptr);
		stage("bz2c_mtf");
		hipLaunchKernelGGL(bz2c_mtf_kernel, dim3(nb), dim3(BZC_MTF_TPB), 0, s, W.offs, W.n_rle, W.used, W.bwt, W.mtf, W.csum, W.ccnt, W.cstart,
		    W.clastnz, W.czrs, W.csyms, W.sym, W.nsym, W.freq);
		stage("bz2c_code");
		hipLaunchKernelGGL(bz2c_code_kernel, dim3(nb), dim3(BZC_CODE_TPB), 0, s, bt->d_src, bt->src_bytes, bb, W.offs, W.used, W.crc, W.origptr,
		    W.sym, W.nsym, W.freq, W.sel, W.gbits, W.bitbuf, stride, W.blk_bits);
	}
	stage("bz2c_link_pack");
	hipLaunchKernelGGL(bz2c_link_kernel, dim3(1), dim3(1), 0, s, W.ctl, bt->d_state, level, bt->flags, nb, W.blk_bits, W.crc, W.seg_off, W.pend,
	    W.trail, W.bitbuf, stride, bt->d_out_bytes, bt->out_cap);
	const uint64_t bound = la_bzip2_compress_bound(bt->src_bytes, level);
	const uint64_t cap = bound < bt->out_cap ? bound : bt->out_cap;
	if (cap) {
		const uint32_t pgrid = (uint32_t)((cap + 16u * BZC_TPB - 1u) / (16u * BZC_TPB));
		hipLaunchKernelGGL(bz2c_pack_kernel, dim3(pgrid), dim3(BZC_TPB), 0, s, W.ctl, nb, W.seg_off, W.pend, W.trail, W.bitbuf, stride,
		    bt->d_out, bt->out_cap);
	}
	stage(nullptr);
}
