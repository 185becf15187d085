/*
 * la_inflate_find.hip -- LA_GZ_OPT_BLOCK_STARTS (gfx950): the block starts of ONE raw-deflate span found on the device,
 * so that an ordinary gzip member -- no flush point, no second header -- is decoded as a chain of pieces
 * (la_inflate.hip, la_inflate_chain.hip).  The rule for a candidate is la_deflate_find_dev.h; this file runs it over
 * every bit position and then decides, from the measured pieces, which candidates were true.
 *
 * The launches, in stream order (no kernel waits on another workgroup; every count the host does not know is read from
 * the control block by the kernel that needs it, and every grid is sized by src_bytes):
 *   find_quick    one lane per 32 bit positions, a tile of LA_FIND_TILE_BYTES per workgroup.  The tile and 16 bytes of
 *                 overhang are staged in LDS as dwords (a position looks at DFL_FIND_QUICK_BITS = 74 bits, the last
 *                 position of a lane starts at bit 31 of its dword: 105 bits, four dwords; neighbouring lanes share
 *                 three of them, so each byte is fetched from memory once and read from LDS four times, consecutive
 *                 lanes on consecutive banks).  Writes one 32-bit mask per lane and the tile's count.
 *   scan          la_scan.hip over the tile counts.
 *   find_write    the masks again, a block scan of their popcounts: the survivors, ascending, at the tile's offset.
 *   find_full     one LANE per survivor: the full rule (dfl_find_full).  A survivor is one position in about 2 200, so
 *                 this pass is small whatever its form; a lane keeps the whole header state in registers (the
 *                 code-length code in three 64-bit words, two Kraft sums), no LDS and no table, and reads the few
 *                 hundred bytes of its header from global memory bytewise -- lanes of a wave sit thousands of bits
 *                 apart, there is nothing to share.
 *   scan, pack    la_scan.hip over the flags; cand[0] = the caller's start bit, cand[1 ..] the candidates behind it.
 *   (measure)     la_launch_inflate_chain_bits: one wave per candidate, each piece runs until its cursor lies on a later
 *                 candidate at the end of a block (dfl_piece_end_at), a final block, the end of the span or an error.
 *   walk          one lane, the shape of bz2_walk_kernel: piece 0 is true by the caller's word; the piece that starts
 *                 where a confirmed piece ended is confirmed, every other candidate is refuted by never being reached.
 *                 The confirmed pieces are compacted (start, measured result, length) and the walk stops in front of
 *                 the first piece whose packed end would pass dst_cap.
 *   (scan, emit, resolve: the chain path, over the compacted table; then la_hash.hip folds the CRC32s and writes the
 *   two results.)
 * A false candidate costs one wave's wasted decode, ended by its first error or by dst_cap; a missing one (the tables
 * are bounded by src_bytes / 32 survivors and src_bytes / 128 candidates; what does not fit is dropped from the high
 * end) makes the piece in front of it longer.  Neither changes a byte of the output.
 */
#include "la_dev.h"
#include "la_deflate_find_dev.h"

#define FIND_TPB 256

static_assert(LA_FIND_TILE_BYTES == 4 * FIND_TPB, "one dword of the tile per lane");

struct find_span {
	const uint8_t *base;
	uint64_t len;
};

/* the span, clamped to the source image */
__device__ __forceinline__ find_span find_clamp(const uint8_t *src, uint64_t src_bytes, const la_gz_member *span)
{
	const la_gz_member m = span[0];
	find_span f;
	f.base = src + m.src_off;
	f.len = m.src_off < src_bytes ? src_bytes - m.src_off : 0;
	if (f.len > m.src_len)
		f.len = m.src_len;
	return f;
}

/* the dword at byte offset `at` of the span, bytes at and behind len read as 0 and not touched */
__device__ __forceinline__ uint32_t find_dword(const find_span &f, uint64_t at)
{
	if (at + 4 <= f.len)
		return ld_u32(f.base + at);
	uint32_t v = 0;
	for (uint32_t k = 0; k < 4; k++)
		if (at + k < f.len)
			v |= (uint32_t)f.base[at + k] << (8 * k);
	return v;
}

__global__ __launch_bounds__(FIND_TPB) void find_quick_kernel(const uint8_t *__restrict__ src, uint64_t src_bytes,
    const la_gz_member *__restrict__ span, uint32_t *__restrict__ mask, uint32_t *__restrict__ tile_cnt)
{
	__shared__ uint32_t stage[FIND_TPB + 4];
	__shared__ uint32_t total;
	const find_span f = find_clamp(src, src_bytes, span);
	const uint64_t t0 = (uint64_t)blockIdx.x * LA_FIND_TILE_BYTES;
	const uint32_t t = threadIdx.x;
	if (t == 0)
		total = 0;
	stage[t] = find_dword(f, t0 + 4 * t);
	if (t < 4)
		stage[FIND_TPB + t] = find_dword(f, t0 + 4 * (FIND_TPB + t));
	__syncthreads();
	const uint64_t lo = stage[t] | (uint64_t)stage[t + 1] << 32, hi = stage[t + 2] | (uint64_t)stage[t + 3] << 32;
	const uint64_t end_bits = 8 * f.len, p0 = 8 * t0 + 32 * t;
	uint32_t msk = 0;
	if (p0 < end_bits) {
#pragma unroll 4
		for (uint32_t j = 0; j < 32; j++) {
			const uint32_t hdr = (uint32_t)(lo >> j) & 0x1FFFFu;
			if ((hdr & 7u) != 4u)
				continue;
			const uint64_t clc = ((lo >> (j + 17)) | (hi << (47 - j))) & ((1ull << 57) - 1ull);
			const uint32_t need = dfl_find_quick(hdr, clc);
			if (need != 0 && p0 + j + need <= end_bits)
				msk |= 1u << j;
		}
	}
	mask[(uint64_t)blockIdx.x * FIND_TPB + t] = msk;
	uint32_t c = (uint32_t)__popc(msk);
	for (int d = 32; d >= 1; d >>= 1)
		c += __shfl_xor(c, d, 64);
	if ((t & 63) == 0 && c)
		atomicAdd(&total, c);
	__syncthreads();
	if (t == 0)
		tile_cnt[blockIdx.x] = total;
}

__global__ __launch_bounds__(FIND_TPB) void find_write_kernel(const uint32_t *__restrict__ mask, const uint64_t *__restrict__ tile_off,
    uint32_t tiles, uint32_t *__restrict__ surv, uint32_t max_surv, uint32_t *ctl)
{
	__shared__ uint32_t wsum[FIND_TPB / 64];
	const uint32_t t = threadIdx.x, lane = t & 63, w = t >> 6;
	uint32_t msk = mask[(uint64_t)blockIdx.x * FIND_TPB + t];
	const uint32_t c = (uint32_t)__popc(msk);
	uint32_t inc = c;
	for (int d = 1; d < 64; d <<= 1) {
		const uint32_t up = __shfl_up(inc, d, 64);
		if ((int)lane >= d) inc += up;
	}
	if (lane == 63)
		wsum[w] = inc;
	__syncthreads();
	uint64_t at = tile_off[blockIdx.x] + inc - c;
	for (uint32_t k = 0; k < w; k++)
		at += wsum[k];
	const uint32_t p0 = blockIdx.x * (8 * LA_FIND_TILE_BYTES) + 32 * t;	/* (below 2^32: the source is below 2^29 bytes) */
	while (msk) {
		const uint32_t j = (uint32_t)__ffs((int)msk) - 1;
		msk &= msk - 1;
		if (at < max_surv)
			surv[at] = p0 + j;
		at++;
	}
	if (blockIdx.x == 0 && t == 0) {
		const uint64_t n = tile_off[tiles];
		ctl[LA_FIND_N_SURV] = n < max_surv ? (uint32_t)n : max_surv;
	}
}

__global__ __launch_bounds__(FIND_TPB) void find_full_kernel(const uint8_t *__restrict__ src, uint64_t src_bytes,
    const la_gz_member *__restrict__ span, uint32_t start_bit, const uint32_t *__restrict__ surv, uint32_t max_surv,
    const uint32_t *__restrict__ ctl, uint32_t *__restrict__ flag)
{
	const uint32_t i = blockIdx.x * FIND_TPB + threadIdx.x;
	if (i >= max_surv)
		return;
	uint32_t ok = 0;
	if (i < ctl[LA_FIND_N_SURV]) {
		const find_span f = find_clamp(src, src_bytes, span);
		const uint32_t p = surv[i];
		/* (a candidate at or in front of the caller's own start names nothing a piece could end on) */
		ok = p > start_bit && dfl_find_full(f.base, p, 8 * f.len);
	}
	flag[i] = ok;
}

__global__ __launch_bounds__(FIND_TPB) void find_pack_kernel(const uint32_t *__restrict__ surv, const uint32_t *__restrict__ flag,
    const uint64_t *__restrict__ flag_off, uint32_t max_surv, uint32_t start_bit, uint32_t *__restrict__ cand, uint32_t max_cand,
    uint32_t *ctl)
{
	const uint32_t i = blockIdx.x * FIND_TPB + threadIdx.x;
	if (i < max_surv && flag[i]) {
		const uint64_t k = 1 + flag_off[i];
		if (k < max_cand)
			cand[k] = surv[i];
	}
	if (i == 0) {
		const uint64_t n = 1 + flag_off[max_surv];
		cand[0] = start_bit;
		ctl[LA_FIND_N_CAND] = n < max_cand ? (uint32_t)n : max_cand;
	}
}

void la_launch_gz_find(hipStream_t s, const uint8_t *d_src, uint64_t src_bytes, const la_gz_member *d_span, uint32_t start_bit,
    const la_gz_find_ws &W)
{
	(void)hipMemsetAsync(W.ctl, 0, LA_FIND_CTL_WORDS * sizeof(uint32_t), s);
	hipLaunchKernelGGL(find_quick_kernel, dim3(W.tiles), dim3(FIND_TPB), 0, s, d_src, src_bytes, d_span, W.mask, W.tile_cnt);
	la_launch_scan_u32(s, W.tile_cnt, W.tiles, W.tile_off, W.scan);
	hipLaunchKernelGGL(find_write_kernel, dim3(W.tiles), dim3(FIND_TPB), 0, s, W.mask, W.tile_off, W.tiles, W.surv, W.max_surv, W.ctl);
	const uint32_t blocks = (W.max_surv + FIND_TPB - 1) / FIND_TPB;
	hipLaunchKernelGGL(find_full_kernel, dim3(blocks), dim3(FIND_TPB), 0, s, d_src, src_bytes, d_span, start_bit, W.surv, W.max_surv,
	    W.ctl, W.flag);
	la_launch_scan_u32(s, W.flag, W.max_surv, W.flag_off, W.scan);
	hipLaunchKernelGGL(find_pack_kernel, dim3(blocks), dim3(FIND_TPB), 0, s, W.surv, W.flag, W.flag_off, W.max_surv, start_bit, W.cand,
	    W.max_cand, W.ctl);
}

/*
 * The confirming walk.  res_all[k] is what the measure instance found for the piece that starts at cand[k]: its status,
 * its length, the bit it ended on and, for LA_ST_GZ_PIECE_END, the index of the candidate that lies there (0xFFFFFFFF:
 * the end of the span, where nothing starts).  Piece 0 starts where the caller says a block starts.  A candidate is
 * confirmed when a confirmed piece ended on it -- then it IS where the next block starts, because the decoder read
 * every bit in front of it as the stream it is.  The walk ends with the first piece that does not end so, which is the
 * last piece of the chain, or in front of the first piece that would not fit (LA_FIND_STOP = LA_ST_GZ_OUT_FULL,
 * LA_FIND_STOP_BIT = where that piece starts).
 */
__global__ void gz_walk_kernel(const la_gz_find_ws W, uint64_t dst_cap)
{
	if (threadIdx.x != 0 || blockIdx.x != 0)
		return;
	const uint32_t n = W.ctl[LA_FIND_N_CAND];
	uint32_t k = 0, nconf = 0, stop = 0, stop_bit = 0;
	uint64_t total = 0;
	while (k < n) {
		const la_gz_result r = W.res_all[k];
		if (r.status == LA_ST_GZ_OUT_FULL || total + r.out_len > dst_cap) {
			stop = LA_ST_GZ_OUT_FULL;
			stop_bit = W.cand[k];
			break;
		}
		W.startc[nconf] = W.cand[k];
		W.resc[nconf] = r;
		W.lenc[nconf] = r.out_len;
		nconf++;
		total += r.out_len;
		/* (the index only ever goes up: the walk ends after at most n steps) */
		if (r.status != LA_ST_GZ_PIECE_END || r.crc32 <= k || r.crc32 >= n)
			break;
		k = r.crc32;
	}
	/* the emit pass ends the last piece where the measure pass ended it: on the start of the piece that did not fit */
	if (stop)
		W.startc[nconf] = stop_bit;
	W.ctl[LA_FIND_N_CONF] = nconf;
	W.ctl[LA_FIND_N_TABLE] = nconf + (stop ? 1u : 0u);
	W.ctl[LA_FIND_STOP] = stop;
	W.ctl[LA_FIND_STOP_BIT] = stop_bit;
}

void la_launch_gz_walk(hipStream_t s, uint64_t dst_cap, const la_gz_find_ws &W)
{
	(void)hipMemsetAsync(W.lenc, 0, (uint64_t)W.max_cand * sizeof(uint32_t), s);
	hipLaunchKernelGGL(gz_walk_kernel, dim3(1), dim3(1), 0, s, W, dst_cap);
}
