/*
 * la_lz4_comp.hip -- LZ4 block COMPRESSION + frame assembly on the device (gfx950): the data
 * plane of the lz4 write filter.
 *
 * Replaces, for a whole stream per call, what libarchive/archive_write_add_filter_lz4.c does
 * per block on the host: LZ4_compress_default of one independent block (:484-532,
 * drive_compressor_independence), the stored-block fallback when a block does not shrink
 * (:505-515), the block checksum XXH32 over the bytes as written (:516-521), the frame
 * descriptor with its check byte (:394-419), the EndMark and the content checksum (:433-447).
 * The compressed bytes are NOT those of liblz4 (an LZ4 stream is not unique): parity for this
 * direction is the round trip -- what the reference's reader, the oracle and liblz4 decode from
 * these frames must be the input, bit for bit -- plus the format rules every decoder checks
 * (last five bytes literal, last match at least 12 bytes before the end, offsets inside the block).
 *
 *   lz4_compress_blocks_kernel   ONE WAVE per block of at most 64 KiB.  A 4096-entry hash table of
 *       16-bit positions in LDS, matched by lz77_match (la_comp_common.h: 64 positions per step, matches
 *       taken in position order); the wave writes each sequence cooperatively: token and length bytes by
 *       the first lanes, the literal run 64 bytes per step.  Input is read from global memory
 *       (it stays in L1 / L2 for the lifetime of a block), so LDS holds only the table and many
 *       waves fit a CU.
 *   lz4c_sizes_kernel / scan     stream bytes each block and frame contributes -> offsets.
 *   lz4_pack_frames_kernel       one workgroup per block: size word, payload (compressed, or the
 *       input itself when it did not shrink), block checksum; the frame's first / last block also
 *       writes the 7-byte header / EndMark + content checksum.
 *   frame_sums_kernel            XXH32 of every frame's input (la_comp_common.h), four lanes per frame.
 * The two kinds of XXH32 (per block over the written payload, per frame over the input) run on
 * xxh32_lane / xxh32_quad of la_dev.h.
 */
#include "la_comp_common.h"

#define LZ4C_MFLIMIT   12u
#define LZ4C_LASTLIT   5u

__host__ __device__ static inline uint32_t lz4c_bound(uint32_t n) { return n + n / 255u + 16u; }

/* length field beyond the token nibble: v - 15 as 255, 255, ..., rest (lanes write in parallel); returns bytes written */
__device__ __forceinline__ uint32_t wave_put_len(uint8_t *d, uint32_t v, uint32_t lane)
{
	const uint32_t rest = v - 15u, cnt = rest / 255u + 1u;
	for (uint32_t i = lane; i < cnt; i += 64)
		d[i] = (i + 1u < cnt) ? (uint8_t)255 : (uint8_t)(rest - 255u * (cnt - 1u));
	return cnt;
}

__global__ __launch_bounds__(64) void lz4_compress_blocks_kernel(const uint8_t *__restrict__ src, uint64_t src_bytes,
    uint32_t block_size, uint32_t n_blocks, uint8_t *__restrict__ tmp, uint32_t tmp_stride,
    uint32_t *__restrict__ csize)
{
	__shared__ uint16_t tab[1u << LZ77_HASH_BITS];
	const uint32_t bi = blockIdx.x, lane = threadIdx.x;
	if (bi >= n_blocks)
		return;
	const uint64_t so = (uint64_t)bi * block_size;
	const uint32_t n = (uint32_t)(src_bytes - so < block_size ? src_bytes - so : block_size);
	const uint8_t *in = src + so;
	uint8_t *out = tmp + (uint64_t)bi * tmp_stride;
	for (uint32_t i = lane; i < (1u << LZ77_HASH_BITS); i += 64)
		tab[i] = 0;
	__syncthreads();

	uint32_t anchor = 0, op = 0;	/* wave-uniform */
	if (n > LZ4C_MFLIMIT) {
		/* matches start at or before n - 12 and end at or before n - 5 */
		anchor = lz77_match(tab, in, n - LZ4C_MFLIMIT, n - LZ4C_LASTLIT, lane,
		    [&](uint32_t pf, uint32_t mf, uint32_t cf, uint32_t anchor) {
			const uint32_t lit = pf - anchor, off = pf - cf, ml = mf - 4u;
			/* one sequence: token, literal length, literals, offset, match length */
			if (lane == 0)
				out[op] = (uint8_t)(((lit < 15u ? lit : 15u) << 4) | (ml < 15u ? ml : 15u));
			op += 1;
			if (lit >= 15u)
				op += wave_put_len(out + op, lit, lane);
			wave_copy(out + op, in + anchor, lit, lane);
			op += lit;
			if (lane == 0) {
				out[op] = (uint8_t)off;
				out[op + 1] = (uint8_t)(off >> 8);
			}
			op += 2;
			if (ml >= 15u)
				op += wave_put_len(out + op, ml, lane);
		});
	}
	/* last sequence: literals only (at least the block's last five bytes) */
	{
		const uint32_t lit = n - anchor;
		if (lane == 0)
			out[op] = (uint8_t)((lit < 15u ? lit : 15u) << 4);
		op += 1;
		if (lit >= 15u)
			op += wave_put_len(out + op, lit, lane);
		wave_copy(out + op, in + anchor, lit, lane);
		op += lit;
	}
	if (lane == 0)
		csize[bi] = op;
}

/* bytes of the stream each block contributes: size word + payload (stored when it did not shrink) + block sum,
 * plus the frame's header in front of its first block and EndMark (+ content sum) behind its last */
__global__ __launch_bounds__(256) void lz4c_sizes_kernel(const uint32_t *__restrict__ csize, uint64_t src_bytes,
    uint32_t block_size, uint32_t n_blocks, uint32_t bpf, uint32_t flags, uint32_t *__restrict__ contrib)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n_blocks)
		return;
	const uint64_t so = (uint64_t)i * block_size;
	const uint32_t n = (uint32_t)(src_bytes - so < block_size ? src_bytes - so : block_size);
	const uint32_t pay = csize[i] < n ? csize[i] : n;
	uint32_t c = 4u + pay + ((flags & LA_LZ4C_BLOCK_SUM) ? 4u : 0u);
	if (i % bpf == 0)
		c += 7u;
	if (i % bpf == bpf - 1 || i + 1 == n_blocks)
		c += 4u + ((flags & LA_LZ4C_CONTENT_SUM) ? 4u : 0u);
	contrib[i] = c;
}

__global__ __launch_bounds__(256) void lz4_pack_frames_kernel(const uint8_t *__restrict__ src, uint64_t src_bytes,
    uint32_t block_size, uint32_t n_blocks, uint32_t bpf, uint32_t flags, const uint8_t *__restrict__ tmp,
    uint32_t tmp_stride, const uint32_t *__restrict__ csize, const uint64_t *__restrict__ off,
    const uint32_t *__restrict__ frame_sum, uint8_t *__restrict__ out, uint64_t out_cap, uint64_t *__restrict__ out_bytes)
{
	const uint32_t bi = blockIdx.x, tid = threadIdx.x;
	if (bi >= n_blocks)
		return;
	const uint64_t so = (uint64_t)bi * block_size;
	const uint32_t n = (uint32_t)(src_bytes - so < block_size ? src_bytes - so : block_size);
	const bool stored = csize[bi] >= n;
	const uint32_t pay = stored ? n : csize[bi];
	const uint8_t *payload = stored ? src + so : tmp + (uint64_t)bi * tmp_stride;
	uint64_t o = off[bi];
	if (bi + 1 == n_blocks && tid == 0)
		*out_bytes = off[n_blocks];
	if (off[bi + 1] > out_cap)
		return;		/* the caller sees out_bytes > out_cap */
	__shared__ uint32_t bsum;
	if (bi % bpf == 0) {
		if (tid == 0) {
			/* magic, FLG (version 01, independent blocks, checksums as asked), BD (block maximum), check byte */
			const uint8_t flg = (uint8_t)(0x60 | ((flags & LA_LZ4C_BLOCK_SUM) ? 0x10 : 0) | ((flags & LA_LZ4C_CONTENT_SUM) ? 0x04 : 0));
			const uint8_t bd = block_size <= 65536u ? 0x40 : block_size <= 262144u ? 0x50 : block_size <= 1048576u ? 0x60 : 0x70;
			st_le32(out + o, 0x184D2204u);
			out[o + 4] = flg;
			out[o + 5] = bd;
			const uint8_t d[2] = { flg, bd };
			out[o + 6] = (uint8_t)(xxh32_lane(d, 2, 0) >> 8);
		}
		o += 7;
	}
	if (tid == 0)
		st_le32(out + o, stored ? (pay | 0x80000000u) : pay);
	o += 4;
	for (uint32_t i = tid; i < pay; i += 256)
		out[o + i] = payload[i];
	if (flags & LA_LZ4C_BLOCK_SUM) {
		/* over the payload as written (archive_write_add_filter_lz4.c:516-521); four lanes share the chain */
		if (tid < 4) {
			const uint32_t h = xxh32_quad(payload, pay, 0, (int)tid);
			if (tid == 0)
				bsum = h;
		}
		__syncthreads();
		if (tid == 0)
			st_le32(out + o + pay, bsum);
	}
	o += pay + ((flags & LA_LZ4C_BLOCK_SUM) ? 4u : 0u);
	if ((bi % bpf == bpf - 1 || bi + 1 == n_blocks) && tid == 0) {
		st_le32(out + o, 0);	/* EndMark */
		if (flags & LA_LZ4C_CONTENT_SUM)
			st_le32(out + o + 4, frame_sum[bi / bpf]);
	}
}

struct lz4c_xxh32 {
	__device__ uint32_t operator()(const uint8_t *p, uint64_t len, uint32_t j) const { return xxh32_quad(p, (uint32_t)len, 0, (int)j); }
};

struct lz4c_ws {
	uint8_t *tmp;
	uint32_t *csize, *contrib, *fsum;
	uint64_t *off;
	void *scan;
};

/* the launcher's workspace on `base` (null: sizes only); returns its bytes before the scan scratch */
static uint64_t lz4c_carve(lz4c_ws *w, uint8_t *base, uint64_t nb, uint64_t nf, uint32_t stride)
{
	la_carve c = { base, 0 };
	w->tmp = c.take<uint8_t>(nb * stride);
	w->csize = c.take<uint32_t>(nb);
	w->contrib = c.take<uint32_t>(nb);
	w->off = c.take<uint64_t>(nb + 1);
	w->fsum = c.take<uint32_t>(nf);
	w->scan = c.take<uint8_t>(0, 256);
	return c.off;
}

static uint32_t lz4c_stride(uint32_t block_size) { return (lz4c_bound(block_size) + 15u) & ~15u; }

extern "C" uint64_t la_gpu_lz4_compress_workspace_bytes(uint64_t src_bytes, uint32_t block_size, uint32_t blocks_per_frame)
{
	if (block_size == 0 || blocks_per_frame == 0)
		return 0;
	const uint64_t nb = (src_bytes + block_size - 1) / block_size, nf = (nb + blocks_per_frame - 1) / blocks_per_frame;
	lz4c_ws w;
	return lz4c_carve(&w, nullptr, nb, nf, lz4c_stride(block_size)) + la_scan_scratch_bytes((uint32_t)nb);
}

extern "C" uint64_t la_gpu_lz4_compress_bound(uint64_t src_bytes, uint32_t block_size, uint32_t bpf)
{
	if (block_size == 0 || bpf == 0)
		return 0;
	const uint64_t nb = (src_bytes + block_size - 1) / block_size, nf = (nb + bpf - 1) / bpf;
	return src_bytes + nb * (block_size / 255u + 16u + 8u) + nf * 15u + 64u;
}

void la_launch_lz4_compress(hipStream_t s, const uint8_t *d_src, uint64_t src_bytes, uint32_t block_size,
    uint32_t bpf, uint32_t flags, uint8_t *d_out, uint64_t out_cap, uint64_t *d_out_bytes, uint8_t *ws)
{
	const uint32_t nb = (uint32_t)((src_bytes + block_size - 1) / block_size);
	const uint32_t nf = (nb + bpf - 1) / bpf;
	const uint32_t stride = lz4c_stride(block_size);
	lz4c_ws w;
	lz4c_carve(&w, ws, nb, nf, stride);
	if (nb == 0) {
		(void)hipMemsetAsync(d_out_bytes, 0, 8, s);
		return;
	}
	hipLaunchKernelGGL(lz4_compress_blocks_kernel, dim3(nb), dim3(64), 0, s, d_src, src_bytes, block_size, nb, w.tmp, stride, w.csize);
	if (flags & LA_LZ4C_CONTENT_SUM)
		hipLaunchKernelGGL(frame_sums_kernel<lz4c_xxh32>, dim3((nf + 15) / 16), dim3(64), 0, s, d_src, src_bytes,
		    (uint64_t)bpf * block_size, nf, w.fsum);
	hipLaunchKernelGGL(lz4c_sizes_kernel, dim3((nb + 255) / 256), dim3(256), 0, s, w.csize, src_bytes, block_size, nb, bpf, flags, w.contrib);
	la_launch_scan_u32(s, w.contrib, nb, w.off, w.scan);
	hipLaunchKernelGGL(lz4_pack_frames_kernel, dim3(nb), dim3(256), 0, s, d_src, src_bytes, block_size, nb, bpf, flags,
	    w.tmp, stride, w.csize, w.off, w.fsum, d_out, out_cap, d_out_bytes);
}
