/*
 * la_lzo_comp.hip -- la_gpu_lzop_compress: a window of input into lzop blocks, back to back (the data plane of the lzop
 * write filter, host/la_write_lzop.c).
 *
 * Replaces, for a whole window per call, what libarchive/archive_write_add_filter_lzop.c does per block on the host:
 * lzo1x_1_compress of one block (:334-351), the Adler-32 of its input (:361), the three info words (:359-366) and the
 * stored form where the stream does not shrink the block (:364-381).  The header and the closing word are the host's.
 * The bytes are NOT liblzo2's (an LZO1X stream is not unique): parity for this direction is the round trip.
 *
 * How a sequence becomes bytes is la_lzo_enc_dev.h's, the text the CPU stand-in of the tests compiles too; this file
 * finds the sequences and moves the bytes.
 *
 *   lzop_compress_blocks_kernel   ONE WAVE per block of at most 64 KiB.  The 4096-entry table of 16-bit positions in
 *       LDS, matched by lz77_match (la_comp_common.h) with matches that may start up to n - 4 and end at n (LZO1X has no
 *       end-of-block margins) and no candidate further back than 49151.  Its emit runs the emitter wave-cooperatively:
 *       instruction bytes and the trail patch from lane 0, zero-run bytes a byte per lane, literals 64 bytes per step.
 *       The slot of a block is the block's own size: a stream that reaches it is only counted, since the block is
 *       stored then.  The wave also writes the block's Adler-32 job.
 *   la_launch_adler32_many        (la_hash.hip) the Adler-32 of every block's input.
 *   lzopc_sizes_kernel / scan     12 info bytes + payload of each block -> offsets.
 *   lzop_pack_blocks_kernel       one workgroup per block: BE32 usize, csize, adler32, then the stream or the input.
 * Nothing is stored at or behind out_cap; *d_out_bytes is the size needed, the lead included.
 */
#include "la_comp_common.h"

struct la_lzoe_io {
	const uint8_t *plain;
	uint8_t *out;
	uint32_t cap, lane;
};
#define LA_LZOE_HOOKS
#define LA_LZO_FN static __host__ __device__ __forceinline__	/* (the host takes the sizes) */
__device__ __forceinline__ void la_lzoe_put(la_lzoe_io *io, uint32_t at, uint32_t b)
{
	if (io->lane == 0 && at < io->cap)
		io->out[at] = (uint8_t)b;
}
__device__ __forceinline__ void la_lzoe_or(la_lzoe_io *io, uint32_t at, uint32_t bits)
{
	/* (lane 0 wrote the byte itself: program order) */
	if (io->lane == 0 && at < io->cap)
		io->out[at] = (uint8_t)(io->out[at] | bits);
}
__device__ __forceinline__ void la_lzoe_zeros(la_lzoe_io *io, uint32_t at, uint32_t n)
{
	for (uint32_t i = io->lane; i < n; i += 64)
		if (at + i < io->cap)
			io->out[at + i] = 0;
}
__device__ __forceinline__ void la_lzoe_literals(la_lzoe_io *io, uint32_t at, uint32_t ip, uint32_t n)
{
	if (at >= io->cap)
		return;
	const uint32_t room = io->cap - at;
	wave_copy(io->out + at, io->plain + ip, n < room ? n : room, io->lane);
}
#include "la_lzo_enc_dev.h"

__global__ __launch_bounds__(64) void lzop_compress_blocks_kernel(const uint8_t *__restrict__ src, uint64_t src_bytes,
    uint32_t block_size, uint32_t n_blocks, uint8_t *__restrict__ tmp, uint32_t tmp_stride, uint32_t *__restrict__ csize,
    la_hash_job *__restrict__ jobs)
{
	__shared__ uint16_t tab[1u << LZ77_HASH_BITS];
	const uint32_t bi = blockIdx.x, lane = threadIdx.x;
	if (bi >= n_blocks)
		return;
	const uint64_t so = (uint64_t)bi * block_size;
	const uint32_t n = (uint32_t)(src_bytes - so < block_size ? src_bytes - so : block_size);
	for (uint32_t i = lane; i < (1u << LZ77_HASH_BITS); i += 64)
		tab[i] = 0;
	__syncthreads();

	/* the stream's room is the block's own size (<= tmp_stride): what reaches it is stored */
	la_lzoe_io io = { src + so, tmp + (uint64_t)bi * tmp_stride, n, lane };
	la_lzoe_state st;
	la_lzoe_begin(&st);
	uint32_t anchor = 0;	/* wave-uniform */
	if (n >= 4u)
		anchor = lz77_match(tab, io.plain, n - 4u, n, lane,
		    [&](uint32_t pf, uint32_t mf, uint32_t cf, uint32_t from) {
			la_lzoe_seq(&io, &st, from, pf - from, pf - cf, mf);
		}, LA_LZOE_MAX_DIST);
	const uint32_t stream = la_lzoe_end(&io, &st, anchor, n - anchor);
	if (lane == 0) {
		csize[bi] = stream;
		la_hash_job j;
		j.off = so; j.len = n; j.seed = 1u;
		jobs[bi] = j;
	}
}

__device__ __forceinline__ uint32_t lzopc_block_bytes(uint64_t src_bytes, uint32_t block_size, uint32_t i)
{
	const uint64_t so = (uint64_t)i * block_size;
	return (uint32_t)(src_bytes - so < block_size ? src_bytes - so : block_size);
}

__global__ __launch_bounds__(256) void lzopc_sizes_kernel(const uint32_t *__restrict__ csize, uint64_t src_bytes, uint32_t block_size,
    uint32_t n_blocks, uint32_t *__restrict__ contrib)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n_blocks)
		return;
	const uint32_t n = lzopc_block_bytes(src_bytes, block_size, i);
	contrib[i] = 12u + (csize[i] < n ? csize[i] : n);
}

__global__ __launch_bounds__(256) void lzop_pack_blocks_kernel(const uint8_t *__restrict__ src, uint64_t src_bytes, uint32_t block_size,
    uint32_t n_blocks, uint32_t lead, const uint8_t *__restrict__ tmp, uint32_t tmp_stride, const uint32_t *__restrict__ csize,
    const uint32_t *__restrict__ sums, const uint64_t *__restrict__ off, uint8_t *out, uint64_t out_cap, uint64_t *__restrict__ out_bytes)
{
	const uint32_t bi = blockIdx.x, tid = threadIdx.x;
	if (bi >= n_blocks)
		return;
	if (bi == 0 && tid == 0)
		*out_bytes = lead + off[n_blocks];
	const uint32_t n = lzopc_block_bytes(src_bytes, block_size, bi);
	const bool stored = csize[bi] >= n;		/* archive_write_add_filter_lzop.c:364-381 */
	const uint32_t pay = stored ? n : csize[bi];
	const uint8_t *payload = stored ? src + (uint64_t)bi * block_size : tmp + (uint64_t)bi * tmp_stride;
	const uint64_t o = lead + off[bi];
	if (tid < 12u && o + tid < out_cap) {
		const uint32_t word = tid < 4u ? n : tid < 8u ? pay : sums[bi];
		out[o + tid] = (uint8_t)(word >> (8u * (3u - (tid & 3u))));
	}
	for (uint32_t i = tid; i < pay; i += 256u)
		if (o + 12u + i < out_cap)
			out[o + 12u + i] = payload[i];
}

__global__ __launch_bounds__(1) void lzopc_lead_only_kernel(uint32_t lead, uint64_t *out_bytes)
{
	*out_bytes = lead;
}

struct lzopc_ws {
	uint8_t *tmp;
	uint32_t *csize, *contrib, *sums;
	la_hash_job *jobs;
	uint64_t *off;
	uint8_t *scan;
};

static uint32_t lzopc_stride(uint32_t block_size) { return la_lzoe_slot_bytes(block_size); }

/* the launcher's workspace on `base` (null: sizes only); returns its bytes */
static uint64_t lzopc_carve(lzopc_ws *w, uint8_t *base, uint64_t nb, uint32_t stride)
{
	la_carve c = { base, 0 };
	w->tmp = c.take<uint8_t>(nb * stride, 256);
	w->csize = c.take<uint32_t>(nb, 256);
	w->contrib = c.take<uint32_t>(nb, 256);
	w->sums = c.take<uint32_t>(nb, 256);
	w->jobs = c.take<la_hash_job>(nb, 256);
	w->off = c.take<uint64_t>(nb + 1, 256);
	w->scan = c.take<uint8_t>(la_scan_scratch_bytes((uint32_t)nb), 256);
	return c.off + 256u;
}

uint64_t la_lzop_compress_ws_bytes(uint64_t src_bytes, uint32_t block_size)
{
	lzopc_ws w;
	return lzopc_carve(&w, nullptr, (src_bytes + block_size - 1) / block_size, lzopc_stride(block_size));
}

void la_launch_lzop_compress(hipStream_t s, const la_lzopc_batch *bt, uint8_t *ws)
{
	const uint32_t nb = (uint32_t)((bt->src_bytes + bt->block_size - 1) / bt->block_size);
	const uint32_t stride = lzopc_stride(bt->block_size);
	lzopc_ws w;
	lzopc_carve(&w, ws, nb, stride);
	if (nb == 0) {
		hipLaunchKernelGGL(lzopc_lead_only_kernel, dim3(1), dim3(1), 0, s, bt->lead_bytes, bt->d_out_bytes);
		return;
	}
	hipLaunchKernelGGL(lzop_compress_blocks_kernel, dim3(nb), dim3(64), 0, s, bt->d_src, bt->src_bytes, bt->block_size, nb, w.tmp, stride,
	    w.csize, w.jobs);
	la_launch_adler32_many(s, bt->d_src, w.jobs, nb, w.sums);
	hipLaunchKernelGGL(lzopc_sizes_kernel, dim3((nb + 255) / 256), dim3(256), 0, s, w.csize, bt->src_bytes, bt->block_size, nb, w.contrib);
	la_launch_scan_u32(s, w.contrib, nb, w.off, w.scan);
	hipLaunchKernelGGL(lzop_pack_blocks_kernel, dim3(nb), dim3(256), 0, s, bt->d_src, bt->src_bytes, bt->block_size, nb, bt->lead_bytes,
	    w.tmp, stride, w.csize, w.sums, w.off, bt->d_out, bt->out_cap, bt->d_out_bytes);
}
