/*
 * la_lzo.hip -- lzop blocks on the device: the launches behind la_gpu_lzop_decode.
 *
 * One WAVE per block, one pass: both sizes of a block stand in its header, so nothing has to be measured first.  The
 * rules are la_lzo_dev.h's; this file gives them wave-wide hooks.  The instruction chain stays wave-uniform (every
 * value of it comes out of v_readlane) and is fed from the 512-byte register window of the payload that
 * lz4_expand_general uses (la_dev.h: src_window).  Literal runs and matches move 64 bytes per step, one per lane.  A
 * match whose distance is below its length replicates its period (byte i comes from i mod distance), so every byte a
 * match reads was stored by an EARLIER instruction of this wave; wave_fence() stands between such a store and the read,
 * and only where the read reaches bytes stored since the last fence.  Stored blocks (src_len == dst_len) are copied by
 * the same launch, 1 KiB per wave and pass.
 *
 * Launches: jobs for the sums over the compressed bytes, CRC32 and Adler-32 of them (la_hash.hip), the decode (a block
 * whose sum fails is not decoded), CRC32 and Adler-32 of the decoded bytes, the last compare.  A block asks for at most
 * one kind of sum per side; the other launch sees a job of length 0 for it.
 *
 * 256 threads per workgroup = 4 blocks, no LDS.  Resource use is recorded in DESIGN.md.
 */
#include "la_zstd_common.h"	/* wave_fence */

struct la_lzo_io {
	src_window W;
	const uint8_t *src;
	uint8_t *dst;
	uint32_t visible;	/* output bytes [0, visible) are known to be visible to loads */
	int lane;
};

__device__ __forceinline__ uint32_t la_lzo_byte(la_lzo_io *io, uint32_t ip)
{
	return win_byte(io->W, io->src + ip, io->lane);
}

__device__ __forceinline__ void la_lzo_literals(la_lzo_io *io, uint32_t op, uint32_t ip, uint32_t n)
{
	for (uint32_t j = (uint32_t)io->lane; j < n; j += LA_WAVE)
		io->dst[op + j] = io->src[ip + j];
}

__device__ __forceinline__ void la_lzo_match(la_lzo_io *io, uint32_t op, uint32_t dist, uint32_t n)
{
	/* the source bytes are [op - dist, op - dist + min(n, dist)): all below op */
	const uint32_t span = n < dist ? n : dist;
	if (op - dist + span > io->visible) {
		wave_fence();
		io->visible = op;
	}
	const uint8_t *from = io->dst + (op - dist);
	for (uint32_t j = (uint32_t)io->lane; j < n; j += LA_WAVE)
		io->dst[op + j] = from[dist < n ? j % dist : j];
}

#define LA_LZO_HOOKS
#define LA_LZO_FN __device__ __forceinline__
#include "la_lzo_dev.h"

/* the hash jobs of one side of every block: the CRC32 launch reads jobs[0, n), the Adler-32 launch jobs[n, 2n) */
__device__ __forceinline__ void lzop_put_jobs(la_hash_job *jobs, uint32_t n, uint32_t b, uint32_t kind, uint64_t off, uint32_t len)
{
	const la_hash_job crc = { kind == LA_LZOP_SUM_CRC ? off : 0u, kind == LA_LZOP_SUM_CRC ? len : 0u, 0u };
	const la_hash_job adl = { kind == LA_LZOP_SUM_ADLER ? off : 0u, kind == LA_LZOP_SUM_ADLER ? len : 0u, 1u };
	jobs[b] = crc;
	jobs[n + b] = adl;
}

__global__ __launch_bounds__(256) void lzop_jobs_kernel(const la_lzop_block *__restrict__ blocks, uint32_t n, uint64_t src_bytes, uint64_t dst_total,
    la_hash_job *__restrict__ jobs)
{
	const uint32_t b = blockIdx.x * 256u + threadIdx.x;
	if (b >= n)
		return;
	const la_lzop_block k = blocks[b];
	const bool ok = la_lzop_entry_ok(&k, src_bytes, dst_total);
	lzop_put_jobs(jobs, n, b, ok ? la_lzop_sum_kind(k.flags, 0) : LA_LZOP_SUM_NONE, k.src_off, k.src_len);
}

__global__ __launch_bounds__(256) void lzop_decode_kernel(const uint8_t *__restrict__ src, uint64_t src_bytes, const la_lzop_block *__restrict__ blocks,
    uint32_t n, uint8_t *dst, uint64_t dst_total, la_lzop_result *__restrict__ results, la_hash_job *jobs, const uint32_t *__restrict__ sums)
{
	const int lane = threadIdx.x & 63;
	const uint32_t b = (uint32_t)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * 256u + threadIdx.x) >> 6));
	if (b >= n)
		return;
	const la_lzop_block k = blocks[b];
	la_lzop_result res = { LA_ST_OK, 0u, 0u, 0u, 0u };
	uint32_t ukind = LA_LZOP_SUM_NONE;
	if (!la_lzop_entry_ok(&k, src_bytes, dst_total))
		res.status = LA_ST_LZOP_REFUSED;
	else {
		const uint32_t ckind = la_lzop_sum_kind(k.flags, 0);
		if (ckind != LA_LZOP_SUM_NONE) {
			res.sum_c = sums[ckind == LA_LZOP_SUM_CRC ? b : n + b];
			if (res.sum_c != k.sum_c)
				res.status = LA_ST_LZOP_BAD_SUM_C;
		}
	}
	if (res.status == LA_ST_OK) {
		const uint8_t *s = src + k.src_off;
		uint8_t *d = dst + k.dst_off;
		if (k.src_len == k.dst_len) {
			/* stored block (lzop.c:435-440): bytes up to the output's 16-byte grid one by one, then 1 KiB per pass */
			uint32_t head = (16u - (uint32_t)((uintptr_t)d & 15u)) & 15u;
			if (head > k.src_len) head = k.src_len;
			if ((uint32_t)lane < head)
				d[lane] = s[lane];
			const uint32_t nvec = (k.src_len - head) >> 4;
			for (uint32_t j = (uint32_t)lane; j < nvec; j += LA_WAVE)
				*(uint4 *)(d + head + 16u * j) = ld_u128(s + head + 16u * j);
			for (uint32_t j = head + (nvec << 4) + (uint32_t)lane; j < k.src_len; j += LA_WAVE)
				d[j] = s[j];
			res.out_len = res.consumed = k.src_len;
		} else {
			la_lzo_io io;
			io.W.limit = src + src_bytes;
			win_reset(io.W, s, lane);
			io.src = s; io.dst = d; io.visible = 0; io.lane = lane;
			res.status = la_lzo1x_decode(&io, k.src_len, k.dst_len, &res.out_len, &res.consumed);
			if (res.status == LA_ST_OK)
				ukind = la_lzop_sum_kind(k.flags, 1);
		}
	}
	if (lane == 0) {
		results[b] = res;
		lzop_put_jobs(jobs, n, b, ukind, k.dst_off, k.dst_len);
	}
}

__global__ __launch_bounds__(256) void lzop_finish_kernel(const la_lzop_block *__restrict__ blocks, uint32_t n, la_lzop_result *results,
    const la_hash_job *__restrict__ jobs, const uint32_t *__restrict__ sums)
{
	const uint32_t b = blockIdx.x * 256u + threadIdx.x;
	if (b >= n)
		return;
	/* (the decode wrote a job with a length only for a block that ended well and asks for this sum) */
	const uint32_t at = jobs[b].len ? b : jobs[n + b].len ? n + b : 0xFFFFFFFFu;
	if (at == 0xFFFFFFFFu)
		return;
	const uint32_t sum = sums[at];
	results[b].sum_u = sum;
	if (sum != blocks[b].sum_u)
		results[b].status = LA_ST_LZOP_BAD_SUM_U;
}

static uint64_t lzop_jobs_bytes(uint32_t n)
{
	return ((uint64_t)2 * n * sizeof(la_hash_job) + 255u) & ~(uint64_t)255u;
}

uint64_t la_lzop_workspace_bytes(uint32_t n)
{
	return lzop_jobs_bytes(n) + (uint64_t)2 * n * sizeof(uint32_t) + 256u;
}

void la_launch_lzop_decode(hipStream_t s, const la_lzop_batch *bt, uint8_t *ws)
{
	const uint32_t n = bt->n;
	if (n == 0)
		return;
	la_hash_job *jobs = (la_hash_job *)ws;
	uint32_t *sums = (uint32_t *)(ws + lzop_jobs_bytes(n));
	const dim3 per_thread((n + 255u) / 256u), per_wave((n + 3u) / 4u);
	hipLaunchKernelGGL(lzop_jobs_kernel, per_thread, dim3(256), 0, s, bt->d_blocks, n, bt->src_bytes, bt->dst_cap, jobs);
	la_launch_crc32_many(s, bt->d_src, jobs, n, sums);
	la_launch_adler32_many(s, bt->d_src, jobs + n, n, sums + n);
	hipLaunchKernelGGL(lzop_decode_kernel, per_wave, dim3(256), 0, s, bt->d_src, bt->src_bytes, bt->d_blocks, n, bt->d_dst, bt->dst_cap, bt->d_results,
	    jobs, (const uint32_t *)sums);
	la_launch_crc32_many(s, bt->d_dst, jobs, n, sums);
	la_launch_adler32_many(s, bt->d_dst, jobs + n, n, sums + n);
	hipLaunchKernelGGL(lzop_finish_kernel, per_thread, dim3(256), 0, s, bt->d_blocks, n, bt->d_results, (const la_hash_job *)jobs, (const uint32_t *)sums);
}
