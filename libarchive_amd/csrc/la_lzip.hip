/*
 * la_lzip.hip -- lzip on the device: the member-header scan behind la_gpu_lzip_scan and the member decode behind
 * la_gpu_lzip_decode.
 *
 * SCAN.  A workgroup of 256 threads takes a tile of 4096 bytes: every thread copies its 16 bytes to LDS with one
 * 16-byte load (coalesced: a wave reads 1 KiB in a row), the first lanes add the 16 bytes behind the tile, so a shape
 * that straddles the tile's edge is seen by the tile it starts in.  Each thread then reads its span and the 8 bytes
 * behind it back as three 64-bit LDS words and tests the 16 offsets in registers; no byte is loaded from global memory
 * twice.  Two passes around a prefix sum, as la_gpu_bzip2_scan does: count, then write in ascending order.
 *
 * DECODE.  One workgroup of one wave per member, as xz_decode_kernel; the rules are la_lzip_dev.h's, which calls the
 * symbol loop of la_xz_dev.h.  All 64 lanes run the one range-coder chain in step on the same values.  The model is fixed
 * at 1846 + 768 * 8 entries: 15 980 bytes of LDS.  The compiled kernel (gfx950, -O3, -Rpass-analysis=kernel-resource-usage)
 * reports 16 016 bytes of LDS per workgroup, 14 VGPRs, 96 SGPRs and no scratch: LDS bounds residency at
 * 160 KiB / 16 016 = 10 workgroups (one wave each) per CU, where xz_decode_kernel's 28 328 bytes give 5; the registers
 * would allow 8 waves per SIMD.
 * CRC32 comes from la_launch_crc32_many over jobs the decode kernel writes; a last launch puts the value into the result
 * and compares it with the trailer's where the entry carries one.
 */
#include "la_dev.h"

#define LA_XZ_FN static __host__ __device__ __forceinline__
#include "la_lzip_dev.h"

#define LZ_TPB  256u
#define LZ_SPAN 16u
#define LZ_TILE (LZ_TPB * LZ_SPAN)

/* write == 0: counts[t] = shapes that start in thread t's 16 bytes; write == 1: they go to out[offs[t] ...) */
__global__ __launch_bounds__(LZ_TPB) void lzip_scan_kernel(const uint8_t *__restrict__ src, uint64_t n, uint64_t nthreads,
    uint32_t *__restrict__ counts, const uint64_t *__restrict__ offs, uint64_t *__restrict__ out, uint32_t cap, uint32_t *d_count, int write)
{
	__shared__ __attribute__((aligned(16))) uint8_t tile[LZ_TILE + LZ_SPAN];
	const uint64_t tile0 = (uint64_t)blockIdx.x * LZ_TILE;
	const uint64_t base = tile0 + (uint64_t)threadIdx.x * LZ_SPAN;
	uint8_t *mine = tile + threadIdx.x * LZ_SPAN;
	if (base + LZ_SPAN <= n) {
		uint4 v;
		__builtin_memcpy(&v, src + base, LZ_SPAN);
		*(uint4 *)(void *)mine = v;
	} else {
		for (uint32_t k = 0; k < LZ_SPAN; k++)
			mine[k] = base + k < n ? src[base + k] : (uint8_t)0;
	}
	if (threadIdx.x < LZ_SPAN) {
		const uint64_t at = tile0 + LZ_TILE + threadIdx.x;
		tile[LZ_TILE + threadIdx.x] = at < n ? src[at] : (uint8_t)0;
	}
	__syncthreads();
	const uint64_t t = (uint64_t)blockIdx.x * LZ_TPB + threadIdx.x;
	if (t >= nthreads)
		return;
	const uint64_t *w = (const uint64_t *)(const void *)mine;
	const uint64_t w0 = w[0], w1 = w[1], w2 = w[2];
	uint32_t cnt = 0;
	const uint64_t o = write ? offs[t] : 0;
	for (uint32_t i = 0; i < LZ_SPAN && base + i + 6 <= n; i++) {
		const uint64_t a = i < 8 ? w0 : w1, b = i < 8 ? w1 : w2;
		const uint32_t s = (i & 7u) * 8u;
		const uint64_t v = s ? (a >> s) | (b << (64u - s)) : a;	/* the 8 bytes at offset base + i, little-endian */
		const uint32_t log2dic = (uint32_t)(v >> 40) & 31u;
		if ((uint32_t)v != 0x50495A4Cu || ((v >> 32) & 0xFFu) > 1u || log2dic < 12u || log2dic > 29u)
			continue;
		if (write && o + cnt < cap)
			out[o + cnt] = base + i;
		cnt++;
	}
	if (!write)
		counts[t] = cnt;
	else if (t == 0) {
		const uint64_t tot = offs[nthreads];
		*d_count = tot > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)tot;
	}
}

uint64_t la_lzip_scan_ws_bytes(uint64_t src_bytes)
{
	const uint64_t nt = (src_bytes + LZ_SPAN - 1) / LZ_SPAN;
	return ((nt * 4 + 255) & ~255ull) + (((nt + 1) * 8 + 255) & ~255ull) + la_scan_scratch_bytes((uint32_t)nt) + 256;
}

void la_launch_lzip_scan(hipStream_t s, const uint8_t *d_src, uint64_t src_bytes, uint64_t *d_offs, uint32_t cap, uint32_t *d_count, uint8_t *ws)
{
	const uint64_t nt = (src_bytes + LZ_SPAN - 1) / LZ_SPAN;
	if (nt == 0) {
		(void)hipMemsetAsync(d_count, 0, 4, s);
		return;
	}
	la_carve cv = { ws, 0 };
	uint32_t *counts = cv.take<uint32_t>(nt, 256);
	uint64_t *offs = cv.take<uint64_t>(nt + 1, 256);
	void *scratch = cv.take<uint8_t>(la_scan_scratch_bytes((uint32_t)nt), 256);
	const uint32_t grid = (uint32_t)((nt + LZ_TPB - 1) / LZ_TPB);
	hipLaunchKernelGGL(lzip_scan_kernel, dim3(grid), dim3(LZ_TPB), 0, s, d_src, src_bytes, nt, counts, (const uint64_t *)offs, d_offs, cap, d_count, 0);
	la_launch_scan_u32(s, counts, (uint32_t)nt, offs, scratch);
	hipLaunchKernelGGL(lzip_scan_kernel, dim3(grid), dim3(LZ_TPB), 0, s, d_src, src_bytes, nt, counts, (const uint64_t *)offs, d_offs, cap, d_count, 1);
}

__global__ __launch_bounds__(64) void lzip_decode_kernel(const uint8_t *d_src, uint64_t src_bytes, const la_lzip_member *d_members, uint32_t n,
    uint8_t *d_dst, uint64_t dst_total, la_lzip_result *d_results, la_hash_job *d_jobs)
{
	__shared__ uint16_t probs[LA_LZIP_PROBS];
	__shared__ la_xz_lzma lz;
	__shared__ la_lzip_result res;
	const uint32_t b = blockIdx.x;
	if (b >= n)
		return;
	const la_lzip_member m = d_members[b];
	la_hash_job job = { m.dst_off, 0u, 0u };
	/* a table entry that points outside the two buffers is not decoded at all */
	if (!la_lzip_entry_ok(&m, src_bytes, dst_total)) {
		if (threadIdx.x == 0) {
			const la_lzip_result bad = { LA_ST_LZIP_REFUSED, 0u, 0u, 0u, 0u };
			d_results[b] = bad;
			job.off = 0;
			d_jobs[b] = job;
		}
		return;
	}
	la_lzip_member_decode(d_src, src_bytes, &m, d_dst + m.dst_off, probs, &lz, &res);
	__syncthreads();
	if (threadIdx.x == 0) {
		d_results[b] = res;
		job.len = (uint32_t)res.out_len;	/* (at most dst_cap, which la_lzip_entry_ok keeps below 2^32) */
		d_jobs[b] = job;
	}
}

__global__ __launch_bounds__(256) void lzip_finish_kernel(const la_lzip_member *d_members, uint32_t n, la_lzip_result *d_results, const uint32_t *d_crc32)
{
	const uint32_t b = blockIdx.x * 256u + threadIdx.x;
	if (b >= n || d_results[b].status == LA_ST_LZIP_REFUSED)
		return;
	const la_lzip_member m = d_members[b];
	const uint32_t crc = d_crc32[b];
	d_results[b].crc32 = crc;
	d_results[b].status = la_lzip_crc_verdict(&m, d_results[b].status, crc);
}

uint64_t la_lzip_workspace_bytes(uint32_t n)
{
	return (((uint64_t)n * sizeof(la_hash_job) + 255u) & ~(uint64_t)255u) + (uint64_t)n * sizeof(uint32_t) + 256u;
}

void la_launch_lzip_decode(hipStream_t s, const la_lzip_batch *bt, uint8_t *ws)
{
	if (bt->n == 0)
		return;
	la_hash_job *jobs = (la_hash_job *)ws;
	uint32_t *crc = (uint32_t *)(ws + (((uint64_t)bt->n * sizeof(la_hash_job) + 255u) & ~(uint64_t)255u));
	hipLaunchKernelGGL(lzip_decode_kernel, dim3(bt->n), dim3(64), 0, s, bt->d_src, bt->src_bytes, bt->d_members, bt->n, bt->d_dst, bt->dst_cap,
	    bt->d_results, jobs);
	la_launch_crc32_many(s, bt->d_dst, jobs, bt->n, crc);
	hipLaunchKernelGGL(lzip_finish_kernel, dim3((bt->n + 255u) / 256u), dim3(256), 0, s, bt->d_members, bt->n, bt->d_results, crc);
}
