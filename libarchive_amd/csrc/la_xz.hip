/*
 * la_xz.hip -- la_gpu_xz_decode: the blocks of .xz streams, one workgroup of one wave per block.
 *
 * DECODE.  The rules are la_xz_dev.h's, the same text the CPU stand-in of the tests compiles.  The probability model
 * (at most 1846 + (768 << 4) 16-bit entries, 28 KiB) and the decoder state live in LDS; the dictionary is the block's
 * own output in d_dst.  LZMA2 inside a block is ONE serial range-coder chain: every bit decides which probability the
 * next bit reads.  All 64 lanes run that chain in step on the same values (the LDS reads are broadcasts, the stores of a
 * literal or a match leave as one request), so the control flow is uniform and the parts that are not a chain can use
 * the whole wave without any signalling between lanes: an uncompressed chunk is copied 64 bytes at a time.  What bounds
 * the kernel is the chain: LDS read, multiply, compare, LDS write per bit, a global byte load per normalisation, and a
 * store-to-load round trip for every match that overlaps its own output.
 *
 * VERIFY.  A second launch, again a wave per block: header sizes against what the decoder found, the zero padding, then
 * the check.  CRC32 comes from la_launch_crc32_many over jobs the decode kernel wrote; CRC64 is computed here, a segment
 * per lane, the segments combined by multiplication with x^(8 n) mod P; SHA-256 is one chain on one lane.
 */
#include "la_dev.h"

#define LA_XZ_FN static __host__ __device__ __forceinline__
#define LA_XZ_COPY(d, s, n) do { \
		for (uint64_t i_ = threadIdx.x; i_ < (n); i_ += 64) (d)[i_] = (s)[i_]; \
		__syncthreads(); \
	} while (0)
#include "la_xz_dev.h"
#include "la_xz_filters_dev.h"	/* la_xz_chain_valid */

/* d_chains: the chain table of a batch with LA_XZ_BATCH_CHAINS, else null */
__global__ __launch_bounds__(64) void xz_decode_kernel(const uint8_t *d_src, uint64_t src_bytes, const la_xz_block *d_blocks,
    const la_xz_chain *d_chains, uint32_t n, uint8_t *d_dst, uint64_t dst_total, la_xz_result *d_results, la_hash_job *d_jobs)
{
	__shared__ uint16_t probs[LA_XZ_PROBS_MAX];
	__shared__ la_xz_lzma lz;
	__shared__ la_xz_result res;
	const uint32_t b = blockIdx.x;
	if (b >= n)
		return;
	const la_xz_block blk = d_blocks[b];
	la_hash_job job = { blk.dst_off, 0u, 0u };
	/* a table entry that points outside the two buffers, or whose chain cannot be undone, is not decoded at all */
	bool refused = blk.src_off > src_bytes || blk.dst_off > dst_total || blk.dst_cap > dst_total - blk.dst_off || blk.dst_cap > LA_XZ_DST_CAP_MAX ||
	    (blk.uncomp_size != LA_XZ_UNKNOWN && blk.uncomp_size > blk.dst_cap);
	if (!refused && d_chains) {
		const la_xz_chain ch = d_chains[b];
		refused = !la_xz_chain_valid(&ch);
	}
	if (refused) {
		if (threadIdx.x == 0) {
			const la_xz_result bad = { LA_ST_XZ_SIZE, 0u, 0u, 0u, 0u };
			d_results[b] = bad;
			d_jobs[b] = job;
		}
		return;
	}
	uint64_t lim = src_bytes;
	uint32_t lim_status = LA_ST_XZ_TRUNCATED;
	if (blk.comp_size != LA_XZ_UNKNOWN && blk.comp_size <= src_bytes - blk.src_off) {
		lim = blk.src_off + blk.comp_size;
		lim_status = LA_ST_XZ_SIZE;
	}
	const bool sized = blk.uncomp_size != LA_XZ_UNKNOWN;
	la_xz_block_decode(d_src, blk.src_off, lim, lim_status, d_dst + blk.dst_off, sized ? blk.uncomp_size : blk.dst_cap,
	    sized ? (uint32_t)LA_ST_XZ_SIZE : (uint32_t)LA_ST_XZ_OUT_FULL, blk.dict_size, probs, &lz, &res);
	__syncthreads();
	if (threadIdx.x == 0) {
		la_xz_result r = res;
		if (r.status == LA_ST_OK && !la_xz_sizes_agree(&blk, &r))
			r.status = LA_ST_XZ_SIZE;
		d_results[b] = r;
		if (r.status == LA_ST_OK && blk.check_id == 1u)
			job.len = (uint32_t)r.out_len;
		d_jobs[b] = job;
	}
}

__global__ __launch_bounds__(64) void xz_verify_kernel(const uint8_t *d_src, uint64_t src_bytes, const la_xz_block *d_blocks, uint32_t n,
    const uint8_t *d_dst, la_xz_result *d_results, const uint32_t *d_crc32)
{
	__shared__ uint64_t table[256];
	__shared__ uint64_t seg_crc[64];
	__shared__ uint8_t have[64];
	const uint32_t b = blockIdx.x, lane = threadIdx.x;
	if (b >= n)
		return;
	const la_xz_result r = d_results[b];
	if (r.status != LA_ST_OK)
		return;
	const la_xz_block blk = d_blocks[b];
	const uint8_t *out = d_dst + blk.dst_off;
	int supported = 1;
	if (blk.check_id == 1u) {
		if (lane < 4u)
			have[lane] = (uint8_t)(d_crc32[b] >> (8u * lane));
	} else if (blk.check_id == 4u) {
		for (uint32_t i = lane; i < 256u; i += 64u)
			table[i] = la_xz_crc64_entry(i);
		__syncthreads();
		const uint64_t seg = (r.out_len + 63u) / 64u;
		const uint64_t from = seg * lane < r.out_len ? seg * lane : r.out_len;
		const uint64_t len = r.out_len - from < seg ? r.out_len - from : seg;
		seg_crc[lane] = la_xz_crc64(table, out + from, len, 0);
		__syncthreads();
		if (lane == 0) {
			/* every segment but the last non-empty one is seg bytes long */
			const uint64_t sh = la_xz_crc64_shift(seg);
			uint64_t acc = seg_crc[0];
			for (uint32_t j = 1; j < 64u; j++) {
				const uint64_t f = seg * j;
				if (f >= r.out_len)
					break;
				const uint64_t l = r.out_len - f < seg ? r.out_len - f : seg;
				acc = la_xz_crc64_mul(l == seg ? sh : la_xz_crc64_shift(l), acc) ^ seg_crc[j];
			}
			for (uint32_t i = 0; i < 8u; i++)
				have[i] = (uint8_t)(acc >> (8u * i));
		}
	} else if (blk.check_id == 10u) {
		if (lane == 0)
			la_xz_sha256_all(out, r.out_len, have);
	} else if (blk.check_id != 0u) {
		supported = 0;
	}
	__syncthreads();
	if (lane == 0) {
		const uint32_t st = la_xz_block_tail(d_src, src_bytes, blk.src_off, r.consumed, blk.check_id, have, supported);
		if (st != LA_ST_OK)
			d_results[b].status = st;
	}
}

uint64_t la_xz_workspace_bytes(uint32_t n)
{
	return (((uint64_t)n * sizeof(la_hash_job) + 255u) & ~(uint64_t)255u) + (uint64_t)n * sizeof(uint32_t) + 256u;
}

void la_launch_xz_decode(hipStream_t s, const la_xz_batch *bt, uint8_t *ws)
{
	if (bt->n == 0)
		return;
	la_hash_job *jobs = (la_hash_job *)ws;
	const la_xz_chain *chains = (bt->reserved & LA_XZ_BATCH_CHAINS) ? (const la_xz_chain *)(bt->d_blocks + bt->n) : nullptr;
	hipLaunchKernelGGL(xz_decode_kernel, dim3(bt->n), dim3(64), 0, s, bt->d_src, bt->src_bytes, bt->d_blocks, chains, bt->n, bt->d_dst,
	    bt->dst_cap, bt->d_results, jobs);
}

void la_launch_xz_verify(hipStream_t s, const la_xz_batch *bt, uint8_t *ws)
{
	if (bt->n == 0)
		return;
	la_hash_job *jobs = (la_hash_job *)ws;
	uint32_t *crc = (uint32_t *)(ws + (((uint64_t)bt->n * sizeof(la_hash_job) + 255u) & ~(uint64_t)255u));
	la_launch_crc32_many(s, bt->d_dst, jobs, bt->n, crc);
	hipLaunchKernelGGL(xz_verify_kernel, dim3(bt->n), dim3(64), 0, s, bt->d_src, bt->src_bytes, bt->d_blocks, bt->n, bt->d_dst, bt->d_results, crc);
}
