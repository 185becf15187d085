/*
 * la_lzip_comp.hip -- la_gpu_lzip_compress: a window of input into complete lzip members, back to back.
 *
 * The rules (member size by level, the chain, the end marker, header, trailer, the bound) are la_lzip_enc_dev.h's over
 * la_xz_enc_dev.h's matcher, symbol choice and range coder, the same text the CPU stand-in of the tests compiles.
 * Members are independent, so the parallel unit is the MEMBER: a 64 MiB window is 1 024 chains at levels 0..6 and 256
 * at levels 7..9.
 *
 * MEMBER.  One workgroup of one wave per member, LDS as in xzc_chunk_kernel: the model (7 990 16-bit entries), the
 * 4 096-entry match table and the step's 64 match results.  The chain is la_xz_comp.hip's (match per lane, symbols and
 * range coder with every lane on the same values, bytes leave from lane 0) into the member's slot of the workspace;
 * behind it the marker and the flush.  There is no signalling between waves and no loop without a bound.
 * Behind the chain the wave computes the CRC32 of the member's input: a table in the match table's place, 64 lane
 * segments, combined on lane 0 by x^(8 n) mod P.
 *
 * PACK.  A prefix sum over the members' framed sizes, then one workgroup per member copies the slot to its place and
 * thread 0 writes header and trailer.  Nothing is stored at or behind out_cap; *d_out_bytes is the size needed.
 * No input at all is one member of no data through the same two kernels.
 */
#include "la_dev.h"

#define LA_XZ_FN static __host__ __device__ __forceinline__
#define LA_XZC_LANE_LOOP(l) for (uint32_t l = threadIdx.x; l < 64u; l += 64u)
#define LA_XZC_SYNC() __syncthreads()
#define LA_XZC_TAB_MAX(p, v) atomicMax((p), (v))
#define LA_XZC_PUT(p, v) do { if (threadIdx.x == 0) *(p) = (v); } while (0)
#include "la_lzip_enc_dev.h"

__global__ __launch_bounds__(64) void lzc_member_kernel(const uint8_t *__restrict__ d_src, uint64_t src_bytes, uint32_t n_members,
    uint32_t member_bytes, uint32_t slot_bytes, uint8_t *slots, uint32_t *member_size, uint32_t *member_stream, uint32_t *member_crc)
{
	__shared__ uint16_t probs[LA_XZC_PROBS];
	__shared__ uint32_t tab[LA_XZC_TAB];
	__shared__ uint32_t m_len[64], m_cand[64];
	const uint32_t c = blockIdx.x, lane = threadIdx.x;
	if (c >= n_members)
		return;
	const uint64_t off = (uint64_t)c * member_bytes;
	const uint32_t n = src_bytes - off < member_bytes ? (uint32_t)(src_bytes - off) : member_bytes;
	const uint8_t *src = d_src + off;	/* (n == 0: never read) */
	const uint32_t stream = la_lzc_member(src, n, probs, tab, m_len, m_cand, slots + (uint64_t)c * slot_bytes, slot_bytes);
	/* the check: a segment per lane (the table takes the match table's place), combined on lane 0 */
	__syncthreads();
	uint32_t *table = tab, *seg_crc = tab + 256;
	for (uint32_t i = lane; i < 256u; i += 64u)
		table[i] = la_lzc_crc32_entry(i);
	__syncthreads();
	const uint32_t seg = (n + 63u) / 64u;
	const uint32_t from = seg * lane < n ? seg * lane : n;
	const uint32_t len = n - from < seg ? n - from : seg;
	seg_crc[lane] = la_lzc_crc32(table, src + from, len, 0);
	__syncthreads();
	if (lane == 0) {
		const uint32_t sh = la_lzc_crc32_shift(seg);
		uint32_t acc = seg_crc[0];
		for (uint32_t j = 1; j < 64u; j++) {
			const uint32_t f = seg * j;
			if (f >= n)
				break;
			const uint32_t l = n - f < seg ? n - f : seg;
			acc = la_lzc_crc32_mul(l == seg ? sh : la_lzc_crc32_shift(l), acc) ^ seg_crc[j];
		}
		member_crc[c] = acc;
		member_stream[c] = stream;
		member_size[c] = LA_LZC_HEADER_BYTES + stream + LA_LZC_TRAILER_BYTES;
	}
}

__global__ __launch_bounds__(256) void lzc_pack_kernel(uint64_t src_bytes, uint32_t n_members, uint32_t member_bytes, uint32_t slot_bytes,
    uint32_t level, const uint8_t *__restrict__ slots, const uint32_t *__restrict__ member_stream, const uint32_t *__restrict__ member_crc,
    const uint64_t *__restrict__ member_off, uint8_t *d_out, uint64_t out_cap, uint64_t *d_out_bytes)
{
	const uint32_t c = blockIdx.x, t = threadIdx.x;
	if (c >= n_members)
		return;
	if (c == 0 && t == 0)
		*d_out_bytes = member_off[n_members];
	const uint64_t off = (uint64_t)c * member_bytes;
	const uint32_t n = src_bytes - off < member_bytes ? (uint32_t)(src_bytes - off) : member_bytes;
	const uint64_t at = member_off[c];
	/* the slot holds the stream up to its end only; the bound says a stream never reaches it */
	const uint32_t stream = member_stream[c], held = stream < slot_bytes ? stream : slot_bytes;
	const uint8_t *s = slots + (uint64_t)c * slot_bytes;
	for (uint32_t i = t; i < held; i += 256u)
		if (at + LA_LZC_HEADER_BYTES + i < out_cap)
			d_out[at + LA_LZC_HEADER_BYTES + i] = s[i];
	if (t != 0)
		return;
	uint8_t h[LA_LZC_TRAILER_BYTES];
	la_lzc_header(h, level);
	for (uint32_t i = 0; i < LA_LZC_HEADER_BYTES; i++)
		if (at + i < out_cap)
			d_out[at + i] = h[i];
	la_lzc_trailer(h, member_crc[c], n, stream);
	const uint64_t tail = at + LA_LZC_HEADER_BYTES + stream;
	for (uint32_t i = 0; i < LA_LZC_TRAILER_BYTES; i++)
		if (tail + i < out_cap)
			d_out[tail + i] = h[i];
}

struct lzc_ws {
	uint8_t *slots;
	uint32_t *member_size, *member_stream, *member_crc;
	uint64_t *member_off;
	uint8_t *scan;
};

static uint64_t lzc_carve(uint8_t *base, uint64_t src_bytes, uint32_t level, lzc_ws *w)
{
	const uint64_t n_members = la_lzc_members(src_bytes, level);
	la_carve cv = { base, 0 };
	w->slots = cv.take<uint8_t>(n_members * la_lzc_slot_bytes(la_lzc_member_bytes(level)), 256);
	w->member_size = cv.take<uint32_t>(n_members, 256);
	w->member_stream = cv.take<uint32_t>(n_members, 256);
	w->member_crc = cv.take<uint32_t>(n_members, 256);
	w->member_off = cv.take<uint64_t>(n_members + 1u, 256);
	w->scan = cv.take<uint8_t>(la_scan_scratch_bytes((uint32_t)n_members), 256);
	return cv.off + 256u;
}

uint32_t la_lzip_compress_member_bytes(uint32_t level)
{
	return la_lzc_member_bytes(level);
}

uint64_t la_lzip_compress_ws_bytes(uint64_t src_bytes, uint32_t level)
{
	lzc_ws w;
	return lzc_carve(NULL, src_bytes, level, &w);
}

uint64_t la_lzip_compress_bound(uint64_t src_bytes, uint32_t level)
{
	return la_lzc_bound(src_bytes, level);
}

void la_launch_lzip_compress(hipStream_t s, const la_lzc_batch *bt, uint8_t *ws, const la_stage_hook *hook)
{
	const uint32_t n_members = (uint32_t)la_lzc_members(bt->src_bytes, bt->level);
	const uint32_t member_bytes = la_lzc_member_bytes(bt->level), slot_bytes = (uint32_t)la_lzc_slot_bytes(member_bytes);
	lzc_ws w;
	lzc_carve(ws, bt->src_bytes, bt->level, &w);
	hook->mark(hook->cx, "lzc_members");
	hipLaunchKernelGGL(lzc_member_kernel, dim3(n_members), dim3(64), 0, s, bt->d_src, bt->src_bytes, n_members, member_bytes, slot_bytes, w.slots,
	    w.member_size, w.member_stream, w.member_crc);
	hook->mark(hook->cx, "lzc_pack");
	la_launch_scan_u32(s, w.member_size, n_members, w.member_off, w.scan);
	hipLaunchKernelGGL(lzc_pack_kernel, dim3(n_members), dim3(256), 0, s, bt->src_bytes, n_members, member_bytes, slot_bytes, bt->level, w.slots,
	    w.member_stream, w.member_crc, w.member_off, bt->d_out, bt->out_cap, bt->d_out_bytes);
	hook->mark(hook->cx, NULL);
}
