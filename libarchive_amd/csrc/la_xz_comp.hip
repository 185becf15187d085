/*
 * la_xz_comp.hip -- la_gpu_xz_compress: a window of input into complete .xz blocks, back to back.
 *
 * The rules (matcher, symbol choice, range coder, chunk and block framing, the stored decision) are la_xz_enc_dev.h's,
 * the same text the CPU stand-in of the tests compiles.  An LZMA2 chunk with a state reset starts a fresh range coder and
 * a fresh model while the dictionary carries on, so the parallel unit is the CHUNK: a 64 MiB window is 1 024 chains.
 *
 * CHUNK.  One workgroup of one wave per chunk.  The model (7 990 16-bit entries), the 4 096-entry match table and the
 * step's 64 match results live in LDS.  Per step of 64 positions:
 *   match    one position per lane: hash, candidate (all reads of the table, a barrier, then the lanes' own positions
 *            enter it by an LDS maximum, which is what the last lane of a loop would have left), extension byte by byte;
 *   symbols  the wave walks the step's positions in order, every lane on the same values (LDS reads are broadcasts), and
 *   code     runs the range coder bit by bit; the bytes leave from lane 0 into the chunk's slot of the workspace.
 * What bounds the kernel is that chain: LDS read, multiply, LDS write per bit, and a global load per literal and per
 * compared byte of a rep.  There is no signalling between waves and no loop without a bound.
 * Behind the chain the wave computes the CRC64 of the chunk's input, 64 segments combined by x^(8 n) mod P.
 *
 * PACK.  A prefix sum over the chunks' framed sizes, block sizes from it, a prefix sum over those, then one workgroup
 * per chunk copies the slot (or the input behind a three-byte header when the chunk is stored) to its place; the
 * block's first chunk writes the block header, its last the end marker, the padding and the CRC64 combined from the
 * chunks'.  Nothing is stored at or behind out_cap; *d_out_bytes is the size needed.
 */
#include "la_dev.h"

#define LA_XZ_FN static __host__ __device__ __forceinline__
#define LA_XZC_LANE_LOOP(l) for (uint32_t l = threadIdx.x; l < 64u; l += 64u)
#define LA_XZC_SYNC() __syncthreads()
#define LA_XZC_TAB_MAX(p, v) atomicMax((p), (v))
#define LA_XZC_PUT(p, v) do { if (threadIdx.x == 0) *(p) = (v); } while (0)
#include "la_xz_enc_dev.h"

#define XZC_CHUNKS_PER_BLOCK (LA_XZC_BLOCK_BYTES / LA_XZC_CHUNK_BYTES)

__global__ __launch_bounds__(64) void xzc_chunk_kernel(const uint8_t *__restrict__ d_src, uint64_t src_bytes, uint32_t n_chunks, uint32_t level,
    uint8_t *slots, uint32_t *chunk_size, uint32_t *chunk_payload, uint64_t *chunk_crc)
{
	__shared__ uint16_t probs[LA_XZC_PROBS];
	__shared__ __attribute__((aligned(8))) uint32_t tab[LA_XZC_TAB];
	__shared__ uint32_t m_len[64], m_cand[64];
	const uint32_t c = blockIdx.x, lane = threadIdx.x;
	if (c >= n_chunks)
		return;
	const uint64_t boff = (uint64_t)(c / XZC_CHUNKS_PER_BLOCK) * LA_XZC_BLOCK_BYTES;
	const uint32_t blen = src_bytes - boff < LA_XZC_BLOCK_BYTES ? (uint32_t)(src_bytes - boff) : LA_XZC_BLOCK_BYTES;
	const uint32_t cs = (c % XZC_CHUNKS_PER_BLOCK) * LA_XZC_CHUNK_BYTES;
	const uint32_t ce = cs + LA_XZC_CHUNK_BYTES < blen ? cs + LA_XZC_CHUNK_BYTES : blen;
	const uint8_t *blk = d_src + boff;
	const uint32_t payload = la_xzc_chunk(blk, cs, ce, level, probs, tab, m_len, m_cand, slots + (uint64_t)c * LA_XZC_SLOT_BYTES);
	/* the check: a segment per lane (the table takes the match table's place), combined on lane 0 */
	__syncthreads();
	uint64_t *table = (uint64_t *)tab, *seg_crc = table + 256;
	for (uint32_t i = lane; i < 256u; i += 64u)
		table[i] = la_xz_crc64_entry(i);
	__syncthreads();
	const uint32_t n = ce - cs, seg = (n + 63u) / 64u;
	const uint32_t from = seg * lane < n ? seg * lane : n;
	const uint32_t len = n - from < seg ? n - from : seg;
	seg_crc[lane] = la_xz_crc64(table, blk + cs + from, len, 0);
	__syncthreads();
	if (lane == 0) {
		const uint64_t sh = la_xz_crc64_shift(seg);
		uint64_t acc = seg_crc[0];
		for (uint32_t j = 1; j < 64u; j++) {
			const uint32_t f = seg * j;
			if (f >= n)
				break;
			const uint32_t l = n - f < seg ? n - f : seg;
			acc = la_xz_crc64_mul(l == seg ? sh : la_xz_crc64_shift(l), acc) ^ seg_crc[j];
		}
		chunk_crc[c] = acc;
		chunk_payload[c] = payload;
		chunk_size[c] = la_xzc_chunk_bytes(n, payload);
	}
}

/* body bytes of block b (its chunks and the end marker) from the chunks' offsets */
__device__ __forceinline__ uint64_t xzc_block_comp(const uint64_t *chunk_off, uint32_t n_chunks, uint32_t b)
{
	const uint32_t first = b * XZC_CHUNKS_PER_BLOCK;
	const uint32_t last = first + XZC_CHUNKS_PER_BLOCK < n_chunks ? first + XZC_CHUNKS_PER_BLOCK : n_chunks;
	return chunk_off[last] - chunk_off[first] + 1u;
}

__global__ __launch_bounds__(256) void xzc_block_sizes_kernel(const uint64_t *__restrict__ chunk_off, uint32_t n_chunks, uint32_t n_blocks,
    uint32_t *block_size)
{
	const uint32_t b = blockIdx.x * 256u + threadIdx.x;
	if (b < n_blocks)
		block_size[b] = (uint32_t)la_xzc_block_bytes(xzc_block_comp(chunk_off, n_chunks, b));
}

__global__ __launch_bounds__(256) void xzc_pack_kernel(const uint8_t *__restrict__ d_src, uint64_t src_bytes, uint32_t n_chunks, uint32_t n_blocks,
    uint32_t head, const uint8_t *__restrict__ slots, const uint32_t *__restrict__ chunk_payload, const uint64_t *__restrict__ chunk_off,
    const uint64_t *__restrict__ chunk_crc, const uint64_t *__restrict__ block_off, uint8_t *d_out, uint64_t out_cap, uint64_t *d_out_bytes)
{
	const uint32_t c = blockIdx.x, t = threadIdx.x;
	if (c == 0 && t == 0) {
		uint8_t h[12];
		la_xzc_stream_header(h);
		for (uint32_t i = 0; i < head; i++)
			if (i < out_cap)
				d_out[i] = h[i];
		*d_out_bytes = head + (n_blocks ? block_off[n_blocks] : 0u);
	}
	if (c >= n_chunks)
		return;
	const uint32_t b = c / XZC_CHUNKS_PER_BLOCK, first = b * XZC_CHUNKS_PER_BLOCK;
	const uint32_t last = first + XZC_CHUNKS_PER_BLOCK < n_chunks ? first + XZC_CHUNKS_PER_BLOCK : n_chunks;
	const uint64_t boff = (uint64_t)b * LA_XZC_BLOCK_BYTES;
	const uint32_t blen = src_bytes - boff < LA_XZC_BLOCK_BYTES ? (uint32_t)(src_bytes - boff) : LA_XZC_BLOCK_BYTES;
	const uint32_t cs = (c - first) * LA_XZC_CHUNK_BYTES;
	const uint32_t n = cs + LA_XZC_CHUNK_BYTES < blen ? LA_XZC_CHUNK_BYTES : blen - cs;
	const uint64_t at_block = head + block_off[b];
	const uint64_t at = at_block + LA_XZC_BLOCK_HDR + (chunk_off[c] - chunk_off[first]);
	const uint32_t payload = chunk_payload[c];
	if (payload) {
		const uint8_t *s = slots + (uint64_t)c * LA_XZC_SLOT_BYTES;
		for (uint32_t i = t; i < 6u + payload; i += 256u)
			if (at + i < out_cap)
				d_out[at + i] = s[i];
	} else {
		const uint8_t *s = d_src + boff + cs;
		if (t == 0) {
			uint8_t h[3];
			la_xzc_stored_header(h, n, c == first);
			for (uint32_t i = 0; i < 3u; i++)
				if (at + i < out_cap)
					d_out[at + i] = h[i];
		}
		for (uint32_t i = t; i < n; i += 256u)
			if (at + 3u + i < out_cap)
				d_out[at + 3u + i] = s[i];
	}
	if (t != 0)
		return;
	const uint64_t comp = xzc_block_comp(chunk_off, n_chunks, b);
	if (c == first) {
		uint8_t h[LA_XZC_BLOCK_HDR];
		la_xzc_block_header(h, comp, blen);
		for (uint32_t i = 0; i < LA_XZC_BLOCK_HDR; i++)
			if (at_block + i < out_cap)
				d_out[at_block + i] = h[i];
	}
	if (c + 1u == last) {
		/* end marker, padding, then the chunks' CRC64s combined: every chunk but the last is LA_XZC_CHUNK_BYTES long */
		uint64_t p = at_block + LA_XZC_BLOCK_HDR + comp - 1u;
		const uint64_t pad_end = at_block + LA_XZC_BLOCK_HDR + ((comp + 3u) & ~(uint64_t)3u);
		for (; p < pad_end; p++)
			if (p < out_cap)
				d_out[p] = 0;
		const uint64_t sh = la_xz_crc64_shift(LA_XZC_CHUNK_BYTES);
		uint64_t acc = chunk_crc[first];
		for (uint32_t j = first + 1u; j < last; j++)
			acc = la_xz_crc64_mul(j + 1u == last ? la_xz_crc64_shift(n) : sh, acc) ^ chunk_crc[j];
		for (uint32_t i = 0; i < 8u; i++)
			if (p + i < out_cap)
				d_out[p + i] = (uint8_t)(acc >> (8u * i));
	}
}

struct xzc_ws {
	uint8_t *slots;
	uint32_t *chunk_size, *chunk_payload, *block_size;
	uint64_t *chunk_off, *chunk_crc, *block_off;
	uint8_t *scan;
};

static uint64_t xzc_carve(uint8_t *base, uint64_t src_bytes, xzc_ws *w)
{
	const uint64_t n_chunks = (src_bytes + LA_XZC_CHUNK_BYTES - 1u) / LA_XZC_CHUNK_BYTES;
	const uint64_t n_blocks = (src_bytes + LA_XZC_BLOCK_BYTES - 1u) / LA_XZC_BLOCK_BYTES;
	la_carve cv = { base, 0 };
	w->slots = cv.take<uint8_t>(n_chunks * LA_XZC_SLOT_BYTES, 256);
	w->chunk_size = cv.take<uint32_t>(n_chunks, 256);
	w->chunk_payload = cv.take<uint32_t>(n_chunks, 256);
	w->block_size = cv.take<uint32_t>(n_blocks, 256);
	w->chunk_off = cv.take<uint64_t>(n_chunks + 1u, 256);
	w->chunk_crc = cv.take<uint64_t>(n_chunks, 256);
	w->block_off = cv.take<uint64_t>(n_blocks + 1u, 256);
	w->scan = cv.take<uint8_t>(la_scan_scratch_bytes((uint32_t)n_chunks), 256);
	return cv.off + 256u;
}

uint64_t la_xz_compress_ws_bytes(uint64_t src_bytes)
{
	xzc_ws w;
	return xzc_carve(NULL, src_bytes, &w);
}

uint64_t la_xz_compress_bound(uint64_t src_bytes)
{
	return la_xzc_bound(src_bytes);
}

void la_launch_xz_compress(hipStream_t s, const la_xzc_batch *bt, uint8_t *ws, const la_stage_hook *hook)
{
	const uint32_t n_chunks = (uint32_t)((bt->src_bytes + LA_XZC_CHUNK_BYTES - 1u) / LA_XZC_CHUNK_BYTES);
	const uint32_t n_blocks = (uint32_t)((bt->src_bytes + LA_XZC_BLOCK_BYTES - 1u) / LA_XZC_BLOCK_BYTES);
	const uint32_t head = (bt->flags & LA_XZC_FIRST) ? 12u : 0u;
	xzc_ws w;
	xzc_carve(ws, bt->src_bytes, &w);
	if (n_chunks) {
		hook->mark(hook->cx, "xzc_chunks");
		hipLaunchKernelGGL(xzc_chunk_kernel, dim3(n_chunks), dim3(64), 0, s, bt->d_src, bt->src_bytes, n_chunks, bt->level, w.slots, w.chunk_size,
		    w.chunk_payload, w.chunk_crc);
		hook->mark(hook->cx, "xzc_pack");
		la_launch_scan_u32(s, w.chunk_size, n_chunks, w.chunk_off, w.scan);
		hipLaunchKernelGGL(xzc_block_sizes_kernel, dim3((n_blocks + 255u) / 256u), dim3(256), 0, s, w.chunk_off, n_chunks, n_blocks, w.block_size);
		la_launch_scan_u32(s, w.block_size, n_blocks, w.block_off, w.scan);
	} else {
		hook->mark(hook->cx, "xzc_pack");
	}
	hipLaunchKernelGGL(xzc_pack_kernel, dim3(n_chunks ? n_chunks : 1u), dim3(256), 0, s, bt->d_src, bt->src_bytes, n_chunks, n_blocks, head,
	    w.slots, w.chunk_payload, w.chunk_off, w.chunk_crc, w.block_off, bt->d_out, bt->out_cap, bt->d_out_bytes);
	hook->mark(hook->cx, NULL);
}
