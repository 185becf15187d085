/*
 * la_xz_filters.hip -- the delta and BCJ filters of an xz block's chain, undone in place over the decoded bytes of all
 * blocks of a batch, between la_launch_xz_decode and la_launch_xz_verify (so the checks see unfiltered bytes).
 *
 * The transforms are la_xz_filters_dev.h's, the text the CPU stand-in of the tests compiles.  A block's bytes
 * [0, len) -- out_len, or the valid bytes of a failed block -- are cut into tiles of XZF_TILE bytes; a workgroup takes
 * tiles of one block (grid: block x a stride over its tiles, so a block of any size is covered by many workgroups and
 * a block without a filter at this chain position costs one early return).  The chain positions run last to first; per
 * position three launches, in which every filter kind does its share:
 *   FIRST   delta: the tile's column sums (tile in LDS, the rows in 256 / dist groups so that every lane has work).
 *           x86: each of 64 lanes finds the first head of its XZF_SUB bytes; nothing is written to the block yet, so
 *           all lanes read the bytes as the decoder left them.  ARM, ARM-Thumb, PowerPC, SPARC, IA-64: a lane per unit,
 *           done.
 *   SCAN    delta: one workgroup per block turns the tiles' column sums into exclusive prefixes, a lane per column.
 *   LAST    delta: the tile in LDS again, every (column, row group) adds its carry downwards, the tile is stored.
 *           x86: each lane that found a head walks liblzma's serial step from it to the first head behind its XZF_SUB
 *           bytes.  Walks never meet (la_xz_filters_dev.h); a run of opcode bytes closer than 6 apart is one lane's.
 * Scratch: per block its length and first tile (PREP, one workgroup, a scan over the batch), and 256 bytes per tile
 * (column sums, or 64 head offsets).  Everything is memory-bound byte traffic beside a decode that is one latency-bound
 * wave per block; DESIGN.md 5j has the measurement.
 */
#include "la_dev.h"

#define LA_XZ_FN static __host__ __device__ __forceinline__
#include "la_xz_filters_dev.h"

#define XZF_TILE    16384u
#define XZF_SUB     256u	/* XZF_TILE / 64 */
#define XZF_THREADS 256u
#define XZF_SLOT    256u	/* scratch bytes per tile */

struct xzf_block {
	uint64_t len;		/* bytes the filters run over; 0: nothing to do */
	uint64_t tile_base;	/* the block's first tile slot */
};

__device__ __forceinline__ uint64_t xzf_len(const la_xz_block &blk, const la_xz_result &r, const la_xz_chain &ch, uint64_t dst_total)
{
	if (ch.count == 0u || blk.dst_off > dst_total || blk.dst_cap > dst_total - blk.dst_off)
		return 0u;
	const uint64_t len = r.status == LA_ST_OK ? r.out_len : r.valid;
	return len < blk.dst_cap ? len : blk.dst_cap;
}

/* one workgroup: validates the chains, gives every block with work its tile slots */
__global__ __launch_bounds__(XZF_THREADS) void xzf_prep_kernel(const la_xz_block *d_blocks, const la_xz_chain *d_chains, uint32_t n,
    uint64_t dst_total, la_xz_result *d_results, la_hash_job *d_jobs, xzf_block *info, uint64_t tiles_cap)
{
	__shared__ uint64_t part[XZF_THREADS];
	const uint32_t tid = threadIdx.x;
	const uint32_t per = (n + XZF_THREADS - 1u) / XZF_THREADS;
	const uint32_t b0 = tid * per < n ? tid * per : n, b1 = b0 + per < n ? b0 + per : n;
	uint64_t tiles = 0;
	for (uint32_t b = b0; b < b1; b++) {
		const la_xz_chain ch = d_chains[b];
		if (!la_xz_chain_valid(&ch)) {
			const la_xz_result bad = { LA_ST_XZ_SIZE, 0u, 0u, 0u, 0u };
			d_results[b] = bad;
			d_jobs[b].len = 0u;
			continue;
		}
		tiles += (xzf_len(d_blocks[b], d_results[b], ch, dst_total) + XZF_TILE - 1u) / XZF_TILE;
	}
	part[tid] = tiles;
	__syncthreads();
	if (tid == 0u) {
		uint64_t acc = 0;
		for (uint32_t k = 0; k < XZF_THREADS; k++) {
			const uint64_t v = part[k];
			part[k] = acc;
			acc += v;
		}
	}
	__syncthreads();
	uint64_t base = part[tid];
	for (uint32_t b = b0; b < b1; b++) {
		const la_xz_chain ch = d_chains[b];
		uint64_t len = la_xz_chain_valid(&ch) ? xzf_len(d_blocks[b], d_results[b], ch, dst_total) : 0u;
		const uint64_t t = (len + XZF_TILE - 1u) / XZF_TILE;
		if (base + t > tiles_cap)	/* (blocks that overlap in d_dst: more tiles than d_dst has) */
			len = 0u;
		const xzf_block e = { len, base };
		info[b] = e;
		if (len)
			base += t;
	}
}

/* what a workgroup works on: false when its block has no filter at chain position `pos` */
struct xzf_work {
	uint8_t *buf;
	uint64_t len, tiles;
	uint8_t *slots;
	uint32_t id, prop;
};
__device__ __forceinline__ bool xzf_work_of(uint32_t b, uint32_t pos, const la_xz_block *d_blocks, const la_xz_chain *d_chains, uint8_t *d_dst,
    const xzf_block *info, uint8_t *slots, xzf_work *w)
{
	const xzf_block e = info[b];
	if (e.len == 0u || pos >= d_chains[b].count)
		return false;
	w->buf = d_dst + d_blocks[b].dst_off;
	w->len = e.len;
	w->tiles = (e.len + XZF_TILE - 1u) / XZF_TILE;
	w->slots = slots + e.tile_base * XZF_SLOT;
	w->id = d_chains[b].id[pos];
	w->prop = d_chains[b].prop[pos];
	return true;
}

/* the row groups of a delta tile: lane (c, s) has column c of the rows [s * per, (s + 1) * per) */
struct xzf_rows {
	uint32_t c, s, groups;
	uint64_t r0, r1;
};
__device__ __forceinline__ xzf_rows xzf_rows_of(uint32_t tid, uint32_t dist, uint64_t lo, uint64_t hi)
{
	xzf_rows q;
	q.groups = XZF_THREADS / dist;
	q.c = tid % dist;
	q.s = tid / dist;
	const uint64_t rows = la_xz_delta_rows(lo, hi, dist), per = (rows + q.groups - 1u) / q.groups;
	q.r0 = q.s * per < rows ? q.s * per : rows;
	q.r1 = q.r0 + per < rows ? q.r0 + per : rows;
	if (q.s >= q.groups)
		q.r0 = q.r1 = 0u;
	return q;
}

template <bool LAST>
__global__ __launch_bounds__(XZF_THREADS) void xzf_tile_kernel(const la_xz_block *d_blocks, const la_xz_chain *d_chains, uint32_t n, uint32_t pos,
    uint8_t *d_dst, const xzf_block *info, uint8_t *slots)
{
	__shared__ uint8_t tile[XZF_TILE];
	__shared__ uint8_t part[XZF_THREADS];
	const uint32_t b = blockIdx.x, tid = threadIdx.x;
	xzf_work w;
	if (b >= n || !xzf_work_of(b, pos, d_blocks, d_chains, d_dst, info, slots, &w))
		return;
	const uint32_t unit_bytes = la_xz_unit_bytes(w.id), unit_stride = la_xz_unit_stride(w.id);
	if (LAST && unit_bytes != 0u)
		return;		/* a map filter is done in the first launch */
	for (uint64_t t = blockIdx.y; t < w.tiles; t += gridDim.y) {
		const uint64_t lo = t * XZF_TILE, hi = lo + XZF_TILE < w.len ? lo + XZF_TILE : w.len;
		uint8_t *slot = w.slots + t * XZF_SLOT;
		if (w.id == LA_XZF_DELTA) {
			const uint32_t dist = w.prop;
			for (uint32_t j = tid; j < (uint32_t)(hi - lo); j += XZF_THREADS)
				tile[j] = w.buf[lo + j];
			__syncthreads();
			const xzf_rows q = xzf_rows_of(tid, dist, lo, hi);
			part[tid] = (uint8_t)la_xz_delta_col_sum(tile, lo, lo, hi, dist, q.c, q.r0, q.r1);
			__syncthreads();
			if (!LAST) {
				if (tid < dist) {
					uint32_t acc = 0;
					for (uint32_t s = 0; s < q.groups; s++)
						acc += part[s * dist + tid];
					slot[tid] = (uint8_t)acc;
				}
			} else {
				uint32_t carry = slot[q.c];
				for (uint32_t s = 0; s < q.s && s < q.groups; s++)
					carry += part[s * dist + q.c];
				la_xz_delta_col_apply(tile, lo, lo, hi, dist, q.c, q.r0, q.r1, carry & 0xFFu);
				__syncthreads();
				for (uint32_t j = tid; j < (uint32_t)(hi - lo); j += XZF_THREADS)
					w.buf[lo + j] = tile[j];
			}
			__syncthreads();
		} else if (w.id == LA_XZF_X86) {
			const uint64_t sub_lo = lo + (uint64_t)tid * XZF_SUB;
			if (tid < XZF_TILE / XZF_SUB && sub_lo < hi) {
				uint32_t *head = (uint32_t *)slot + tid;
				if (!LAST) {
					const uint64_t h = la_xz_x86_first_head(w.buf, w.len, sub_lo, sub_lo + XZF_SUB < hi ? sub_lo + XZF_SUB : hi);
					*head = h < w.len ? (uint32_t)(h - sub_lo) + 1u : 0u;
				} else if (*head != 0u) {
					la_xz_x86_walk(w.buf, w.len, w.prop, sub_lo + *head - 1u, sub_lo + XZF_SUB);
				}
			}
		} else {
			for (uint64_t i = lo + (uint64_t)tid * unit_stride; i < hi && i + unit_bytes <= w.len; i += (uint64_t)XZF_THREADS * unit_stride)
				la_xz_unit(w.id, w.buf, i, w.prop);
		}
	}
}

/* delta: the tiles' column sums become exclusive prefixes, a lane per column */
__global__ __launch_bounds__(XZF_THREADS) void xzf_scan_kernel(const la_xz_block *d_blocks, const la_xz_chain *d_chains, uint32_t n, uint32_t pos,
    uint8_t *d_dst, const xzf_block *info, uint8_t *slots)
{
	const uint32_t b = blockIdx.x, tid = threadIdx.x;
	xzf_work w;
	if (b >= n || !xzf_work_of(b, pos, d_blocks, d_chains, d_dst, info, slots, &w))
		return;
	if (w.id != LA_XZF_DELTA || tid >= w.prop)
		return;
	uint32_t acc = 0;
	for (uint64_t t = 0; t < w.tiles; t++) {
		const uint32_t v = w.slots[t * XZF_SLOT + tid];
		w.slots[t * XZF_SLOT + tid] = (uint8_t)acc;
		acc += v;
	}
}

static uint64_t xzf_tiles_cap(uint32_t n, uint64_t dst_cap)
{
	return dst_cap / XZF_TILE + n;
}
static uint64_t xzf_info_bytes(uint32_t n)
{
	return ((uint64_t)n * sizeof(xzf_block) + 255u) & ~(uint64_t)255u;
}

uint64_t la_xz_unfilter_ws_bytes(uint32_t n, uint64_t dst_cap)
{
	return xzf_info_bytes(n) + xzf_tiles_cap(n, dst_cap) * XZF_SLOT;
}

void la_launch_xz_unfilter(hipStream_t s, const la_xz_batch *bt, uint8_t *jobs_ws, uint8_t *ws)
{
	if (bt->n == 0)
		return;
	const la_xz_chain *chains = (const la_xz_chain *)(bt->d_blocks + bt->n);
	xzf_block *info = (xzf_block *)ws;
	uint8_t *slots = ws + xzf_info_bytes(bt->n);
	hipLaunchKernelGGL(xzf_prep_kernel, dim3(1), dim3(XZF_THREADS), 0, s, bt->d_blocks, chains, bt->n, bt->dst_cap, bt->d_results,
	    (la_hash_job *)jobs_ws, info, xzf_tiles_cap(bt->n, bt->dst_cap));
	/* workgroups per block: twice the batch's mean tiles per block; a larger block's workgroups stride over its tiles */
	uint64_t gy = (bt->dst_cap / XZF_TILE + bt->n) / bt->n * 2u;
	if (gy > 1024u)
		gy = 1024u;
	const dim3 grid(bt->n, (uint32_t)gy);
	for (uint32_t pos = LA_XZ_CHAIN_MAX; pos-- > 0u;) {
		hipLaunchKernelGGL(xzf_tile_kernel<false>, grid, dim3(XZF_THREADS), 0, s, bt->d_blocks, chains, bt->n, pos, bt->d_dst, info, slots);
		hipLaunchKernelGGL(xzf_scan_kernel, dim3(bt->n), dim3(XZF_THREADS), 0, s, bt->d_blocks, chains, bt->n, pos, bt->d_dst, info, slots);
		hipLaunchKernelGGL(xzf_tile_kernel<true>, grid, dim3(XZF_THREADS), 0, s, bt->d_blocks, chains, bt->n, pos, bt->d_dst, info, slots);
	}
}
