/*
 * la_lz4_slices.h -- how the LAST expand slice of an lz4 batch is cut into launches: THE place where that is decided.
 * Plain C: la_api.hip (the launch sequence), la_lz4_fast.hip (the block a workgroup takes), la_hash.hip (what a hash
 * pass may read) and tests/test_lz4_slice_rule.py (compiled into a host object) all ask here.
 *
 * The last slice covers the blocks [first, last) of the batch.  It is not expanded front to back but by POSITION IN
 * THE PERIOD: with a period P (on the shapes that take this path, the blocks of one frame) and group bounds
 * 0 = h[0] < h[1] < ... < h[G] = P, block i belongs to group g when h[g] <= (i - first) % P < h[g + 1].  Group 0 is
 * launched first: the head positions of every frame, then the middle ones, and the last few positions of every frame
 * last.  Every block below `first` counts as done (the earlier slices, in stream order in front of group 0).
 *
 * Why: a frame's content checksum is one serial chain over its bytes.  Hashed behind a contiguous slice, every chain of
 * that slice starts when the slice ends, and the step waits for a whole chain.  Behind group g a frame's leading blocks
 * up to its first block of a later group are in the slab (the READY PREFIX), so its chain can advance over them beside
 * group g + 1, and the step waits only for the chain over the last group's blocks.  Nothing here depends on how the
 * frames sit on the period: a frame that is short, long or shifted has a shorter ready prefix in the early passes and
 * a longer last pass, never a wrong one.
 */
#ifndef LA_LZ4_SLICES_H
#define LA_LZ4_SLICES_H

#include <stdint.h>

#if defined(__HIPCC__)
#define LA_SLICE_FN __host__ __device__ static inline
#else
#define LA_SLICE_FN static inline
#endif

#define LA_LZ4_SPLIT_MAX_GROUPS 4u
#define LA_LZ4_SPLIT_MIN_PERIOD 4u
#define LA_LZ4_SPLIT_MAX_PERIOD 64u

typedef struct la_lz4_split {
	uint32_t first, last;	/* the slice: blocks [first, last) */
	uint32_t period;	/* P */
	uint32_t n_groups;	/* G, 1 .. LA_LZ4_SPLIT_MAX_GROUPS */
	uint32_t bound[LA_LZ4_SPLIT_MAX_GROUPS + 1];	/* h[0] = 0 < ... < h[G] = P */
} la_lz4_split;

/* The period of a batch, from what the host knows without reading the frame table back: the blocks per frame when
 * that is the same whole number for every frame of the batch on average and lies in 4 .. 64; 0: do not split. */
LA_SLICE_FN uint32_t la_lz4_split_period(uint32_t n_blocks, uint32_t n_frames)
{
	if (n_frames == 0 || n_blocks % n_frames != 0)
		return 0;
	const uint32_t p = n_blocks / n_frames;
	return (p >= LA_LZ4_SPLIT_MIN_PERIOD && p <= LA_LZ4_SPLIT_MAX_PERIOD) ? p : 0;
}

/* Group bounds given in sixteenths of the period (ascending, the last one 16), rounded down; a bound that does not
 * lie above the one in front of it is dropped, so every group has at least one position.  P >= 1, 1 <= n <= MAX_GROUPS. */
LA_SLICE_FN void la_lz4_split_init(la_lz4_split *sp, uint32_t first, uint32_t last, uint32_t period,
    const uint32_t *sixteenths, uint32_t n)
{
	sp->first = first;
	sp->last = last;
	sp->period = period;
	sp->bound[0] = 0;
	uint32_t g = 0;
	for (uint32_t k = 0; k < n; k++) {
		const uint32_t h = k + 1 == n ? period : period * sixteenths[k] / 16u;
		if (h > sp->bound[g] && h <= period)
			sp->bound[++g] = h;
	}
	sp->n_groups = g;
}

/* the blocks of group g: whole periods have h[g + 1] - h[g] of them, the last, partial period what lies below `last` */
LA_SLICE_FN uint32_t la_lz4_split_group_blocks(const la_lz4_split *sp, uint32_t g)
{
	const uint32_t len = sp->last - sp->first, whole = len / sp->period, rest = len % sp->period;
	const uint32_t lo = sp->bound[g], hi = sp->bound[g + 1];
	return whole * (hi - lo) + (rest > lo ? (rest < hi ? rest : hi) - lo : 0u);
}

/* The launch of group g is a two-dimensional grid: x counts the periods that have a block of the group (the last one
 * may be partial), y the positions inside the group.  Workgroup (x, y) takes la_lz4_split_block(); the ones of a partial
 * last period whose block lies at or behind `last` leave at once, all others are the group's blocks, each once. */
LA_SLICE_FN uint32_t la_lz4_split_grid_x(const la_lz4_split *sp, uint32_t g)
{
	const uint32_t len = sp->last - sp->first, lo = sp->bound[g];
	return len > lo ? (len - lo + sp->period - 1u) / sp->period : 0u;
}
LA_SLICE_FN uint32_t la_lz4_split_grid_y(const la_lz4_split *sp, uint32_t g)
{
	return sp->bound[g + 1] - sp->bound[g];
}
/* base = first + h[g]: no division, no list */
LA_SLICE_FN uint32_t la_lz4_split_block(uint32_t base, uint32_t period, uint32_t x, uint32_t y)
{
	return base + x * period + y;
}

/* The ready prefix of a frame (first_block, n_blocks) once every block of the slice at a period position below h is
 * expanded (h = bound[g + 1]: groups 0 .. g are done; h = 0: none is): how many of the frame's leading blocks are in the
 * slab.  The run up to the frame's first block at a position >= h, capped at n_blocks; blocks below `first` are done.
 * For a frame that ends inside the slice (first_block + n_blocks <= last). */
LA_SLICE_FN uint32_t la_lz4_split_ready(uint32_t first, uint32_t period, uint32_t h, uint32_t first_block, uint32_t n_blocks)
{
	if (h >= period)
		return n_blocks;
	const uint32_t s = first_block > first ? first_block : first;	/* the frame's first block inside the slice */
	const uint32_t r = (s - first) % period;
	const uint32_t stop = r < h ? s + (h - r) : s;			/* the first block from s on that is not done */
	const uint32_t run = stop - first_block;
	return run < n_blocks ? run : n_blocks;
}

/* Hash pass g (behind group g) advances a frame over its blocks [lo, hi) of
 *     lo = g == 0 ? 0 : ready(bound[g]),   hi = ready(bound[g + 1]):
 * pass 0 also takes what the earlier slices left (blocks below `first`), and the passes of a frame follow each other
 * without gap or overlap.  The state between passes is the frame's carry, kept at the position of the frame's LAST block
 * in the slice: unique among frames that have blocks, and a frame without blocks hashes no bytes. */
LA_SLICE_FN uint32_t la_lz4_split_pass_lo(uint32_t first, uint32_t period, uint32_t h_lo, uint32_t first_block, uint32_t n_blocks)
{
	return h_lo == 0 ? 0u : la_lz4_split_ready(first, period, h_lo, first_block, n_blocks);
}
LA_SLICE_FN uint32_t la_lz4_split_carry_index(uint32_t first, uint32_t first_block, uint32_t n_blocks)
{
	return first_block + n_blocks - 1u - first;	/* n_blocks != 0, first < first_block + n_blocks */
}

#endif
