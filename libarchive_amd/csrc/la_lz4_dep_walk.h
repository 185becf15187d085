/*
 * la_lz4_dep_walk.h -- the forward walk of the lz4 dependency kernel over a block's output positions, by LOOKS at
 * several positions at once: THE place where that is stated.  Plain C: la_lz4_deps.hip (the positions in LDS) and
 * tests/test_lz4_dep_walk_rule.py (compiled into a host object, and into a sanitized host program) both ask here.
 *
 * The rule, as the one-step walk states it (the search inside the window kernel, DEPS = false, still does):
 *
 *     while (q + 1 < bound && pos[q + 1] <= x) q++;
 *
 * pos[] holds 16-bit positions in LA_LZ4_WALK_CAP entries, of which only those below `bound` mean anything: what lies
 * at or behind `bound` may be uninitialised and decides nothing.  As a loop, every step is a round trip to the array
 * with a wait behind it and a trip through the loop's bookkeeping, and a wave stays for the longest walk of its 64
 * lanes plus the failing test.  A look requests the LA_LZ4_WALK_LOOK entries from q + 1 on together, waits once, and
 * the advance is the run of entries at or below x in front of the first one above it, cut at `bound`.  Another look is
 * needed only when all of them were at or below x and entries below `bound` follow: a 32-byte output chunk holds one
 * sequence start on average.  Nothing is assumed about the order of the positions: the result is the one-step walk's
 * for any content.
 *
 * Every read is one entry, 2 bytes at an even address, naturally aligned wherever the look starts, and each is an
 * access of its own (a relaxed atomic load, which is an ordinary 2-byte read): left to itself the compiler joins the
 * four into ONE 8-byte read at a 2-byte-aligned address, and an unaligned LDS access costs a cycle per lane whatever
 * its width.  The reads are requested together and waited for once.
 *
 * The first look is straight-line code, taken from every start q < CAP: it reads up to index q + LOOK, so the array
 * has LA_LZ4_WALK_LOOK readable entries behind the CAP that mean something; they lie at or behind every bound and
 * decide nothing.  The kernel keeps the match starts behind the positions in one LDS array, so that those entries are
 * the first match starts: no padding, the LDS size is what it was.
 *
 * Forms that were measured and lost (profiles/r33_lz4_deps_looks.md): a look at ONE naturally aligned group of four or
 * eight positions (8- and 16-byte reads) needs a second look whenever the walk crosses the group's end, which some lane
 * of a wave does in 99.7 % of the walks; two aligned groups per look cost more vector instructions for the eight
 * entries' bits than the steps they replace.
 */
#ifndef LA_LZ4_DEP_WALK_H
#define LA_LZ4_DEP_WALK_H

#include <stdint.h>

#if defined(__HIPCC__)
#define LA_WALK_FN __host__ __device__ static inline __attribute__((always_inline))
#else
#define LA_WALK_FN static inline
#endif

#define LA_LZ4_WALK_CAP  4096u	/* entries of the position array (LA_LZ4_FAST_MAXSEQ) */
#ifndef LA_LZ4_WALK_LOOK
#define LA_LZ4_WALK_LOOK 4u	/* entries per look */
#endif

/* One look at p[0 .. LOOK - 1] = pos[q + 1 ...], avail = the entries from q + 1 on that lie below the bound.  Returns
 * the advance; *more: every entry of the look was passed and entries below the bound follow. */
LA_WALK_FN uint32_t la_lz4_walk_look(const uint16_t *p, uint32_t avail, uint32_t x, uint32_t *more)
{
	uint32_t e[LA_LZ4_WALK_LOOK];
	for (uint32_t i = 0; i < LA_LZ4_WALK_LOOK; i++)	/* every read requested before the first entry is used */
		e[i] = __atomic_load_n(p + i, __ATOMIC_RELAXED);
	uint32_t run = LA_LZ4_WALK_LOOK;		/* the index of the first entry above x */
	for (uint32_t i = LA_LZ4_WALK_LOOK; i-- > 0; )
		run = e[i] <= x ? run : i;
	*more = (run == LA_LZ4_WALK_LOOK && avail > LA_LZ4_WALK_LOOK) ? 1u : 0u;
	return run < avail ? run : avail;
}

/* The walk.  pos: LA_LZ4_WALK_CAP entries and LA_LZ4_WALK_LOOK readable ones behind them, q < CAP, bound <= CAP. */
LA_WALK_FN uint32_t la_lz4_dep_walk(const uint16_t *pos, uint32_t q, uint32_t bound, uint32_t x)
{
	uint32_t more, t = q + 1u;
	q += la_lz4_walk_look(pos + t, bound > t ? bound - t : 0u, x, &more);
	while (more) {	/* the rare path */
		t = q + 1u;
		q += la_lz4_walk_look(pos + t, bound > t ? bound - t : 0u, x, &more);
	}
	return q;
}

#endif
