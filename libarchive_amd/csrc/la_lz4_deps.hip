/*
 * la_lz4_deps.hip -- what every match of an LDS-window block has to wait for, found ahead of the
 * window kernel (la_lz4_fast.hip) in a kernel of its own.
 *
 * The window kernel holds one block per workgroup in a 64 KiB window, two workgroups per CU, and
 * used to open its match phase with a search: for every sequence the earlier sequences under its
 * match source (chunk map, two walks over the output positions, one look at the last touched
 * sequence's table entry in global memory).  That search needs no payload and no window, only the
 * block's sequence table, and it was paid at the worst occupancy on the chip.  Here it runs with
 * 20 KiB of LDS per workgroup, eight workgroups per CU:
 *
 *   pass 1   the block's table entries, all loads of a thread in flight together and the entries
 *            kept in registers: output position and literal end (lit_src + lit_len) go to LDS
 *   plan     the block's LITERAL PLAN (la_lz4_lit_chunk_edge, la_dev.h): for every 32-byte chunk
 *            of the payload the first sequence with literals in or behind it, from each sequence's
 *            own literal end and the one before it; 16-bit entries to lit_plan + table_off.  The
 *            window kernel's literal phase starts from them: it used to load every sequence's
 *            predecessor, build this index in LDS and stand at a barrier before its first literal
 *            load (profiles/r27_lz4_literal_plan.md).  Every entry of the block's
 *            ceil(src_len / 32) chunks and the count behind them is written in every launch:
 *            the buffer is never cleared.
 *   pass 2   match starts (dst + lit_len) take the literal ends' place behind a barrier; the chunk
 *            map: for every 32-byte chunk of the output the sequence that holds the chunk's first
 *            byte (from the output positions in LDS)
 *   pass 3   per sequence: the source's last byte by la_lz4_dep_source (la_dev.h), the map
 *            entries under the source's first and last byte, two short walks forward to q and
 *            to the last sequence under the source (la_lz4_dep_walk.h: by looks at four positions
 *            at once, not step by step), that sequence's match start from LDS
 *            (la_lz4_dep_drops_last), and the word  q | count << 16  to deps[table_off + k]
 *
 * Pass 3 has no branch per sequence but the one to the rare second look of a walk and the one around
 * the store: both map entries and the block's first position are read by every lane, whatever its
 * flags say, behind one wait; each walk's first look is four reads behind one wait; the last
 * sequence's match start is read by every lane.  Step by step and with a branch per flag it was seven
 * to eight round trips per sequence, each walk's with a trip through the loop's exec bookkeeping
 * (profiles/r33_lz4_deps_looks.md; requesting the first looks of both walks together was measured too
 * and gave nothing more).
 *
 * The word is the one the window kernel's own search hands its poll loop (same rule, same
 * functions), so the kernel given the words (DEPS = true) skips the search and nothing else
 * changes.  A word that waited for too little would show in the decoded bytes only as a race:
 * la_gpu_lz4_debug_deps fetches the words, tests/test_gpu_lz4_deps.py compares them with the rule.
 *
 * The four fill loops (plan entries, "none" entries, the two map fills) run 0.5 to 1 times on average and stay
 * scalar: vectorised, each one brought a trip-count guard, 16-byte LDS stores or 8-byte global stores to 2-byte-aligned
 * addresses and a remainder loop that every wave walked through (6 088 static instructions and 62 VGPRs against 4 193 and
 * 55; the kernel is bound by instruction issue, profiles/r30_lz4_literal_dwords.md).
 *
 * Blocks: exactly those la_lz4_route sends to LA_XR_WINDOW (asked with the window kernel's
 * arguments); stored, failed, general and segmented blocks are left alone -- the segmented launch
 * numbers its sequences per segment and keeps its own search.  Every loop is bounded by the
 * block's sequence count or its chunk count; nothing here waits for another thread.
 *
 * Every index is inside its array whatever the table holds: positions are 16-bit, so a map index
 * is below 2048; q and qe stay below k < ns <= LA_LZ4_FAST_MAXSEQ, and a look reads the positions
 * up to index q + LA_LZ4_WALK_LOOK, at most four entries into the match starts of the same array;
 * deps is written at table_off + k with k < ns, inside the block's table slot; plan entries are written at
 * c <= ceil(src_len / 32), two bytes each from byte table_off on, inside one byte per slot entry.
 */
#include "la_dev.h"
#include "la_lz4_dep_walk.h"

static_assert(LA_LZ4_WALK_CAP == LA_LZ4_FAST_MAXSEQ && LA_LZ4_WALK_LOOK <= LA_LZ4_FAST_MAXSEQ,
    "the walk's array is the kernel's positions; a look's entries behind them lie in the match starts");

#define DEPS_THREADS 256
#define DEPS_SLOTS   (LA_LZ4_FAST_MAXSEQ / DEPS_THREADS)	/* sequences per thread */

__global__ __launch_bounds__(DEPS_THREADS) void lz4_deps_kernel(const la_lz4_block *__restrict__ blocks, uint32_t n,
    uint64_t dst_cap, const uint64_t *__restrict__ dst_off, const uint32_t *__restrict__ out_len,
    const uint32_t *__restrict__ status, const uint32_t *__restrict__ nseq, const la_lz4_seq *__restrict__ table,
    const uint64_t *__restrict__ table_off, uint32_t long_thr, uint32_t *__restrict__ deps, uint8_t *__restrict__ lit_plan)
{
	__shared__ uint16_t posm[2 * LA_LZ4_FAST_MAXSEQ];	/* (20 KiB in all with the map: eight workgroups per CU) */
	uint16_t *const dstpos = posm;				/* output position per sequence */
	uint16_t *const mstart = posm + LA_LZ4_FAST_MAXSEQ;	/* dst + lit_len: where the sequence's match starts; until the literal
								 * plan is out, lit_src + lit_len: where its literals end in the payload.
								 * One array with the positions in front: a look from the last positions
								 * (la_lz4_dep_walk.h) reads up to LA_LZ4_WALK_LOOK entries into this half,
								 * which decide nothing */
	__shared__ uint16_t cmap[2048];				/* per 32-byte output chunk: the sequence that holds its first byte */

	const uint32_t bi = blockIdx.x;
	if (bi >= n)
		return;
	const uint32_t olen = out_len[bi], ns = nseq[bi];
	if (la_lz4_route(blocks[bi], status[bi], olen, ns, dst_off[bi], dst_cap, true, long_thr) != LA_XR_WINDOW)
		return;
	const uint32_t tid = threadIdx.x;
	const uint64_t *const tab = (const uint64_t *)(const void *)(table + table_off[bi]);	/* lit_src | lit_len << 16 | dst << 32 | off << 48 */
	uint32_t *const out = deps + table_off[bi];
	uint16_t *const plan = (uint16_t *)(void *)(lit_plan + table_off[bi]);	/* (slots are multiples of eight entries: even) */
	const uint32_t nchunks = la_lz4_lit_chunk_edge(blocks[bi].src_len);	/* <= 2048: an eligible block has src_len <= 65536 */

	/* the thread's entries (sequences tid, tid + 256, ...), all requested before the first one is used and kept in
	 * registers for pass 3: the table is read from memory once, with one latency and not one per 256 sequences */
	uint64_t ent[DEPS_SLOTS];
#pragma unroll
	for (uint32_t r = 0; r < DEPS_SLOTS; r++) {
		const uint32_t k = r * DEPS_THREADS + tid;
		ent[r] = k < ns ? tab[k] : 0;
	}
#pragma unroll
	for (uint32_t r = 0; r < DEPS_SLOTS; r++) {
		if (r * DEPS_THREADS >= ns)
			break;
		const uint32_t k = r * DEPS_THREADS + tid;
		if (k < ns) {
			dstpos[k] = (uint16_t)((uint32_t)(ent[r] >> 32) & 0xFFFFu);
			mstart[k] = (uint16_t)(((uint32_t)ent[r] & 0xFFFFu) + ((uint32_t)(ent[r] >> 16) & 0xFFFFu));	/* literal end, for now */
		}
	}
	__syncthreads();
	/* the literal plan (la_lz4_lit_chunk_edge): sequence k is the entry of the payload chunks between the edge of the
	 * literal end before it and its own, the last sequence closes the plan with "none" up to the payload's last chunk
	 * and the count behind that.  The parse kernels keep literals inside the payload; a table that did not would
	 * still write inside the slot (c < nchunks).  Only the end of the run BEFORE a sequence is read back from the
	 * 16-bit array, and that run has its match offset behind it: it ends below 65536. */
#pragma unroll
	for (uint32_t r = 0; r < DEPS_SLOTS; r++) {
		if (r * DEPS_THREADS >= ns)
			break;
		const uint32_t k = r * DEPS_THREADS + tid;
		if (k < ns) {
			const uint32_t le = ((uint32_t)ent[r] & 0xFFFFu) + ((uint32_t)(ent[r] >> 16) & 0xFFFFu);
			const uint32_t pe = k ? (uint32_t)mstart[k - 1] : 0u;
			uint32_t cend = la_lz4_lit_chunk_edge(le);
			if (cend > nchunks)
				cend = nchunks;
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)
			for (uint32_t c = la_lz4_lit_chunk_edge(pe); c < cend; c++)
				plan[c] = (uint16_t)k;
			if (k + 1 == ns) {
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)
				for (uint32_t c = cend; c < nchunks; c++)
					plan[c] = (uint16_t)LA_LZ4_PLAN_NONE;
				plan[nchunks] = (uint16_t)cend;
			}
		}
	}
	/* pass 2.  Where sequence k's match ends is the next sequence's position, the block's end behind the last one
	 * (positions are 16-bit: an end at 65536 reads 0).  It replaces lit_src in the entry's low 16 bits, which
	 * nothing here reads: pass 3 has the match length without another look at LDS. */
#pragma unroll
	for (uint32_t r = 0; r < DEPS_SLOTS; r++) {
		if (r * DEPS_THREADS >= ns)
			break;
		const uint32_t k = r * DEPS_THREADS + tid;
		const uint32_t after = k + 1 < ns ? (uint32_t)dstpos[k + 1] : (olen & 0xFFFFu);
		ent[r] = (ent[r] & ~0xFFFFull) | after;
	}
	__syncthreads();	/* every literal end has been read: the array takes the match starts */
#pragma unroll
	for (uint32_t r = 0; r < DEPS_SLOTS; r++) {
		if (r * DEPS_THREADS >= ns)
			break;
		const uint32_t k = r * DEPS_THREADS + tid;
		if (k < ns) {
			const uint32_t d = (uint32_t)(ent[r] >> 32) & 0xFFFFu;
			uint32_t nxt = (uint32_t)ent[r] & 0xFFFFu;
			if (nxt < d)
				nxt = 65536u;
			mstart[k] = (uint16_t)(d + ((uint32_t)(ent[r] >> 16) & 0xFFFFu));	/* (65536 reads 0: only behind a last, empty sequence, which nobody waits for) */
			if (k == 0)
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)
				for (uint32_t c = 0; (c << 5) < d; c++)
					cmap[c] = 0;
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)
			for (uint32_t c = (d + 31) >> 5; (c << 5) < nxt; c++)
				cmap[c] = (uint16_t)k;
		}
	}
	__syncthreads();

	/* pass 3.  q is the largest index below k whose sequence starts at or before the source's first byte, qe the
	 * same for its last byte (la_lz4_dep_source).  Both start from the map -- the sequence that holds the first
	 * byte of the 32-byte chunk -- and walk up; a chunk holds at most eight sequence starts, one on average.  One
	 * sequence at a time: a loop over several sequences at once runs as long as the longest walk of all of them. */
#pragma unroll
	for (uint32_t r = 0; r < DEPS_SLOTS; r++) {
		if (r * DEPS_THREADS >= ns)
			break;
		const uint32_t k = r * DEPS_THREADS + tid;
		const uint64_t e = ent[r];
		const uint32_t d = (uint32_t)(e >> 32) & 0xFFFFu, mdst = d + ((uint32_t)(e >> 16) & 0xFFFFu), off = (uint32_t)(e >> 48);
		const bool valid = k > 0 && k < ns;	/* (sequence 0 waits for nobody: its word is 0) */
		const uint32_t mlen = valid ? (((uint32_t)e & 0xFFFFu) - mdst) & 0xFFFFu : 0;
		const uint32_t s0 = mdst - off;
		uint32_t hi = 0;
		const bool src = la_lz4_dep_source(d, mdst, off, mlen, &hi);	/* (false where valid is: mlen is 0 then) */
		/* the map entries under the source's first and last byte and the block's first position, requested together and
		 * whatever the flags say: s0 is cut to the map, hi < d <= 65535 (0 without a source), and a value that is not
		 * wanted is not used */
		const uint32_t q0 = cmap[(s0 < 65535u ? s0 : 65535u) >> 5], e0 = cmap[hi >> 5], first = dstpos[0];
		const bool waits = src && first <= hi;
		const uint32_t kq = valid ? k : 0, ke = waits ? k : 0;	/* the walks' bounds: 0 stops them at once */
		const uint32_t km1 = valid ? k - 1 : 0;
		uint32_t q = q0 < km1 ? q0 : km1;
		const uint32_t e1 = e0 < km1 ? e0 : km1;
		uint32_t qe = waits && e1 > q ? e1 : q;
		q = la_lz4_dep_walk(dstpos, q, kq, s0);
		if (qe < q)
			qe = q;
		qe = la_lz4_dep_walk(dstpos, qe, ke, hi);
		const uint32_t last = mstart[qe];	/* (qe < LA_LZ4_FAST_MAXSEQ; read by every lane, used where the sequence waits) */
		if (k < ns) {
			const uint32_t cnt = waits ? qe - q + 1 - (la_lz4_dep_drops_last(hi, last) ? 1u : 0u) : 0u;
			out[k] = q | (cnt << 16);
		}
	}
}

void la_launch_lz4_deps(hipStream_t s, const la_expand_job &j, uint32_t *d_deps, uint8_t *d_plan)
{
	if (j.n == 0) return;
	hipLaunchKernelGGL(lz4_deps_kernel, dim3(j.n), dim3(DEPS_THREADS), 0, s, j.blocks, j.n, j.dst_cap, j.dst_off,
	    j.out_len, j.status, j.nseq, j.table, j.table_off, j.long_thr, d_deps, d_plan);
}
