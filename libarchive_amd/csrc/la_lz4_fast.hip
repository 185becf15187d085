/*
 * la_lz4_fast.hip -- LDS-window LZ4 expand kernel (gfx950): the hot kernel of
 * the lz4 filter path for independent blocks of at most 64 KiB
 * (libarchive/archive_read_support_filter_lz4.c:557-561, the
 * LZ4_decompress_safe call of BD=4 frames).
 *
 * One 512-thread workgroup owns one block; its whole output lives in a 64 KiB
 * LDS window (two workgroups per CU: 2 x 77 KiB of the 160 KiB LDS).  The
 * parse kernel has already reduced the token chain to a table of sequences
 * {literal source, literal length, output position, match offset}, so inside
 * the block every copy is known up front:
 *
 *   prepass             every thread loads its sequences' entries (kept in
 *       registers for all phases), publishes their output positions in LDS and
 *       builds the chunk index: for every 32-byte chunk of the payload, the
 *       first sequence that still has literals in or after it.
 *   phase L (literals)  one thread per 32-byte payload chunk: two coalesced
 *       16-byte loads of the compressed stream, the chunk's sequences from the
 *       chunk index, literal bytes into the window as whole dwords with static
 *       register indices.  Work is balanced by bytes, not by sequences; every
 *       payload byte is read once.
 *   phase M (matches)   one thread per sequence, sequences taken in increasing
 *       order.  A match may read bytes an earlier match produces, so every
 *       sequence publishes a "done" bit in LDS and a match waits only for the
 *       (typically one or two) earlier MATCHES that overlap its source range,
 *       found by a binary search over the output positions.  Dependencies
 *       always point to lower sequence numbers and waves take sequences in
 *       increasing order, so the lowest unfinished sequence can always run: no
 *       deadlock, no barrier inside the phase; every spin is bounded anyway.
 *   phase F (flush)     the window goes to the decoded slab with 16-byte
 *       coalesced stores (the window is placed so that LDS and HBM addresses
 *       are congruent modulo 16).
 *
 * HBM traffic per block: payload once, sequence table once in (plus the entries
 * phase L looks up), decoded bytes once out.
 *
 * What bounds it (PMC, C2 workload): the LDS pipe is 58 % busy, the SIMDs a little
 * under half, and behind both sits the dependency chain of phase M (DAG depth 16 per
 * block, about 31 poll iterations per wave).  What a poll iteration costs is LDS
 * round trips in series, LDS instructions, and VALU instructions, in that order.
 * Measured on the way here (16 GiB C2 stream, expand ms):
 *   - all loads of a match copy before any store, ragged end as an overlapping
 *     end-aligned store                                           39.1 -> 32.8
 *   - literal chunks as whole dwords, static register indices     32.7 -> 27.8
 *   - no wait for a sequence touched only in its literals          27.8 -> 26.9
 *   - short (4..7 byte) matches in the same load batch            26.9 -> 24.8
 *   - one look at the flag word per iteration                      24.8 -> 23.5
 *   - round 2: 16-byte unaligned accesses for matches of 16 bytes and more, two
 *     8-byte ones below, no load a lane does not need (an unaligned LDS access
 *     costs one cycle per active lane whatever its width)         23.2 -> 21.7
 * and slower, so not kept: neighbouring literal dwords paired into 8-byte stores
 * (22.3 from 21.7: the extra predicates cost more than the lane-stores saved),
 * skipping the register slots beyond the block's last sequence in the prepass and
 * the search (no change: those phases wait for memory, not for issue slots), a match
 * phase in two passes (every slot gets one to three looks, the stragglers of all slots
 * are taken in a second pass: 23.3 / 23.5 / 23.8 from 21.8 -- the lanes a slot waits for
 * are not a few stragglers, the whole in-flight set advances one dependency level per look),
 * pulling the table and payload of the block 512 / 1024 / 2048 places ahead towards L2 at the
 * start of the match phase (22.4 / 22.5 / 22.8 from 21.8: the prepass is not waiting for HBM),
 * the source loads of a match issued right behind its flag look instead of after it (safe: the LDS
 * serves a wave in order; one round trip per level instead of two, but 24.3 from 21.8 -- the loads of
 * lanes that are not ready yet are lane-accesses the LDS pipe has no room for),
 * wave-cooperative match copies (four matches per pass
 * through ds_bpermute, 35.1), flag look requested one iteration ahead (28.3),
 * speculative source read behind the flag look (27.6), 8-ary search (26.9 from
 * 23.5: more LDS instructions), per-sequence literal copies from global memory
 * (43.6), 256- and 1024-thread workgroups (no gain), longer poll sleeps (+1..4 %), every
 * lane walking through its own sequences at its own pace instead of the wave finishing
 * slot r first (28.0 from 23.2: the per-lane register picks cost more than the waits);
 * and without effect: 1, 2, 8 or 16 consecutive sequences per lane group instead of 4,
 * the early payload loads moved behind the table loads / made branch-free (the compiler
 * waits for them right behind the loads because a byte-wise tail path defines the same
 * registers; removing that wait changed nothing measurable).
 *
 * Round 4, the poll iteration of phase M: each slot's copy class is fixed once (six classes, one flat test
 * each against the ready lanes), the spin bound counts per wave in a scalar register, and the body keeps only
 * the flag look, the copies, the done bit and one exit ballot.  Per wave VALU -16 %, SALU -8 %, wave cycles
 * -3 %; expand 5.34 -> 5.18 ms per C2 launch, 25.7 -> 24.7 ms for gzip C3.  The per-slot register picks were
 * already outside the loop (hoisted by the compiler), so the iteration did not halve: a level's time is the
 * LDS round trips in series, not issue.  s_sleep 0 instead of 1: no change beyond noise.
 *
 * The search out of the kernel (profiles/r25_lz4_deps.md): which earlier matches a match waits for -- the chunk
 * map over the output, the two walks, the look at the last touched sequence's entry in global memory, 16.6 k of a
 * block's 95 k cycles here at two blocks per CU -- needs only the sequence table.  The lz4 path now finds it in
 * la_lz4_deps.hip at eight workgroups per CU and hands this kernel one word per sequence (DEPS = true): the four C2
 * launches 20.8 -> 18.0 ms, the dependency kernel 1.9 ms in front of them.  The rule itself is la_lz4_dep_source /
 * la_lz4_dep_drops_last (la_dev.h), asked by both.  DEPS = false is the kernel as it was: the segmented launch, the
 * deflate front end (inflate_expand) and LA_LZ4_OPT_SEARCH_IN_EXPAND run it.
 *
 * The chunk index out of the kernel (profiles/r27_lz4_literal_plan.md): where a payload chunk's literals start in the
 * table follows from the table alone too (la_lz4_lit_chunk_edge, la_dev.h).  With DEPS = true the prepass above no
 * longer loads every sequence's predecessor, builds no index in LDS and has no barrier in front of phase L: a thread
 * asks for its chunks' entries of the block's literal plan (written by the dependency kernel, 16 bits per chunk) with
 * the chunks themselves, ahead of the table entries, and the output positions and the cleared flags go to LDS behind
 * the literal stores, where only the barrier that ends phase L waits for them.  Of a block's 79.4 k cycles the
 * stretch in front of the first literal store went from 13.7 k to 8.9 k, the block to 75.1 k; the four C2 launches
 * 17.97 -> 17.05 ms, the dependency kernel 1.91 -> 2.32 ms.  84 VGPRs and 74 368 B of LDS against 90 and 78 480.
 * DEPS = false builds the index here as before, by the same rule.
 *
 * Phase L dword by dword (profiles/r30_lz4_literal_dwords.md): put() walks a chunk's eight dwords once per run, 96
 * predicated stores per thread for sixteen dwords to place, and 2 069 of the kernel's 2 449 static instructions stood
 * in front of the barrier that ends phase L.  Which dwords of a chunk a run stores is stated once, la_lz4_lit_run_dwords
 * (la_dev.h); two runs of a parsed table are at least three payload bytes apart, so a dword of the chunk's grid has one
 * owner or none.  With DEPS = true the six runs a chunk fetches leave their window offset under the bits of their 8-bit
 * range mask (one bit extract and one and-or per run and dword), and each dword goes out with one store under one
 * predicate: the same (address, dword) stores as before.  1 818 instructions in front of the barrier, 33 ds_write_b32
 * where there were 113, 114 s_and_saveexec where there were 206; 87 VGPRs (84), no scratch, 74 368 B of LDS.  The
 * literal stores of a block 17.0 k -> 12.5 k cycles, the block 74.9 k -> 71.7 k; the four C2 launches 17.06 -> 16.35 ms.
 * Picking the owner with ordered thresholds (compare and select: 1 950 instructions) gave 16.54 ms and was not kept.
 * DEPS = false and SEG keep put(), now over the same function; their device code is the parent's, instruction for
 * instruction.
 *
 * A block's words in one round trip (profiles/r31_lz4_block_words.md): la_lz4_route is a chain of ||, and each word it is
 * asked with used to be loaded where the chain first needs it -- six scalar loads one behind another, each with its own
 * wait and branch, kernel arguments fetched one or two at a time between them, and table_off[bi] read again for every
 * slot's dependency words.  The kernel now opens with la_lz4_load_block_words (la_dev.h): one clause of arguments, one
 * clause with the block's words and the late arguments (table, deps, lit_plan, src, dst) behind one wait, then the routing
 * test; no scalar load between the first payload load and the barrier that ends phase L.  Registers, LDS and occupancy
 * of all three instantiations are unchanged.  The four C2 launches 16.31 -> 16.02 ms.  The stretch the stamps call "up to
 * the loads requested" fell by 0.7 k cycles only: the first stamp stands behind the routing test, most of the removed
 * trips were in front of it, and what is left there is the payload chunks' own round trip.
 *
 * The last slice by position in the frame (profiles/r32_lz4_last_slice.md): the step used to end with the content checksums
 * of the last slice's frames, one serial chain per frame that could only start when the slice's launch had ended (0.86 ms
 * in the sixteen-lane form, bound by the chain, not by the number of frames).  The last slice is now launched in groups of
 * period positions (la_lz4_slices.h: positions 0..7 of every frame of sixteen, then 8..12, then 13..15), and behind each
 * group the frames' chains advance over the blocks that exist by then (la_hash.hip).  For this kernel that is one more
 * instantiation, STRIDED, which differs in how the workgroup finds its block and in nothing else: a two-dimensional grid,
 * bi = base + blockIdx.x * period + blockIdx.y, still a scalar value at kernel entry, in front of the same two clauses.
 * Registers, LDS and occupancy are the contiguous instantiation's (87 VGPRs, 74 368 B, no scratch, 4 waves per SIMD), and
 * the three older instantiations' device code is the parent's, instruction for instruction.  The window launches of the
 * last slice take together what the contiguous one took; what they lose is what every slice beside a hash launch loses
 * (about 0.28 ms per slice), now that the last slice has its own frames hashed beside it instead of behind it.
 */
#include "la_dev.h"

#ifndef POLL_SLEEP
#define POLL_SLEEP 1
#endif
#ifndef FAST_THREADS
#define FAST_THREADS 512
#endif
#ifndef LBATCH
#define LBATCH 2	/* payload chunks a thread has in flight in phase L */
#endif
#ifndef FAST_MIN_WAVES
#define FAST_MIN_WAVES 4
#endif
#define FAST_WAVES   (FAST_THREADS / 64)

/* Diagnostic build only (make diag, -DLA_DIAG): per-workgroup phase stamps go to a
 * buffer of their own; no output value depends on them. */
#ifdef LA_DIAG
__device__ unsigned long long *la_diag_stamps;
#define STAMP(slot)                                                                       \
	do {                                                                              \
		if (threadIdx.x == 0 && la_diag_stamps)                                    \
			la_diag_stamps[(size_t)blockIdx.x * 8 + (slot)] = __builtin_readcyclecounter(); \
	} while (0)
#else
#define STAMP(slot) do { } while (0)
#endif

/* A sequence-table entry travels in registers as one 64-bit value
 * (lit_src | lit_len << 16 | dst << 32 | off << 48): plain integers keep the
 * compiler from parking small structs in scratch memory. */
typedef uint64_t seq_t;

/*
 * Ownership of sequences in the match phase: a STEP is sixteen consecutive sequences
 * (16g .. 16g+15); step g belongs to wave g % 8, which runs its steps in increasing
 * order.  Register slot r of lane l in wave w holds sequence
 *     k = (((4 r + l/16) * 8 + w) * 16) + l % 16
 * so that the step a wave executes at (r, t) sits in lanes 16t .. 16t+15.
 */
#ifndef STEP_SHIFT
#define STEP_SHIFT  2u		/* log2(sequences per step) */
#endif
#define STEP_SEQS   (1u << STEP_SHIFT)		/* sequences per step */
#define STEP_LANES  (64u >> STEP_SHIFT)		/* lanes per sequence, 8 bytes each per pass */
#define STEPS_PER_SLOT (64u >> STEP_SHIFT)	/* steps held by one register slot of a wave */
__device__ __forceinline__ uint32_t fast_seq_index(uint32_t r, uint32_t wave, uint32_t lane)
{
	return (((r * STEPS_PER_SLOT + (lane >> STEP_SHIFT)) * FAST_WAVES + wave) << STEP_SHIFT) + (lane & (STEP_SEQS - 1));
}
__device__ __forceinline__ seq_t seq_load(const la_lz4_seq *t, uint32_t k)
{
	return *(const uint64_t *)(const void *)(t + k);
}
#define SEQ_LIT_SRC(e) ((uint32_t)((e) & 0xFFFFu))
#define SEQ_LIT_LEN(e) ((uint32_t)(((e) >> 16) & 0xFFFFu))
#define SEQ_DST(e)     ((uint32_t)(((e) >> 32) & 0xFFFFu))
#define SEQ_OFF(e)     ((uint32_t)((e) >> 48))

/* SEG = false: one workgroup per block of the table, blocks of at most MAXSEQ sequences (the
 * usual case).  SEG = true: the workgroups share out the few blocks with MORE sequences, listed
 * by lz4_classify_kernel, and run them in segments of MAXSEQ sequences. */
/* DEPS = true: every sequence's dependency word comes from the dependency kernel (la_lz4_deps.hip, one word per table
 * entry) and the search in front of the match phase is compiled out; DEPS = false: the kernel searches for itself
 * (the segmented launch, whose sequence numbers are segment-local, the deflate front end, and the cross-check
 * LA_LZ4_OPT_SEARCH_IN_EXPAND). */
/* STRIDED = true: one group of a split last slice (la_lz4_slices.h).  The grid is two-dimensional, periods in x and the
 * positions inside the group in y; the workgroup's block is la_lz4_split_block(), n is the slice's end in the batch's own
 * numbering and every array is the whole batch's.  Nothing else differs: the block index is still a scalar value known at
 * kernel entry.  Such a launch has no list of blocks, and the stride travels in the list's place among the arguments
 * (same size, same offset), so the other instantiations' arguments, and with them their code, are what they were. */
struct fast_stride { uint32_t base, period; };	/* first + h[g], P */
template <bool STRIDED> struct fast_list_arg { typedef const uint32_t *__restrict__ type; };
template <> struct fast_list_arg<true> { typedef fast_stride type; };
static_assert(sizeof(fast_stride) == sizeof(const uint32_t *), "the stride takes the list's place");

template <uint32_t MAXSEQ, bool SEG, bool DEPS, bool STRIDED = false>
__global__ __launch_bounds__(FAST_THREADS, FAST_MIN_WAVES) void lz4_expand_fast_kernel(
    const uint8_t *__restrict__ src, uint64_t src_bytes, const la_lz4_block *__restrict__ blocks,
    uint32_t n, uint8_t *__restrict__ dst, uint64_t dst_cap, const uint64_t *__restrict__ dst_off,
    const uint32_t *__restrict__ out_len, uint32_t *status_out,
    const uint32_t *__restrict__ nseq, const la_lz4_seq *__restrict__ table,
    const uint64_t *__restrict__ table_off, typename fast_list_arg<STRIDED>::type big_list /* STRIDED: the stride */,
    const uint32_t *__restrict__ big_count, uint32_t long_thr, const uint32_t *__restrict__ deps,
    const uint8_t *__restrict__ lit_plan)
{
	static_assert(!(SEG && DEPS), "the dependency words number a block's sequences from its first one");
	static_assert(!(SEG && STRIDED), "the segmented launch takes its blocks from a list");
	const uint32_t *status = status_out;
	__shared__ __attribute__((aligned(16))) uint8_t win[16 + 65536 + 96];	/* 16 headroom (literal stores may start 3 bytes early) + 16 alignment shift + slack for over-reads */
	__shared__ uint16_t dstpos[MAXSEQ + 4];
	__shared__ uint32_t donebits[MAXSEQ / 32];	/* one bit per sequence: its match is in the window */
	__shared__ uint16_t chunk_first[DEPS ? 8 : 2048 + 8];	/* per 32-byte payload chunk: first sequence with literals in or after it
								 * (DEPS: the index comes from the dependency kernel, nothing is kept here) */

	auto do_block = [&](const uint32_t bi) __attribute__((always_inline)) {
	if (bi >= n)
		return;
	/* the block's words in one round trip (la_lz4_load_block_words, la_dev.h) */
	const la_lz4_block_words b = la_lz4_load_block_words<true, SEG>(bi, blocks, status, out_len, nseq, dst_off, table_off);
	/* and with them every argument the block needs later: no round trip of its own in front of the plan, the table
	 * entries or the dependency words */
	LA_PIN_SCALARS("s"(src), "s"(src_bytes), "s"(dst), "s"(dst_cap), "s"(table), "s"(long_thr), "s"(deps), "s"(lit_plan));
	const uint32_t olen = b.out_len;
	const uint32_t ns_all = b.nseq;
	const uint64_t doff = b.dst_off;
	/* this launch's share of the table: blocks of one LDS segment, or (SEG) of more */
	static_assert(MAXSEQ == LA_LZ4_FAST_MAXSEQ, "la_lz4_route splits the window kernels' blocks at LA_LZ4_FAST_MAXSEQ");
	if (la_lz4_route_words(b, dst_cap, true, long_thr) != (SEG ? LA_XR_WINDOW_SEG : LA_XR_WINDOW))
		return;

	STAMP(0);
	const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const la_lz4_seq *const tab_all = table + b.table_off;
	const uint8_t *s = src + b.src_off;
	const uint64_t s_room = src_bytes - b.src_off;	/* bytes of the image from s on */
	uint8_t *g_out = dst + doff;
	uint8_t *W = win + 16 + ((uintptr_t)g_out & 15);	/* W[i] <-> g_out[i], congruent mod 16 */

	/* This thread's sequences (fast_seq_index): their table entries are fetched once, up
	 * front, and stay in registers for every pass over them.  The entry of the sequence
	 * before each one comes along: its literal end tells which payload chunks START their
	 * literals with this sequence. */
	constexpr uint32_t MAXSTEPS = MAXSEQ / FAST_THREADS;
	/* the first two payload chunks of this thread (phase L) are requested right away:
	 * they depend on nothing, and their latency overlaps the table prepass */
	uint64_t vv[LBATCH][4];
#pragma unroll
	for (int u = 0; u < LBATCH; u++) {
		const uint32_t c0 = (u * FAST_THREADS + tid) << 5;
		vv[u][0] = vv[u][1] = vv[u][2] = vv[u][3] = 0;
		if (c0 < b.src_len) {
			if ((uint64_t)c0 + 32 <= s_room) {
				const uint4 a = ld_u128(s + c0), bq = ld_u128(s + c0 + 16);
				vv[u][0] = ((uint64_t)a.y << 32) | a.x; vv[u][1] = ((uint64_t)a.w << 32) | a.z;
				vv[u][2] = ((uint64_t)bq.y << 32) | bq.x; vv[u][3] = ((uint64_t)bq.w << 32) | bq.z;
			} else {
				/* last chunk of the image: never read past it */
				for (uint32_t i = 0; c0 + i < s_room && i < 32; i++) {
					const uint64_t by = (uint64_t)s[c0 + i] << (8 * (i & 7));
					if (i < 8) vv[u][0] |= by; else if (i < 16) vv[u][1] |= by;
					else if (i < 24) vv[u][2] |= by; else vv[u][3] |= by;
				}
			}
		}
	}
	/* DEPS: where each of those chunks starts in the table is the block's literal plan (la_lz4_lit_chunk_edge), written
	 * by the dependency kernel: requested with the chunks, in front of the table entries, so that the chunk's sequences
	 * can be asked for as soon as it is back.  No predecessor entries, no index built in LDS, no barrier in front of
	 * phase L (profiles/r27_lz4_literal_plan.md). */
	const uint16_t *const plan = DEPS ? (const uint16_t *)(const void *)(lit_plan + b.table_off) : nullptr;
	const uint32_t plan_chunks = la_lz4_lit_chunk_edge(b.src_len);	/* the plan has an entry for every chunk of the payload */
	uint32_t kk0[LBATCH];
#pragma unroll
	for (int u = 0; u < LBATCH; u++) {
		kk0[u] = LA_LZ4_PLAN_NONE;
		if constexpr (DEPS) {
			const uint32_t c = u * FAST_THREADS + tid;
			if (c < plan_chunks)
				kk0[u] = plan[c];
		}
	}
	/* Blocks with more sequences than the LDS arrays hold are done in SEGMENTS of MAXSEQ
	 * sequences: prepass, literals and matches per segment, a barrier between segments.
	 * Sequences of earlier segments are complete by then, so a segment only ever waits on
	 * its own.  Inside a segment all sequence numbers are local (tab points at its first
	 * entry); payload chunks are numbered from cb, the chunk in which the segment's
	 * literals begin (it may be shared with the end of the previous segment: each side
	 * stores only its own sequences' bytes). */
	auto segment = [&](const uint32_t kb) __attribute__((always_inline)) {
	const la_lz4_seq *const tab = tab_all + kb;
	const uint32_t ns = ns_all - kb < MAXSEQ ? ns_all - kb : MAXSEQ;
	uint32_t cb = 0, seg_prev_end = 0;
	if (kb) {
		const seq_t pvb = seq_load(tab_all, kb - 1);	/* same address in every thread */
		seg_prev_end = SEQ_LIT_SRC(pvb) + SEQ_LIT_LEN(pvb);
		cb = seg_prev_end >> 5;
	}
	seq_t ent[MAXSTEPS];
	uint32_t prev_end[MAXSTEPS];
	uint32_t dw[MAXSTEPS];	/* DEPS: the dependency word of the slot's sequence (la_lz4_deps.hip), loaded at the end of phase L */
#pragma unroll
	for (uint32_t r = 0; r < MAXSTEPS; r++) {
		ent[r] = 0;
		prev_end[r] = 0;
		dw[r] = 0;
	}
	/* (slot r holds sequences r * FAST_THREADS and up: slots beyond the segment's last sequence
	 * are skipped wave-uniformly in every pass below -- the kernel is bound by instruction issue) */
#pragma unroll
	for (uint32_t r = 0; r < MAXSTEPS; r++) {
		if (r * FAST_THREADS >= ns)
			break;
		const uint32_t k = fast_seq_index(r, wave, lane);
		ent[r] = k < ns ? seq_load(tab, k) : 0;
		if constexpr (!DEPS) {
			const seq_t pv = ((k > 0 || kb > 0) && k < ns) ? seq_load(tab_all, kb + k - 1) : 0;
			prev_end[r] = SEQ_LIT_SRC(pv) + SEQ_LIT_LEN(pv);
		}
	}
	/* what the match phase finds in LDS: the flags cleared, every sequence's output position, and behind the last one
	 * the position where the segment ends (the match length of its last sequence).  Without the plan it goes out with
	 * the chunk index, in front of phase L's barrier; with it, behind phase L's stores. */
	auto publish = [&]() __attribute__((always_inline)) {
		if (tid < MAXSEQ / 32)
			donebits[tid] = 0;
		if (tid == 0)
			dstpos[ns] = kb + ns < ns_all ? (uint16_t)SEQ_DST(seq_load(tab_all, kb + ns)) : (uint16_t)olen;
#pragma unroll
		for (uint32_t r = 0; r < MAXSTEPS; r++) {
			if (r * FAST_THREADS >= ns)
				break;
			const uint32_t k = fast_seq_index(r, wave, lane);
			if (k < ns)
				dstpos[k] = (uint16_t)SEQ_DST(ent[r]);
		}
	};
	if constexpr (!DEPS) {
		publish();
		if (tid == 0 && (cb << 5) < seg_prev_end)
			chunk_first[0] = 0;	/* chunk shared with the previous segment: this side starts with its first sequence */
		/* chunk_first[c] = first sequence whose literals end beyond payload offset 32c (la_lz4_lit_chunk_edge) */
#pragma unroll
		for (uint32_t r = 0; r < MAXSTEPS; r++) {
			if (r * FAST_THREADS >= ns)
				break;
			const uint32_t k = fast_seq_index(r, wave, lane);
			if (k < ns) {
				const uint32_t le = SEQ_LIT_SRC(ent[r]) + SEQ_LIT_LEN(ent[r]);
				for (uint32_t c = la_lz4_lit_chunk_edge(prev_end[r]); c < la_lz4_lit_chunk_edge(le); c++)
					chunk_first[c - cb] = (uint16_t)k;
				if (k + 1 == ns)
					chunk_first[2048] = (uint16_t)(la_lz4_lit_chunk_edge(le) - cb);	/* chunks from here on hold no literals of this segment */
			}
		}
		__syncthreads();
	}
#ifdef LA_DIAG_L
	STAMP(6);
#endif

	/* ---- phase L: literals, one thread per 32-byte payload chunk ----
	 * Two coalesced 16-byte loads of the compressed stream per chunk; the chunk's
	 * sequences come from chunk_first (LDS; DEPS: from the literal plan) and six table entries fetched together;
	 * literal bytes go to the window with unaligned 8-byte LDS stores.  Work is balanced
	 * by payload bytes, and every payload byte is read once. */
	uint32_t nlit_chunks = plan_chunks;	/* DEPS: every chunk of the payload has a plan entry, "none" behind the last literal */
	if constexpr (!DEPS)
		nlit_chunks = chunk_first[2048];
	for (uint32_t base = 0; base < nlit_chunks; base += LBATCH * FAST_THREADS) {
		uint32_t kk[LBATCH];
		seq_t pe[LBATCH][6];
#pragma unroll
		for (int u = 0; u < LBATCH; u++) {
			const uint32_t c = base + u * FAST_THREADS + tid;	/* chunk number inside the segment */
			if constexpr (DEPS) {
				const uint32_t e = base == 0 ? kk0[u] : c < nlit_chunks ? (uint32_t)plan[c] : (uint32_t)LA_LZ4_PLAN_NONE;
				kk[u] = e == LA_LZ4_PLAN_NONE ? 0xFFFFFFFFu : e;
			} else {
				kk[u] = c < nlit_chunks ? (uint32_t)chunk_first[c] : 0xFFFFFFFFu;
			}
			if (base != 0 || kb != 0) {	/* payloads beyond 32 KiB, later segments: chunks are loaded here */
				vv[u][0] = vv[u][1] = vv[u][2] = vv[u][3] = 0;
				const uint32_t c0 = (cb + c) << 5;
				if (c < nlit_chunks) {
					if ((uint64_t)c0 + 32 <= s_room) {
						const uint4 a = ld_u128(s + c0), bq = ld_u128(s + c0 + 16);
						vv[u][0] = ((uint64_t)a.y << 32) | a.x; vv[u][1] = ((uint64_t)a.w << 32) | a.z;
						vv[u][2] = ((uint64_t)bq.y << 32) | bq.x; vv[u][3] = ((uint64_t)bq.w << 32) | bq.z;
					} else {
						for (uint32_t i = 0; c0 + i < s_room && i < 32; i++) {
							const uint64_t by = (uint64_t)s[c0 + i] << (8 * (i & 7));
							if (i < 8) vv[u][0] |= by; else if (i < 16) vv[u][1] |= by;
							else if (i < 24) vv[u][2] |= by; else vv[u][3] |= by;
						}
					}
				}
			}
		}
#pragma unroll
		for (int u = 0; u < LBATCH; u++) {
#pragma unroll
			for (int t = 0; t < 6; t++)
				pe[u][t] = (kk[u] != 0xFFFFFFFFu && kk[u] + t < ns) ? seq_load(tab, kk[u] + t) : 0;
		}
#ifdef LA_DIAG_L
		if (base == 0) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); STAMP(7); }
#endif
#pragma unroll
		for (int u = 0; u < LBATCH; u++) {
			if (kk[u] == 0xFFFFFFFFu)
				continue;
			const uint32_t c0 = (cb + base + u * FAST_THREADS + tid) << 5, c1 = c0 + 32;
			/* The chunk's eight dwords go out with STATIC register indices: dword m of
			 * the chunk belongs to at most one literal run (two runs are at least a
			 * 3-byte sequence header apart), and a whole-dword store may spill up to
			 * three bytes over either end of the run: those bytes lie in the match
			 * before / after the run (a match is at least four bytes long), which
			 * phase M writes after the barrier.  No shifting, no register selects. */
			const uint32_t dd[8] = { (uint32_t)vv[u][0], (uint32_t)(vv[u][0] >> 32), (uint32_t)vv[u][1], (uint32_t)(vv[u][1] >> 32),
			    (uint32_t)vv[u][2], (uint32_t)(vv[u][2] >> 32), (uint32_t)vv[u][3], (uint32_t)(vv[u][3] >> 32) };
			/* returns true when the chunk is finished.  exact_head: the run is the first of a
			 * later segment -- the match in front of it is FINAL (previous segment), so the
			 * first dword must not spill backwards: its bytes go out one by one. */
			auto put = [&](const seq_t e, const bool exact_head) -> bool {
				const uint32_t ls = SEQ_LIT_SRC(e), le = ls + SEQ_LIT_LEN(e);
				if (ls >= c1)
					return true;
				uint32_t m0, mend;	/* the chunk's dwords [m0, mend) are the run's, dword m at wb + 4 m */
				uint8_t *wb;		/* wb[p - c0] <-> payload[p]; W has 16 bytes of headroom */
				if (la_lz4_lit_run_dwords(ls, le, SEQ_DST(e), c0, W, &m0, &mend, &wb)) {
					const uint32_t lo = ls > c0 ? ls : c0, hi = le < c1 ? le : c1;	/* the run's bytes inside the chunk */
					if (exact_head && lo == ls && ((lo - c0) & 3u)) {
						const uint32_t stop = hi < c0 + 4 * m0 + 4 ? hi : c0 + 4 * m0 + 4;
						for (uint32_t pp = lo; pp < stop; pp++)	/* (once per segment: straight from the image) */
							wb[pp - c0] = (uint64_t)pp < s_room ? s[pp] : (uint8_t)0;
						m0++;
					}
					const uint32_t cnt = mend > m0 ? mend - m0 : 0;
#pragma unroll
					for (uint32_t m = 0; m < 8; m++)
						if (m - m0 < cnt)
							lds_st4(wb + 4 * m, dd[m]);
				}
				return le >= c1;
			};
			bool fin = false;
			if constexpr (DEPS) {
				/* The six runs at once, dword by dword (profiles/r30_lz4_literal_dwords.md).  put() tests each of a
				 * chunk's eight dwords once per run, 48 predicated stores for eight dwords to place.  The runs'
				 * dword ranges are disjoint (la_lz4_lit_run_dwords), so each dword has one owner or none: every run
				 * leaves its window offset in the dwords of its 8-bit range mask, and each dword goes out with ONE
				 * store under one predicate, to the same address with the same value as put() would send it.  An
				 * entry behind the table's last one is zero and owns nothing, like a run outside the chunk; the
				 * chunk is finished when the table is, or a run reaches the chunk's end.  A run slot that no lane
				 * of the wave has is skipped wave-uniformly. */
				uint32_t wo[8] = { 0, 0, 0, 0, 0, 0, 0, 0 }, any = 0;
				fin = kk[u] + 5 >= ns;
#pragma unroll
				for (int t = 0; t < 6; t++) {
					const uint32_t ls = SEQ_LIT_SRC(pe[u][t]), le = ls + SEQ_LIT_LEN(pe[u][t]);
					uint32_t m0 = 0, mend = 0, w0 = 0;
					la_lz4_lit_run_dwords(ls, le, SEQ_DST(pe[u][t]), c0, (uint32_t)(W - win), &m0, &mend, &w0);	/* (offsets from win: 13 and up) */
					const uint32_t own = (((1u << (mend - m0)) - 1u) << m0) & ~any;	/* (one owner whatever the table holds) */
					fin = fin || le >= c1;
					if (__ballot(own != 0) == 0)
						continue;
					any |= own;
#pragma unroll
					for (uint32_t m = 0; m < 8; m++)
						wo[m] |= w0 & (0u - ((own >> m) & 1u));	/* (one bit extract, one and-or) */
				}
#pragma unroll
				for (uint32_t m = 0; m < 8; m++)
					if ((any >> m) & 1u)
						lds_st4(win + wo[m] + 4 * m, dd[m]);
			} else {
#pragma unroll
				for (int t = 0; t < 6; t++)
					if (!fin)
						fin = (kk[u] + t >= ns) || put(pe[u][t], kb != 0 && kk[u] + t == 0);
			}
			for (uint32_t k = kk[u] + 6; !fin && k < ns; k++)	/* more than six sequences touch this chunk: rare */
				fin = put(seq_load(tab, k), false);
		}
	}
	/* DEPS: the slots' dependency words are requested here, in front of the barrier that ends phase L: the wait for
	 * the slowest wave covers their latency.  Requested in the prepass, beside the table entries, they hold eight
	 * registers through phase L (97 VGPRs instead of 90) and the four C2 launches took 18.4 ms instead of 18.0. */
	if (DEPS) {
#pragma unroll
		for (uint32_t r = 0; r < MAXSTEPS; r++) {
			const uint32_t k = fast_seq_index(r, wave, lane);
			dw[r] = (r * FAST_THREADS < ns && k < ns) ? deps[b.table_off + k] : 0;
		}
		publish();
	}
	STAMP(1);
	__syncthreads();
	STAMP(2);

	/* ---- phase M: matches, one thread per sequence ----
	 * First every step's dependency range [q, qend] (branch-free binary searches over
	 * the output positions, interleaved across steps), then the steps in order. */
	uint32_t qcur[MAXSTEPS];	/* search cursor, then (first dependency | count << 16) */
	if constexpr (DEPS) {
#pragma unroll
		for (uint32_t r = 0; r < MAXSTEPS; r++)
			qcur[r] = dw[r];
#ifdef LA_DIAG_M
		STAMP(6);	/* (no search: stamps 6 and 7 sit right behind the barrier) */
#endif
	} else {
#ifndef FAST_BSEARCH
	/* The sequence under a source position comes from a MAP, not from a binary search over the output
	 * positions (twelve dependent LDS reads per sequence: a third of the kernel's LDS cycles, PMC + count
	 * in DESIGN.md 5c): for every 32-byte chunk of the output the sequence that holds the chunk's first
	 * byte, then a short walk forward (a chunk holds at most eight sequence starts; half a one on the C2
	 * stream).  The map lives where phase L kept its chunk index: that is dead behind the barrier above. */
	uint16_t *const cmap = chunk_first;
#pragma unroll
	for (uint32_t r = 0; r < MAXSTEPS; r++) {
		if (r * FAST_THREADS >= ns)
			break;
		const uint32_t k = fast_seq_index(r, wave, lane);
		if (k < ns) {
			const uint32_t d = SEQ_DST(ent[r]);
			uint32_t nxt = dstpos[k + 1];
			if (nxt < d)
				nxt = 65536u;	/* (positions are 16-bit: an end at 65536 reads 0; a lone sequence that
						 * fills the window leaves the map unset, and nobody asks) */
			if (k == 0)
				for (uint32_t c = 0; (c << 5) < d; c++)
					cmap[c] = 0;	/* (later segments: positions in front of the segment) */
			for (uint32_t c = (d + 31) >> 5; (c << 5) < nxt; c++)
				cmap[c] = (uint16_t)k;
		}
	}
	__syncthreads();
#pragma unroll
	for (uint32_t r = 0; r < MAXSTEPS; r++) {
		qcur[r] = 0;
		if (r * FAST_THREADS >= ns)
			continue;
		const uint32_t k = fast_seq_index(r, wave, lane);
		const uint32_t s0 = SEQ_DST(ent[r]) + SEQ_LIT_LEN(ent[r]) - SEQ_OFF(ent[r]);
		if (k > 0 && k < ns) {
			const uint32_t q0 = cmap[(s0 < 65535u ? s0 : 65535u) >> 5];
			qcur[r] = q0 < k - 1 ? q0 : k - 1;	/* largest idx < k with dstpos[idx] <= s0, from below */
		}
	}
	{
		uint32_t act = 0;	/* wave-uniform: slots in which some lane is still walking */
#pragma unroll
		for (uint32_t r = 0; r < MAXSTEPS; r++)
			if (r * FAST_THREADS < ns)
				act |= 1u << r;
		while (act) {
#pragma unroll
			for (uint32_t r = 0; r < MAXSTEPS; r++) {
				if (!((act >> r) & 1u))
					continue;
				const uint32_t k = fast_seq_index(r, wave, lane);
				const uint32_t s0 = SEQ_DST(ent[r]) + SEQ_LIT_LEN(ent[r]) - SEQ_OFF(ent[r]);
				const bool adv = k < ns && qcur[r] + 1 < k && dstpos[qcur[r] + 1] <= s0;
				if (adv)
					qcur[r]++;
				if (__ballot(adv) == 0)
					act &= ~(1u << r);
			}
		}
	}
#else
#pragma unroll
	for (uint32_t r = 0; r < MAXSTEPS; r++)
		qcur[r] = 0;
	for (uint32_t bit = MAXSEQ / 2; bit; bit >>= 1) {
#pragma unroll
		for (uint32_t r = 0; r < MAXSTEPS; r++) {
			if (r * FAST_THREADS >= ns)
				break;
			/* largest idx < k with dstpos[idx] <= s0 */
			const uint32_t k = fast_seq_index(r, wave, lane);
			const uint32_t s0 = SEQ_DST(ent[r]) + SEQ_LIT_LEN(ent[r]) - SEQ_OFF(ent[r]);
			const uint32_t cand = qcur[r] + bit;
			if (cand < k && k < ns && dstpos[cand] <= s0)
				qcur[r] = cand;
		}
	}
#endif
	/* Literals are all in the window already (phase L), so a match only has to wait for
	 * earlier MATCHES under its source range.  The last sequence the range touches is
	 * often touched in its literal part only (a sequence is literals first, match second):
	 * its entry tells, and then it drops out of the wait -- about a third of all waits,
	 * and many sequences end up waiting for nothing at all. */
	uint32_t qlh[MAXSTEPS];	/* last sequence under the source range | last source byte << 16; ~0: none */
#pragma unroll
	for (uint32_t r = 0; r < MAXSTEPS; r++) {
		qlh[r] = 0xFFFFFFFFu;
		if (r * FAST_THREADS >= ns)
			continue;
		const uint32_t k = fast_seq_index(r, wave, lane);
		const uint32_t d = SEQ_DST(ent[r]), mdst = d + SEQ_LIT_LEN(ent[r]), off = SEQ_OFF(ent[r]);
		const uint32_t next = k < ns ? dstpos[k + 1] : 0;	/* dstpos[ns] = where the segment's output ends */
		const uint32_t mlen = k < ns ? (next - mdst) & 0xFFFFu : 0;	/* (positions are 16-bit: an end at 65536 reads 0) */
		uint32_t cnt = 0;	/* number of earlier sequences (of this segment) to wait for */
		uint32_t hi_byte = 0;
		qlh[r] = 0xFFFFFFFFu;
		if (la_lz4_dep_source(d, mdst, off, mlen, &hi_byte)) {
			/* sources that end before this segment's first output byte need nothing here:
			 * earlier segments are complete */
			if (k > 0 && dstpos[0] <= hi_byte) {
				uint32_t qe = qcur[r];
				while (qe + 1 < k && dstpos[qe + 1] <= hi_byte)
					qe++;
				cnt = qe - qcur[r] + 1;
				qlh[r] = qe | (hi_byte << 16);
			}
		}
		qcur[r] = (qcur[r] & 0xFFFFu) | (cnt << 16);
	}
#ifdef LA_DIAG_M
	STAMP(6);	/* chunk map, walks and dependency ranges done */
#endif
#pragma unroll
	for (uint32_t h = 0; h < MAXSTEPS; h += 4) {	/* four entries in flight at a time: registers */
		if (h * FAST_THREADS >= ns)
			break;
		seq_t le[4];
#pragma unroll
		for (uint32_t r = 0; r < 4; r++)
			le[r] = qlh[h + r] != 0xFFFFFFFFu ? seq_load(tab, qlh[h + r] & 0xFFFFu) : 0;
#pragma unroll
		for (uint32_t r = 0; r < 4; r++)
			if (qlh[h + r] != 0xFFFFFFFFu && la_lz4_dep_drops_last(qlh[h + r] >> 16, SEQ_DST(le[r]) + SEQ_LIT_LEN(le[r])))
				qcur[h + r] -= 1u << 16;	/* source ends inside the literals of the last sequence: its match is not needed */
	}
	}	/* !DEPS */

#ifdef LA_DIAG_M
	STAMP(7);	/* the last touched sequence's entry looked up (global memory) */
#endif
#pragma unroll 1
	for (uint32_t r = 0; r < MAXSTEPS; r++) {
		if (r * FAST_THREADS >= ns)
			break;
		/* ---- per-slot setup, once per slot: everything the poll iteration needs ---- */
		const uint32_t k = fast_seq_index(r, wave, lane);
		const bool active = k < ns;
		/* registers of step r (the array is indexed by a loop counter: pick by selects) */
		seq_t e = ent[0];
		uint32_t qp = qcur[0];
#pragma unroll
		for (uint32_t t = 1; t < MAXSTEPS; t++)
			if (r == t) { e = ent[t]; qp = qcur[t]; }
		const uint32_t off = SEQ_OFF(e);
		const uint32_t mdst = SEQ_DST(e) + SEQ_LIT_LEN(e);
		const uint32_t next = active ? dstpos[k + 1] : 0;
		const uint32_t mlen = active ? (next - mdst) & 0xFFFFu : 0;
		const uint32_t s0 = mdst - off;
		uint32_t q = qp & 0xFFFFu;
#ifdef FAST_EXP_NODEP
		const uint32_t qstop = q;	/* what-if (wrong output): nobody waits for anybody */
#else
		const uint32_t qstop = q + (qp >> 16);	/* exclusive; q == qstop: nothing to wait for */
#endif
		uint8_t *const mp = W + mdst;
		const uint8_t *const fp = W + s0;
		/* The copy class of the lane's match, fixed for the slot.  The iteration tests each class
		 * against the ready lanes once: a class without ready lanes is one skipped branch.
		 *   c_long   no overlap, 16 bytes and more: 16-byte pieces, the last one placed so that it
		 *            ENDS with the match (overlapping stores instead of a ragged tail)
		 *   c_mid    no overlap, 8..15 bytes: two 8-byte pieces, the second one end-aligned
		 *   c_short  no overlap, 4..7 bytes: one 8-byte load (it may read up to 7 bytes past the
		 *            source: window bytes or slack), two overlapping 4-byte stores
		 *   c_tiny   no overlap, 1..3 bytes (only the deflate front end makes these): one 8-byte
		 *            load, the bytes stored piece by piece
		 *   c_per8   overlapping, period >= 8: forward 8-byte steps only read bytes stored at
		 *            least one step earlier
		 *   c_per1   overlapping, period < 8: byte by byte
		 * An unaligned LDS access costs one cycle per ACTIVE LANE whatever its width
		 * (tools/ubench_lds.hip): every lane moves its match with as few, as wide accesses as it
		 * takes, and the loads of a class are all issued before anything is stored.  Nothing is
		 * read outside the source from 8 bytes up. */
		const bool disjoint = off >= mlen;
		/* c_long: 32 bytes per trip from i = 0 to tl, then 16..47 bytes left: one piece from tl, a
		 * second one behind it from 33 left, an end-aligned one from 17 left */
		const uint32_t tl = mlen >= 16 ? (mlen - 16) & ~31u : 0u;
		const bool l33 = mlen - tl > 32, l17 = mlen - tl > 16;
		uint8_t *const mpt = mp + tl;
		const uint8_t *const fpt = fp + tl;
		const bool c_long = disjoint && mlen >= 16;
		const bool c_mid = disjoint && mlen >= 8 && mlen < 16;
		const bool c_short = disjoint && mlen >= 4 && mlen < 8;
		const bool c_tiny = disjoint && mlen != 0 && mlen < 4;
		const bool c_per8 = !disjoint && off >= 8;
		const bool c_per1 = !disjoint && off < 8;
		bool todo = mlen != 0;	/* the lane's match is not in the window yet */
		if (active && !todo)
			atomicOr(&donebits[k >> 5], 1u << (k & 31));
		uint32_t spins = 0;	/* wave-uniform: iterations of this slot that left some lane waiting */

		/* ---- the poll iteration: one flag look for the waiting lanes, the copies of the ready
		 * lanes class by class, their done bits, one ballot ---- */
		for (;;) {
#if defined(LA_DIAG) && !defined(LA_DIAG_L) && !defined(LA_DIAG_M)
			if (lane == 0 && la_diag_stamps) atomicAdd(&la_diag_stamps[(size_t)blockIdx.x * 8 + 6], 1ull);
			const unsigned long long t_it0 = __builtin_readcyclecounter();
#endif
			/* advance q over finished sequences: ONE look at the flag word of q per iteration (a
			 * second look in the same iteration would only be another LDS round trip for the whole
			 * wave; a wait that spans two words takes two iterations).  Bit 0 of `word` is the flag
			 * of q; the zeros shifted in from the top end the run at the word boundary.  (Only lanes
			 * that still have their match to copy have q < qstop.) */
			if (q < qstop) {
				const uint32_t word = __hip_atomic_load(&donebits[q >> 5], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) >> (q & 31);
				const uint32_t inv = ~word;
				q += inv ? (uint32_t)__builtin_ctz(inv) : 32u;
			}
			if (todo && q >= qstop) {
				asm volatile("" ::: "memory");
#ifndef FAST_EXP_NOCOPY	/* (what-if, wrong output: the flag protocol alone) */
				if (c_long) {
					if (tl != 0) {	/* 48 bytes and more */
						for (uint32_t i = 0; i < tl; i += 32) {
							const uint4 v0 = lds_ld16(fp + i), v1 = lds_ld16(fp + i + 16);
							lds_st16(mp + i, v0);
							lds_st16(mp + i + 16, v1);
						}
					}
					uint4 vb, vt;	/* (loaded and stored under the same tests) */
					const uint4 va = lds_ld16(fpt);
					if (l33)
						vb = lds_ld16(fpt + 16);
					if (l17)
						vt = lds_ld16(fp + mlen - 16);
					lds_st16(mpt, va);
					if (l33)
						lds_st16(mpt + 16, vb);
					if (l17)
						lds_st16(mp + mlen - 16, vt);
				}
				if (c_mid) {
					const uint64_t a0 = lds_ld8(fp), at = lds_ld8(fp + mlen - 8);
					lds_st8(mp, a0);
					lds_st8(mp + mlen - 8, at);
				}
				if (c_short) {
					const uint64_t a0 = lds_ld8(fp);
					lds_st4(mp, (uint32_t)a0);
					lds_st4(mp + mlen - 4, (uint32_t)(a0 >> (8 * (mlen - 4))));
				}
				if (c_tiny)
					lds_st_tail(mp, lds_ld8(fp), mlen);
				if (c_per8) {
					uint32_t i = 0;
					for (; i + 8 <= mlen; i += 8) {
						uint64_t a = lds_ld8(mp + i - off);
						lds_st8(mp + i, a);
						asm volatile("" ::: "memory");	/* keep load/store order: the ranges overlap */
					}
					for (; i < mlen; i++)
						{ uint8_t bq = mp[(int)i - (int)off]; asm volatile("" ::: "memory"); mp[i] = bq; asm volatile("" ::: "memory"); }
				}
				if (c_per1) {
					/* replicate with period `off`: every byte read is one this lane (or an earlier
					 * sequence) already wrote */
					for (uint32_t i = 0; i < mlen; i++)
						{ uint8_t bq = mp[(int)i - (int)off]; asm volatile("" ::: "memory"); mp[i] = bq; asm volatile("" ::: "memory"); }
				}
#else
				(void)mp; (void)fp; (void)mpt; (void)fpt; (void)l33; (void)l17; (void)c_long; (void)c_mid; (void)c_short; (void)c_tiny; (void)c_per8; (void)c_per1;
#endif
				asm volatile("" ::: "memory");
				atomicOr(&donebits[k >> 5], 1u << (k & 31));
				todo = false;
			}
#if defined(LA_DIAG) && !defined(LA_DIAG_L) && !defined(LA_DIAG_M)
			if (lane == 0 && la_diag_stamps) atomicAdd(&la_diag_stamps[(size_t)blockIdx.x * 8 + 7], __builtin_readcyclecounter() - t_it0);
#endif
			if (__ballot(todo) == 0)
				break;
			/* every wait is bounded: a dependency that never completes (impossible for a table
			 * the parse kernel produced) fails the block instead of hanging the GPU; the lanes
			 * still waiting then copy in the next iteration */
			if (++spins > (1u << 20)) {
				if (todo) {
					status_out[bi] = LA_ST_LZ4_DECODE;
					q = qstop;
				}
			}
			__builtin_amdgcn_s_sleep(POLL_SLEEP);	/* back off: polling waves share the LDS with copying ones */
		}
	}
	STAMP(3);
	__syncthreads();
	};
	/* the usual block is one segment: that copy of the body is compiled with kb = 0 folded in
	 * (and without the register pressure of a loop around it) */
	if (!SEG) {
		segment(0u);
	} else {
		for (uint32_t kb = 0; kb < ns_all; kb += MAXSEQ)
			segment(kb);
	}
	STAMP(4);

	/* ---- phase F: window -> decoded slab, 16 bytes per lane per step ---- */
	uint32_t head = (16u - (uint32_t)((uintptr_t)g_out & 15)) & 15u;
	if (head > olen) head = olen;
	if (tid < head)
		g_out[tid] = W[tid];
	const uint32_t nflush = (olen - head) >> 4;
	const uint4 *wsrc = (const uint4 *)(W + head);
	uint4 *gdst = (uint4 *)(g_out + head);
	for (uint32_t c = tid; c < nflush; c += FAST_THREADS)
		gdst[c] = wsrc[c];
	const uint32_t tail0 = head + (nflush << 4);
	if (tail0 + tid < olen)
		g_out[tail0 + tid] = W[tail0 + tid];
	STAMP(5);
	};	/* do_block */
	if constexpr (STRIDED) {
		do_block(la_lz4_split_block(big_list.base, big_list.period, blockIdx.x, blockIdx.y));
	} else if constexpr (!SEG) {
		do_block(blockIdx.x);
	} else {
		const uint32_t cnt = *big_count;
		for (uint32_t li = blockIdx.x; li < cnt; li += gridDim.x) {
			do_block(big_list[li]);
			__syncthreads();	/* the window is reused */
		}
	}
}

/* blocks the SEG launch must take.  (This kernel is not given the slab: it lists a block without that bound, and the
 * SEG launch asks again with it before it touches the block.) */
__global__ __launch_bounds__(256) void lz4_classify_kernel(const la_lz4_block *__restrict__ blocks, uint32_t n,
    const uint32_t *__restrict__ status, const uint32_t *__restrict__ nseq, uint32_t *__restrict__ big_list,
    uint32_t *__restrict__ big_count, const uint32_t *__restrict__ out_len, uint32_t long_thr)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n)
		return;
	if (la_lz4_route(blocks[i], status[i], out_len[i], nseq[i], 0, ~0ull, true, long_thr) == LA_XR_WINDOW_SEG)
		big_list[atomicAdd(big_count, 1u)] = i;
}

#ifdef LA_DIAG
extern "C" int la_diag_set_stamps(void *d_buf)
{
	unsigned long long *p = (unsigned long long *)d_buf;
	return (int)hipMemcpyToSymbol(HIP_SYMBOL(la_diag_stamps), &p, sizeof(p));
}
#endif

void la_launch_lz4_expand_fast(hipStream_t s, const la_expand_job &j)
{
	if (j.n == 0) return;
	if (j.deps && j.lit_plan)
		hipLaunchKernelGGL((lz4_expand_fast_kernel<LA_LZ4_FAST_MAXSEQ, false, true>), dim3(j.n), dim3(FAST_THREADS), 0, s,
		    j.src, j.src_bytes, j.blocks, j.n, j.dst, j.dst_cap, j.dst_off, j.out_len, j.status, j.nseq,
		    j.table, j.table_off, (const uint32_t *)nullptr, (const uint32_t *)nullptr, j.long_thr, j.deps, j.lit_plan);
	else
		hipLaunchKernelGGL((lz4_expand_fast_kernel<LA_LZ4_FAST_MAXSEQ, false, false>), dim3(j.n), dim3(FAST_THREADS), 0, s,
		    j.src, j.src_bytes, j.blocks, j.n, j.dst, j.dst_cap, j.dst_off, j.out_len, j.status, j.nseq,
		    j.table, j.table_off, (const uint32_t *)nullptr, (const uint32_t *)nullptr, j.long_thr, (const uint32_t *)nullptr,
		    (const uint8_t *)nullptr);
}

/* Group g of a split last slice: j is the WHOLE batch's job (with dependency words and literal plans), sp the slice's
 * schedule.  One workgroup per position of the group in every period that has one; a block at or behind sp.last leaves
 * at the kernel's `bi >= n` test. */
void la_launch_lz4_expand_fast_group(hipStream_t s, const la_expand_job &j, const la_lz4_split &sp, uint32_t g)
{
	const uint32_t gx = la_lz4_split_grid_x(&sp, g), gy = la_lz4_split_grid_y(&sp, g);
	if (gx == 0 || gy == 0) return;
	const fast_stride st = { sp.first + sp.bound[g], sp.period };
	hipLaunchKernelGGL((lz4_expand_fast_kernel<LA_LZ4_FAST_MAXSEQ, false, true, true>), dim3(gx, gy), dim3(FAST_THREADS), 0, s,
	    j.src, j.src_bytes, j.blocks, sp.last, j.dst, j.dst_cap, j.dst_off, j.out_len, j.status, j.nseq,
	    j.table, j.table_off, st, (const uint32_t *)nullptr, j.long_thr, j.deps, j.lit_plan);
}

/* blocks with more than LA_LZ4_FAST_MAXSEQ sequences, over the WHOLE table: classify + a small
 * grid that shares them out.  d_big: n + 1 words of workspace (count first). */
void la_launch_lz4_expand_fast_big(hipStream_t s, const la_expand_job &j, uint32_t *d_big)
{
	if (j.n == 0) return;
	(void)hipMemsetAsync(d_big, 0, sizeof(uint32_t), s);
	hipLaunchKernelGGL(lz4_classify_kernel, dim3((j.n + 255) / 256), dim3(256), 0, s, j.blocks, j.n, j.status, j.nseq,
	    d_big + 1, d_big, j.out_len, j.long_thr);
	const uint32_t grid = j.n < 1024u ? j.n : 1024u;
	hipLaunchKernelGGL((lz4_expand_fast_kernel<LA_LZ4_FAST_MAXSEQ, true, false>), dim3(grid), dim3(FAST_THREADS), 0, s,
	    j.src, j.src_bytes, j.blocks, j.n, j.dst, j.dst_cap, j.dst_off, j.out_len, j.status, j.nseq,
	    j.table, j.table_off, (const uint32_t *)(d_big + 1), (const uint32_t *)d_big, j.long_thr, (const uint32_t *)nullptr,
	    (const uint8_t *)nullptr);
}
