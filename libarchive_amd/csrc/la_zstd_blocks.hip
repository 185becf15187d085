/*
 * la_zstd_blocks.hip -- LA_ZSTD_OPT_BLOCK_PARALLEL (gfx950): the blocks of ONE Zstandard frame decoded in parallel, for
 * the one-frame .zst that la_zstd.hip runs on a single wave.  A frame is a chain of blocks of at most 128 KiB; what ties
 * a block to the ones before it is (a) the entropy tables it repeats, (b) the three repeat offsets, (c) the bytes its
 * matches copy.  Each is cut here:
 *   (a) the index stage notes, per block and table, the block that last DEFINED the table; a block that repeats a table
 *       re-parses the definer's description (header-sized work) instead of waiting for it;
 *   (b) which history entry a repeat code picks depends on the Offset_Value and on ll == 0, never on the history's
 *       contents: a block's offsets are decoded SYMBOLICALLY ("incoming repeat offset k minus d") and made concrete
 *       once a serial walk of a few instructions per block has handed every block its incoming offsets;
 *   (c) match bytes are not copied but named: one source pointer per output byte, resolved by the pointer-jumping
 *       passes and the gather of la_inflate_chain.hip (no waiting inside a launch, no order between workgroups).
 *
 * Stages, all queued on the stream without a host round trip (grids come from capacities, loops stride over counts that
 * only the device knows):
 *   index    one LANE per frame: frame header, block headers, per compressed block the literals header, the sequence
 *            count and the modes byte; definers; running literal / sequence-record offsets; the workspace rules
 *   (scan)   la_scan.hip over the frames' block counts: work item -> (frame, block) by binary search
 *   entropy  one WAVE per compressed block: tables, literals into the literal buffer, sequences into records
 *   place    one LANE per frame: output position and incoming repeat offsets of every block, totals
 *   emit     one WAVE per block: raw / RLE / literal bytes to d_dst, one pointer per match byte
 *   resolve  la_launch_chain_resolve_range
 *   verdict  one WAVE per frame: XXH64, result (status OK, path 1)
 * The block path only reports success.  Whatever it cannot finish -- any damage, any rule below -- raises the frame's
 * `todo` word, and the frame kernels of la_zstd.hip, launched behind these stages with the todo words as their d_only
 * argument, decode that frame from scratch: every refusal and its status come from there.
 *
 * Workspace rules per frame: at most 4 + src_len / 16 + dst_cap / 65536 blocks (the last term is for RLE blocks, 4 bytes
 * of input for up to 128 KiB of output: libzstd writes a megabyte of one byte as nine of them in 45 bytes), 16 +
 * dst_cap / 3 sequences, dst_cap literal bytes, dst_cap at most ZB_MAX_FRAME_OUT, and the table's frames in ascending,
 * disjoint order in d_src and d_dst (the host walker's order): frame i's block entries then start at
 * 4 i + src_off / 16 + dst_off / 65536, its sequence records at 16 i + dst_off / 3, its literals at dst_off, and no
 * scan over frames is needed to place them.  A table out of order hands every frame back.
 *
 * Nothing outside a frame's slot is written: the entropy stage bounds what a block produces (128 KiB, the literals
 * within the section), the place stage bounds the frame's total by dst_cap before any byte goes out, and the emit stage
 * compares every offset with the match's position in the frame before it stores a pointer.
 */
#include "la_dev.h"
#include "la_zstd_common.h"

#define ZB_MAX_WAVES 4096u		/* the largest grid of the per-block and per-frame wave kernels */
#define ZB_MAX_INDEX_BLOCKS 1024u	/* workgroups of 64 lanes of the per-frame lane kernels */
#define ZB_NONE 0xFFFFFFFFu
/* a frame's todo word: 0 = the block path has it; otherwise the stage that handed it back (any nonzero value sends it to
 * the frame kernels; the value tells which, for whoever inspects the workspace) */
enum { ZB_TODO_INDEX = 1, ZB_TODO_PLACE = 2, ZB_TODO_EMIT = 3, ZB_TODO_CHECKSUM = 4, ZB_TODO_ORDER = 5, ZB_TODO_ENTROPY = 32 /* + where */ };
/* symbolic repeat offsets: incoming offset k less d is 0xFFFFFFFF - (k << 20) - d (d < 2^20: a block has fewer than
 * 2^17 sequences); stated offsets up there are refused, and a frame's slot is smaller than the lowest of them */
#define ZB_SYM_MIN 0xFFD00000u
#define ZB_SYM(k) (0xFFFFFFFFu - ((uint32_t)(k) << 20))
#define ZB_MAX_FRAME_OUT 0xFF000000ull

struct zb_block {
	uint32_t src;		/* the block's content, from the frame's first byte */
	uint32_t hdr;		/* Block_Header: Block_Size << 3 | type << 1 | last */
	uint32_t lit_off;	/* literal bytes of the frame's earlier blocks */
	uint32_t seq_off;	/* sequences of the frame's earlier blocks */
	uint32_t regen;		/* literals of this block */
	uint32_t nseq;
	uint32_t seq_src;	/* the modes byte, from the block's first byte (nseq > 0) */
	uint32_t def[4];	/* block of the frame that last defined the Huffman tree / LL / OF / ML table (this one included) */
	uint32_t out_len;	/* entropy stage: bytes the block produces */
	uint32_t rep_out[3];	/* entropy stage: the repeat offsets behind it, concrete or symbolic */
	uint32_t out_pos;	/* place stage: where it starts in the frame */
	uint32_t rep_in[3];	/* place stage: the repeat offsets in front of it */
};
struct zb_frame { uint64_t fcs; uint32_t nblk, bmax, csum_at, has_fcs, total; };
struct zb_seq { uint32_t ll, ml, off; };

struct zb_ws {
	uint32_t *todo;		/* [n] first: la_zstd_blocks_todo */
	uint32_t *nblk;		/* [n] */
	uint64_t *blk_start;	/* [n + 1] */
	void *scan;
	zb_frame *fr;		/* [n] */
	zb_block *blk;		/* [4 n + src_bytes / 16 + dst_cap / 65536] */
	zb_seq *seq;		/* [16 n + dst_cap / 3] */
	uint8_t *lit;		/* [dst_cap] */
	uint32_t *ptr;		/* [dst_cap] */
	uint32_t *ctl;		/* [LA_CHAIN_CTL_WORDS] the jump passes' flags, then [1]: the frame table is out of order */
	uint64_t total;
};

static void zb_carve(zb_ws *w, uint8_t *base, uint32_t n, uint64_t src_bytes, uint64_t dst_cap)
{
	la_carve cv = { base, 0 };
	w->todo = cv.take<uint32_t>(n, 256);
	w->nblk = cv.take<uint32_t>(n, 256);
	w->blk_start = cv.take<uint64_t>((uint64_t)n + 1, 256);
	w->scan = cv.take<uint8_t>(la_scan_scratch_bytes(n), 256);
	w->fr = cv.take<zb_frame>(n, 256);
	w->blk = cv.take<zb_block>(4ull * n + src_bytes / 16 + dst_cap / 65536, 256);
	w->seq = cv.take<zb_seq>(16ull * n + dst_cap / 3, 256);
	w->lit = cv.take<uint8_t>(dst_cap, 256);
	w->ptr = cv.take<uint32_t>(dst_cap, 256);
	w->ctl = cv.take<uint32_t>(LA_CHAIN_CTL_WORDS + 1, 256);
	w->total = ((cv.off + 255) & ~255ull) + 4096;
}

uint64_t la_zstd_blocks_workspace_bytes(uint32_t n_frames, uint64_t src_bytes, uint64_t dst_cap)
{
	zb_ws w;
	zb_carve(&w, NULL, n_frames, src_bytes, dst_cap);
	return w.total;
}

const uint32_t *la_zstd_blocks_todo(const uint8_t *ws) { return (const uint32_t *)ws; }

__device__ __forceinline__ static zb_block *zb_blocks_of(zb_block *blk, uint32_t i, const la_zstd_frame &fr) { return blk + 4ull * i + fr.src_off / 16 + fr.dst_off / 65536; }

/* ---- index: one lane per frame ---- */

/* what the index notes of one compressed block b[0..bsize): literals, sequence count, where the modes byte stands, and
 * the definers (def[], updated).  Returns 0, or -1 to hand the frame back.
 * Why __noinline__, and why the walk below stores an entry field by field: the first form of this code built the entry in
 * a local `zb_block e = {}` inside the walk, with this parse inlined, and stored it with `B[nb++] = e`.  hipcc -O3 for
 * gfx950 (ROCm's clang, the version this library is built with) then stored 0 for `regen` and `nseq` of every block that
 * has sequences: in the ISA the registers of those two fields are set to 0 on the `ns != 0` path behind the modes loop
 * and never reloaded before the entry's global_store_dwordx4, while the sums `lit += regen; nsq += ns` use the right
 * values; the same source compiled for the host (g++ with the address and undefined-behaviour sanitizers) gives the
 * right entries and no report.  No undefined behaviour was found in the source, so this is recorded as a compiler
 * finding, not explained: source and ISA excerpt in profiles/r14_zstd_index_isa.txt.  The guard against its return is
 * the entropy stage, which compares its own sequence count with the entry's and hands the frame back on a difference
 * (a valid frame then fails `path == 1` in tests/test_gpu_zstd_blocks.py, as it did). */
__device__ __noinline__ static int zb_index_compressed(const uint8_t *b, uint32_t bsize, uint32_t nb, uint32_t *def, uint32_t *out /* regen, nseq, seq_src */)
{
	zlit_hdr lh;
	if (zstd_lit_header(b, bsize, lh) < 0) return -1;
	const size_t lsz = lh.hl + (lh.ltype == 0 ? lh.regen : (lh.ltype == 1 ? 1 : lh.comp));
	if (lsz > bsize) return -1;
	if (lh.ltype == 2) def[0] = nb;
	else if (lh.ltype == 3 && def[0] == ZB_NONE) return -1;
	size_t ns = 0;
	const int c = zstd_nseq(b + lsz, bsize - lsz, &ns);
	if (c < 0) return -1;
	uint32_t seq_src = 0;
	if (ns != 0) {
		seq_src = (uint32_t)(lsz + (size_t)c);
		if (seq_src >= bsize) return -1;
		const uint32_t modes = b[seq_src];
		for (int t = 0; t < 3; t++) {	/* LL, OF, ML: any mode but Repeat defines the table */
			if (((modes >> (6 - 2 * t)) & 3u) != 3u) def[1 + t] = nb;
			else if (def[1 + t] == ZB_NONE) return -1;
		}
	}
	out[0] = (uint32_t)lh.regen; out[1] = (uint32_t)ns; out[2] = seq_src;
	return 0;
}

/* Returns the frame's blocks, or -1 to hand it back */
__device__ static int zb_index_frame(const uint8_t *s, size_t len, uint64_t dst_cap, zb_block *B, zb_frame *F)
{
	zframe_hdr fh;
	if (zstd_frame_header(s, len, fh) < 0 || fh.skippable) return -1;
	const uint64_t cap_b = 4u + len / 16 + dst_cap / 65536;
	const uint64_t cap_s = 16 + dst_cap / 3;
	size_t p = fh.p;
	uint64_t lit = 0, nsq = 0;
	uint32_t nb = 0, def[4] = { ZB_NONE, ZB_NONE, ZB_NONE, ZB_NONE };
	for (;;) {
		if (p + 3 > len) return -1;
		const uint32_t bh = s[p] | ((uint32_t)s[p + 1] << 8) | ((uint32_t)s[p + 2] << 16);
		p += 3;
		const int last = bh & 1, type = (bh >> 1) & 3;
		const uint32_t bsize = bh >> 3;
		if (zstd_block_header_bad(type, bsize, fh.bmax) || nb >= cap_b) return -1;
		uint32_t v[3] = { 0, 0, 0 };	/* regen, nseq, seq_src */
		const uint32_t at = (uint32_t)p;
		if (type == 1) {
			if (p + 1 > len) return -1;
			p += 1;
		} else {
			if (p + bsize > len) return -1;
			if (type == 2 && zb_index_compressed(s + p, bsize, nb, def, v) < 0) return -1;
			p += bsize;
		}
		zb_block *e = B + nb;	/* (the fields the later stages fill stay as they are) */
		e->src = at; e->hdr = bh; e->lit_off = (uint32_t)lit; e->seq_off = (uint32_t)nsq;
		e->regen = v[0]; e->nseq = v[1]; e->seq_src = v[2];
		for (int t = 0; t < 4; t++) e->def[t] = def[t];
		lit += v[0]; nsq += v[1];
		if (lit > dst_cap || nsq > cap_s) return -1;
		nb++;
		if (last) break;
	}
	F->csum_at = ZB_NONE;
	if (fh.csum) {
		if (p + 4 > len) return -1;
		F->csum_at = (uint32_t)p;
		p += 4;
	}
	if (p != len) return -1;	/* (the host cut the frame here) */
	F->fcs = fh.fcs; F->has_fcs = fh.fcs_len != 0; F->bmax = fh.bmax; F->nblk = nb; F->total = 0;
	return (int)nb;
}

__global__ __launch_bounds__(64) void zb_index_kernel(const uint8_t *__restrict__ src, uint64_t src_bytes, const la_zstd_frame *__restrict__ frames,
    uint32_t n, uint64_t dst_cap, zb_ws W)
{
	for (uint32_t i = blockIdx.x * 64u + threadIdx.x; i < n; i += gridDim.x * 64u) {
		const la_zstd_frame fr = frames[i];
		int nb = -1;
		const bool inside = fr.src_off <= src_bytes && fr.src_len <= src_bytes - fr.src_off && fr.dst_off <= dst_cap && fr.dst_cap <= dst_cap - fr.dst_off;
		if (i != 0) {
			const la_zstd_frame pv = frames[i - 1];
			if (pv.src_off > fr.src_off || pv.src_len > fr.src_off - pv.src_off || pv.dst_off > fr.dst_off || pv.dst_cap > fr.dst_off - pv.dst_off)
				W.ctl[LA_CHAIN_CTL_WORDS] = 1;	/* out of order: table regions would overlap, every frame is handed back */
		}
		if (inside && fr.src_len < 0xFFFFFFF0ull && fr.dst_cap <= ZB_MAX_FRAME_OUT)
			nb = zb_index_frame(src + fr.src_off, (size_t)fr.src_len, fr.dst_cap, zb_blocks_of(W.blk, i, fr), &W.fr[i]);
		W.todo[i] = nb < 0 ? ZB_TODO_INDEX : 0u;
		W.nblk[i] = nb < 0 ? 0u : (uint32_t)nb;
	}
}

/* work item w of the per-block kernels -> frame (the largest f with blk_start[f] <= w) */
__device__ __forceinline__ static uint32_t zb_frame_of(const uint64_t *__restrict__ blk_start, uint32_t n, uint64_t w)
{
	uint32_t lo = 0, hi = n;
	while (hi - lo > 1) {
		const uint32_t mid = lo + (hi - lo) / 2;
		if (blk_start[mid] <= w) lo = mid; else hi = mid;
	}
	return lo;
}

/* ---- entropy: one wave per compressed block ---- */

/* table `which` (0 LL, 1 OF, 2 ML) from the sequences section of the block that defined it */
__device__ static int zb_definer_table(zframe *f, const uint8_t *dp, uint32_t dsize, uint32_t seq_src, int which)
{
	if (seq_src == 0 || seq_src >= dsize) return -1;
	const uint8_t *q = dp + seq_src;
	size_t left = dsize - seq_src;
	const int modes = q[0];
	q += 1; left -= 1;
	const int max_al[3] = { 9, 8, 9 }, max_sym[3] = { 35, 31, 52 };
	for (int t = 0; t < which; t++) {	/* the descriptions in front of it */
		const int m = (modes >> (6 - 2 * t)) & 3;
		int c = 0;
		if (m == 1) c = 1;
		else if (m == 2) {
			int16_t norm[64]; int ns, al;
			c = fse_read_ncount(q, left, max_al[t], max_sym[t], norm, &ns, &al);
			if (c < 0) return -1;
		}
		if ((size_t)c > left) return -1;
		q += c; left -= (size_t)c;
	}
	const int m = (modes >> (6 - 2 * which)) & 3;
	if (m == 3) return -1;
	int have = 0;
	if (which == 0) return seq_table(&f->ll, &have, m, q, left, 9, 35, LL_DEF, 36, 6) < 0 ? -1 : 0;
	if (which == 1) return seq_table(&f->of, &have, m, q, left, 8, 31, OF_DEF, 29, 5) < 0 ? -1 : 0;
	return seq_table(&f->ml, &have, m, q, left, 9, 52, ML_DEF, 53, 6) < 0 ? -1 : 0;
}

/* returns 0 with *out_len and rep_out, or a negative number that says where it stopped (kept in the todo word) */
__device__ static int zb_entropy_block(zframe *f, const uint8_t *fs, const zb_block *B, const zb_block *ep, uint8_t *lit, zb_seq *S,
    uint32_t bmax, uint32_t *out_len, uint32_t *rep_out)
{
	const zb_block &e = *ep;
	const uint8_t *src = fs + e.src;
	const size_t len = e.hdr >> 3;
	zlit_hdr lh;
	if (zstd_lit_header(src, len, lh) < 0) return -1;
	f->have_huf = 0;
	if (lh.ltype == 3) {	/* treeless: the tree of the block that last sent one */
		if (e.def[0] == ZB_NONE) return -2;
		const zb_block &d = B[e.def[0]];
		const uint8_t *dp = fs + d.src;
		const size_t dsize = d.hdr >> 3;
		zlit_hdr dh;
		if (zstd_lit_header(dp, dsize, dh) < 0 || dh.ltype != 2 || dh.hl + dh.comp > dsize) return -3;
		if (huf_read(&f->huf, dp + dh.hl, dh.comp) < 0) return -4;
		f->have_huf = 1;
	}
	const int64_t lu = zstd_literals<true>(f, src, len, lh, lit);
	if (lu < 0) return -5;
	const uint32_t regen = (uint32_t)lh.regen;
	const uint8_t *p = src + lu;
	size_t left = len - (size_t)lu;
	size_t nseq;
	{ const int c = zstd_nseq(p, left, &nseq); if (c < 0) return -6; p += c; left -= (size_t)c; }
	uint32_t out = 0, lit_pos = 0;
	rep_out[0] = ZB_SYM(0); rep_out[1] = ZB_SYM(1); rep_out[2] = ZB_SYM(2);
	if (nseq) {
		if (nseq != e.nseq || left < 1) return -7;
		const int modes = p[0];
		p += 1; left -= 1;
		int c, have = 0;
		if ((modes >> 6) != 3) { c = seq_table(&f->ll, &have, modes >> 6, p, left, 9, 35, LL_DEF, 36, 6); if (c < 0) return -8; p += c; left -= (size_t)c; }
		else { const zb_block &d = B[e.def[1]]; if (zb_definer_table(f, fs + d.src, d.hdr >> 3, d.seq_src, 0) < 0) return -9; }
		if (((modes >> 4) & 3) != 3) { c = seq_table(&f->of, &have, (modes >> 4) & 3, p, left, 8, 31, OF_DEF, 29, 5); if (c < 0) return -10; p += c; left -= (size_t)c; }
		else { const zb_block &d = B[e.def[2]]; if (zb_definer_table(f, fs + d.src, d.hdr >> 3, d.seq_src, 1) < 0) return -11; }
		if (((modes >> 2) & 3) != 3) { c = seq_table(&f->ml, &have, (modes >> 2) & 3, p, left, 9, 52, ML_DEF, 53, 6); if (c < 0) return -12; p += c; left -= (size_t)c; }
		else { const zb_block &d = B[e.def[3]]; if (zb_definer_table(f, fs + d.src, d.hdr >> 3, d.seq_src, 2) < 0) return -13; }
		seqdec<rbits> sd;
		sd.pos = (int32_t)rev_init(p, left);
		if (sd.pos < 0) return -14;
		bits_init(sd.rb, p, left);
		sd.sl = bits_read<false>(sd.rb, &sd.pos, (unsigned)f->ll.al);
		sd.so = bits_read<false>(sd.rb, &sd.pos, (unsigned)f->of.al);
		sd.sm = bits_read<false>(sd.rb, &sd.pos, (unsigned)f->ml.al);
		if (sd.pos < 0) return -15;
		sd.r0 = ZB_SYM(0); sd.r1 = ZB_SYM(1); sd.r2 = ZB_SYM(2);
		const uint32_t lane = __lane_id();
		for (size_t base = 0; base < nseq; base += 64) {
			const uint32_t cnt = nseq - base < 64 ? (uint32_t)(nseq - base) : 64u;
			zb_seq mine = { 0, 0, 0 };
			for (uint32_t j = 0; j < cnt; j++) {	/* the wave decodes (uniform), lane j keeps sequence j */
				uint32_t ll, ml, offset, ov;
				if (seq_next<false>(f, sd, base + j + 1 == nseq, ll, ml, offset, ov) < 0) return -16;
				if (ov > 3 && offset >= ZB_SYM_MIN) return -17;	/* (beyond any slot this path takes) */
				if (ll > regen - lit_pos) return -18;
				if (out + ll + ml > ZBLOCK_MAX) return -19;
				if (lane == j) { mine.ll = ll; mine.ml = ml; mine.off = offset; }
				out += ll + ml; lit_pos += ll;
			}
			if (lane < cnt) S[base + lane] = mine;
		}
		rep_out[0] = sd.r0; rep_out[1] = sd.r1; rep_out[2] = sd.r2;
		if (sd.pos != 0) return -20;
	} else if (left != 0) return -21;
	out += regen - lit_pos;
	if (out > ZBLOCK_MAX || out > bmax) return -22;
	*out_len = out;
	return 0;
}

__global__ __launch_bounds__(64) void zb_entropy_kernel(const uint8_t *__restrict__ src, const la_zstd_frame *__restrict__ frames, uint32_t n, zb_ws W)
{
	__shared__ zframe sf;
	for (uint32_t i = threadIdx.x; i < sizeof(seq_tabs) / 4; i += 64)
		((uint32_t *)&sf.tabs)[i] = ((const uint32_t *)&SEQ_TABS)[i];
	__syncthreads();
	if (W.ctl[LA_CHAIN_CTL_WORDS]) return;
	const uint64_t total = W.blk_start[n];
	for (uint64_t w = blockIdx.x; w < total; w += gridDim.x) {
		const uint32_t fi = zb_frame_of(W.blk_start, n, w);
		const la_zstd_frame fr = frames[fi];
		zb_block *B = zb_blocks_of(W.blk, fi, fr);
		zb_block *e = B + (w - W.blk_start[fi]);
		if (((e->hdr >> 1) & 3) != 2) continue;
		uint32_t out_len = 0, rep_out[3];
		const zb_block ev = *e;
		const int r = zb_entropy_block(&sf, src + fr.src_off, B, e, W.lit + fr.dst_off + ev.lit_off,
		    W.seq + 16ull * fi + fr.dst_off / 3 + ev.seq_off, W.fr[fi].bmax, &out_len, rep_out);
		if (threadIdx.x == 0) {
			if (r < 0) W.todo[fi] = ZB_TODO_ENTROPY + (uint32_t)-r;
			else { e->out_len = out_len; e->rep_out[0] = rep_out[0]; e->rep_out[1] = rep_out[1]; e->rep_out[2] = rep_out[2]; }
		}
		wave_fence();
	}
}

/* ---- place: one lane per frame ---- */
__global__ __launch_bounds__(64) void zb_place_kernel(const la_zstd_frame *__restrict__ frames, uint32_t n, zb_ws W)
{
	if (W.ctl[LA_CHAIN_CTL_WORDS]) return;
	for (uint32_t i = blockIdx.x * 64u + threadIdx.x; i < n; i += gridDim.x * 64u) {
		if (W.todo[i]) continue;
		const la_zstd_frame fr = frames[i];
		zb_block *B = zb_blocks_of(W.blk, i, fr);
		zb_frame *F = &W.fr[i];
		uint64_t pos = 0;
		uint32_t r[3] = { 1, 4, 8 };
		bool bad = false;
		for (uint32_t b = 0; b < F->nblk && !bad; b++) {
			zb_block *e = B + b;
			e->out_pos = (uint32_t)pos;
			e->rep_in[0] = r[0]; e->rep_in[1] = r[1]; e->rep_in[2] = r[2];
			if (((e->hdr >> 1) & 3) == 2) {
				pos += e->out_len;
				uint32_t nr[3];
				for (int k = 0; k < 3; k++) {
					const uint32_t v = e->rep_out[k];
					if (v >= ZB_SYM_MIN) {
						const uint32_t t = 0xFFFFFFFFu - v;
						const int64_t c = (int64_t)r[t >> 20] - (int64_t)(t & 0xFFFFFu);
						if (c <= 0) bad = true;	/* (a sequence of the block used it: the emit stage would say the same) */
						nr[k] = (uint32_t)c;
					} else nr[k] = v;
				}
				r[0] = nr[0]; r[1] = nr[1]; r[2] = nr[2];
			} else pos += e->hdr >> 3;
			if (pos > fr.dst_cap) bad = true;
		}
		if (F->has_fcs && pos != F->fcs) bad = true;
		F->total = (uint32_t)pos;
		if (bad) W.todo[i] = ZB_TODO_PLACE;
	}
}

/* ---- emit: one wave per block ---- */
__device__ __forceinline__ static uint32_t zb_wave_incl(uint32_t v, uint32_t lane)
{
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
		const uint32_t t = (uint32_t)__shfl_up((int)v, d, 64);
		if (lane >= (uint32_t)d) v += t;
	}
	return v;
}

#define ZB_SHORT 32u	/* literal runs and matches up to this many bytes are written by their own lane, longer ones by the wave */

__global__ __launch_bounds__(64) void zb_emit_kernel(const uint8_t *__restrict__ src, const la_zstd_frame *__restrict__ frames, uint32_t n,
    uint8_t *dst, zb_ws W)
{
	if (W.ctl[LA_CHAIN_CTL_WORDS]) return;
	const uint32_t lane = threadIdx.x;
	const uint64_t total = W.blk_start[n];
	for (uint64_t w = blockIdx.x; w < total; w += gridDim.x) {
		const uint32_t fi = zb_frame_of(W.blk_start, n, w);
		if (W.todo[fi]) continue;
		const la_zstd_frame fr = frames[fi];
		const zb_block e = zb_blocks_of(W.blk, fi, fr)[w - W.blk_start[fi]];
		const int type = (e.hdr >> 1) & 3;
		uint8_t *df = dst + fr.dst_off;		/* the frame's first byte */
		if (type == 0) { t_copy<true>(df + e.out_pos, src + fr.src_off + e.src, e.hdr >> 3); continue; }
		if (type == 1) { t_fill<true>(df + e.out_pos, src[fr.src_off + e.src], e.hdr >> 3); continue; }
		uint32_t *pf = W.ptr + fr.dst_off;	/* pointer of the frame's first byte; coordinates are places in d_dst */
		const uint32_t c0 = (uint32_t)fr.dst_off;
		const uint8_t *L = W.lit + fr.dst_off + e.lit_off;
		const zb_seq *S = W.seq + 16ull * fi + fr.dst_off / 3 + e.seq_off;
		uint32_t out = e.out_pos, lp = 0;
		bool bad = false;
		for (uint32_t base = 0; base < e.nseq; base += 64) {
			const bool have = base + lane < e.nseq;
			zb_seq q = { 0, 0, 1 };
			if (have) q = S[base + lane];
			if (q.off >= ZB_SYM_MIN) {	/* incoming repeat offset k less d */
				const uint32_t t = 0xFFFFFFFFu - q.off;
				const int64_t c = (int64_t)e.rep_in[t >> 20] - (int64_t)(t & 0xFFFFFu);
				q.off = c <= 0 ? 0u : (uint32_t)c;
			}
			const uint32_t ix = zb_wave_incl(q.ll + q.ml, lane), il = zb_wave_incl(q.ll, lane);
			const uint32_t my_out = out + ix - (q.ll + q.ml), my_lit = lp + il - q.ll, mpos = my_out + q.ll;
			if (have && (q.off == 0 || q.off > mpos)) { bad = true; q.ml = 0; }	/* offset 0, or a source in front of the frame's first byte */
			if (q.ll <= ZB_SHORT)
				for (uint32_t k = 0; k < q.ll; k++) df[my_out + k] = L[my_lit + k];
			if (q.ml <= ZB_SHORT) {
				/* an overlapping match names the `offset` bytes in front of it over and over: a long run is no long chain */
				uint32_t m = 0;
				for (uint32_t k = 0; k < q.ml; k++) { pf[mpos + k] = c0 + mpos - q.off + m; m = m + 1 == q.off ? 0 : m + 1; }
			}
			uint64_t big = __ballot(q.ll > ZB_SHORT || q.ml > ZB_SHORT);
			while (big) {
				const int j = __ffsll((unsigned long long)big) - 1;
				big &= big - 1;
				const uint32_t jl = (uint32_t)__shfl((int)q.ll, j, 64), jm = (uint32_t)__shfl((int)q.ml, j, 64), jo = (uint32_t)__shfl((int)q.off, j, 64);
				const uint32_t jout = (uint32_t)__shfl((int)my_out, j, 64), jlit = (uint32_t)__shfl((int)my_lit, j, 64);
				if (jl > ZB_SHORT)
					for (uint32_t k = lane; k < jl; k += 64) df[jout + k] = L[jlit + k];
				if (jm > ZB_SHORT) {
					const uint32_t mp = jout + jl, s0 = c0 + mp - jo;
					if (jo >= jm) for (uint32_t k = lane; k < jm; k += 64) pf[mp + k] = s0 + k;
					else for (uint32_t k = lane; k < jm; k += 64) pf[mp + k] = s0 + k % jo;
				}
			}
			out += (uint32_t)__shfl((int)ix, 63, 64);
			lp += (uint32_t)__shfl((int)il, 63, 64);
		}
		for (uint32_t k = lp + lane; k < e.regen; k += 64) df[out + (k - lp)] = L[k];	/* the literals behind the last sequence */
		if (__ballot(bad) != 0 && lane == 0) W.todo[fi] = ZB_TODO_EMIT;
	}
}

/* ---- verdict: one wave per frame ---- */
__global__ __launch_bounds__(64) void zb_verdict_kernel(const uint8_t *__restrict__ src, const la_zstd_frame *__restrict__ frames, uint32_t n,
    const uint8_t *dst, la_zstd_result *results, uint32_t options, zb_ws W)
{
	const bool disorder = W.ctl[LA_CHAIN_CTL_WORDS] != 0;
	for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
		if (disorder) { if (threadIdx.x == 0) W.todo[i] = ZB_TODO_ORDER; continue; }
		if (W.todo[i]) continue;
		const la_zstd_frame fr = frames[i];
		const zb_frame F = W.fr[i];
		bool ok = true;
		if (F.csum_at != ZB_NONE && !(options & LA_ZSTD_OPT_NO_VERIFY))
			ok = (uint32_t)wave_xxh64(dst + fr.dst_off, F.total, 0) == rd32(src + fr.src_off + F.csum_at);
		if (threadIdx.x == 0) {
			if (!ok) W.todo[i] = ZB_TODO_CHECKSUM;
			else { la_zstd_result r; r.status = LA_ST_OK; r.path = 1; r.out_len = F.total; results[i] = r; }
		}
	}
}

void la_launch_zstd_blocks(hipStream_t s, const uint8_t *d_src, uint64_t src_bytes, const la_zstd_frame *d_frames, uint32_t n,
    uint8_t *d_dst, uint64_t dst_cap, la_zstd_result *d_results, uint8_t *ws, uint32_t options)
{
	if (n == 0) return;
	zb_ws W;
	zb_carve(&W, ws, n, src_bytes, dst_cap);
	/* every byte a root until a match says otherwise */
	if (dst_cap) (void)hipMemsetAsync(W.ptr, 0xFF, dst_cap * sizeof(uint32_t), s);
	(void)hipMemsetAsync(W.ctl, 0, (LA_CHAIN_CTL_WORDS + 1) * sizeof(uint32_t), s);
	uint32_t lane_blocks = (n + 63u) / 64u;
	if (lane_blocks > ZB_MAX_INDEX_BLOCKS) lane_blocks = ZB_MAX_INDEX_BLOCKS;
	hipLaunchKernelGGL(zb_index_kernel, dim3(lane_blocks), dim3(64), 0, s, d_src, src_bytes, d_frames, n, dst_cap, W);
	la_launch_scan_u32(s, W.nblk, n, W.blk_start, W.scan);
	/* as many waves as there can be blocks, up to the cap: the kernels stride over the count the scan left */
	const uint64_t cap_blocks = 4ull * n + src_bytes / 16 + dst_cap / 65536;
	const uint32_t waves = cap_blocks < ZB_MAX_WAVES ? (uint32_t)cap_blocks : ZB_MAX_WAVES;
	hipLaunchKernelGGL(zb_entropy_kernel, dim3(waves), dim3(64), 0, s, d_src, d_frames, n, W);
	hipLaunchKernelGGL(zb_place_kernel, dim3(lane_blocks), dim3(64), 0, s, d_frames, n, W);
	hipLaunchKernelGGL(zb_emit_kernel, dim3(waves), dim3(64), 0, s, d_src, d_frames, n, d_dst, W);
	la_launch_chain_resolve_range(s, d_dst, W.ptr, (uint32_t)dst_cap, W.ctl);
	hipLaunchKernelGGL(zb_verdict_kernel, dim3(n < ZB_MAX_WAVES ? n : ZB_MAX_WAVES), dim3(64), 0, s, d_src, d_frames, n, d_dst, d_results,
	    options, W);
}
