/*
 * la_zstd_comp.hip -- Zstandard COMPRESSION + frame assembly on the device (gfx950): the data plane of the zstd write
 * filter (host/la_write_zstd.c).
 *
 * Replaces, for a whole stream per call, what libarchive/archive_write_add_filter_zstd.c gets from libzstd's
 * ZSTD_compressStream2 with ZSTD_c_checksumFlag set.  The bytes are not libzstd's (a zstd stream is not unique);
 * parity for this direction is the round trip -- libzstd, the oracle and this repository's device decoder must
 * return the input -- plus the format rules RFC 8878 sets on every frame and block.  Written from the RFC alone.
 *
 * Shape.  The input is cut into blocks of at most 128 KiB (Block_Maximum_Size); blocks_per_frame of them form one
 * frame with Single_Segment_Flag set and the Frame_Content_Size present, so the read walker reserves exact output
 * slots.  Blocks are compressed INDEPENDENTLY: no match reaches into an earlier block, the repeat-offset codes are
 * never used (every sequence writes Offset_Value = offset + 3), every block states its own tables.  So all blocks of
 * all frames run in parallel:
 *   zstd_compress_blocks_kernel   ONE WAVE per block.  A block whose bytes are all equal is an RLE_Block.  Otherwise
 *       the LZ77 matcher of lz4_compress_blocks_kernel (lz77_match, la_comp_common.h): 64 positions per step, a
 *       4096-entry table of 32-bit positions in LDS (16 KiB), 4-byte minimum match at any offset inside the block, matches verified and extended, taken
 *       in position order with ballot; literals and sequences (ll, ml, offset) go to the workspace.
 *       Literals section: RLE when all literals are one byte; Raw under LA_ZSTDC_RAW_LITERALS, for fewer than 32
 *       literals or, without LA_ZSTDC_FULL_ALPHABET, a largest byte above 128; otherwise Huffman: an LDS histogram, Shannon lengths clamped to 11 bits
 *       and made complete (Kraft sum exactly 1) by greedy lengthening / shortening with wave-wide arg-max rounds,
 *       direct 4-bit weights (zc_weight), one stream up to 1023 literals and four with the jump table above.  Streams are encoded
 *       in parallel: every literal's bit position is a wave prefix sum of code lengths (reverse symbol order, a
 *       Huffman stream is read backwards), lanes OR their bits into an LDS stage and whole dwords leave
 *       (wave_bits_append, shared with deflate_fixed_kernel).  Sections whose coded form would not be smaller are written raw.
 *       LA_ZSTDC_FULL_ALPHABET: any largest byte; the weights also go through zc_weights_fse (their histogram
 *       normalised a lane per weight, two interleaved FSE states, written backwards by the serial bit writer zc_bw) and the
 *       smaller allowed description is written; weights that are all equal have no FSE form (raw above 128 of them).
 *       Sequences section (zc_sequences_predefined): Predefined_Mode for LL, OF and ML, with encoder tables (symbol x
 *       next state -> state, zc_enc_predefined) spread from the decoder's own fse_build in LDS; the interleaved FSE
 *       stream is written last sequence first, uniformly by the wave (zc_seq_chain, the one chain of both table
 *       forms: 64 sequences' codes and extra bits computed lane-parallel, then taken one by one with v_readlane).
 *       LA_ZSTDC_FIT_TABLES (zc_sequences_fit): LDS histograms of the three codes, per field
 *       RLE_Mode for a single code, FSE_Compressed_Mode when counts normalised from the histogram (accuracy log from
 *       the sequence count, 5 .. 9, 8 for offsets) are estimated cheaper than the predefined table by more than a
 *       byte, Predefined_Mode otherwise, never Repeat_Mode; the same chain then runs on compact encoder tables (the
 *       states of every symbol in next-state order, zc_fse_step, zc_enc_fitted) with every field's own accuracy log.
 *       Flags without the two run the kernel's <false> instance, which holds none of this: the code and the bytes
 *       they had.
 *       A block whose compressed form is not smaller than its input is a Raw_Block.
 *   frame_sums_kernel             XXH64 of every frame's input (la_comp_common.h), four lanes per frame.
 *   zstdc_sizes_kernel / scan     stream bytes of every block (header + payload, frame header and checksum).
 *   zstd_pack_frames_kernel       one workgroup per block: frame header, block header, payload, checksum.
 * LDS per wave: 16 KiB table (the FSE tables of either form and the weight tables reuse it after matching: 11 KiB
 * at most) + 1.9 KiB histogram / code / stage: 8 waves per CU by LDS.
 */
#include "la_comp_common.h"
#include "la_zstd_common.h"

#define ZC_MINMATCH  4u
#define ZC_BLOCK_MAX 131072u
#define ZC_RAW_LIT_MIN 32u	/* fewer literals than this are never worth a Huffman table */

__host__ __device__ static inline uint64_t zc_tmp_stride(uint32_t bs) { return ((uint64_t)bs + 64u + 15u) & ~15ull; }
__host__ __device__ static inline uint64_t zc_lit_stride(uint32_t bs) { return ((uint64_t)bs + 15u) & ~15ull; }
__host__ __device__ static inline uint64_t zc_seq_stride(uint32_t bs) { return ((uint64_t)bs / ZC_MINMATCH + 1u) * 8u; }

struct zc_fse_lds {
	fse_tab ll, ml, of;		/* decoder tables of the predefined distributions (fse_build: the decoder's spread) */
	uint8_t ell[36 * 64];		/* encoder: [symbol][next state] -> state whose range holds it */
	uint8_t eml[53 * 64];
	uint8_t eof[29 * 32];
};
/* LA_ZSTDC_FIT_TABLES: per-block tables.  Field 0 = LL, 1 = OF, 2 = ML (the order of the descriptions in the block).
 * The encoder is compact: st lists the states of every symbol in ascending order (symbol s from start(s) on),
 * sinfo[s] = count | start << 16; a symbol of normalised count c owns the next-state values c .. 2c - 1 in that
 * order (the decoder's spread, fse_build), so the state that leads to next state t is found by arithmetic. */
struct zc_fit_lds {
	fse_tab t[3];			/* decoder form, built by the decoder's own fse_build */
	uint16_t st[3][512];
	uint32_t sinfo[3][64];
	uint32_t hist[3][64];
	int16_t norm[3][64];
};
/* LA_ZSTDC_FULL_ALPHABET: the FSE form of the Huffman tree description (weights 0..11, accuracy log 5 or 6) */
struct zc_wfse_lds {
	fse_tab t;
	uint16_t st[64];
	uint32_t sinfo[16];
	int16_t norm[16];
	uint8_t tree[136];		/* normalised counts + weight stream: usable below 128 bytes */
};
struct zc_lds {
	union {
		uint32_t tab[1u << LZ77_HASH_BITS];
		zc_fse_lds f;
		zc_fit_lds fit;
		zc_wfse_lds wf;
	} u;
	uint32_t hist[256];
	uint16_t code[256];
	uint8_t len[256];
	uint32_t wcnt[16];
	uint32_t stage[32];
};
static_assert(sizeof(zc_fse_lds) <= sizeof(uint32_t) * (1u << LZ77_HASH_BITS), "FSE tables must fit in the match table");
static_assert(sizeof(zc_fit_lds) <= sizeof(uint32_t) * (1u << LZ77_HASH_BITS), "fitted tables must fit in the match table");
static_assert(sizeof(zc_wfse_lds) <= sizeof(uint32_t) * (1u << LZ77_HASH_BITS), "weight tables must fit in the match table");
static_assert(sizeof(zc_lds) <= 20u * 1024u, "8 waves per CU by LDS");

/* literal-length / match-length codes (RFC 8878 3.1.1.3.2.1.1) */
__device__ __forceinline__ uint32_t ll_code(uint32_t ll)
{
	if (ll < 16u) return ll;
	if (ll >= 64u) return (uint32_t)highbit(ll) + 19u;
	uint32_t c = 16;
	while (c < 24u && SEQ_TABS.ll_base[c + 1] <= ll) c++;
	return c;
}
__device__ __forceinline__ uint32_t ml_code(uint32_t ml)
{
	if (ml < 35u) return ml - 3u;
	if (ml >= 131u) return (uint32_t)highbit(ml - 3u) + 36u;
	uint32_t c = 32;
	while (c < 42u && SEQ_TABS.ml_base[c + 1] <= ml) c++;
	return c;
}

/* Huffman weight of a symbol whose code is len bits long in a tree whose longest code is lmax (RFC 8878 4.2.1) */
__device__ __forceinline__ uint32_t zc_weight(uint32_t len, uint32_t lmax) { return len ? lmax + 1u - len : 0u; }

/* literals section header for Raw (type 0) / RLE (type 1): 1, 2 or 3 bytes */
__device__ __forceinline__ uint32_t lit_hdr_rr(uint8_t *o, uint32_t type, uint32_t regen, bool write)
{
	if (regen < 32u) {
		if (write) o[0] = (uint8_t)(type | (regen << 3));
		return 1;
	}
	if (regen < 4096u) {
		const uint32_t v = type | (1u << 2) | (regen << 4);
		if (write) { o[0] = (uint8_t)v; o[1] = (uint8_t)(v >> 8); }
		return 2;
	}
	const uint32_t v = type | (3u << 2) | (regen << 4);
	if (write) { o[0] = (uint8_t)v; o[1] = (uint8_t)(v >> 8); o[2] = (uint8_t)(v >> 16); }
	return 3;
}

/* one Huffman stream of literals [a, b): written last literal first, then the end-mark bit; returns its bytes */
__device__ static uint32_t huf_stream_enc(zc_lds &L, const uint8_t *lits, uint32_t a, uint32_t b, uint8_t *out, uint32_t lane)
{
	uint64_t bp = 0;
	for (uint32_t i = lane; i < 32; i += 64)
		L.stage[i] = 0;
	__builtin_amdgcn_wave_barrier();
	uint32_t e = b;
	while (e > a) {
		const uint32_t cnt = e - a < 64u ? e - a : 64u;
		uint32_t nb = 0, bits = 0;
		if (lane < cnt) {
			const uint32_t s = lits[e - 1u - lane];
			nb = L.len[s];
			bits = L.code[s];
		}
		/* whole dwords leave (64 x 11 + 31 bits: at most 22 of them), four bytes each: the destination is not aligned */
		bp += wave_bits_append(bp, bits, nb, L.stage, lane, [&](uint32_t i, uint32_t w) { st_le32(out + 4u * i, w); });
		e -= cnt;
	}
	/* end mark, then the last bytes */
	const uint32_t last = L.stage[0] | (1u << (bp & 31u));
	bp += 1;
	const uint32_t bytes = (uint32_t)((bp + 7u) >> 3);
	const uint32_t g0 = (uint32_t)(bp - 1u) >> 5;
	if (lane < bytes - 4u * g0)
		out[4u * g0 + lane] = (uint8_t)(last >> (8u * lane));
	__builtin_amdgcn_wave_barrier();
	return bytes;
}

/* serial LSB-first bit writer (wave-uniform state; lane 0 stores) */
struct zc_bw {
	uint8_t *out;
	uint32_t op, cap;
	uint64_t acc;
	uint32_t n;
	bool over;
};
/* an empty writer that continues out at byte op and stores nothing at or past cap */
__device__ __forceinline__ zc_bw bw_open(uint8_t *out, uint32_t op, uint32_t cap)
{
	zc_bw w;
	w.out = out; w.op = op; w.cap = cap; w.acc = 0; w.n = 0; w.over = false;
	return w;
}
__device__ __forceinline__ void bw_put(zc_bw &w, uint32_t v, uint32_t nb, uint32_t lane)
{
	w.acc |= (uint64_t)v << w.n;
	w.n += nb;
	if (w.n >= 32u) {
		if (w.op + 4u > w.cap) {
			w.over = true;
		} else if (lane == 0) {
			st_le32(w.out + w.op, (uint32_t)w.acc);
		}
		w.op += 4u;
		w.acc >>= 32;
		w.n -= 32u;
	}
}

/* the bytes still in the accumulator leave (the stream is byte-aligned afterwards); returns the stream's end */
__device__ __forceinline__ uint32_t bw_close(zc_bw &w, uint32_t lane)
{
	const uint32_t tail = (w.n + 7u) >> 3;
	if (w.op + tail > w.cap) {
		w.over = true;
	} else if (lane == 0) {
		for (uint32_t k = 0; k < tail; k++)
			w.out[w.op + k] = (uint8_t)(w.acc >> (8u * k));
	}
	w.op += tail;
	w.acc = 0;
	w.n = 0;
	return w.op;
}

/* the one prefix sum written out in this file (wave_bits_append, la_comp_common.h, carries its own) */
__device__ __forceinline__ uint32_t wave_excl_sum(uint32_t v, uint32_t lane)
{
	uint32_t inc = v;
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
		const uint32_t t = __shfl_up(inc, d, 64);
		if ((int)lane >= d) inc += t;
	}
	return inc - v;
}

/* ---- FSE tables fitted to a histogram (LA_ZSTDC_FULL_ALPHABET: the Huffman weights; LA_ZSTDC_FIT_TABLES: the
 * sequence codes), a lane per symbol ---- */

/* normalised counts: floor(h * 2^al / total), 1 for a present symbol that would get less, and the difference to 2^al
 * on the most frequent symbol (the lowest of equals).  False when that symbol would be left below 1.  At most
 * 2^15 * 2^9: 32-bit arithmetic. */
__device__ __forceinline__ bool zc_normalize(uint32_t h, uint32_t total, uint32_t al, uint32_t lane, uint32_t &norm)
{
	uint32_t c = 0;
	if (h) {
		c = (h << al) / total;
		c = c ? c : 1u;
	}
	const uint32_t sum = wave_sum(c);
	const uint32_t big = 63u - (wave_max(h ? (h << 6) | (63u - lane) : 0u) & 63u);
	const int32_t fixed = (int32_t)c + (int32_t)(1u << al) - (int32_t)sum;
	if (lane == big)
		c = fixed < 1 ? 0u : (uint32_t)fixed;
	norm = c;
	return __ballot(lane == big && fixed < 1) == 0;
}

/* cost of one symbol of normalised count c in a table of 2^al states, in 1/256 bit */
__device__ __forceinline__ uint32_t zc_bits256(uint32_t al, uint32_t c)
{
	return (uint32_t)(((float)al - __log2f((float)c)) * 256.0f + 0.5f);
}

/* normalised counts in the layout fse_read_ncount reads (RFC 8878 4.1.1): accuracy log, then count + 1 per symbol in
 * as many bits as what remains allows, a zero count followed by 2-bit repeat flags; the symbols behind the one that
 * completes the sum are not written.  Wave-uniform; every count is 0 or positive ("less than one" is not used). */
__device__ static void zc_put_ncount(zc_bw &w, const int16_t *norm, uint32_t n_sym, uint32_t al, uint32_t lane)
{
	bw_put(w, al - 5u, 4, lane);
	uint32_t remaining = (1u << al) + 1u, threshold = 1u << al, nbits = al + 1u, s = 0;
	while (remaining > 1u && s < n_sym) {
		const uint32_t c = (uint32_t)norm[s], mx = 2u * threshold - 1u - remaining, v = c + 1u;
		if (v < mx)
			bw_put(w, v, nbits - 1u, lane);
		else if (v < threshold)
			bw_put(w, v, nbits, lane);
		else
			bw_put(w, v + mx, nbits, lane);
		remaining -= c;
		s++;
		if (c == 0) {
			uint32_t z = 0;
			while (s + z < n_sym && norm[s + z] == 0) z++;
			s += z;
			for (; z >= 3u; z -= 3u)
				bw_put(w, 3, 2, lane);
			bw_put(w, z, 2, lane);
		}
		while (remaining < threshold) { nbits--; threshold >>= 1; }
	}
}

/* compact encoder table from the decoder's: state u, whose range starts at base and is 2^nbits wide, owns the
 * next-state value (base + size) >> nbits of its symbol; the symbol's states go into st in that order */
__device__ __forceinline__ void zc_enc_table(const fse_tab *t, uint32_t al, const uint32_t *sinfo, uint16_t *st, uint32_t lane)
{
	const uint32_t size = 1u << al;
	for (uint32_t u = lane; u < size; u += 64) {
		const fse_ent e = t->e[u];
		const uint32_t w = sinfo[e.sym];
		st[(w >> 16) + ((e.base + size) >> e.nbits) - (w & 0xFFFFu)] = (uint16_t)u;
	}
}

/* one encoder step: the state of symbol `sym` whose range holds the next state t, and the bits that select t in it.
 * A symbol of count c has next-state values c .. 2c - 1; t + size shifted by the symbol's larger bit count lands on
 * one of them or, below c, belongs to a state with one bit less.  (A one-state table, al = 0, gives no bits.) */
__device__ __forceinline__ uint32_t zc_fse_step(const uint16_t *st, const uint32_t *sinfo, uint32_t al, uint32_t sym,
    uint32_t t, uint32_t &bits, uint32_t &nb)
{
	const uint32_t w = sinfo[sym], c = w & 0xFFFFu, v = t + (1u << al);
	uint32_t n = al - (31u - (uint32_t)__clz((int)c));
	uint32_t nx = v >> n;
	if (nx < c) {
		n--;
		nx = v >> n;
	}
	nb = n;
	bits = v & ((1u << n) - 1u);
	return st[(w >> 16) + nx - c];
}
/* a state of `sym` to end on: the one with the most update bits */
__device__ __forceinline__ uint32_t zc_fse_first(const uint16_t *st, const uint32_t *sinfo, uint32_t sym)
{
	return st[sinfo[sym] >> 16];
}

/* The FSE form of the Huffman tree description (RFC 8878 4.2.1.1) for the weights of symbols 0 .. nw - 1 (nw >= 2),
 * into L.u.wf.tree: normalised counts of the weights, then the weights through two interleaved states (the first
 * decodes the even positions), written backwards with an end mark.  The stream carries no count: the decoder stops
 * when a state update runs out of bits, so the state it ends on must need a bit -- each chain ends on its symbol's
 * state with the most bits, which is none only when all weights are equal.  Returns the bytes (below 128), or 0 when
 * this form cannot be used. */
__device__ static uint32_t zc_weights_fse(zc_lds &L, uint32_t nw, uint32_t lmax, uint32_t lane)
{
	zc_wfse_lds &F = L.u.wf;
	if (lane < 16)
		L.wcnt[lane] = 0;
	__syncthreads();
	for (uint32_t s = lane; s < nw; s += 64)
		atomicAdd(&L.wcnt[zc_weight(L.len[s], lmax)], 1u);
	__syncthreads();
	const uint32_t h = lane < 16 ? L.wcnt[lane] : 0u;
	const uint64_t present = __ballot(h != 0);
	if (__popcll(present) < 2)
		return 0;
	const uint32_t n_sym = 64u - (uint32_t)__clzll((long long)present);
	const uint32_t al = nw > 64u ? 6u : 5u;
	uint32_t c;
	if (!zc_normalize(h, nw, al, lane, c))
		return 0;
	const uint32_t start = wave_excl_sum(c, lane);
	if (lane < 16) {
		F.norm[lane] = (int16_t)c;
		F.sinfo[lane] = c | (start << 16);
	}
	__syncthreads();
	if (lane == 0)
		fse_build(&F.t, F.norm, (int)n_sym, (int)al);
	__syncthreads();
	zc_enc_table(&F.t, al, F.sinfo, F.st, lane);
	__syncthreads();
	zc_bw w = bw_open(F.tree, 0, 132);
	zc_put_ncount(w, F.norm, n_sym, al, lane);
	bw_close(w, lane);
	auto weight = [&](uint32_t s) { return zc_weight(L.len[s], lmax); };
	/* s0 / s1: the state of the even / odd chain at the position reached so far, from the end */
	uint32_t s0 = zc_fse_first(F.st, F.sinfo, weight(nw - 1u)), s1 = zc_fse_first(F.st, F.sinfo, weight(nw - 2u));
	if (!(nw & 1u)) {	/* the last weight stands at an odd position */
		const uint32_t t = s0; s0 = s1; s1 = t;
	}
	for (uint32_t i = nw - 2u; i-- > 0;) {
		uint32_t bits, nb;
		const uint32_t u = zc_fse_step(F.st, F.sinfo, al, weight(i), (i & 1u) ? s1 : s0, bits, nb);
		bw_put(w, bits, nb, lane);
		if (i & 1u) s1 = u; else s0 = u;
	}
	bw_put(w, s1, al, lane);	/* the decoder reads the even chain's state first: it is written last */
	bw_put(w, s0, al, lane);
	bw_put(w, 1, 1, lane);		/* end mark */
	const uint32_t end = bw_close(w, lane);
	__syncthreads();
	return (w.over || end >= 128u) ? 0u : end;
}

/* ---- the sequence chain over either form of encoder table.  An Enc answers, for field 0 = LL, 1 = OF, 2 = ML (a
 * literal constant at every call): al(field), the accuracy log; first(field, sym), a state of sym for the block's last
 * sequence; step(field, sym, t, bits, nb), the state of sym whose range holds next state t and the bits selecting t ---- */
/* the predefined tables: [symbol][next state] bytes beside the decoder's entries */
struct zc_enc_predefined {
	const zc_fse_lds *f;
	__device__ __forceinline__ const uint8_t *enc(uint32_t field) const { return field == 0 ? f->ell : field == 1 ? f->eof : f->eml; }
	__device__ __forceinline__ const fse_tab &dec(uint32_t field) const { return field == 0 ? f->ll : field == 1 ? f->of : f->ml; }
	__device__ __forceinline__ uint32_t al(uint32_t field) const { return field == 1 ? 5u : 6u; }
	__device__ __forceinline__ uint32_t first(uint32_t field, uint32_t sym) const { return enc(field)[sym << al(field)]; }
	__device__ __forceinline__ uint32_t step(uint32_t field, uint32_t sym, uint32_t t, uint32_t &bits, uint32_t &nb) const
	{
		const uint32_t u = enc(field)[(sym << al(field)) + t];
		const fse_ent e = dec(field).e[u];
		bits = t - e.base; nb = e.nbits;
		return u;
	}
};
/* tables fitted to the block: the compact encoder, every field with its own accuracy log (als: a byte each) */
struct zc_enc_fitted {
	const zc_fit_lds *f;
	uint32_t als;
	__device__ __forceinline__ uint32_t al(uint32_t field) const { return (als >> (8u * field)) & 255u; }
	__device__ __forceinline__ uint32_t first(uint32_t field, uint32_t sym) const { return zc_fse_first(f->st[field], f->sinfo[field], sym); }
	__device__ __forceinline__ uint32_t step(uint32_t field, uint32_t sym, uint32_t t, uint32_t &bits, uint32_t &nb) const
	{ return zc_fse_step(f->st[field], f->sinfo[field], al(field), sym, t, bits, nb); }
};

/* The interleaved FSE stream of a block's sequences: last sequence first, 64 at a time (lane j prepares sequence
 * hi - 1 - j), then the initial states and the end mark.  The caller closes the writer. */
template <typename Enc>
__device__ __forceinline__ void zc_seq_chain(zc_bw &w, const Enc enc, const uint64_t *seqs, uint32_t nseq, uint32_t lane)
{
	uint32_t sl = 0, sm = 0, sof = 0;
	for (uint32_t hi = nseq; hi > 0;) {
		const uint32_t cnt = hi < 64u ? hi : 64u;
		uint32_t codes = 0, lmx = 0, lmbits = 0, ov = 0;
		if (lane < cnt) {
			const uint64_t s = seqs[hi - 1u - lane];
			const uint32_t ll = (uint32_t)(s & 0xFFFFFu), ml = (uint32_t)((s >> 20) & 0xFFFFFu), off = (uint32_t)(s >> 40);
			const uint32_t lc = ll_code(ll), mc = ml_code(ml);
			ov = off + 3u;
			const uint32_t oc = (uint32_t)highbit(ov);
			codes = lc | (mc << 8) | (oc << 16);
			lmx = (ll - SEQ_TABS.ll_base[lc]) | ((ml - SEQ_TABS.ml_base[mc]) << 16);
			lmbits = SEQ_TABS.ll_bits[lc] | ((uint32_t)SEQ_TABS.ml_bits[mc] << 8);
			ov -= 1u << oc;
		}
		for (uint32_t j = 0; j < cnt; j++) {
			const uint32_t c = (uint32_t)__builtin_amdgcn_readlane((int)codes, (int)j);
			const uint32_t x = (uint32_t)__builtin_amdgcn_readlane((int)lmx, (int)j);
			const uint32_t b = (uint32_t)__builtin_amdgcn_readlane((int)lmbits, (int)j);
			const uint32_t ox = (uint32_t)__builtin_amdgcn_readlane((int)ov, (int)j);
			const uint32_t lc = c & 255u, mc = (c >> 8) & 255u, oc = c >> 16;
			if (hi == nseq && j == 0) {
				/* the block's last sequence: any state of its symbols */
				sl = enc.first(0, lc);
				sof = enc.first(1, oc);
				sm = enc.first(2, mc);
			} else {
				/* state of this sequence whose range holds the next one's state; the bits select it */
				uint32_t bo, no, bm, nm, bl, nl;
				sof = enc.step(1, oc, sof, bo, no);
				sm = enc.step(2, mc, sm, bm, nm);
				sl = enc.step(0, lc, sl, bl, nl);
				bw_put(w, bo, no, lane);
				bw_put(w, bm, nm, lane);
				bw_put(w, bl, nl, lane);
			}
			/* extra bits: the decoder reads offset, match length, literal length */
			bw_put(w, x & 0xFFFFu, b & 255u, lane);
			bw_put(w, x >> 16, b >> 8, lane);
			bw_put(w, ox, oc, lane);
		}
		hi -= cnt;
	}
	/* initial states, each as wide as its table's accuracy log: the decoder reads LL, OF, ML */
	bw_put(w, sm, enc.al(2), lane);
	bw_put(w, sof, enc.al(1), lane);
	bw_put(w, sl, enc.al(0), lane);
	bw_put(w, 1, 1, lane);	/* end mark */
}

/* The sequences section with Predefined_Mode for LL, OF and ML: the decoder's tables, the encoder bytes spread from
 * them (for every state u, the next states its range covers lead back to u), the chain.  Returns as zc_sequences_fit. */
__device__ __forceinline__ uint32_t zc_sequences_predefined(zc_fse_lds &F, const uint64_t *seqs, uint32_t nseq, uint8_t *out,
    uint32_t op, uint32_t cap, uint32_t lane, bool &over)
{
	if (lane == 0) {
		out[op] = 0;	/* Symbol_Compression_Modes */
		fse_build(&F.ll, LL_DEF, 36, 6);
		fse_build(&F.ml, ML_DEF, 53, 6);
		fse_build(&F.of, OF_DEF, 29, 5);
	}
	__syncthreads();
	const fse_ent e = F.ll.e[lane];
	for (uint32_t t = 0; t < (1u << e.nbits); t++) F.ell[e.sym * 64u + e.base + t] = (uint8_t)lane;
	const fse_ent m = F.ml.e[lane];
	for (uint32_t t = 0; t < (1u << m.nbits); t++) F.eml[m.sym * 64u + m.base + t] = (uint8_t)lane;
	if (lane < 32) {
		const fse_ent o = F.of.e[lane];
		for (uint32_t t = 0; t < (1u << o.nbits); t++) F.eof[o.sym * 32u + o.base + t] = (uint8_t)lane;
	}
	__syncthreads();
	zc_bw w = bw_open(out, op + 1u, cap);
	zc_seq_chain(w, zc_enc_predefined{ &F }, seqs, nseq, lane);
	const uint32_t end = bw_close(w, lane);
	over = w.over;
	return end;
}

/* The sequences section behind Number_of_Sequences under LA_ZSTDC_FIT_TABLES (RFC 8878 3.1.1.3.2.1): the block's
 * histograms of LL, OF and ML codes, a mode per field -- RLE_Mode when one code is all there is, FSE_Compressed_Mode
 * when a table normalised from the histogram is estimated cheaper (description + sum of count * log2(size / norm))
 * than the predefined one by more than a byte, Predefined_Mode otherwise -- then the interleaved stream with every
 * field's own table and accuracy log.  Returns the section's end; over: it did not fit cap. */
__device__ static uint32_t zc_sequences_fit(zc_lds &L, const uint64_t *seqs, uint32_t nseq, uint8_t *out, uint32_t op,
    uint32_t cap, uint32_t lane, bool &over)
{
	zc_fit_lds &F = L.u.fit;
	for (uint32_t f = 0; f < 3; f++)
		F.hist[f][lane] = 0;
	__syncthreads();
	for (uint32_t i = lane; i < nseq; i += 64) {
		const uint64_t s = seqs[i];
		atomicAdd(&F.hist[0][ll_code((uint32_t)(s & 0xFFFFFu))], 1u);
		atomicAdd(&F.hist[1][(uint32_t)highbit((uint32_t)(s >> 40) + 3u)], 1u);
		atomicAdd(&F.hist[2][ml_code((uint32_t)((s >> 20) & 0xFFFFFu))], 1u);
	}
	__syncthreads();
	zc_bw w = bw_open(out, op + 1u, cap);
	uint32_t modes = 0, als = 0;	/* als: the three accuracy logs, a byte each */
	bool stuck = false;
	for (uint32_t f = 0; f < 3; f++) {
		const int16_t *def = f == 0 ? LL_DEF : f == 1 ? OF_DEF : ML_DEF;
		const uint32_t def_n = f == 0 ? 36u : f == 1 ? 29u : 53u, def_al = f == 1 ? 5u : 6u, max_al = f == 1 ? 8u : 9u;
		const uint32_t h = F.hist[f][lane];
		const uint64_t present = __ballot(h != 0);
		const uint32_t np = (uint32_t)__popcll(present), n_sym = 64u - (uint32_t)__clzll((long long)present);
		const int32_t d = lane < def_n ? def[lane] : 0;
		const uint32_t dc = d < 0 ? 1u : (uint32_t)d;
		const bool def_ok = __ballot(h != 0 && dc == 0) == 0;	/* the predefined table knows every code used */
		const uint32_t cost_def = wave_sum(h && dc ? h * zc_bits256(def_al, dc) : 0u);
		uint32_t mode = 0, al = def_al, c = dc;
		int32_t nv = d;		/* the counts fse_build gets */
		if (np == 1u) {
			if (!def_ok || 8u * 256u < cost_def) {
				mode = 1; al = 0; c = h ? 1u : 0u;
				if (w.op + 1u > cap) w.over = true;
				else if (lane == 0) out[w.op] = (uint8_t)(n_sym - 1u);
				w.op += 1u;
			}
		} else {
			/* accuracy log: two bits below the sequence count's, enough states for every code present */
			uint32_t a = (uint32_t)highbit(nseq - 1u);
			a = a > 2u ? a - 2u : 0u;
			const uint32_t need = (uint32_t)highbit(np - 1u) + 1u;
			a = a < need ? need : a;
			a = a < 5u ? 5u : (a > max_al ? max_al : a);
			uint32_t nc;
			const bool fits = zc_normalize(h, nseq, a, lane, nc);
			if (fits) {
				F.norm[f][lane] = (int16_t)nc;
				__syncthreads();
				zc_bw t = w;	/* written where it would stand; kept only if this mode is chosen */
				zc_put_ncount(t, F.norm[f], n_sym, a, lane);
				bw_close(t, lane);
				const uint32_t cost_fit = wave_sum(h ? h * zc_bits256(a, nc) : 0u) + (t.op - w.op) * 8u * 256u;
				if (!def_ok || cost_fit + 8u * 256u < cost_def) {
					mode = 2; al = a; c = nc; nv = (int32_t)nc;
					w = t;
				}
			}
			stuck |= !def_ok && mode == 0;
		}
		__syncthreads();
		F.norm[f][lane] = (int16_t)nv;
		F.sinfo[f][lane] = c | (wave_excl_sum(c, lane) << 16);
		modes |= mode << (6u - 2u * f);
		als |= al << (8u * f);
	}
	if (lane == 0)
		out[op] = (uint8_t)modes;	/* Symbol_Compression_Modes; Repeat_Mode never: blocks are independent */
	__syncthreads();
	if (lane < 3u) {
		if (((modes >> (6u - 2u * lane)) & 3u) == 1u)
			F.st[lane][0] = 0;
		else
			fse_build(&F.t[lane], F.norm[lane], 64, (int)((als >> (8u * lane)) & 255u));
	}
	__syncthreads();
	const zc_enc_fitted enc = { &F, als };
	for (uint32_t f = 0; f < 3; f++)
		if (((modes >> (6u - 2u * f)) & 3u) != 1u)
			zc_enc_table(&F.t[f], enc.al(f), F.sinfo[f], F.st[f], lane);
	__syncthreads();
	zc_seq_chain(w, enc, seqs, nseq, lane);
	const uint32_t end = bw_close(w, lane);
	over = w.over || stuck;
	return end;
}

/* ENTROPY: the instance for flags with LA_ZSTDC_FULL_ALPHABET or LA_ZSTDC_FIT_TABLES.  The other instance holds none
 * of their code, so the flags from before them run the kernel they always ran.  The body up to the sequences section
 * is one piece on purpose: with the matcher or the literals section as functions, inlined or called, and even with only
 * the small steps around them moved out, it measured 0.4 .. 2 % slower (profiles/r16_zstd_comp_refactor.txt). */
template <bool ENTROPY>
__global__ __launch_bounds__(64) void zstd_compress_blocks_kernel(const uint8_t *__restrict__ src, uint64_t src_bytes,
    uint32_t block_size, uint32_t n_blocks, uint32_t flags, uint8_t *__restrict__ tmp, uint8_t *__restrict__ lits_ws,
    uint64_t *__restrict__ seqs_ws, uint32_t *__restrict__ btype, uint32_t *__restrict__ csize)
{
	__shared__ zc_lds L;
	const uint32_t bi = blockIdx.x, lane = threadIdx.x;
	if (bi >= n_blocks)
		return;
	const uint64_t so = (uint64_t)bi * block_size;
	const uint32_t n = src_bytes > so ? (uint32_t)(src_bytes - so < block_size ? src_bytes - so : block_size) : 0u;
	const uint8_t *in = src + so;
	uint8_t *out = tmp + (uint64_t)bi * zc_tmp_stride(block_size);
	uint8_t *lits = lits_ws + (uint64_t)bi * zc_lit_stride(block_size);
	uint64_t *seqs = (uint64_t *)(void *)((uint8_t *)seqs_ws + (uint64_t)bi * zc_seq_stride(block_size));
	const uint32_t cap = (uint32_t)zc_tmp_stride(block_size);

	/* ---- RLE_Block: every byte equal ---- */
	if (n == 0) {
		if (lane == 0) { btype[bi] = 0; csize[bi] = 0; }
		return;
	}
	{
		const uint8_t b0 = in[0];
		bool same = true;
		for (uint32_t base = 0; base < n && same; base += 64 * 16) {
			bool diff = false;
			for (uint32_t k = 0; k < 16; k++) {
				const uint32_t i = base + k * 64 + lane;
				diff |= i < n && in[i] != b0;
			}
			same = __ballot(diff) == 0;
		}
		if (same && n > 1) {
			if (lane == 0) { btype[bi] = 1; csize[bi] = 1; }
			return;
		}
	}

	for (uint32_t i = lane; i < (1u << LZ77_HASH_BITS); i += 64)
		L.u.tab[i] = 0;
	for (uint32_t i = lane; i < 256; i += 64)
		L.hist[i] = 0;
	__syncthreads();

	/* ---- matching: sequences and literals ---- */
	uint32_t anchor = 0, nseq = 0, nlit = 0;	/* wave-uniform */
	if (n >= ZC_MINMATCH) {
		/* matches start at or before n - 4 and may run to the block's end */
		anchor = lz77_match(L.u.tab, in, n - ZC_MINMATCH, n, lane, [&](uint32_t pf, uint32_t mf, uint32_t cf, uint32_t anchor) {
			const uint32_t lit = pf - anchor;
			wave_copy(lits + nlit, in + anchor, lit, lane);
			if (lane == 0)
				seqs[nseq] = (uint64_t)lit | ((uint64_t)mf << 20) | ((uint64_t)(pf - cf) << 40);
			nlit += lit;
			nseq++;
		});
	}
	wave_copy(lits + nlit, in + anchor, n - anchor, lane);
	nlit += n - anchor;
	__syncthreads();	/* literals and sequences are in the workspace */

	/* ---- literals section ---- */
	for (uint32_t i = lane; i < nlit; i += 64)
		atomicAdd(&L.hist[lits[i]], 1u);
	__syncthreads();
	uint32_t maxsym = 0, nsym = 0;
	for (uint32_t s = lane; s < 256; s += 64)
		if (L.hist[s]) { maxsym = s; nsym++; }
	maxsym = wave_max(maxsym);
	nsym = wave_sum(nsym);
	uint32_t op = 0;	/* bytes of the block written so far */
	bool lit_done = false;
	if (nlit > 0 && nsym == 1) {	/* RLE_Literals_Block */
		op = lit_hdr_rr(out, 1, nlit, lane == 0);
		if (lane == 0) out[op] = lits[0];
		op += 1;
		lit_done = true;
	} else if (!(flags & LA_ZSTDC_RAW_LITERALS) && nlit >= ZC_RAW_LIT_MIN && (maxsym <= 128u || (ENTROPY && (flags & LA_ZSTDC_FULL_ALPHABET)))) {
		/* code lengths: Shannon lengths ceil(log2(nlit / f)) clamped to [1, 11], then made complete.
		 * K = sum of 2^(11 - len) over the used symbols; complete means K == 2048. */
		uint32_t Ls[4];
		uint32_t K = 0;
#pragma unroll
		for (int k = 0; k < 4; k++) {
			const uint32_t f = L.hist[lane + 64 * k];
			uint32_t l = 0;
			if (f) {
				while (((uint64_t)f << l) < nlit) l++;
				l = l < 1u ? 1u : (l > 11u ? 11u : l);
				K += 1u << (11u - l);
			}
			Ls[k] = l;
		}
		K = wave_sum(K);
		/* too long a code after clamping: lengthen the rarest symbol that can still grow */
		for (uint32_t it = 0; it < 4096u && K > 2048u; it++) {
			uint32_t key = 0;
#pragma unroll
			for (int k = 0; k < 4; k++) {
				const uint32_t s = lane + 64 * k, f = L.hist[s];
				if (f && Ls[k] < 11u) {
					const uint32_t c = ((0x3FFFFu - f) << 8) | s;
					key = c > key ? c : key;
				}
			}
			key = wave_max(key);
			if (key == 0)
				break;
			const uint32_t s = key & 255u;
			if ((s & 63u) == lane) {
				K -= 1u << (10u - Ls[s >> 6]);
				Ls[s >> 6]++;
			}
			K = (uint32_t)__shfl((int)K, (int)(s & 63u), 64);
		}
		/* room left: shorten the most frequent symbol whose code can shrink without overflowing */
		for (uint32_t it = 0; it < 4096u && K < 2048u; it++) {
			const uint32_t room = 2048u - K;
			uint32_t key = 0;
#pragma unroll
			for (int k = 0; k < 4; k++) {
				const uint32_t s = lane + 64 * k, f = L.hist[s];
				if (f && Ls[k] > 1u && (1u << (11u - Ls[k])) <= room) {
					const uint32_t c = (f << 8) | s | 0x80000000u;
					key = c > key ? c : key;
				}
			}
			key = wave_max(key);
			if (key == 0)
				break;
			const uint32_t s = key & 255u;
			if ((s & 63u) == lane) {
				K += 1u << (11u - Ls[s >> 6]);
				Ls[s >> 6]--;
			}
			K = (uint32_t)__shfl((int)K, (int)(s & 63u), 64);
		}
		uint32_t lmax = 0;
#pragma unroll
		for (int k = 0; k < 4; k++) {
			L.len[lane + 64 * k] = (uint8_t)Ls[k];
			lmax = Ls[k] > lmax ? Ls[k] : lmax;
		}
		lmax = wave_max(lmax);
		__syncthreads();
		if (K == 2048u) {
			/* canonical codes exactly as the decoder lays them out: by weight ascending, then by symbol (a used symbol's weight) */
			if (lane == 0) {
				for (uint32_t w = 0; w < 16; w++) L.wcnt[w] = 0;
				for (uint32_t s = 0; s <= maxsym; s++)
					if (L.len[s]) L.wcnt[lmax + 1u - L.len[s]]++;
				uint32_t pos = 0;
				for (uint32_t w = 1; w <= lmax; w++) {
					const uint32_t c = L.wcnt[w];
					L.wcnt[w] = pos;
					pos += c << (w - 1u);
				}
				for (uint32_t s = 0; s <= maxsym; s++)
					if (L.len[s]) {
						const uint32_t w = lmax + 1u - L.len[s];
						L.code[s] = (uint16_t)(L.wcnt[w] >> (w - 1u));
						L.wcnt[w] += 1u << (w - 1u);
					}
			}
			__syncthreads();
			/* exact sizes: bits of every stream */
			const uint32_t four = nlit > 1023u;
			const uint32_t q = four ? (nlit + 3u) / 4u : nlit;
			uint32_t sb[4] = { 0, 0, 0, 0 };
			for (uint32_t i = lane; i < nlit; i += 64) {
				const uint32_t l = L.len[lits[i]], j = i / q;
				sb[0] += j == 0 ? l : 0u; sb[1] += j == 1 ? l : 0u; sb[2] += j == 2 ? l : 0u; sb[3] += j == 3 ? l : 0u;
			}
			uint32_t sbytes[4], body = 0;
#pragma unroll
			for (int j = 0; j < 4; j++) {
				sbytes[j] = wave_sum(sb[j]) / 8u + 1u;	/* bits + end mark, rounded up */
				if (j == 0 || four) body += sbytes[j];
			}
			const uint32_t nw = maxsym;	/* weights written: symbols 0 .. maxsym - 1 (the last one is implied) */
			/* tree description: the direct form holds at most 128 weights; under LA_ZSTDC_FULL_ALPHABET the FSE form
			 * is taken when it is the only one or the smaller one.  tree = 0: no form, the literals stay raw. */
			uint32_t tree = nw <= 128u ? 1u + (nw + 1u) / 2u : 0u, fse_bytes = 0;
			if (ENTROPY && (flags & LA_ZSTDC_FULL_ALPHABET) && nw >= 2u) {
				const uint32_t fb = zc_weights_fse(L, nw, lmax, lane);
				if (fb && (tree == 0 || 1u + fb < tree)) {
					tree = 1u + fb;
					fse_bytes = fb;
				}
			}
			const uint32_t comp = tree + (four ? 6u : 0u) + body;
			const uint32_t hl = !four ? 3u : (nlit < 16384u && comp < 16384u) ? 4u : 5u;
			const uint32_t raw_size = lit_hdr_rr(out, 0, nlit, false) + nlit;
			if (tree && hl + comp < raw_size && (four || comp < 1024u)) {
				if (lane == 0) {
					const uint32_t sf = !four ? 0u : hl == 4u ? 2u : 3u;
					const uint64_t v = 2u | (sf << 2) | ((uint64_t)nlit << 4) | ((uint64_t)comp << (hl == 3u ? 14 : hl == 4u ? 18 : 22));
					for (uint32_t k = 0; k < hl; k++) out[k] = (uint8_t)(v >> (8u * k));
					out[hl] = (uint8_t)(fse_bytes ? fse_bytes : 127u + nw);
				}
				if (fse_bytes) {
					for (uint32_t k = lane; k < fse_bytes; k += 64)
						out[hl + 1u + k] = L.u.wf.tree[k];
				}
				/* direct 4-bit weights, two per byte, the first in the high nibble */
				for (uint32_t k = lane; k < (fse_bytes ? 0u : (nw + 1u) / 2u); k += 64) {
					const uint32_t s0 = 2u * k, s1 = 2u * k + 1u;
					const uint32_t w0 = zc_weight(L.len[s0], lmax), w1 = s1 < nw ? zc_weight(L.len[s1], lmax) : 0u;
					out[hl + 1u + k] = (uint8_t)((w0 << 4) | w1);
				}
				op = hl + tree;
				if (four) {
					if (lane == 0) {
						out[op] = (uint8_t)sbytes[0]; out[op + 1] = (uint8_t)(sbytes[0] >> 8);
						out[op + 2] = (uint8_t)sbytes[1]; out[op + 3] = (uint8_t)(sbytes[1] >> 8);
						out[op + 4] = (uint8_t)sbytes[2]; out[op + 5] = (uint8_t)(sbytes[2] >> 8);
					}
					op += 6;
					for (uint32_t j = 0; j < 4; j++) {
						const uint32_t a = j * q, b = (j + 1u) * q < nlit ? (j + 1u) * q : nlit;
						op += huf_stream_enc(L, lits, a, b, out + op, lane);
					}
				} else {
					op += huf_stream_enc(L, lits, 0, nlit, out + op, lane);
				}
				lit_done = true;
			}
		}
	}
	if (!lit_done) {	/* Raw_Literals_Block */
		op = lit_hdr_rr(out, 0, nlit, lane == 0);
		wave_copy(out + op, lits, nlit, lane);
		op += nlit;
	}
	__syncthreads();	/* the FSE tables below reuse the match table */

	/* ---- sequences section ---- */
	if (op + 4u > cap || op >= n) {
		if (lane == 0) { btype[bi] = 0; csize[bi] = n; }
		return;
	}
	if (nseq < 128u) {
		if (lane == 0) out[op] = (uint8_t)nseq;
		op += 1;
	} else if (nseq < 0x7F00u) {
		if (lane == 0) { out[op] = (uint8_t)((nseq >> 8) + 128u); out[op + 1] = (uint8_t)nseq; }
		op += 2;
	} else {
		if (lane == 0) { out[op] = 255; out[op + 1] = (uint8_t)(nseq - 0x7F00u); out[op + 2] = (uint8_t)((nseq - 0x7F00u) >> 8); }
		op += 3;
	}
	bool over = false;
	if (ENTROPY && nseq > 0 && (flags & LA_ZSTDC_FIT_TABLES)) {
		op = zc_sequences_fit(L, seqs, nseq, out, op, cap, lane, over);
	} else if (nseq > 0) {
		op = zc_sequences_predefined(L.u.f, seqs, nseq, out, op, cap, lane, over);
	}
	if (lane == 0) {
		const bool comp = !over && op < n;
		btype[bi] = comp ? 2u : 0u;
		csize[bi] = comp ? op : n;
	}
}

/* XXH64 by FOUR adjacent lanes (lane j of the quad owns accumulator j and reads the j-th word of every 32-byte
 * stripe); the result is valid in all four lanes */
__device__ static uint64_t xxh64_quad(const uint8_t *p, uint64_t len, uint32_t j)
{
	const uint8_t *end = p + len;
	uint64_t h;
	if (len >= 32) {
		uint64_t v = j == 0 ? P64_1 + P64_2 : (j == 1 ? P64_2 : (j == 2 ? 0ull : 0ull - P64_1));
		const uint64_t stripes = len / 32;
		const uint8_t *q = p + 8u * j;
#pragma unroll 8
		for (uint64_t s = 0; s < stripes; s++)
			v = xxh64_round(v, rd64(q + 32u * s));
		const uint32_t q0 = threadIdx.x & ~3u;
		uint64_t a[4];
		for (uint32_t k = 0; k < 4; k++) {
			const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, (int)(q0 + k), 64);
			const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), (int)(q0 + k), 64);
			a[k] = (uint64_t)lo | ((uint64_t)hi << 32);
		}
		h = rotl64(a[0], 1) + rotl64(a[1], 7) + rotl64(a[2], 12) + rotl64(a[3], 18);
		h = xxh64_merge(h, a[0]); h = xxh64_merge(h, a[1]); h = xxh64_merge(h, a[2]); h = xxh64_merge(h, a[3]);
		p += stripes * 32u;
	} else {
		h = P64_5;
	}
	h += len;
	while (p + 8 <= end) { h ^= xxh64_round(0, rd64(p)); h = rotl64(h, 27) * P64_1 + P64_4; p += 8; }
	if (p + 4 <= end) { h ^= (uint64_t)rd32(p) * P64_1; h = rotl64(h, 23) * P64_2 + P64_3; p += 4; }
	while (p < end) { h ^= (uint64_t)(*p++) * P64_5; h = rotl64(h, 11) * P64_1; }
	h ^= h >> 33; h *= P64_2; h ^= h >> 29; h *= P64_3; h ^= h >> 32;
	return h;
}

struct zc_xxh64 {
	__device__ uint32_t operator()(const uint8_t *p, uint64_t len, uint32_t j) const { return (uint32_t)xxh64_quad(p, len, j); }
};

__host__ __device__ static inline uint32_t zc_fcs_len(uint64_t fcs) { return fcs < 256u ? 1u : fcs < 65536u + 256u ? 2u : 4u; }

/* bytes of the stream each block contributes: block header + payload, plus the frame header in front of the
 * frame's first block and the checksum behind its last */
__global__ __launch_bounds__(256) void zstdc_sizes_kernel(const uint32_t *__restrict__ csize, uint64_t src_bytes,
    uint32_t block_size, uint32_t n_blocks, uint32_t bpf, uint32_t flags, uint32_t *__restrict__ contrib)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n_blocks)
		return;
	uint32_t c = 3u + csize[i];
	if (i % bpf == 0) {
		const uint64_t fo = (uint64_t)i * block_size, fb = (uint64_t)bpf * block_size;
		const uint64_t fcs = src_bytes - fo < fb ? src_bytes - fo : fb;
		c += 5u + zc_fcs_len(fcs);
	}
	if ((i % bpf == bpf - 1 || i + 1 == n_blocks) && (flags & LA_ZSTDC_CHECKSUM))
		c += 4u;
	contrib[i] = c;
}

__global__ __launch_bounds__(256) void zstd_pack_frames_kernel(const uint8_t *__restrict__ src, uint64_t src_bytes,
    uint32_t block_size, uint32_t n_blocks, uint32_t bpf, uint32_t flags, const uint8_t *__restrict__ tmp,
    const uint32_t *__restrict__ btype, const uint32_t *__restrict__ csize, const uint64_t *__restrict__ off,
    const uint32_t *__restrict__ frame_sum, uint8_t *__restrict__ out, uint64_t out_cap, uint64_t *__restrict__ out_bytes)
{
	const uint32_t bi = blockIdx.x, tid = threadIdx.x;
	if (bi >= n_blocks)
		return;
	const uint64_t so = (uint64_t)bi * block_size;
	const uint32_t n = src_bytes > so ? (uint32_t)(src_bytes - so < block_size ? src_bytes - so : block_size) : 0u;
	const uint32_t type = btype[bi], pay = csize[bi];
	const bool last = bi % bpf == bpf - 1 || bi + 1 == n_blocks;
	uint64_t o = off[bi];
	if (bi + 1 == n_blocks && tid == 0)
		*out_bytes = off[n_blocks];
	if (off[bi + 1] > out_cap)
		return;		/* the caller sees out_bytes > out_cap */
	if (bi % bpf == 0) {
		const uint64_t fb = (uint64_t)bpf * block_size;
		const uint64_t fcs = src_bytes - so < fb ? src_bytes - so : fb;
		const uint32_t fl = zc_fcs_len(fcs);
		if (tid == 0) {
			/* magic; FHD: FCS_Field_Size flag, Single_Segment_Flag, Content_Checksum_Flag, no dictionary */
			st_le32(out + o, 0xFD2FB528u);
			out[o + 4] = (uint8_t)((fl == 1u ? 0u : fl == 2u ? 0x40u : 0x80u) | 0x20u | ((flags & LA_ZSTDC_CHECKSUM) ? 4u : 0u));
			const uint64_t v = fl == 2u ? fcs - 256u : fcs;
			for (uint32_t k = 0; k < fl; k++)
				out[o + 5 + k] = (uint8_t)(v >> (8u * k));
		}
		o += 5u + fl;
	}
	if (tid == 0) {
		const uint32_t bh = (last ? 1u : 0u) | (type << 1) | ((type == 2u ? pay : n) << 3);
		out[o] = (uint8_t)bh; out[o + 1] = (uint8_t)(bh >> 8); out[o + 2] = (uint8_t)(bh >> 16);
	}
	o += 3;
	const uint8_t *payload = type == 2u ? tmp + (uint64_t)bi * zc_tmp_stride(block_size) : src + so;
	for (uint32_t i = tid; i < pay; i += 256)
		out[o + i] = payload[i];
	o += pay;
	if (last && (flags & LA_ZSTDC_CHECKSUM) && tid == 0)
		st_le32(out + o, frame_sum[bi / bpf]);
}

static uint64_t zc_blocks(uint64_t src_bytes, uint32_t bs) { return src_bytes ? (src_bytes + bs - 1) / bs : 1u; }

struct zc_ws {
	uint8_t *tmp, *lits;
	uint64_t *seqs, *off;
	uint32_t *btype, *csize, *contrib, *fsum;
	void *scan;
};

/* the launcher's workspace on `base` (null: sizes only); returns its bytes before the scan scratch */
static uint64_t zc_carve(zc_ws *w, uint8_t *base, uint64_t nb, uint64_t nf, uint32_t bs)
{
	la_carve c = { base, 0 };
	w->tmp = c.take<uint8_t>(nb * zc_tmp_stride(bs));
	w->lits = c.take<uint8_t>(nb * zc_lit_stride(bs));
	w->seqs = c.take<uint64_t>(nb * zc_seq_stride(bs) / 8u);
	w->btype = c.take<uint32_t>(nb);
	w->csize = c.take<uint32_t>(nb);
	w->contrib = c.take<uint32_t>(nb);
	w->off = c.take<uint64_t>(nb + 1);
	w->fsum = c.take<uint32_t>(nf);
	w->scan = c.take<uint8_t>(0, 256);
	return c.off;
}

extern "C" uint64_t la_gpu_zstd_compress_workspace_bytes(uint64_t src_bytes, uint32_t block_size, uint32_t blocks_per_frame)
{
	if (block_size == 0 || block_size > ZC_BLOCK_MAX || blocks_per_frame == 0)
		return 0;
	const uint64_t nb = zc_blocks(src_bytes, block_size), nf = (nb + blocks_per_frame - 1) / blocks_per_frame;
	zc_ws w;
	return zc_carve(&w, nullptr, nb, nf, block_size) + la_scan_scratch_bytes((uint32_t)nb);
}

extern "C" uint64_t la_gpu_zstd_compress_bound(uint64_t src_bytes, uint32_t block_size, uint32_t blocks_per_frame)
{
	if (block_size == 0 || block_size > ZC_BLOCK_MAX || blocks_per_frame == 0)
		return 0;
	const uint64_t nb = zc_blocks(src_bytes, block_size), nf = (nb + blocks_per_frame - 1) / blocks_per_frame;
	return src_bytes + nb * 3u + nf * 13u + 64u;	/* a block is at most its input (raw); frame header 9, checksum 4 */
}

void la_launch_zstd_compress(hipStream_t s, const uint8_t *d_src, uint64_t src_bytes, uint32_t block_size,
    uint32_t bpf, uint32_t flags, uint8_t *d_out, uint64_t out_cap, uint64_t *d_out_bytes, uint8_t *ws)
{
	const uint32_t nb = (uint32_t)zc_blocks(src_bytes, block_size);
	const uint32_t nf = (nb + bpf - 1) / bpf;
	zc_ws w;
	zc_carve(&w, ws, nb, nf, block_size);
	if (flags & (LA_ZSTDC_FULL_ALPHABET | LA_ZSTDC_FIT_TABLES))
		hipLaunchKernelGGL(zstd_compress_blocks_kernel<true>, dim3(nb), dim3(64), 0, s, d_src, src_bytes, block_size, nb, flags,
		    w.tmp, w.lits, w.seqs, w.btype, w.csize);
	else
		hipLaunchKernelGGL(zstd_compress_blocks_kernel<false>, dim3(nb), dim3(64), 0, s, d_src, src_bytes, block_size, nb, flags,
		    w.tmp, w.lits, w.seqs, w.btype, w.csize);
	if (flags & LA_ZSTDC_CHECKSUM)
		hipLaunchKernelGGL(frame_sums_kernel<zc_xxh64>, dim3((nf + 15) / 16), dim3(64), 0, s, d_src, src_bytes,
		    (uint64_t)bpf * block_size, nf, w.fsum);
	hipLaunchKernelGGL(zstdc_sizes_kernel, dim3((nb + 255) / 256), dim3(256), 0, s, w.csize, src_bytes, block_size, nb, bpf, flags, w.contrib);
	la_launch_scan_u32(s, w.contrib, nb, w.off, w.scan);
	hipLaunchKernelGGL(zstd_pack_frames_kernel, dim3(nb), dim3(256), 0, s, d_src, src_bytes, block_size, nb, bpf, flags,
	    w.tmp, w.btype, w.csize, w.off, w.fsum, d_out, out_cap, d_out_bytes);
}
