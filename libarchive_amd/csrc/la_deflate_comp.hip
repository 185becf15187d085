/*
 * la_deflate_comp.hip -- DEFLATE compression + gzip member assembly on the device (gfx950):
 * the data plane of the gzip write filter.
 *
 * Replaces, for a whole stream per call, what libarchive/archive_write_add_filter_gzip.c does
 * through zlib on the host: deflateInit2(-15) / deflate() per write (:293-345, drive_compressor),
 * the 10-byte header it builds by hand (:201-237), CRC32 of the input (:263-266) and the trailer
 * [crc32 LE][isize LE] (:309-331).  The compressed bytes are not zlib's (a deflate stream is not
 * unique); parity for this direction is the round trip: zlib's inflate (what every gzip reader runs,
 * the reference's included), the oracle's gzip filter and this repository's device decoder must
 * return the input.
 *
 * Shape.  The input is cut into chunks of at most 48 KiB and every chunk becomes ONE gzip member --
 * the many-member shape the read side is built for -- whose header carries the BGZF-compatible "BC"
 * size subfield, so that the read filter indexes members without searching (C3's stream shape).
 *   deflate_fixed_kernel    one wave per chunk.  Per window of 64 positions every lane hashes three bytes,
 *       takes and replaces the candidate in a 4096-entry table of 16-bit positions (LDS), verifies it
 *       and extends the match to at most 258 bytes within 32 KiB; the wave takes the matches in position
 *       order and marks what they cover; then every lane knows its token -- literal, match start or
 *       nothing -- as at most 31 bits of a FIXED-Huffman block (RFC 1951 3.2.6), a wave prefix sum of
 *       the bit counts gives every token its place, lanes OR their bits into a small LDS stage and whole
 *       dwords go out coalesced (wave_bits_append, la_comp_common.h).  A chunk that would not shrink is written as a stored block instead.
 *   deflate_dynamic_kernel  (LA_GZC_DYNAMIC) the same matcher, but a token is kept and its symbols counted; the wave
 *       then builds length-limited complete codes for the chunk (RFC 1951 3.2.7), knows the exact size of the dynamic,
 *       the fixed and the stored block, and writes the smallest in a second pass over the tokens.
 *   gz_jobs_kernel + crc32_many  CRC32 of every chunk (la_hash.hip).
 *   gz_pack_kernel          header, body (Huffman or stored), trailer at their scanned offsets.
 *
 * Second shape (LA_GZC_FRAME_STREAM).  The same chunks, the same kernels, but the output is a byte-aligned piece of ONE
 * raw-deflate stream that the caller continues or ends: no gzip header, no trailer, no CRC32, no block with BFINAL
 * set.  A Huffman chunk is a non-final block followed by zlib's sync-flush shape -- the three header bits of an empty
 * non-final stored block, zero bits up to the byte boundary, 00 00 FF FF -- so that the next chunk starts on a byte; a
 * stored chunk is 00 LEN NLEN data.  Matches still end with their chunk, so a chunk's bytes do not depend on its
 * neighbours.  The kernels take the shape as a template parameter: the members build of each is the code it was.
 *
 * Third shape (la_gpu_zip_compress, at the end of this file).  The stream shape for a whole write window of ZIP
 * entries in one call: the chunks are cut per entry segment, not on an even grid, so the four kernels take where a
 * chunk lies as a second template parameter (dfl_even / dfl_spans below); the even instances are the code they were.
 */
#include "la_comp_common.h"

#define DFL_CHUNK_MAX 49152u
#define DFL_HASH_BITS 12
#define DFL_HDR       18u	/* 10 fixed + XLEN(2) + "BC" 2 0 BSIZE(2) */

/* Room of one chunk's Huffman body in the workspace.  The longest is the fixed block of n 9-bit literals: 3 header
 * bits, 9 n, 7 of end-of-block, so at most ((9 n + 7) >> 3) + 2 bytes.  The stream shape's tail (DFL_TAIL_MAX) and the
 * three bytes a last whole-dword store may add make that + 10 at most: inside the 16 bytes of slack. */
__host__ __device__ static inline uint32_t dfl_body_bound(uint32_t n) { return ((n * 9u + 7u) >> 3) + 16u; }

/* Stream shape: what follows a Huffman block's end-of-block symbol -- 3 bits, 0..7 bits of padding, 4 bytes.  It
 * adds at most 5 bytes to the block's whole bytes: ((bits + 3 + 7) >> 3) + 4 <= ((bits + 7) >> 3) + 1 + 4. */
#define DFL_TAIL_MAX 5u
__device__ __forceinline__ uint32_t dfl_block_bytes(uint32_t bits, bool stream)
{
	return stream ? ((bits + 3u + 7u) >> 3) + 4u : (bits + 7u) >> 3;
}
/* The tail as three tokens for the bit stage, bp = the bits before it: lane 0 the empty stored block's header with
 * the padding, lane 1 its LEN 0000, lane 2 its NLEN FFFF. */
__device__ __forceinline__ uint32_t dfl_tail_token(uint64_t bp, uint32_t lane, uint32_t *bits)
{
	*bits = lane == 2u ? 0xFFFFu : 0u;
	return lane == 0 ? 3u + ((0u - ((uint32_t)bp + 3u)) & 7u) : (lane < 3u ? 16u : 0u);
}

__device__ __forceinline__ uint32_t rev_bits(uint32_t v, uint32_t n) { return __builtin_bitreverse32(v) >> (32u - n); }

/* literal / end-of-block code of the fixed tree, ready for LSB-first packing; *nb = its length */
__device__ __forceinline__ uint32_t fixed_lit(uint32_t sym, uint32_t *nb)
{
	if (sym < 144u) { *nb = 8; return rev_bits(0x30u + sym, 8); }
	if (sym < 256u) { *nb = 9; return rev_bits(0x190u + (sym - 144u), 9); }
	if (sym < 280u) { *nb = 7; return rev_bits(sym - 256u, 7); }
	*nb = 8; return rev_bits(0xC0u + (sym - 280u), 8);
}

/* length symbol (257..285) of a match length 3..258, with its extra bits (RFC 1951 3.2.5) */
__device__ __forceinline__ uint32_t dfl_len_code(uint32_t len, uint32_t *eb, uint32_t *ex)
{
	const uint32_t l = len - 3u;
	*eb = 0; *ex = 0;
	if (l < 8u)
		return 257u + l;
	if (l == 255u)
		return 285u;
	const uint32_t n = 31u - (uint32_t)__builtin_clz(l);
	*eb = n - 2u;
	*ex = (l - (1u << n)) & ((1u << (n - 2u)) - 1u);
	return 257u + 4u * (n - 1u) + ((l - (1u << n)) >> (n - 2u));
}

/* distance symbol (0..29) of a distance 1..32768, with its extra bits */
__device__ __forceinline__ uint32_t dfl_dist_code(uint32_t dist, uint32_t *eb, uint32_t *ex)
{
	const uint32_t d = dist - 1u;
	*eb = 0; *ex = 0;
	if (d < 4u)
		return d;
	const uint32_t n = 31u - (uint32_t)__builtin_clz(d);
	*eb = n - 1u;
	*ex = d & ((1u << (n - 1u)) - 1u);
	return 2u * n + ((d >> (n - 1u)) & 1u);
}

/* a match of `len` (3..258) at `dist` (1..32768) as bits; returns the bit count (at most 31) */
__device__ __forceinline__ uint32_t fixed_match(uint32_t len, uint32_t dist, uint32_t *bits)
{
	uint32_t leb, lex, deb, dex;
	const uint32_t lcode = dfl_len_code(len, &leb, &lex), dcode = dfl_dist_code(dist, &deb, &dex);
	uint32_t nb, v = fixed_lit(lcode, &nb);
	v |= lex << nb; nb += leb;
	v |= rev_bits(dcode, 5) << nb; nb += 5u;
	v |= dex << nb; nb += deb;
	*bits = v;
	return nb;
}

/* Where chunk ci of a launch lies.  dfl_even: chunk ci is src[ci * chunk, ...), the members and stream shapes.  dfl_spans:
 * a table built on the device says it (la_gpu_zip_compress: no chunk crosses a segment), its length is known on the
 * device only -- n_chunks is then the bound the launch is sized by -- and a chunk has its own room in `tmp`.  The
 * kernels take the geometry as a template parameter and the table as their last parameter; with dfl_even the table is
 * not read and each kernel is the code it was. */
#define DFL_SPAN_COPY 0x80000000u	/* dfl_span.seg: the segment is LA_ZIPC_STORE, the chunk is copied as it is */
struct dfl_span {
	uint64_t off;	/* in src */
	uint32_t len;	/* 1 .. chunk */
	uint32_t seg;	/* its segment | DFL_SPAN_COPY */
};
struct dfl_span_table {
	const dfl_span *tab;
	const uint64_t *tmp_off;	/* [count + 1]: chunk ci's room in tmp, a multiple of 16 at a multiple of 16 */
	const uint64_t *n;		/* how many there are */
	const uint64_t *delta;		/* [segments]: pack kernel, what to add to a chunk's scanned offset */
};

struct dfl_even {
	uint64_t src_bytes;
	uint32_t chunk, n_chunks;
	static constexpr bool SPANS = false;
	__device__ __forceinline__ dfl_even(uint64_t src_bytes_, uint32_t chunk_, uint32_t n_chunks_, const dfl_span_table &)
	    : src_bytes(src_bytes_), chunk(chunk_), n_chunks(n_chunks_) {}
	__device__ __forceinline__ uint32_t count() const { return n_chunks; }
	__device__ __forceinline__ uint32_t span(uint32_t ci, uint64_t *so) const
	{
		*so = (uint64_t)ci * chunk;
		return (uint32_t)(src_bytes - *so < chunk ? src_bytes - *so : chunk);
	}
	__device__ __forceinline__ bool deflates(uint32_t) const { return true; }
	__device__ __forceinline__ uint64_t tmp_at(uint32_t ci, uint32_t stride) const { return (uint64_t)ci * stride; }
	__device__ __forceinline__ uint32_t tmp_room(uint32_t, uint32_t stride) const { return stride; }
};

struct dfl_spans : dfl_span_table {
	uint32_t chunk;
	static constexpr bool SPANS = true;
	__device__ __forceinline__ dfl_spans(uint64_t, uint32_t chunk_, uint32_t, const dfl_span_table &t) : dfl_span_table(t), chunk(chunk_) {}
	__device__ __forceinline__ uint32_t count() const { return (uint32_t)*n; }
	__device__ __forceinline__ uint32_t span(uint32_t ci, uint64_t *so) const { *so = tab[ci].off; return tab[ci].len; }
	__device__ __forceinline__ bool deflates(uint32_t ci) const { return !(tab[ci].seg & DFL_SPAN_COPY); }
	__device__ __forceinline__ uint64_t tmp_at(uint32_t ci, uint32_t) const { return tmp_off[ci]; }
	__device__ __forceinline__ uint32_t tmp_room(uint32_t ci, uint32_t) const { return (uint32_t)(tmp_off[ci + 1] - tmp_off[ci]); }
};

template <bool STREAM, typename GEO>
__global__ __launch_bounds__(64) void deflate_fixed_kernel(const uint8_t *__restrict__ src, uint64_t src_bytes,
    uint32_t chunk, uint32_t n_chunks, uint8_t *__restrict__ tmp, uint32_t tmp_stride, uint32_t *__restrict__ body_len,
    const dfl_span_table spans)
{
	const GEO geo(src_bytes, chunk, n_chunks, spans);
	__shared__ uint16_t tab[1u << DFL_HASH_BITS];
	__shared__ uint32_t stage[72];
	const uint32_t ci = blockIdx.x, lane = threadIdx.x;
	if (ci >= geo.count() || !geo.deflates(ci))
		return;
	uint64_t so;
	const uint32_t n = geo.span(ci, &so);
	const uint8_t *in = src + so;
	uint32_t *out = (uint32_t *)(void *)(tmp + geo.tmp_at(ci, tmp_stride));	/* dword aligned: the stride is a multiple of 16 */
	for (uint32_t i = lane; i < (1u << DFL_HASH_BITS); i += 64)
		tab[i] = 0;
	for (uint32_t i = lane; i < 72; i += 64)
		stage[i] = 0;
	__syncthreads();
	if (lane == 0)
		stage[0] = STREAM ? 2u : 3u;	/* block header: BFINAL = 1 (0 in a stream), BTYPE = 01 (fixed Huffman), LSB first */
	uint64_t bp = 3;	/* bits written so far (wave-uniform) */
	uint32_t anchor = 0;	/* first position not covered by a match taken so far */
	__builtin_amdgcn_wave_barrier();

	for (uint32_t base = 0; base < n; base += 64) {
		const uint32_t p = base + lane;
		const bool have = p < n;
		uint32_t cand = 0, mlen = 0, v3 = 0;
		const bool can = have && p + 3u <= n;
		if (can) {
			v3 = (uint32_t)in[p] | ((uint32_t)in[p + 1] << 8) | ((uint32_t)in[p + 2] << 16);
			cand = tab[(v3 * 2654435761u) >> (32 - DFL_HASH_BITS)];
		}
		__builtin_amdgcn_wave_barrier();
		bool ok = false;
		if (can) {
			tab[(v3 * 2654435761u) >> (32 - DFL_HASH_BITS)] = (uint16_t)p;
			if (cand < p && p - cand <= 32768u) {
				const uint32_t c3 = (uint32_t)in[cand] | ((uint32_t)in[cand + 1] << 8) | ((uint32_t)in[cand + 2] << 16);
				if (c3 == v3) {
					const uint32_t lim = n - p < 258u ? n - p : 258u;
					mlen = 3;
					while (mlen < lim && in[p + mlen] == in[cand + mlen])
						mlen++;
					ok = true;
				}
			}
		}
		/* the matches of this window in position order; `covered` = inside a match taken earlier */
		bool covered = have && p < anchor, taken = false;
		uint64_t mask = __ballot(ok);
		while (mask != 0) {
			const uint32_t f = (uint32_t)__builtin_ctzll(mask);
			mask &= mask - 1;
			const uint32_t pf = base + f;
			if (pf < anchor)
				continue;
			const uint32_t mf = (uint32_t)__builtin_amdgcn_readlane((int)mlen, (int)f);
			if (lane == f)
				taken = true;
			covered = covered || (p > pf && p < pf + mf);
			anchor = pf + mf;
		}
		/* this lane's token */
		uint32_t bits = 0, nb = 0;
		if (have && !covered) {
			if (taken)
				nb = fixed_match(mlen, p - cand, &bits);
			else
				bits = fixed_lit(in[p], &nb);
		}
		/* its place in the stream; whole dwords go out aligned */
		bp += wave_bits_append(bp, bits, nb, stage, lane, [&](uint32_t i, uint32_t w) { out[i] = w; });
	}
	/* end-of-block (seven zero bits), then the partial dword */
	if constexpr (STREAM) {
		/* lane 0's token of the tail takes the seven bits along */
		uint32_t bits;
		const uint32_t nb = dfl_tail_token(bp + 7, lane, &bits) + (lane == 0 ? 7u : 0u);
		bp += wave_bits_append(bp, bits, nb, stage, lane, [&](uint32_t i, uint32_t w) { out[i] = w; });
		if (lane == 0 && (bp & 31u))
			out[bp >> 5] = stage[0];
	} else {
		bp += 7;
		const uint32_t g0 = (uint32_t)((bp - 7) >> 5);
		const uint32_t tb = (uint32_t)((bp - 7) & 31u) + 7u;
		if (lane == 0) {
			out[g0] = stage[0];
			if (tb > 32u)
				out[g0 + 1] = 0;
		}
	}
	if (lane == 0)
		body_len[ci] = (uint32_t)((bp + 7) >> 3);	/* (a stream's tail ends on a byte) */
}

/* ------------------------------------------------------------------ dynamic Huffman (RFC 1951 3.2.7) */

#define DFL_NLL   286u		/* literal / length symbols */
#define DFL_ND    30u		/* distance symbols */
#define DFL_DOFF  288u		/* the distance symbols' place in the 320-entry histogram and code tables */
#define DFL_WAVES 3328u		/* waves of deflate_dynamic_kernel: 13 per CU by LDS on 256 CUs; each owns a token buffer */
#define DFL_TOK_MATCH 0x80000000u	/* token: a literal byte, or this | (len - 3) << 16 | (dist - 1) */

/* wave_bits_append for tokens of up to 48 bits: a length symbol with its extra bits and a distance symbol with its
 * extra bits are 15 + 5 + 15 + 13 bits.  The stage holds two dwords more than 64 such tokens can fill. */
template <uint32_t N, typename Store>
__device__ __forceinline__ uint32_t wave_bits_append64(uint64_t bp, uint64_t bits, uint32_t nb, uint32_t (&stage)[N],
    uint32_t lane, Store store)
{
	static_assert(N >= (31u + 64u * 48u) / 32u + 3u, "stage too small for 64 tokens of 48 bits");
	uint32_t inc = nb;
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
		const uint32_t t = __shfl_up(inc, d, 64);
		if ((int)lane >= d) inc += t;
	}
	const uint32_t total = __shfl(inc, 63, 64);
	const uint32_t at = (uint32_t)(bp & 31u) + inc - nb;
	if (nb) {
		const uint32_t sh = at & 31u;
		const uint64_t rest = (bits >> 1) >> (31u - sh);	/* what the first dword does not take */
		atomicOr(&stage[at >> 5], (uint32_t)(bits << sh));
		if ((uint32_t)rest)
			atomicOr(&stage[(at >> 5) + 1], (uint32_t)rest);
		if ((uint32_t)(rest >> 32))
			atomicOr(&stage[(at >> 5) + 2], (uint32_t)(rest >> 32));
	}
	__builtin_amdgcn_wave_barrier();
	const uint32_t nd = ((uint32_t)(bp & 31u) + total) >> 5;	/* at most 96 */
	const uint32_t g0 = (uint32_t)(bp >> 5);
	const uint32_t carry = stage[nd];
	const uint32_t m0 = lane < nd ? stage[lane] : 0, m1 = lane + 64u < nd ? stage[lane + 64u] : 0;
	__builtin_amdgcn_wave_barrier();
	if (lane < nd)
		store(g0 + lane, m0);
	if (lane + 64u < nd)
		store(g0 + lane + 64u, m1);
	if (lane <= nd)
		stage[lane] = 0;
	if (lane + 64u <= nd)
		stage[lane + 64u] = 0;
	__builtin_amdgcn_wave_barrier();
	if (lane == 0)
		stage[0] = carry;
	__builtin_amdgcn_wave_barrier();
	return total;
}

/* A code must have two symbols to be complete: with fewer in use, give symbol 0 (or 1, when 0 is the one in use) a
 * count of one, as zlib's build_tree does.  F = this lane's count, lane = its symbol. */
__device__ __forceinline__ uint32_t dfl_force_two(uint32_t F, uint32_t lane)
{
	const uint64_t used = __ballot(F != 0);
	const uint32_t nused = (uint32_t)__builtin_popcountll(used);
	if (nused >= 2u)
		return F;
	const uint32_t extra = (used & 1u) ? 1u : 0u;
	return (lane == extra || (nused == 0 && lane == 1u)) ? 1u : F;
}

/* Code lengths of a complete prefix code (Kraft sum exactly 1) of at most `maxbits` bits for the symbols with a
 * count; lane `lane` holds the symbols lane + 64 k.  At least two symbols have a count.  Shannon lengths
 * ceil(log2(N / f)) clamped to maxbits; where the clamp over-subscribes the code, the rarest symbols that can still
 * grow are lengthened; the room left is then given to the symbol whose count is largest for the code space it holds
 * (f * 2^len: the one the rounding-up cost most), one wave arg-max round per step.  Every step has a candidate (the
 * longest code always fits the room), so the rounds end in a complete code; the return value says that they did. */
template <int SLOTS>
__device__ __forceinline__ bool dfl_code_lengths(const uint32_t (&F)[SLOTS], uint32_t (&Ls)[SLOTS], uint32_t maxbits,
    uint32_t lane)
{
	uint32_t N = 0;
#pragma unroll
	for (int k = 0; k < SLOTS; k++)
		N += F[k];
	N = wave_sum(N);
	const uint32_t full = 1u << maxbits;
	uint32_t K = 0;
#pragma unroll
	for (int k = 0; k < SLOTS; k++) {
		uint32_t l = 0;
		if (F[k]) {
			while ((F[k] << l) < N) l++;
			l = l < 1u ? 1u : (l > maxbits ? maxbits : l);
			K += full >> l;
		}
		Ls[k] = l;
	}
	K = wave_sum(K);
	for (uint32_t it = 0; it < 8192u && K != full; it++) {
		const bool grow = K > full;
		const uint32_t room = full - K;
		uint32_t key = 0;
#pragma unroll
		for (int k = 0; k < SLOTS; k++) {
			const uint32_t s = lane + 64u * k;
			uint32_t c = 0;
			if (grow) {
				if (F[k] && Ls[k] < maxbits)
					c = 0x80000000u | ((0xFFFFu - F[k]) << 9) | s;
			} else if (F[k] && Ls[k] > 1u && (full >> Ls[k]) <= room) {
				const uint32_t w = F[k] << Ls[k];
				c = 0x80000000u | ((w < 0x3FFFFFu ? w : 0x3FFFFFu) << 9) | s;
			}
			key = c > key ? c : key;
		}
		key = wave_max(key);
		if (key == 0)
			break;
		const uint32_t s = key & 511u;
#pragma unroll
		for (int k = 0; k < SLOTS; k++)
			if (s == lane + 64u * k) {
				if (grow) { Ls[k]++; K -= full >> Ls[k]; }
				else { K += full >> Ls[k]; Ls[k]--; }
			}
		K = (uint32_t)__shfl((int)K, (int)(s & 63u), 64);
	}
	return K == full;
}

/* canonical codes (RFC 1951 3.2.2) for the lengths of dfl_code_lengths, bit-reversed for LSB-first packing, into
 * tab[symbol] = code | length << 16 (0 for a symbol without a code) */
template <int SLOTS>
__device__ __forceinline__ void dfl_assign_codes(const uint32_t (&Ls)[SLOTS], uint32_t maxbits, uint32_t *tab,
    uint32_t lane)
{
	const uint64_t below = ((uint64_t)1 << lane) - 1u;
	uint32_t next = 0;
#pragma unroll
	for (int k = 0; k < SLOTS; k++)
		if (Ls[k] == 0)
			tab[lane + 64u * k] = 0;
	for (uint32_t L = 1; L <= maxbits; L++) {
		next <<= 1;
#pragma unroll
		for (int k = 0; k < SLOTS; k++) {
			const bool m = Ls[k] == L;
			const uint64_t b = __ballot(m);
			if (m)
				tab[lane + 64u * k] = rev_bits(next + (uint32_t)__builtin_popcountll(b & below), L) | (L << 16);
			next += (uint32_t)__builtin_popcountll(b);
		}
	}
}

__device__ __forceinline__ uint32_t fixed_lit_len(uint32_t sym) { return sym < 144u ? 8u : (sym < 256u ? 9u : (sym < 280u ? 7u : 8u)); }

/* One wave per chunk, chunks ci = blockIdx.x + k * gridDim.x.  Pass 1 is deflate_fixed_kernel's matcher; instead of
 * coding a token it counts its symbols in LDS histograms and keeps the token in this wave's token buffer.  Then the
 * wave builds the two codes and the block header's code-length code, and knows the exact size of the dynamic, the
 * fixed and the stored block; it writes the smallest (nothing for a stored block: body_len >= n + 5 tells the pack
 * kernel) in a second pass over the tokens, with codes from an LDS table.  In a stream the sizes it compares include
 * the tail, which then follows the end-of-block symbol through the bit stage. */
template <bool STREAM, typename GEO>
__global__ __launch_bounds__(64) void deflate_dynamic_kernel(const uint8_t *__restrict__ src, uint64_t src_bytes,
    uint32_t chunk, uint32_t n_chunks_, uint8_t *__restrict__ tmp, uint32_t tmp_stride, uint32_t *__restrict__ body_len,
    uint32_t *__restrict__ tokbuf, const dfl_span_table spans)
{
	const GEO geo(src_bytes, chunk, n_chunks_, spans);
	__shared__ uint16_t tab[1u << DFL_HASH_BITS];
	__shared__ uint32_t stage[104];
	__shared__ uint32_t hist[320];		/* [0, 286) literal / length, [288, 318) distance */
	__shared__ uint32_t code[DFL_DOFF + 64];	/* same places: code | length << 16 */
	__shared__ uint32_t clh[64], clc[64];	/* code-length alphabet: counts, codes */
	__shared__ uint32_t hdr[4];		/* ncls, extra bits of the 16 / 17 / 18 symbols */
	uint16_t *cls = tab;	/* the header's code-length symbols, symbol | extra bits << 8: the match table is free by then */
	const uint32_t lane = threadIdx.x;
	const uint64_t below = ((uint64_t)1 << lane) - 1u;
	uint32_t *toks = tokbuf + (uint64_t)blockIdx.x * geo.chunk;
	const uint32_t n_chunks = geo.count();
	for (uint32_t ci = blockIdx.x; ci < n_chunks; ci += gridDim.x) {
		if (!geo.deflates(ci))
			continue;
		uint64_t so;
		const uint32_t n = geo.span(ci, &so);
		const uint8_t *in = src + so;
		uint32_t *out = (uint32_t *)(void *)(tmp + geo.tmp_at(ci, tmp_stride));
		__syncthreads();	/* the previous chunk's tables are done with */
		for (uint32_t i = lane; i < (1u << DFL_HASH_BITS); i += 64)
			tab[i] = 0;
		for (uint32_t i = lane; i < 104; i += 64)
			stage[i] = 0;
		for (uint32_t i = lane; i < 320; i += 64)
			hist[i] = 0;
		clh[lane] = 0;
		__syncthreads();

		/* ---- pass 1: tokens and histograms ---- */
		uint32_t anchor = 0, ntok = 0, xbits = 0, nmatch = 0;	/* xbits, nmatch: this lane's share */
		for (uint32_t base = 0; base < n; base += 64) {
			const uint32_t p = base + lane;
			const bool have = p < n;
			uint32_t cand = 0, mlen = 0, v3 = 0;
			const bool can = have && p + 3u <= n;
			if (can) {
				v3 = (uint32_t)in[p] | ((uint32_t)in[p + 1] << 8) | ((uint32_t)in[p + 2] << 16);
				cand = tab[(v3 * 2654435761u) >> (32 - DFL_HASH_BITS)];
			}
			__builtin_amdgcn_wave_barrier();
			bool ok = false;
			if (can) {
				tab[(v3 * 2654435761u) >> (32 - DFL_HASH_BITS)] = (uint16_t)p;
				if (cand < p && p - cand <= 32768u) {
					const uint32_t c3 = (uint32_t)in[cand] | ((uint32_t)in[cand + 1] << 8) | ((uint32_t)in[cand + 2] << 16);
					if (c3 == v3) {
						const uint32_t lim = n - p < 258u ? n - p : 258u;
						mlen = 3;
						while (mlen < lim && in[p + mlen] == in[cand + mlen])
							mlen++;
						ok = true;
					}
				}
			}
			bool covered = have && p < anchor, taken = false;
			uint64_t mask = __ballot(ok);
			while (mask != 0) {
				const uint32_t f = (uint32_t)__builtin_ctzll(mask);
				mask &= mask - 1;
				const uint32_t pf = base + f;
				if (pf < anchor)
					continue;
				const uint32_t mf = (uint32_t)__builtin_amdgcn_readlane((int)mlen, (int)f);
				if (lane == f)
					taken = true;
				covered = covered || (p > pf && p < pf + mf);
				anchor = pf + mf;
			}
			const bool tok = have && !covered;
			uint32_t t = 0;
			if (tok) {
				if (taken) {
					uint32_t leb, lex, deb, dex;
					atomicAdd(&hist[dfl_len_code(mlen, &leb, &lex)], 1u);
					atomicAdd(&hist[DFL_DOFF + dfl_dist_code(p - cand, &deb, &dex)], 1u);
					xbits += leb + deb;
					nmatch++;
					t = DFL_TOK_MATCH | ((mlen - 3u) << 16) | (p - cand - 1u);
				} else {
					t = in[p];
					atomicAdd(&hist[t], 1u);
				}
			}
			const uint64_t tb = __ballot(tok);
			if (tok)
				toks[ntok + (uint32_t)__builtin_popcountll(tb & below)] = t;
			ntok += (uint32_t)__builtin_popcountll(tb);
		}
		xbits = wave_sum(xbits);
		nmatch = wave_sum(nmatch);
		__syncthreads();	/* histograms complete; the tokens are visible to the whole wave */
		if (lane == 0)
			hist[256] = 1;	/* end-of-block */
		__syncthreads();

		/* ---- the two codes; the cost of the symbols under them and under the fixed code ---- */
		uint32_t F[5], Ls[5], Fd[1], Ld[1];
		uint32_t dyn_bits = 0, fix_bits = 0, top = 0;
#pragma unroll
		for (int k = 0; k < 5; k++) {
			const uint32_t s = lane + 64u * k;
			F[k] = s < DFL_NLL ? hist[s] : 0;
		}
		bool complete = dfl_code_lengths<5>(F, Ls, 15u, lane);
#pragma unroll
		for (int k = 0; k < 5; k++) {
			const uint32_t s = lane + 64u * k;
			dyn_bits += F[k] * Ls[k];
			fix_bits += F[k] * fixed_lit_len(s);
			if (Ls[k])
				top = s;
		}
		const uint32_t fd = lane < DFL_ND ? hist[DFL_DOFF + lane] : 0;
		Fd[0] = dfl_force_two(fd, lane);
		complete = dfl_code_lengths<1>(Fd, Ld, 15u, lane) && complete;
		dyn_bits += fd * Ld[0];
		dyn_bits = wave_sum(dyn_bits) + xbits;
		fix_bits = wave_sum(fix_bits) + 5u * nmatch + xbits + 3u;
		const uint32_t nlit = wave_max(top) + 1u;			/* 257 .. 286 */
		const uint32_t ndist = wave_max(Ld[0] ? lane : 0u) + 1u;	/* 2 .. 30 */

		/* ---- the header: both length arrays as one run-length coded sequence (one lane: 316 steps at most) ---- */
#pragma unroll
		for (int k = 0; k < 5; k++)
			code[lane + 64u * k] = Ls[k];	/* lengths for now; the codes replace them below */
		__builtin_amdgcn_wave_barrier();
		if (lane < DFL_ND)
			code[DFL_DOFF + lane] = Ld[0];
		__syncthreads();
		if (lane == 0) {
			const uint32_t total = nlit + ndist;
			uint32_t nc = 0, i = 0;
			while (i < total) {
				const uint32_t v = code[i < nlit ? i : DFL_DOFF + i - nlit];
				uint32_t run = 1;
				while (i + run < total && code[i + run < nlit ? i + run : DFL_DOFF + i + run - nlit] == v)
					run++;
				i += run;
				if (v != 0) {
					cls[nc++] = (uint16_t)v; clh[v]++;
					run--;
				}
				while (run >= 3u) {
					uint32_t r, sym, base;
					if (v != 0) { sym = 16; base = 3; r = run < 6u ? run : 6u; }
					else if (run < 11u) { sym = 17; base = 3; r = run; }
					else { sym = 18; base = 11; r = run < 138u ? run : 138u; }
					cls[nc++] = (uint16_t)(sym | ((r - base) << 8)); clh[sym]++;
					run -= r;
				}
				for (; run > 0; run--) {
					cls[nc++] = (uint16_t)v; clh[v]++;
				}
			}
			hdr[0] = nc;
			hdr[1] = 2u * clh[16] + 3u * clh[17] + 7u * clh[18];
		}
		__syncthreads();
		const uint32_t ncls = hdr[0];
		/* the code-length code, at most 7 bits; lane j < 19 also looks after place j of the RFC's order */
		uint32_t Fc[1], Lc[1];
		Fc[0] = dfl_force_two(lane < 19u ? clh[lane] : 0u, lane);
		complete = dfl_code_lengths<1>(Fc, Lc, 7u, lane) && complete;
		dfl_assign_codes<1>(Lc, 7u, clc, lane);
		uint32_t hbits = wave_sum((lane < 19u ? clh[lane] : 0u) * Lc[0]) + hdr[1];
		__syncthreads();
		/* place j of the RFC's order 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15 */
		const uint32_t osym = lane < 3u ? 16u + lane : (uint32_t)((0xF1E2D3C4B5A69780ull >> (4u * ((lane - 3u) & 15u))) & 15u);
		const uint32_t olen = lane < 19u ? (clc[osym] >> 16) : 0u;
		uint32_t hclen = 64u - (uint32_t)__builtin_clzll(__ballot(olen != 0) | 1u);
		hclen = hclen < 4u ? 4u : hclen;
		dyn_bits += 3u + 14u + 3u * hclen + hbits;

		/* ---- the smallest of the three; a stored block is n + 5 bytes and is not written here ---- */
		const uint32_t dyn_bytes = dfl_block_bytes(dyn_bits, STREAM), fix_bytes = dfl_block_bytes(fix_bits, STREAM);
		const bool dyn = complete && dyn_bytes < fix_bytes;
		const uint32_t bytes = dyn ? dyn_bytes : fix_bytes;
		if (bytes >= n + 5u) {
			if (lane == 0)
				body_len[ci] = n + 5u;
			continue;
		}
		const auto put = [&](uint32_t i, uint32_t w) { if (i < geo.tmp_room(ci, tmp_stride) / 4u) out[i] = w; };	/* (bytes < n + 5 fits) */
		uint64_t bp = 0;
		if (dyn) {
			dfl_assign_codes<5>(Ls, 15u, code, lane);
			__builtin_amdgcn_wave_barrier();
			dfl_assign_codes<1>(Ld, 15u, code + DFL_DOFF, lane);
			__syncthreads();
			/* BFINAL = 1 (0 in a stream), BTYPE = 10, HLIT, HDIST, HCLEN from lane 0; the code-length code's lengths from lanes 1 .. HCLEN */
			const uint32_t prev = (uint32_t)__shfl_up((int)olen, 1, 64);
			uint64_t hb = prev;
			uint32_t hn = lane <= hclen ? 3u : 0u;
			if (lane == 0) {
				hb = (STREAM ? 4u : 5u) | ((nlit - 257u) << 3) | ((ndist - 1u) << 8) | ((hclen - 4u) << 13);
				hn = 17u;
			}
			bp += wave_bits_append64(bp, hb, hn, stage, lane, put);
			for (uint32_t b0 = 0; b0 < ncls; b0 += 64) {
				uint64_t v = 0;
				uint32_t nb = 0;
				if (b0 + lane < ncls) {
					const uint32_t c = cls[b0 + lane], sym = c & 255u, cc = clc[sym];
					nb = cc >> 16;
					v = (cc & 0xFFFFu) | ((c >> 8) << nb);
					nb += sym == 16u ? 2u : (sym == 17u ? 3u : (sym == 18u ? 7u : 0u));
				}
				bp += wave_bits_append64(bp, v, nb, stage, lane, put);
			}
		} else {
#pragma unroll
			for (int k = 0; k < 5; k++) {
				uint32_t nb;
				const uint32_t s = lane + 64u * k, c = fixed_lit(s, &nb);
				code[s] = s < DFL_NLL ? (c | (nb << 16)) : 0u;
			}
			__builtin_amdgcn_wave_barrier();
			if (lane < DFL_ND)
				code[DFL_DOFF + lane] = rev_bits(lane, 5) | (5u << 16);
			__syncthreads();
			bp += wave_bits_append64(bp, STREAM ? 2u : 3u, lane == 0 ? 3u : 0u, stage, lane, put);	/* BFINAL = 1 (0 in a stream), BTYPE = 01 */
		}

		/* ---- pass 2: the tokens, 64 at a time, then end-of-block from the lane after the last one ---- */
		for (uint32_t b0 = 0; b0 <= ntok; b0 += 64) {
			uint64_t v = 0;
			uint32_t nb = 0;
			if (b0 + lane < ntok) {
				const uint32_t t = toks[b0 + lane];
				if (t & DFL_TOK_MATCH) {
					uint32_t leb, lex, deb, dex;
					const uint32_t cl = code[dfl_len_code(((t >> 16) & 255u) + 3u, &leb, &lex)];
					const uint32_t cd = code[DFL_DOFF + dfl_dist_code((t & 0x7FFFu) + 1u, &deb, &dex)];
					nb = cl >> 16;
					v = (cl & 0xFFFFu) | (lex << nb);
					nb += leb;
					v |= (uint64_t)((cd & 0xFFFFu) | (dex << (cd >> 16))) << nb;
					nb += (cd >> 16) + deb;
				} else {
					const uint32_t cl = code[t];
					v = cl & 0xFFFFu;
					nb = cl >> 16;
				}
			} else if (b0 + lane == ntok) {
				v = code[256] & 0xFFFFu;
				nb = code[256] >> 16;
			}
			bp += wave_bits_append64(bp, v, nb, stage, lane, put);
		}
		if constexpr (STREAM) {
			uint32_t bits;
			const uint32_t nb = dfl_tail_token(bp, lane, &bits);
			bp += wave_bits_append64(bp, bits, nb, stage, lane, put);
		}
		if (lane == 0) {
			if (bp & 31u)
				out[bp >> 5] = stage[0];
			body_len[ci] = (uint32_t)((bp + 7) >> 3);	/* == bytes */
		}
	}
}

__global__ __launch_bounds__(256) void gz_jobs_kernel(uint64_t src_bytes, uint32_t chunk, uint32_t n_chunks,
    const uint32_t *__restrict__ body_len, la_hash_job *__restrict__ jobs, uint32_t *__restrict__ contrib)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n_chunks)
		return;
	const uint64_t so = (uint64_t)i * chunk;
	const uint32_t n = (uint32_t)(src_bytes - so < chunk ? src_bytes - so : chunk);
	jobs[i].off = so; jobs[i].len = n; jobs[i].seed = 0;
	const uint32_t body = body_len[i] < n + 5u ? body_len[i] : n + 5u;	/* stored block: 01 LEN NLEN data */
	contrib[i] = DFL_HDR + body + 8u;
}

/* a stream's contributions: the chunk's Huffman block with its tail, or the stored block when that is no larger */
template <typename GEO>
__global__ __launch_bounds__(256) void dfl_stream_contrib_kernel(uint64_t src_bytes, uint32_t chunk, uint32_t n_chunks,
    const uint32_t *__restrict__ body_len, uint32_t *__restrict__ contrib, const dfl_span_table spans)
{
	const GEO geo(src_bytes, chunk, n_chunks, spans);
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= geo.count())
		return;
	uint64_t so;
	const uint32_t n = geo.span(i, &so);
	if (!geo.deflates(i)) {	/* (a copied chunk: its bytes) */
		contrib[i] = n;
		return;
	}
	contrib[i] = body_len[i] < n + 5u ? body_len[i] : n + 5u;
}

/* STREAM: the bodies alone, back to back (no header, no trailer; `mtime` and `crc` are not read) */
template <bool STREAM, typename GEO>
__global__ __launch_bounds__(256) void gz_pack_kernel(const uint8_t *__restrict__ src, uint64_t src_bytes,
    uint32_t chunk, uint32_t n_chunks_, uint32_t mtime, const uint8_t *__restrict__ tmp, uint32_t tmp_stride,
    const uint32_t *__restrict__ body_len, const uint32_t *__restrict__ crc, const uint64_t *__restrict__ off,
    uint8_t *__restrict__ out, uint64_t out_cap, uint64_t *__restrict__ out_bytes, const dfl_span_table spans)
{
	const GEO geo(src_bytes, chunk, n_chunks_, spans);
	const uint32_t ci = blockIdx.x, tid = threadIdx.x;
	const uint32_t n_chunks = geo.count();
	if (ci >= n_chunks)
		return;
	uint64_t so;
	const uint32_t n = geo.span(ci, &so);
	if constexpr (GEO::SPANS) {
		/* the chunk's place is its scanned offset moved to its segment's stream bytes; the segments' sizes and the total
		 * are zip_finish_kernel's to report */
		const uint64_t at = off[ci] + geo.delta[geo.tab[ci].seg & ~DFL_SPAN_COPY];
		if (at + (off[ci + 1] - off[ci]) > out_cap)
			return;
		if (!geo.deflates(ci)) {
			for (uint32_t i = tid; i < n; i += 256)
				out[at + i] = src[so + i];
			return;
		}
		out += at - off[ci];
	}
	const bool stored = body_len[ci] >= n + 5u;
	const uint32_t body = stored ? n + 5u : body_len[ci];
	const uint64_t o = off[ci];
	if constexpr (!GEO::SPANS) {
		if (ci + 1 == n_chunks && tid == 0)
			*out_bytes = off[n_chunks];
		if (off[ci + 1] > out_cap)
			return;
	}
	constexpr uint32_t HDR = STREAM ? 0u : DFL_HDR;
	const uint32_t total = DFL_HDR + body + 8u;
	if (!STREAM && tid == 0) {
		uint8_t *h = out + o;
		h[0] = 0x1f; h[1] = 0x8b; h[2] = 8; h[3] = 4;	/* FEXTRA */
		st_le32(h + 4, mtime);
		h[8] = 0; h[9] = 3;				/* XFL 0, OS = Unix (archive_write_add_filter_gzip.c:230-231) */
		h[10] = 6; h[11] = 0; h[12] = 'B'; h[13] = 'C'; h[14] = 2; h[15] = 0;
		h[16] = (uint8_t)(total - 1u); h[17] = (uint8_t)((total - 1u) >> 8);
		uint8_t *t = out + o + DFL_HDR + body;
		st_le32(t, crc[ci]);
		st_le32(t + 4, n);
	}
	uint8_t *b = out + o + HDR;
	if (stored) {
		if (tid == 0) {
			b[0] = STREAM ? 0 : 1;	/* BFINAL = 1 (0 in a stream), BTYPE = 00 */
			b[1] = (uint8_t)n; b[2] = (uint8_t)(n >> 8); b[3] = (uint8_t)~n; b[4] = (uint8_t)(~n >> 8);
		}
		for (uint32_t i = tid; i < n; i += 256)
			b[5 + i] = src[so + i];
	} else {
		const uint8_t *t = tmp + geo.tmp_at(ci, tmp_stride);
		for (uint32_t i = tid; i < body; i += 256)
			b[i] = t[i];
	}
}

struct gzc_ws {
	uint8_t *tmp;
	uint32_t *body_len, *contrib, *crc;
	la_hash_job *jobs;
	uint64_t *off;
	void *scan;
	uint32_t *toks;	/* deflate_dynamic_kernel: `chunk` tokens per wave */
};

/* the launcher's workspace on `base` (null: sizes only); returns its bytes before the scan scratch */
static uint64_t gzc_carve(gzc_ws *w, uint8_t *base, uint64_t nc, uint32_t stride, uint32_t chunk, uint32_t options)
{
	la_carve c = { base, 0 };
	w->tmp = c.take<uint8_t>(nc * stride);
	w->body_len = c.take<uint32_t>(nc);
	w->contrib = c.take<uint32_t>(nc);
	w->crc = c.take<uint32_t>(nc);
	w->jobs = c.take<la_hash_job>(nc, 16);
	w->off = c.take<uint64_t>(nc + 1);
	w->toks = c.take<uint32_t>(options == LA_GZC_DYNAMIC ? (nc < DFL_WAVES ? nc : DFL_WAVES) * chunk : 0, 16);
	w->scan = c.take<uint8_t>(0, 256);
	return c.off;
}

static uint32_t gzc_stride(uint32_t chunk) { return (dfl_body_bound(chunk) + 15u) & ~15u; }

/* the workspace one mode needs; the public function answers for the largest, LA_GZC_DYNAMIC */
uint64_t la_gzip_compress_ws_bytes(uint64_t src_bytes, uint32_t chunk, uint32_t options)
{
	if (chunk == 0)
		return 0;
	const uint64_t nc = (src_bytes + chunk - 1) / chunk;
	gzc_ws w;
	return gzc_carve(&w, nullptr, nc, gzc_stride(chunk), chunk, options) + la_scan_scratch_bytes((uint32_t)nc);
}

extern "C" uint64_t la_gpu_gzip_compress_workspace_bytes(uint64_t src_bytes, uint32_t chunk)
{
	return la_gzip_compress_ws_bytes(src_bytes, chunk, LA_GZC_DYNAMIC);
}

extern "C" uint64_t la_gpu_gzip_compress_bound(uint64_t src_bytes, uint32_t chunk)
{
	if (chunk == 0)
		return 0;
	const uint64_t nc = (src_bytes + chunk - 1) / chunk;
	return src_bytes + nc * (18u + 8u + 5u) + 64u;	/* a chunk that does not shrink is stored: 5 bytes of block header */
}

void la_launch_gzip_compress(hipStream_t s, const uint8_t *d_src, uint64_t src_bytes, uint32_t chunk, uint32_t mtime,
    uint32_t options, uint32_t framing, uint8_t *d_out, uint64_t out_cap, uint64_t *d_out_bytes, uint8_t *ws)
{
	const bool stream = framing == LA_GZC_FRAME_STREAM;
	const uint32_t nc = (uint32_t)((src_bytes + chunk - 1) / chunk);
	const uint32_t stride = gzc_stride(chunk);
	gzc_ws w;
	gzc_carve(&w, ws, nc, stride, chunk, options);
	if (nc == 0) {
		(void)hipMemsetAsync(d_out_bytes, 0, 8, s);
		return;
	}
	const dfl_span_table none = {};
	if (options == LA_GZC_STORED)	/* a body length no chunk can have: every chunk comes out stored */
		(void)hipMemsetAsync(w.body_len, 0xFF, (uint64_t)nc * 4u, s);
	else if (options == LA_GZC_DYNAMIC)
		hipLaunchKernelGGL((stream ? deflate_dynamic_kernel<true, dfl_even> : deflate_dynamic_kernel<false, dfl_even>),
		    dim3(nc < DFL_WAVES ? nc : DFL_WAVES), dim3(64), 0, s, d_src, src_bytes, chunk, nc, w.tmp, stride, w.body_len, w.toks, none);
	else
		hipLaunchKernelGGL((stream ? deflate_fixed_kernel<true, dfl_even> : deflate_fixed_kernel<false, dfl_even>), dim3(nc), dim3(64),
		    0, s, d_src, src_bytes, chunk, nc, w.tmp, stride, w.body_len, none);
	if (stream) {	/* no member, so no CRC32: the caller hashes what it frames (la_gpu_crc32_many) */
		hipLaunchKernelGGL(dfl_stream_contrib_kernel<dfl_even>, dim3((nc + 255) / 256), dim3(256), 0, s, src_bytes, chunk, nc, w.body_len, w.contrib, none);
	} else {
		hipLaunchKernelGGL(gz_jobs_kernel, dim3((nc + 255) / 256), dim3(256), 0, s, src_bytes, chunk, nc, w.body_len, w.jobs, w.contrib);
		la_launch_crc32_many(s, d_src, w.jobs, nc, w.crc);
	}
	la_launch_scan_u32(s, w.contrib, nc, w.off, w.scan);
	hipLaunchKernelGGL((stream ? gz_pack_kernel<true, dfl_even> : gz_pack_kernel<false, dfl_even>), dim3(nc), dim3(256), 0, s, d_src, src_bytes,
	    chunk, nc, mtime, w.tmp, stride, w.body_len, w.crc, w.off, d_out, out_cap, d_out_bytes, none);
}

/* ------------------------------------------------------------------ ZIP entries (la_gpu_zip_compress)
 *
 * One call, a write window of segments: the stream shape above, cut so that no chunk crosses a segment, with room for
 * what the host writes around every entry.  The chunks of all segments form one span table, built here from the
 * segment table (a count per segment, a scan, a fill), so the compress kernels run once over all of them however
 * small the entries are.  The host does not learn how many spans there are: launches are sized by the bound
 * ceil(src_bytes / chunk) + n_segs and return early above the scanned total.  A segment's stream bytes are a
 * difference of the chunk scan, so a segment without a chunk needs none; a second scan over the segments' whole
 * sizes places them.  No workgroup waits for another.
 */
#define ZIPC_FLAGS    (LA_ZIPC_LAST | LA_ZIPC_STORE)
#define ZIPC_ERR_SEG   1u	/* a segment's fields */
#define ZIPC_ERR_SPANS 2u	/* more chunks, or more room for their bodies, than segments that do not overlap can need */

struct zipc_ws {
	uint32_t *err;			/* one word, first in the workspace: la_zip_compress_check reads it */
	uint32_t *cnt;			/* [n_segs] chunks of a segment */
	uint64_t *span_off;		/* [n_segs + 1] their scan */
	dfl_span *spans;		/* [nb] */
	uint32_t *need, *body_len, *contrib;	/* [nb] */
	uint64_t *tmp_off, *off;	/* [nb + 1] scans of need, contrib */
	uint32_t *seg_bytes, *crc;	/* [n_segs] */
	uint64_t *seg_off;		/* [n_segs + 1] */
	uint64_t *delta;		/* [n_segs] */
	la_hash_job *jobs;		/* [n_segs] */
	uint32_t *toks;
	uint8_t *tmp;
	void *scan;
};

static uint64_t zipc_spans_bound(uint64_t src_bytes, uint32_t n_segs, uint32_t chunk) { return (src_bytes + chunk - 1) / chunk + n_segs; }
/* room for the Huffman bodies: every chunk takes dfl_body_bound() of its length rounded up to 16, at most 9/8 n + 32 */
static uint64_t zipc_tmp_cap(uint64_t src_bytes, uint64_t nb) { return (((src_bytes * 9u + 7u) >> 3) + 32u * nb + 15u) & ~(uint64_t)15u; }

static uint64_t zipc_carve(zipc_ws *w, uint8_t *base, uint64_t src_bytes, uint32_t n_segs, uint32_t chunk, uint32_t options)
{
	const uint64_t nb = zipc_spans_bound(src_bytes, n_segs, chunk);
	la_carve c = { base, 0 };
	w->err = c.take<uint32_t>(4);
	w->cnt = c.take<uint32_t>(n_segs);
	w->span_off = c.take<uint64_t>((uint64_t)n_segs + 1);
	w->spans = c.take<dfl_span>(nb, 16);
	w->need = c.take<uint32_t>(nb);
	w->body_len = c.take<uint32_t>(nb);
	w->contrib = c.take<uint32_t>(nb);
	w->tmp_off = c.take<uint64_t>(nb + 1);
	w->off = c.take<uint64_t>(nb + 1);
	w->seg_bytes = c.take<uint32_t>(n_segs);
	w->crc = c.take<uint32_t>(n_segs);
	w->seg_off = c.take<uint64_t>((uint64_t)n_segs + 1);
	w->delta = c.take<uint64_t>(n_segs);
	w->jobs = c.take<la_hash_job>(n_segs, 16);
	w->toks = c.take<uint32_t>(options == LA_GZC_DYNAMIC ? (nb < DFL_WAVES ? nb : DFL_WAVES) * chunk : 0, 16);
	w->tmp = c.take<uint8_t>(options == LA_GZC_STORED ? 0 : zipc_tmp_cap(src_bytes, nb), 16);
	w->scan = c.take<uint8_t>(0, 256);
	return c.off;
}

uint64_t la_zip_compress_ws_bytes(uint64_t src_bytes, uint32_t n_segs, uint32_t chunk, uint32_t options)
{
	if (chunk == 0)
		return 0;
	const uint64_t nb = zipc_spans_bound(src_bytes, n_segs, chunk);
	zipc_ws w;
	return zipc_carve(&w, nullptr, src_bytes, n_segs, chunk, options) + la_scan_scratch_bytes((uint32_t)(nb > n_segs ? nb : n_segs));
}

extern "C" uint64_t la_gpu_zip_compress_workspace_bytes(uint64_t src_bytes, uint32_t n_segs, uint32_t chunk)
{
	return la_zip_compress_ws_bytes(src_bytes, n_segs, chunk, LA_GZC_DYNAMIC);
}

extern "C" uint64_t la_gpu_zip_compress_bound(uint64_t src_bytes, uint32_t n_segs, uint32_t chunk, uint64_t gap_bytes_total)
{
	if (chunk == 0)
		return 0;
	/* a chunk that does not shrink is stored: 5 bytes of block header; 03 00 behind a last segment */
	return src_bytes + zipc_spans_bound(src_bytes, n_segs, chunk) * 5u + (uint64_t)n_segs * 2u + gap_bytes_total + 64u;
}

/* one thread per segment: its fields checked, its chunks counted, its CRC32 job */
__global__ __launch_bounds__(256) void zip_count_kernel(const la_zipc_seg *__restrict__ segs, uint32_t n_segs,
    uint64_t src_bytes, uint32_t chunk, uint32_t *__restrict__ cnt, la_hash_job *__restrict__ jobs, uint32_t *err)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n_segs)
		return;
	const la_zipc_seg g = segs[i];
	bool bad = (g.flags & ~ZIPC_FLAGS) != 0 || g.reserved != 0 || g.src_len >= 0x80000000u || g.src_off > src_bytes ||
	    g.src_len > src_bytes - g.src_off;
	const uint32_t c = bad ? 0u : (uint32_t)(((uint64_t)g.src_len + chunk - 1) / chunk);
	/* the segment's whole size is a 32-bit term of the second scan */
	bad = bad || (uint64_t)g.gap_before + g.gap_after + g.src_len + (uint64_t)c * 5u + 2u > 0xFFFFFFFFull;
	cnt[i] = bad ? 0u : c;
	jobs[i].off = bad ? 0 : g.src_off; jobs[i].len = bad ? 0u : g.src_len; jobs[i].seed = g.crc_seed;
	if (bad)
		atomicOr(err, ZIPC_ERR_SEG);
}

/* one thread per span: its segment is the one whose scanned range holds it */
__global__ __launch_bounds__(256) void zip_fill_kernel(const la_zipc_seg *__restrict__ segs, uint32_t n_segs, uint32_t chunk,
    const uint64_t *__restrict__ span_off, uint32_t nb, dfl_span *__restrict__ spans, uint32_t *__restrict__ need, uint32_t *err)
{
	const uint32_t ci = blockIdx.x * blockDim.x + threadIdx.x;
	const uint64_t total = span_off[n_segs];
	if (ci == 0 && total > nb)
		atomicOr(err, ZIPC_ERR_SPANS);
	if (ci >= nb || ci >= total)
		return;
	uint32_t lo = 0, hi = n_segs;	/* the first segment whose range starts behind ci lies in (lo, hi] */
	while (hi - lo > 1u) {
		const uint32_t mid = lo + (hi - lo) / 2u;
		if (span_off[mid] > ci) hi = mid; else lo = mid;
	}
	const la_zipc_seg g = segs[lo];
	const uint64_t k = (uint64_t)(ci - span_off[lo]) * chunk;
	dfl_span sp;
	sp.off = g.src_off + k;
	sp.len = (uint32_t)(g.src_len - k < chunk ? g.src_len - k : chunk);
	sp.seg = lo | ((g.flags & LA_ZIPC_STORE) ? DFL_SPAN_COPY : 0u);
	spans[ci] = sp;
	need[ci] = (g.flags & LA_ZIPC_STORE) ? 0u : (dfl_body_bound(sp.len) + 15u) & ~15u;
}

__global__ void zip_room_kernel(const uint64_t *__restrict__ tmp_off, uint32_t nb, uint64_t tmp_cap, uint32_t *err)
{
	if (tmp_off[nb] > tmp_cap)
		atomicOr(err, ZIPC_ERR_SPANS);
}

/* a segment's whole size: gap, stream bytes (its chunks' share of the chunk scan, and 03 00 where the entry ends), gap */
__device__ __forceinline__ uint32_t zip_stream_bytes(const la_zipc_seg &g, const uint64_t *span_off, const uint64_t *off, uint32_t i)
{
	const uint32_t body = (uint32_t)(off[span_off[i + 1]] - off[span_off[i]]);
	return body + ((g.flags & ZIPC_FLAGS) == LA_ZIPC_LAST ? 2u : 0u);
}

__global__ __launch_bounds__(256) void zip_seg_bytes_kernel(const la_zipc_seg *__restrict__ segs, uint32_t n_segs,
    const uint64_t *__restrict__ span_off, const uint64_t *__restrict__ off, uint32_t *__restrict__ seg_bytes)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n_segs)
		return;
	const la_zipc_seg g = segs[i];
	seg_bytes[i] = g.gap_before + zip_stream_bytes(g, span_off, off, i) + g.gap_after;
}

/* results, the end of an entry's stream, where the pack kernel puts a segment's chunks, the total */
__global__ __launch_bounds__(256) void zip_finish_kernel(const la_zipc_seg *__restrict__ segs, uint32_t n_segs,
    const uint64_t *__restrict__ span_off, const uint64_t *__restrict__ off, const uint64_t *__restrict__ seg_off,
    const uint32_t *__restrict__ crc, uint64_t *__restrict__ delta, la_zipc_result *__restrict__ results,
    uint8_t *__restrict__ out, uint64_t out_cap, uint64_t *__restrict__ out_bytes)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n_segs)
		return;
	const la_zipc_seg g = segs[i];
	const uint32_t len = zip_stream_bytes(g, span_off, off, i);
	const uint64_t o = seg_off[i] + g.gap_before;
	delta[i] = o - off[span_off[i]];
	results[i].out_off = o; results[i].out_len = len; results[i].crc32 = crc[i];
	if ((g.flags & ZIPC_FLAGS) == LA_ZIPC_LAST && o + len <= out_cap) {	/* the empty final fixed block */
		out[o + len - 2u] = 0x03;
		out[o + len - 1u] = 0x00;
	}
	if (i == 0)
		*out_bytes = seg_off[n_segs];
}

/* first half of the call: the span table and the checks whose answer the host waits for (4 bytes at the start of ws) */
void la_launch_zip_spans(hipStream_t s, uint64_t src_bytes, const la_zipc_seg *d_segs, uint32_t n_segs, uint32_t chunk,
    uint32_t options, uint8_t *ws)
{
	const uint32_t nb = (uint32_t)zipc_spans_bound(src_bytes, n_segs, chunk);
	zipc_ws w;
	zipc_carve(&w, ws, src_bytes, n_segs, chunk, options);
	(void)hipMemsetAsync(w.err, 0, 16, s);
	(void)hipMemsetAsync(w.need, 0, (uint64_t)nb * 4u, s);
	hipLaunchKernelGGL(zip_count_kernel, dim3((n_segs + 255) / 256), dim3(256), 0, s, d_segs, n_segs, src_bytes, chunk, w.cnt, w.jobs, w.err);
	la_launch_scan_u32(s, w.cnt, n_segs, w.span_off, w.scan);
	hipLaunchKernelGGL(zip_fill_kernel, dim3((nb + 255) / 256), dim3(256), 0, s, d_segs, n_segs, chunk, w.span_off, nb, w.spans, w.need, w.err);
	la_launch_scan_u32(s, w.need, nb, w.tmp_off, w.scan);
	hipLaunchKernelGGL(zip_room_kernel, dim3(1), dim3(1), 0, s, w.tmp_off, nb, options == LA_GZC_STORED ? ~(uint64_t)0 : zipc_tmp_cap(src_bytes, nb), w.err);
}

/* second half, for a table that passed: compress, place, pack */
void la_launch_zip_compress(hipStream_t s, const uint8_t *d_src, uint64_t src_bytes, const la_zipc_seg *d_segs, uint32_t n_segs,
    uint32_t chunk, uint32_t options, uint8_t *d_out, uint64_t out_cap, la_zipc_result *d_results, uint64_t *d_out_bytes,
    uint8_t *ws)
{
	const uint32_t nb = (uint32_t)zipc_spans_bound(src_bytes, n_segs, chunk);
	zipc_ws w;
	zipc_carve(&w, ws, src_bytes, n_segs, chunk, options);
	const dfl_span_table geo = { w.spans, w.tmp_off, w.span_off + n_segs, w.delta };
	if (options == LA_GZC_STORED)
		(void)hipMemsetAsync(w.body_len, 0xFF, (uint64_t)nb * 4u, s);
	else if (options == LA_GZC_DYNAMIC)
		hipLaunchKernelGGL((deflate_dynamic_kernel<true, dfl_spans>), dim3(nb < DFL_WAVES ? nb : DFL_WAVES), dim3(64), 0, s, d_src, src_bytes,
		    chunk, nb, w.tmp, 0u, w.body_len, w.toks, geo);
	else
		hipLaunchKernelGGL((deflate_fixed_kernel<true, dfl_spans>), dim3(nb), dim3(64), 0, s, d_src, src_bytes, chunk, nb, w.tmp, 0u, w.body_len, geo);
	(void)hipMemsetAsync(w.contrib, 0, (uint64_t)nb * 4u, s);	/* (the scan runs over the bound) */
	hipLaunchKernelGGL(dfl_stream_contrib_kernel<dfl_spans>, dim3((nb + 255) / 256), dim3(256), 0, s, src_bytes, chunk, nb, w.body_len, w.contrib, geo);
	la_launch_scan_u32(s, w.contrib, nb, w.off, w.scan);
	hipLaunchKernelGGL(zip_seg_bytes_kernel, dim3((n_segs + 255) / 256), dim3(256), 0, s, d_segs, n_segs, w.span_off, w.off, w.seg_bytes);
	la_launch_scan_u32(s, w.seg_bytes, n_segs, w.seg_off, w.scan);
	la_launch_crc32_many(s, d_src, w.jobs, n_segs, w.crc);
	hipLaunchKernelGGL(zip_finish_kernel, dim3((n_segs + 255) / 256), dim3(256), 0, s, d_segs, n_segs, w.span_off, w.off, w.seg_off,
	    w.crc, w.delta, d_results, d_out, out_cap, d_out_bytes);
	hipLaunchKernelGGL((gz_pack_kernel<true, dfl_spans>), dim3(nb), dim3(256), 0, s, d_src, src_bytes, chunk, nb, 0u, w.tmp, 0u,
	    w.body_len, (const uint32_t *)nullptr, w.off, d_out, out_cap, d_out_bytes, geo);
}
