/*
 * la_inflate.hip -- raw DEFLATE decode for batches of independent gzip members
 * (gfx950).  Replaces the zlib inflate() loop of gzip_filter_read
 * (libarchive/archive_read_support_filter_gzip.c:431-511, inflateInit2(-15)
 * at :363) for a whole table of members per launch, and adds the trailer
 * CRC32/ISIZE check the reference leaves as a TODO (gzip.c:423).
 *
 * One WAVE per member.  A deflate stream is a serial bit chain, so the wave
 * keeps the chain wave-uniform (bit buffer and positions in SGPRs, fed from a
 * 512-byte register window of the compressed bytes via v_readlane) and uses
 * its lanes where the format allows it:
 *   - Huffman tables live in LDS (per wave: 10-bit lit/len and 8-bit distance
 *     lookup tables plus the canonical count/symbol arrays for longer codes);
 *   - literals are gathered in a 64-entry lane buffer and stored 64 at a time;
 *   - match copies are wave-wide (64 bytes per step) with the same
 *     store->load visibility rule as the general LZ4 kernel.
 * Accept/reject rules follow zlib 1.2.11 (oracle/orc_inflate.c); the block-header rules are stated in
 * la_deflate_dev.h, shared with la_inflate_lanes.hip, and read here through `wave_reader`.
 * Byte/integer work; no MFMA.
 *
 * Speed (one 64 KiB member, ms): 21.8 at first -- the bit reader and the window lived in SCRATCH memory
 * because inflate_codes() was an out-of-line function taking them by reference (scratch_load /
 * scratch_store + s_waitcnt vmcnt(0) on every refill); inlined: 9.1.  Length / distance bases by
 * arithmetic instead of constant-table loads and no division for non-overlapping copies: see
 * DESIGN.md §5.  What is left (ISA of this build): the chain state (bit buffer, bit count, byte cursor,
 * the decoded symbol) still sits in VGPRs and every uniform `if` is an exec-mask sequence (about 900
 * s_and_saveexec in the kernel against a dozen s_cbranch_scc): the compiler's uniformity analysis loses
 * the state somewhere; readfirstlane on the member record, on the slow-path LDS loads and on maxlen did
 * not bring it back, and forcing it (readfirstlane on the whole chain state once per symbol: 43 scalar
 * branches instead of 7) made the kernel 7 % slower -- so the exec-mask form is not what the ~1 800
 * cycles per symbol are made of either, and neither are the table builds (huff_build inlined, no scratch
 * left: 9.08 against 9.16 ms).  Cycle counters in the diagnostic build (tools/exp_inflate_stamps.py, zlib -6
 * members of the bench stream): 24 216 symbols per 64 KiB member of which 2 251 matches, 930 cycles per
 * symbol; literal/length decode with refill 357 per symbol (38 %), literal bookkeeping 244 per symbol (26 %),
 * length + distance decode 1 074 per match (11 %), flush + copy 648 per match (6.5 %), block headers and
 * table builds 18 %.  Nine symbols in ten are literals at ~600 cycles each: two literals per table look
 * (pair table) and a chain that really lives in SGPRs are what to build next.  Tried and not kept: the output in a 64 KiB LDS ring per wave (match copies LDS to
 * LDS, 16-byte drains to the slab) instead of store / fence / load through global memory: 9.8 ms for one
 * member and, with only two waves per CU, 77.6 instead of 12.5 ms for 4 096 members.
 */
#include "la_dev.h"
#include "la_deflate_dev.h"

/* Diagnostic build only (make diag, -DLA_DIAG): per-member cycle totals of the symbol loop's parts go to a
 * buffer of their own (8 x u64 per member); no output value depends on them. */
#ifdef LA_DIAG
__device__ unsigned long long *la_inf_diag;
extern "C" int la_diag_set_inflate_stamps(void *d_buf)
{
	unsigned long long *p = (unsigned long long *)d_buf;
	return (int)hipMemcpyToSymbol(HIP_SYMBOL(la_inf_diag), &p, sizeof(p));
}
struct inf_diag { unsigned long long t, acc[8]; };
#define DIAG_DECL      inf_diag DG = {}
#define DIAG_ARG       , inf_diag &DG
#define DIAG_PASS      , DG
#define DIAG_T0()      (DG.t = __builtin_readcyclecounter())
#define DIAG_ACC(k)    do { unsigned long long n_ = __builtin_readcyclecounter(); DG.acc[k] += n_ - DG.t; DG.t = n_; } while (0)
#define DIAG_CNT(k)    (DG.acc[k] += 1)
#else
#define DIAG_DECL      do { } while (0)
#define DIAG_ARG
#define DIAG_PASS
#define DIAG_T0()      do { } while (0)
#define DIAG_ACC(k)    do { } while (0)
#define DIAG_CNT(k)    do { } while (0)
#endif

#define INF_WAVES_PER_WG 4
#define LL_FAST_BITS 10
#define D_FAST_BITS  8

struct inf_tables {	/* one per wave, in LDS */
	uint16_t ll_fast[1 << LL_FAST_BITS];	/* (symbol << 4) | length, 0 = long code / unassigned */
	uint16_t d_fast[1 << D_FAST_BITS];
	uint16_t ll_count[16], d_count[16];
	uint16_t ll_symbol[288], d_symbol[32];
	uint8_t  lens[320];
	uint16_t ll_maxlen, d_maxlen;
};

struct bitreader {
	uint64_t hold;
	int bits;
	const uint8_t *ip, *iend;
	src_window W;
};

__device__ __forceinline__ void br_refill(bitreader &B, int lane)
{
	if (B.bits <= 32) {
		int nbytes = (int)(B.iend - B.ip);
		if (nbytes > 4) nbytes = 4;
		if (nbytes > 0) {
			uint32_t v = win_u32(B.W, B.ip, lane);
			if (nbytes < 4)
				v &= (1u << (8 * nbytes)) - 1u;
			B.hold |= (uint64_t)v << B.bits;
			B.bits += 8 * nbytes;
			B.ip += nbytes;
		}
	}
}
__device__ __forceinline__ bool br_need(bitreader &B, int n, int lane)
{
	br_refill(B, lane);
	return B.bits >= n;
}
__device__ __forceinline__ uint32_t br_take(bitreader &B, int n)
{
	uint32_t v = (uint32_t)(B.hold & ((1ull << n) - 1ull));
	B.hold >>= n;
	B.bits -= n;
	return v;
}

__device__ __forceinline__ uint32_t bitrev(uint32_t v, int n) { return __builtin_bitreverse32(v) >> (32 - n); }

/*
 * Canonical Huffman table from lens[0..n): counts, sorted symbols and the fast
 * lookup table.  All lanes run it redundantly on uniform values; lane 0 stores.
 * Returns 0 complete, >0 incomplete, <0 over-subscribed.
 */
__device__ int huff_build(const uint8_t *lens, int n, uint16_t *count, uint16_t *symbol,
    uint16_t *fast, int fast_bits, uint16_t *maxlen_out, int lane)
{
	uint32_t cnt[16];
	for (int l = 0; l < 16; l++) cnt[l] = 0;
	/* lane-parallel histogram */
	for (int i = lane; i < n; i += LA_WAVE) {
		int l = lens[i];
		for (int k = 1; k < 16; k++) cnt[k] += (l == k);
	}
	int left = 1, maxlen = 0;
	uint32_t offs[16], code[16];
	offs[0] = 0; offs[1] = 0; code[0] = 0;
	uint32_t c = 0;
	for (int l = 1; l < 16; l++) {
		uint32_t t = cnt[l];
		for (int d = 32; d >= 1; d >>= 1) t += __shfl_xor(t, d, 64);
		cnt[l] = t;
		if (t) maxlen = l;
		left = left * 2 - (int)t;
		if (left < 0) left = -100000;	/* stays negative */
	}
	for (int l = 1; l < 16; l++) {
		c = (c + (l > 1 ? cnt[l - 1] : 0)) << 1;
		code[l] = c;
		if (l < 15) offs[l + 1] = offs[l] + cnt[l];
	}
	if (lane == 0) {
		for (int l = 0; l < 16; l++) count[l] = (uint16_t)cnt[l];
		*maxlen_out = (uint16_t)maxlen;
	}
	for (int i = lane; i < (1 << fast_bits); i += LA_WAVE)
		fast[i] = 0;
	if (left < 0)
		return -1;
	/* sorted symbol list and fast table: serial in symbol order (stable), lane 0 */
	if (lane == 0) {
		uint32_t next_off[16], next_code[16];
		for (int l = 0; l < 16; l++) { next_off[l] = offs[l]; next_code[l] = code[l]; }
		for (int s = 0; s < n; s++) {
			int l = lens[s];
			if (l == 0) continue;
			symbol[next_off[l]++] = (uint16_t)s;
			uint32_t cw = next_code[l]++;
			if (l <= fast_bits) {
				uint32_t r = bitrev(cw, l);
				uint16_t e = (uint16_t)((s << 4) | l);
				for (uint32_t idx = r; idx < (1u << fast_bits); idx += (1u << l))
					fast[idx] = e;
			}
		}
	}
	return left;
}

/* decode one symbol: >= 0 symbol, -1 input exhausted, -2 unassigned code */
__device__ __forceinline__ int huff_decode(bitreader &B, const uint16_t *fast, int fast_bits,
    const uint16_t *count, const uint16_t *symbol, int maxlen, int lane)
{
	br_refill(B, lane);
	uint32_t e = fast[(uint32_t)B.hold & ((1u << fast_bits) - 1u)];
	e = (uint32_t)__builtin_amdgcn_readfirstlane((int)e);
	int l = (int)(e & 15);
	if (l != 0) {
		if (l > B.bits)
			return -1;
		B.hold >>= l;
		B.bits -= l;
		return (int)(e >> 4);
	}
	/* long or unassigned code: canonical walk, one bit at a time */
	int codev = 0, first = 0, index = 0;
	int ml = maxlen ? maxlen : 1;
	for (int k = 1; k <= ml; k++) {
		if (B.bits < 1) {
			br_refill(B, lane);
			if (B.bits < 1)
				return -1;
		}
		codev |= (int)(B.hold & 1);
		B.hold >>= 1;
		B.bits -= 1;
		int cn = count[k];
		if (codev - cn < first)
			return symbol[index + (codev - first)];
		index += cn;
		first += cn;
		first <<= 1;
		codev <<= 1;
	}
	return -2;
}

struct out_state {
	uint8_t *d;
	uint32_t op, cap;
	uint32_t visible;	/* bytes [0, visible) are known visible to this wave's loads */
	uint32_t npend;		/* literals waiting in the lane buffer */
	uint32_t litbuf;	/* lane i holds pending literal i */
};

__device__ __forceinline__ void out_flush(out_state &O, int lane)
{
	if (O.npend) {
		if ((uint32_t)lane < O.npend)
			O.d[O.op + lane] = (uint8_t)O.litbuf;
		O.op += O.npend;
		O.npend = 0;
	}
}

/*
 * Chain mode (LA_GZ_OPT_CHAIN, the rule is in la_deflate_dev.h): a second template parameter, so the other instances
 * do not hold a byte of it.  The pieces are decoded TWICE by instances of this kernel, a scan between them:
 *   LA_CHAIN_MEASURE  the entropy decode alone: nothing is stored but the piece's result (out_len bounded by the
 *                     piece's dst_cap, consumed, status); no distance is judged, the piece's place is not known yet;
 *   LA_CHAIN_EMIT     with the packed place of the piece (exclusive scan of the measured out_len): literals and stored
 *                     bytes go straight to their packed place, and for EVERY byte one source pointer goes to the
 *                     pointer table -- itself for a literal, the byte the match names for a match byte.  No match is
 *                     copied and nothing is read back from the output: la_inflate_chain.hip follows the pointers.
 * Coordinates: byte k of the chain (history included) is hist_len + its packed position; X.in_front is that of the
 * piece's first byte.  A wave writes only inside [packed offset, + measured out_len) of the output and of the pointer
 * table: the emit pass takes the measured length as its capacity, so a decode that came out longer the second time
 * (it cannot: same bytes, same code) would end in LA_ST_GZ_OUT_FULL, never in a store outside.
 */
enum { LA_CHAIN_OFF = 0, LA_CHAIN_MEASURE = 1, LA_CHAIN_EMIT = 2 };

struct chain_out {
	uint32_t *ptr;		/* pointer table entry of the piece's first byte */
	uint32_t in_front;	/* hist_len + packed bytes in front of the piece */
};

template <int CHAIN>
__device__ __forceinline__ void flush_lits(out_state &O, const chain_out &X, int lane)
{
	if constexpr (CHAIN == LA_CHAIN_OFF)
		out_flush(O, lane);
	else if constexpr (CHAIN == LA_CHAIN_EMIT) {
		if (O.npend) {
			if ((uint32_t)lane < O.npend) {
				O.d[O.op + lane] = (uint8_t)O.litbuf;
				X.ptr[O.op + lane] = X.in_front + O.op + lane;
			}
			O.op += O.npend;
			O.npend = 0;
		}
	}
	/* (LA_CHAIN_MEASURE counts its literals in O.op at once: nothing is ever pending) */
}

/* returns LA_ST_OK, LA_ST_GZ_DATA, LA_ST_GZ_TRUNCATED or LA_ST_GZ_OUT_FULL (PIECES without CHAIN: or LA_ST_GZ_NEEDS_HISTORY) */
template <bool PIECES, int CHAIN>
__device__ __forceinline__ uint32_t inflate_codes(bitreader &B, out_state &O, const chain_out &X, const inf_tables *T, int lane DIAG_ARG)
{
	for (;;) {
		DIAG_T0();
		int sym = huff_decode(B, T->ll_fast, LL_FAST_BITS, T->ll_count, T->ll_symbol, T->ll_maxlen, lane);
		DIAG_ACC(0); DIAG_CNT(6);
		if (sym == -1) return LA_ST_GZ_TRUNCATED;
		if (sym < 0) return LA_ST_GZ_DATA;
		if (sym < 256) {
			if (O.op + O.npend >= O.cap) return LA_ST_GZ_OUT_FULL;
			if constexpr (CHAIN == LA_CHAIN_MEASURE) {
				O.op++;
				continue;
			}
			if ((uint32_t)lane == O.npend)
				O.litbuf = (uint32_t)sym;
			O.npend++;
			if (O.npend == LA_WAVE)
				flush_lits<CHAIN>(O, X, lane);
			DIAG_ACC(1);
			continue;
		}
		if (sym == 256)
			return LA_ST_OK;
		sym -= 257;
		uint32_t bs, xb;
		if (!dfl_len_sym((uint32_t)sym, bs, xb)) return LA_ST_GZ_DATA;
		if (!br_need(B, (int)xb, lane)) return LA_ST_GZ_TRUNCATED;
		uint32_t length = bs + br_take(B, (int)xb);
		int ds = huff_decode(B, T->d_fast, D_FAST_BITS, T->d_count, T->d_symbol, T->d_maxlen, lane);
		if (ds == -1) return LA_ST_GZ_TRUNCATED;
		if (ds < 0 || !dfl_dist_sym((uint32_t)ds, bs, xb)) return LA_ST_GZ_DATA;
		if (!br_need(B, (int)xb, lane)) return LA_ST_GZ_TRUNCATED;
		uint32_t dist = bs + br_take(B, (int)xb);
		DIAG_ACC(2); DIAG_CNT(7);
		flush_lits<CHAIN>(O, X, lane);
		if constexpr (CHAIN == LA_CHAIN_OFF) {
			if (dist > O.op) return dfl_far_back<PIECES>();
		} else if constexpr (CHAIN == LA_CHAIN_EMIT) {
			if (dfl_chain_too_far(dist, O.op, X.in_front)) return LA_ST_GZ_DATA;
		}
		if (O.op + length > O.cap) return LA_ST_GZ_OUT_FULL;
		if constexpr (CHAIN != LA_CHAIN_OFF) {
			if constexpr (CHAIN == LA_CHAIN_EMIT) {
				/* the source of byte j: where the wave-wide copy below would read it (the modulo form names a
				 * byte in front of the match at once, not the byte `dist` back that is itself a copy) */
				const uint32_t from = X.in_front + O.op - dist;
				if (dist >= length) {
					for (uint32_t j = (uint32_t)lane; j < length; j += LA_WAVE)
						X.ptr[O.op + j] = from + j;
				} else {
					for (uint32_t j = (uint32_t)lane; j < length; j += LA_WAVE)
						X.ptr[O.op + j] = from + j % dist;
				}
			}
			O.op += length;
			continue;
		}
		/* wave-wide copy; the modulo form only reads bytes below op */
		uint32_t span = length < dist ? length : dist;
		if (O.op - dist + span > O.visible) {
			wave_mem_fence();
			O.visible = O.op;
		}
		if (dist >= length) {	/* (wave-uniform) no overlap: no division */
			for (uint32_t j = (uint32_t)lane; j < length; j += LA_WAVE)
				O.d[O.op + j] = O.d[O.op - dist + j];
		} else {
			for (uint32_t j = (uint32_t)lane; j < length; j += LA_WAVE)
				O.d[O.op + j] = O.d[O.op - dist + j % dist];
		}
		O.op += length;
		DIAG_ACC(3);
	}
}

/* the block-header walks of la_deflate_dev.h over this kernel's bit reader and LDS tables.  All lanes hold the
 * same values; lens[] is written by lane 0, or by up to three lane-strided stores for a repeat (<= 138).  The
 * code-length code borrows the distance table's slots (19 symbols, codes of <= 7 bits). */
struct wave_reader {
	bitreader &B;
	inf_tables *T;
	int lane;
	int cl_max;
	__device__ __forceinline__ bool take(uint32_t n, uint32_t &v)
	{
		/* (n == 32: br_refill tops up to MORE than 32 bits whenever four bytes are left, and fewer are
		 * left for good when it does not) */
		if (!br_need(B, (int)n, lane))
			return false;
		v = br_take(B, (int)n);
		return true;
	}
	__device__ __forceinline__ void to_byte() { br_take(B, B.bits & 7); }
	__device__ __forceinline__ void store(uint32_t idx, uint32_t val, uint32_t rep)
	{
		if ((uint32_t)lane < rep) T->lens[idx + lane] = (uint8_t)val;
		if (rep > 64 && (uint32_t)lane + 64 < rep) T->lens[idx + lane + 64] = (uint8_t)val;
		if (rep > 128 && (uint32_t)lane + 128 < rep) T->lens[idx + lane + 128] = (uint8_t)val;
	}
	__device__ __forceinline__ uint32_t len_at(uint32_t idx) { return T->lens[idx]; }
	__device__ __forceinline__ int clc_build(uint32_t &maxlen)
	{
		const int e = huff_build(T->lens, 19, T->d_count, T->d_symbol, T->d_fast, D_FAST_BITS, &T->d_maxlen, lane);
		cl_max = __builtin_amdgcn_readfirstlane((int)T->d_maxlen);
		maxlen = (uint32_t)cl_max;
		return e;
	}
	__device__ __forceinline__ int clc_sym()
	{
		return huff_decode(B, T->d_fast, D_FAST_BITS, T->d_count, T->d_symbol, cl_max, lane);
	}
};

/* PIECES: the members are pieces of one raw-deflate stream (LA_GZ_OPT_PIECES; the rules are in la_deflate_dev.h);
 * CHAIN: see above (C is read by the chain instances only);
 * BITS (LA_GZ_OPT_BLOCK_STARTS, chain instances only; the other instances do not hold a byte of it): members[0] is ONE
 * span and piece mi starts at bit C.starts[mi] of it, of *C.n_starts pieces (n bounds that number: the grid was sized
 * before the device knew it).  The piece ends as dfl_piece_end_at says, and consumed is reported in bits. */
template <bool PIECES, int CHAIN, bool BITS = false>
__global__ __launch_bounds__(64 * INF_WAVES_PER_WG) void inflate_kernel(const uint8_t *__restrict__ src,
    uint64_t src_bytes, const la_gz_member *__restrict__ members, uint32_t n, uint8_t *dst,
    uint64_t dst_cap, la_gz_result *__restrict__ results, la_inflate_chain C)
{
	static_assert(!BITS || (PIECES && CHAIN != LA_CHAIN_OFF), "bit-granular pieces exist in chain mode only");
	__shared__ inf_tables tabs[INF_WAVES_PER_WG];
	const int lane = threadIdx.x & 63;
	const int wv = threadIdx.x >> 6;
	const uint32_t mi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * INF_WAVES_PER_WG + wv));
	if (mi >= n)
		return;
	uint32_t n_starts = 0, next_start = 0, start_bit = 0;
	if constexpr (BITS) {
		const uint32_t n_pieces = (uint32_t)__builtin_amdgcn_readfirstlane((int)*C.n_starts);
		if (mi >= n_pieces)
			return;
		/* (the table may name one start more than there are pieces: the piece the walk stopped in front of) */
		n_starts = (uint32_t)__builtin_amdgcn_readfirstlane((int)*C.n_table);
		if (n_starts > n + 1)
			n_starts = n + 1;
		start_bit = (uint32_t)__builtin_amdgcn_readfirstlane((int)C.starts[mi]);
		next_start = mi + 1;
	}
	inf_tables *T = &tabs[wv];
	la_gz_member m = members[BITS ? 0 : mi];
	/* (the first byte of the span; m becomes the piece: the span from the byte that holds its first bit) */
	const uint64_t span_off = m.src_off;
	if constexpr (BITS) {
		const uint32_t skip = start_bit >> 3 < m.src_len ? start_bit >> 3 : m.src_len;
		m.src_off += skip;
		m.src_len -= skip;
	}
	uint32_t status = LA_ST_OK;
	DIAG_DECL;
#ifdef LA_DIAG
	const unsigned long long dg_start = __builtin_readcyclecounter();
#endif
	bitreader B;
	B.hold = 0; B.bits = 0;
	B.ip = src + m.src_off;
	B.iend = B.ip + m.src_len;
	if (m.src_off + m.src_len > src_bytes)
		B.iend = src + src_bytes;
	B.W.limit = src + src_bytes;
	win_reset(B.W, B.ip, lane);
	out_state O;
	O.op = 0; O.visible = 0; O.npend = 0; O.litbuf = 0;
	chain_out X = { nullptr, 0 };
	if constexpr (CHAIN == LA_CHAIN_OFF) {
		O.d = dst + m.dst_off;
		O.cap = m.dst_cap;
		if (m.dst_off + m.dst_cap > dst_cap)
			O.cap = m.dst_off < dst_cap ? (uint32_t)(dst_cap - m.dst_off) : 0;
	} else if constexpr (CHAIN == LA_CHAIN_MEASURE) {
		O.d = nullptr;
		O.cap = m.dst_cap;
	} else {
		/* the packed place: [first piece's dst_off + scan, + measured length), inside dst_cap bytes from the first
		 * piece's dst_off or not written at all */
		const uint32_t measured = results[mi].out_len;
		const uint64_t at = C.packed_off[mi];
		if (at + measured > dst_cap) {
			if (lane == 0) {
				results[mi].status = LA_ST_GZ_OUT_FULL;
				results[mi].out_len = 0;
			}
			return;
		}
		O.d = dst + members[0].dst_off + at;
		O.cap = measured;
		X.ptr = C.ptr + at;
		X.in_front = C.hist_len + (uint32_t)at;
	}

	wave_reader R = { B, T, lane, 0 };
	if constexpr (BITS) {
		/* the bits of the first byte in front of the piece belong to the block before it */
		if (br_need(B, (int)(start_bit & 7u), lane))
			br_take(B, (int)(start_bit & 7u));
	}
	for (;;) {
		if (!br_need(B, 3, lane)) { status = LA_ST_GZ_TRUNCATED; break; }
		int last = (int)br_take(B, 1);
		int type = (int)br_take(B, 2);
		if (type == 0) {
			uint32_t len;
			status = dfl_stored_header(R, len);
			if (status != LA_ST_OK) break;
			flush_lits<CHAIN>(O, X, lane);
			/* whole bytes still in the bit buffer go back to the byte stream */
			B.ip -= B.bits >> 3;
			B.bits = 0; B.hold = 0;
			uint32_t avail = (uint32_t)(B.iend - B.ip);
			uint32_t take = len < avail ? len : avail;
			if (O.op + take > O.cap) { status = LA_ST_GZ_OUT_FULL; break; }
			if constexpr (CHAIN != LA_CHAIN_MEASURE) {
				for (uint32_t j = (uint32_t)lane; j < take; j += LA_WAVE)
					O.d[O.op + j] = B.ip[j];
			}
			if constexpr (CHAIN == LA_CHAIN_EMIT) {
				for (uint32_t j = (uint32_t)lane; j < take; j += LA_WAVE)
					X.ptr[O.op + j] = X.in_front + O.op + j;
			}
			O.op += take;
			B.ip += take;
			if (take < len) { status = LA_ST_GZ_TRUNCATED; break; }
			/* the cursor stepped BACK over the whole bytes of the bit buffer: when the window had just slid it
			 * can now lie up to 4 bytes in front of it, and win_u32 only looks forward (a distance of -4..-1
			 * wraps to one it takes for a hit) */
			if (B.ip < B.W.base)
				win_reset(B.W, B.ip, lane);
		} else if (type == 1 || type == 2) {
			int nlen = 288, ndist = 32;
			if (type == 1) {
				for (int i = lane; i < 320; i += LA_WAVE)
					T->lens[i] = (uint8_t)dfl_fixed_len(i);
			} else {
				status = dfl_dynamic_header(R, nlen, ndist);
				if (status != LA_ST_OK) break;
			}
			int e = huff_build(T->lens, nlen, T->ll_count, T->ll_symbol, T->ll_fast, LL_FAST_BITS, &T->ll_maxlen, lane);
			int llm = __builtin_amdgcn_readfirstlane((int)T->ll_maxlen);
			status = dfl_code_verdict(e, (uint32_t)llm, DFL_CODE_LITLEN);
			if (status != LA_ST_OK) break;
			e = huff_build(T->lens + nlen, ndist, T->d_count, T->d_symbol, T->d_fast, D_FAST_BITS, &T->d_maxlen, lane);
			int dm = __builtin_amdgcn_readfirstlane((int)T->d_maxlen);
			status = dfl_code_verdict(e, (uint32_t)dm, DFL_CODE_DIST);
			if (status != LA_ST_OK) break;
			status = inflate_codes<PIECES, CHAIN>(B, O, X, T, lane DIAG_PASS);
			if (status != LA_ST_OK) break;
		} else {
			status = LA_ST_GZ_DATA;
			break;
		}
		if (last)
			break;
		/* (the bit buffer only ever holds bytes from inside the span, and behind a stored block it is empty
		 * with the cursor stepped back: both counts are exact here) */
		if (dfl_piece_end<PIECES>((int64_t)B.bits + 8 * (int64_t)(B.iend - B.ip))) {
			status = LA_ST_GZ_PIECE_END;
			if constexpr (BITS)
				next_start = 0xFFFFFFFFu;
			break;
		}
		if constexpr (BITS) {
			/* (below 2^32: la_api.hip refuses a source of 2^29 bytes or more) */
			const uint32_t cursor = (uint32_t)(8 * (int64_t)(B.ip - (src + span_off)) - (int64_t)B.bits);
			if (dfl_piece_end_at<BITS>(cursor, C.starts, n_starts, next_start)) {
				status = LA_ST_GZ_PIECE_END;
				break;
			}
		}
	}
	/* what zlib would have emitted before noticing: whole symbols, stored data bytewise */
	if constexpr (CHAIN == LA_CHAIN_OFF) {
		if (status != LA_ST_GZ_OUT_FULL)
			out_flush(O, lane);
	} else if constexpr (CHAIN == LA_CHAIN_EMIT) {
		/* (a literal is only taken while op + npend < cap: the pending ones always fit) */
		flush_lits<CHAIN>(O, X, lane);
		/* a piece that ends here in front of its measured length (a distance too far back): the rest of its
		 * range names itself, so that every pointer of the packed range is one the passes may follow */
		for (uint32_t j = O.op + (uint32_t)lane; j < O.cap; j += LA_WAVE)
			X.ptr[j] = X.in_front + j;
	}
#ifdef LA_DIAG
	if (lane == 0 && la_inf_diag) {
		for (int k = 0; k < 8; k++)
			la_inf_diag[(size_t)mi * 8 + k] = DG.acc[k];
		la_inf_diag[(size_t)mi * 8 + 4] = __builtin_readcyclecounter() - dg_start;	/* whole member */
	}
#endif
	uint32_t consumed = (uint32_t)(B.ip - (src + m.src_off)) - (uint32_t)(B.bits >> 3);
	if (lane == 0) {
		la_gz_result r;
		r.status = status;
		r.out_len = O.op;
		r.consumed = consumed;
		r.crc32 = 0;
		if constexpr (BITS) {
			r.consumed = (uint32_t)(8 * (int64_t)(B.ip - (src + span_off)) - (int64_t)B.bits);
			r.crc32 = next_start;
		}
		results[mi] = r;
	}
}

void la_launch_inflate(hipStream_t s, const uint8_t *d_src, uint64_t src_bytes,
    const la_gz_member *d_members, uint32_t n, uint8_t *d_dst, uint64_t dst_cap, la_gz_result *d_results, bool pieces)
{
	if (n == 0) return;
	const auto kernel = pieces ? inflate_kernel<true, LA_CHAIN_OFF> : inflate_kernel<false, LA_CHAIN_OFF>;
	hipLaunchKernelGGL(kernel, dim3((n + INF_WAVES_PER_WG - 1) / INF_WAVES_PER_WG),
	    dim3(64 * INF_WAVES_PER_WG), 0, s, d_src, src_bytes, d_members, n, d_dst, dst_cap, d_results, la_inflate_chain{});
}

/* the two chain instances: emit = false measures (C is not read), emit = true writes bytes and pointers */
void la_launch_inflate_chain(hipStream_t s, const uint8_t *d_src, uint64_t src_bytes, const la_gz_member *d_members,
    uint32_t n, uint8_t *d_dst, uint64_t dst_cap, la_gz_result *d_results, const la_inflate_chain &C, bool emit)
{
	if (n == 0) return;
	const auto kernel = emit ? inflate_kernel<true, LA_CHAIN_EMIT> : inflate_kernel<true, LA_CHAIN_MEASURE>;
	hipLaunchKernelGGL(kernel, dim3((n + INF_WAVES_PER_WG - 1) / INF_WAVES_PER_WG),
	    dim3(64 * INF_WAVES_PER_WG), 0, s, d_src, src_bytes, d_members, n, d_dst, dst_cap, d_results, C);
}

/* the chain instances for pieces that start at a bit (LA_GZ_OPT_BLOCK_STARTS): n_max waves, of which *C.n_starts work */
void la_launch_inflate_chain_bits(hipStream_t s, const uint8_t *d_src, uint64_t src_bytes, const la_gz_member *d_span,
    uint32_t n_max, uint8_t *d_dst, uint64_t dst_cap, la_gz_result *d_results, const la_inflate_chain &C, bool emit)
{
	if (n_max == 0) return;
	const auto kernel = emit ? inflate_kernel<true, LA_CHAIN_EMIT, true> : inflate_kernel<true, LA_CHAIN_MEASURE, true>;
	hipLaunchKernelGGL(kernel, dim3((n_max + INF_WAVES_PER_WG - 1) / INF_WAVES_PER_WG),
	    dim3(64 * INF_WAVES_PER_WG), 0, s, d_src, src_bytes, d_span, n_max, d_dst, dst_cap, d_results, C);
}
