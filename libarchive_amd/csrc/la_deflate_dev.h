/*
 * la_deflate_dev.h -- what RFC 1951 and zlib 1.2.11 say about a deflate block header, stated ONCE for the
 * two inflate kernels (la_inflate.hip: one wave per member; la_inflate_lanes.hip: one lane per member), and with
 * them the two rules a PIECE of a stream adds.
 * The written statement of the rules is oracle/orc_inflate.c; this is its device form.  Include after la_dev.h.
 *
 * Here: the code-length order, the fixed code's lengths, the length / distance symbol arithmetic, the verdict on
 * a built code, and the header walks (stored: LEN / NLEN; dynamic: HLIT to lens[256]) as templates over a READER
 * that each kernel supplies.  Bit readers, table builders, symbol loops, literal / sequence emission, match
 * copies and the stored block's byte copy stay in the kernels: that is where they differ on purpose.
 *
 * A reader R is a thin adapter over the kernel's own machinery:
 *   bool     take(uint32_t n, uint32_t &v)   the next n <= 32 bits, first bit lowest; false: the input ended
 *   void     to_byte()                       drop the bits up to the next byte boundary
 *   void     store(idx, val, rep)            lens[idx .. idx + rep) = val
 *   uint32_t len_at(idx)                     lens[idx]
 *   int      clc_build(uint32_t &maxlen)     build the code-length code from lens[0..19); returns what the
 *                                            builders return (0 complete, >0 incomplete, <0 over-subscribed)
 *   int      clc_sym()                       next code-length symbol; -1: the input ended, -2: unassigned code
 *
 * The order of verdicts the walks guarantee (which one wins when two apply is part of the result: the filter
 * delivers the bytes before the error and the reference's string):
 *   stored   1. LA_ST_GZ_TRUNCATED  LEN / NLEN not all there
 *            2. LA_ST_GZ_DATA       LEN != ~NLEN
 *            (then the kernel: LA_ST_GZ_OUT_FULL, the byte copy, LA_ST_GZ_TRUNCATED for a short body)
 *   dynamic  1. LA_ST_GZ_TRUNCATED  the 14 bits of HLIT / HDIST / HCLEN not all there
 *            2. LA_ST_GZ_DATA       HLIT > 286 or HDIST > 30
 *            3. LA_ST_GZ_TRUNCATED  inside the HCLEN code-length-code lengths
 *            4. LA_ST_GZ_DATA       code-length code over-subscribed, or incomplete and not all-zero
 *            5. per code length, in stream order: LA_ST_GZ_TRUNCATED (the symbol's bits), LA_ST_GZ_DATA
 *               (unassigned code), LA_ST_GZ_TRUNCATED (a repeat's extra bits) BEFORE LA_ST_GZ_DATA (16 with
 *               nothing before it), LA_ST_GZ_DATA (repeat past HLIT + HDIST)
 *            6. LA_ST_GZ_DATA       no end-of-block code (lens[256] == 0)
 *            (then the kernel builds the literal/length code, then the distance code: dfl_code_verdict each)
 *
 * Pieces (LA_GZ_OPT_PIECES, a template parameter of the kernels: the other builds do not hold a byte of it).  A
 * span that claims to start on a byte-aligned block boundary is decoded like a member, with two rules more:
 *   end      behind a block WITHOUT BFINAL, and BEFORE the next three header bits are asked for: when not one bit
 *            of the span is unread -- none pending in the current byte, the byte cursor on src_len -- the piece
 *            is over, LA_ST_GZ_PIECE_END (dfl_piece_end).  A block that ends mid-byte on the span's last byte
 *            leaves padding bits unread: no piece end, the header read runs out of input as it always did.
 *   history  a distance that reaches in front of the piece's first output byte is LA_ST_GZ_NEEDS_HISTORY, not
 *            LA_ST_GZ_DATA (dfl_far_back): the bytes it points at exist, in the piece before.
 *
 * A chain (LA_GZ_OPT_CHAIN on top of the pieces, a second template parameter of the wave kernel only).  The pieces are
 * decoded as ONE stream: a distance may reach over the piece's first byte into the packed bytes of the pieces before
 * it and then into the hist_len bytes the caller put in front of the chain.  The kernel copies no match (it writes
 * one source pointer per byte, la_inflate_chain.hip follows them), so the only rule left is zlib's own:
 *   too far  a distance above (bytes of this piece so far) + (packed bytes in front of the piece) + hist_len is
 *            LA_ST_GZ_DATA (dfl_chain_too_far), "invalid distance too far back"; LA_ST_GZ_NEEDS_HISTORY does not occur.
 */
#ifndef LA_DEFLATE_DEV_H
#define LA_DEFLATE_DEV_H

static __device__ __constant__ uint8_t dfl_clc_order[19] = { 16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15 };

/* the fixed code: 288 literal/length lengths (8 / 9 / 7 / 8), then 32 distance lengths of 5 */
__device__ __forceinline__ uint32_t dfl_fixed_len(int i)
{
	return i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5;
}

/* length / distance symbol -> base value and extra bits, by arithmetic (RFC 1951 3.2.5): no table in memory,
 * a divergent table read (lane kernel) or a scalar memory round trip in the middle of the serial chain (wave
 * kernel) costs more than these few operations.  false: a symbol the format does not have (length symbols
 * 286 / 287, i.e. sy 29 / 30; distance symbols 30 / 31) */
__device__ __forceinline__ bool dfl_len_sym(uint32_t sy, uint32_t &base, uint32_t &extra)
{
	extra = sy < 8 ? 0u : sy == 28 ? 0u : (sy - 4) >> 2;
	base = sy < 8 ? 3u + sy : sy == 28 ? 258u : ((4u + (sy & 3u)) << extra) + 3u;
	return sy < 29;
}
__device__ __forceinline__ bool dfl_dist_sym(uint32_t ds, uint32_t &base, uint32_t &extra)
{
	extra = ds < 4 ? 0u : (ds >> 1) - 1u;
	base = ds < 4 ? ds + 1u : ((2u + (ds & 1u)) << extra) + 1u;
	return ds < 30;
}

/* The verdict on a built code.  `left` is what the builders return, maxlen the longest code length.  zlib 1.2.11
 * lets an incomplete code through only so: literal/length when its longest code is 1 bit, distance when it is at
 * most 1 bit (an empty distance code is fine: a block of literals), the code-length code never -- except the
 * all-zero one, which it reads as one-bit "length 0" symbols (dfl_dynamic_header). */
enum dfl_code_kind { DFL_CODE_LITLEN, DFL_CODE_DIST, DFL_CODE_CLEN };
__device__ __forceinline__ uint32_t dfl_code_verdict(int left, uint32_t maxlen, dfl_code_kind kind)
{
	if (left == 0)
		return LA_ST_OK;
	if (left < 0)
		return LA_ST_GZ_DATA;
	const bool ok = kind == DFL_CODE_LITLEN ? maxlen == 1 : kind == DFL_CODE_DIST ? maxlen <= 1 : maxlen == 0;
	return ok ? LA_ST_OK : LA_ST_GZ_DATA;
}

/* The end-of-piece rule, behind a block without BFINAL.  unread_bits: the bits of the span [src_off, src_off +
 * src_len) that the kernel's bit reader has not handed out -- those in its buffer that came from inside the span
 * plus eight per byte the cursor has not fetched. */
template <bool PIECES>
__device__ __forceinline__ bool dfl_piece_end(int64_t unread_bits)
{
	return PIECES && unread_bits == 0;
}
/* The end-of-piece rule of a piece that starts at a BIT (LA_GZ_OPT_BLOCK_STARTS; a third template parameter of the wave
 * kernel), tested at the same place as dfl_piece_end and beside it.  starts[0 .. n) are bit offsets from the span's first
 * byte, ascending: the candidate block starts (la_deflate_find_dev.h), or the confirmed ones.  cursor is the bit the next
 * block header would be read from.  The piece is over when a start behind its own lies exactly on the cursor; idx walks up
 * the table as the cursor advances (it begins one above the piece's own entry), so a start the piece passed in mid-block
 * is stepped over and never looked at again. */
template <bool BITS>
__device__ __forceinline__ bool dfl_piece_end_at(uint32_t cursor, const uint32_t *starts, uint32_t n, uint32_t &idx)
{
	if (!BITS)
		return false;
	while (idx < n && starts[idx] < cursor)
		idx++;
	return idx < n && starts[idx] == cursor;
}
/* the verdict on a match distance above the bytes produced so far */
template <bool PIECES>
__device__ __forceinline__ uint32_t dfl_far_back() { return PIECES ? LA_ST_GZ_NEEDS_HISTORY : LA_ST_GZ_DATA; }

/* chain mode: in_front = packed bytes of the earlier pieces + hist_len (below 2^32 with op: la_api.hip checks the batch) */
__device__ __forceinline__ bool dfl_chain_too_far(uint32_t dist, uint32_t op, uint32_t in_front)
{
	return (uint64_t)dist > (uint64_t)op + in_front;
}

/* stored block, behind the three header bits: to the byte boundary, LEN against ~NLEN */
template <class R>
__device__ __forceinline__ uint32_t dfl_stored_header(R &r, uint32_t &len)
{
	r.to_byte();
	uint32_t v;
	if (!r.take(32, v))
		return LA_ST_GZ_TRUNCATED;
	len = v & 0xFFFFu;
	return len == ((v >> 16) ^ 0xFFFFu) ? LA_ST_OK : LA_ST_GZ_DATA;
}

/* dynamic block, behind the three header bits: HLIT / HDIST / HCLEN, the code-length code, the nlen + ndist
 * code lengths into lens[0 .. nlen + ndist) */
template <class R>
__device__ __forceinline__ uint32_t dfl_dynamic_header(R &r, int &nlen, int &ndist)
{
	uint32_t v;
	if (!r.take(14, v))
		return LA_ST_GZ_TRUNCATED;
	nlen = (int)(v & 31u) + 257;
	ndist = (int)((v >> 5) & 31u) + 1;
	const int ncode = (int)(v >> 10) + 4;
	if (nlen > 286 || ndist > 30)
		return LA_ST_GZ_DATA;
	r.store(0, 0, 19);
	for (int i = 0; i < ncode; i++) {
		if (!r.take(3, v))
			return LA_ST_GZ_TRUNCATED;
		r.store(dfl_clc_order[i], v, 1);
	}
	/* from here on lens[] is overwritten in place: the code-length code is built */
	uint32_t clmax;
	const int left = r.clc_build(clmax);
	if (dfl_code_verdict(left, clmax, DFL_CODE_CLEN) != LA_ST_OK)
		return LA_ST_GZ_DATA;
	const int total = nlen + ndist;
	int idx = 0;
	uint32_t prev = 0;
	if (clmax == 0) {
		/* zlib 1.2.11: an all-zero code-length code yields one-bit "length 0" symbols (and the missing
		 * end-of-block code is caught below) */
		for (; idx < total; idx++) {
			if (!r.take(1, v))
				return LA_ST_GZ_TRUNCATED;
			r.store(idx, 0, 1);
		}
	}
	while (idx < total) {
		const int sym = r.clc_sym();
		if (sym == -1)
			return LA_ST_GZ_TRUNCATED;
		if (sym < 0)
			return LA_ST_GZ_DATA;
		if (sym < 16) {
			r.store(idx, (uint32_t)sym, 1);
			prev = (uint32_t)sym;
			idx++;
			continue;
		}
		/* 16: the previous length 3..6 times; 17: zero 3..10 times; 18: zero 11..138 times */
		if (!r.take(sym == 16 ? 2u : sym == 17 ? 3u : 7u, v))
			return LA_ST_GZ_TRUNCATED;
		if (sym == 16 && idx == 0)
			return LA_ST_GZ_DATA;
		const uint32_t val = sym == 16 ? prev : 0u;
		const int rep = (sym == 18 ? 11 : 3) + (int)v;
		if (idx + rep > total)
			return LA_ST_GZ_DATA;
		r.store(idx, val, rep);
		prev = val;
		idx += rep;
	}
	return r.len_at(256) == 0 ? LA_ST_GZ_DATA : LA_ST_OK;
}

#endif
