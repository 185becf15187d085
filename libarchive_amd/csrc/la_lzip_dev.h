/*
 * la_lzip_dev.h -- what the lzip format (version 0 and 1 members) and liblzma 5.2's raw LZMA1 decoder say about one
 * member's LZMA stream, stated ONCE: the kernel (la_lzip.hip), the CPU stand-in of the tests (tests/mock_lzip) and its
 * sanitizer program all compile this file.  The LZMA symbol loop itself is la_xz_dev.h's (la_xz_lzma_run): this file is
 * its second caller and adds no second copy of it.  Common subset of C and C++; LA_XZ_FN as in la_xz_dev.h.
 *
 * The rules (lzma_decoder.c, lz_decoder.c; where the format text and liblzma differ, liblzma is pinned, because the
 * filter has to give liblzma's bytes and verdicts):
 *   header   "LZIP", version 0 or 1, a dictionary byte b with 12 <= (b & 31) <= 29.  The dictionary size is
 *            1 << (b & 31), less (size / 16) * (b >> 5) when the exponent is above 12 (xz.c:557-563).
 *   model    lc 3, lp 0, pb 2, fixed: 1846 + 768 * 8 probabilities.  There is no chunk layer and no reset.
 *   init     the range decoder reads 5 bytes; the first has to be 0, else LA_ST_LZIP_DATA with nothing written (the
 *            liblzma pinned here refuses it in its raw LZMA1 decoder as it does in an LZMA2 chunk).
 *   bits     normalise BEFORE every bit.
 *   distance a match, rep or short rep whose distance is not below min(bytes so far, la_xz_dict_cap(dictionary size))
 *            is LA_ST_LZIP_DATA.
 *   end      a match with distance 0xFFFFFFFF, whatever its length, is the end-of-payload marker.  Behind it liblzma
 *            normalises once more (a byte it needs there is part of the stream) and the code has to be 0, else
 *            LA_ST_LZIP_DATA.  Bytes behind the marker are the trailer's business, not the stream's.
 *   limits   the source ends at src_lim and asking for src[src_lim] is lim_status; the output ends at cap and a symbol
 *            that does not fit in front of it is cap_status -- tested when the symbol is known, so a stream whose
 *            marker follows exactly cap bytes ends well.
 * A symbol is written only when all of it could be decoded (a match that meets cap is copied up to it), so on every
 * failure out_len is the count of valid bytes: what liblzma has emitted when it stops in the same place.
 */
#ifndef LA_LZIP_DEV_H
#define LA_LZIP_DEV_H

#include "la_xz_dev.h"

#define LA_LZIP_PROBS (LA_XZ_P_LITERAL + (768u << 3))	/* 7990 entries, 15 980 bytes */

/* 1: p[0, 6) has the shape of a member header (xz.c:343-374) */
LA_XZ_FN int la_lzip_header_shape(const uint8_t *p)
{
	return p[0] == 'L' && p[1] == 'Z' && p[2] == 'I' && p[3] == 'P' && p[4] <= 1u && (p[5] & 31u) >= 12u && (p[5] & 31u) <= 29u;
}

/* xz.c:557-563 */
LA_XZ_FN uint32_t la_lzip_dict_size(uint32_t b)
{
	const uint32_t log2dic = b & 31u;
	uint32_t size = 1u << log2dic;
	if (log2dic > 12u)
		size -= (size / 16u) * (b >> 5);
	return size;
}

/* One member's stream: src[src_off, src_lim) into dst[0, cap).  probs holds LA_LZIP_PROBS entries.  Fills status
 * (LA_ST_OK: the marker was found and the code behind it is 0), out_len, consumed (through the marker; what was read so
 * far on a failure) and valid; crc32 is the caller's. */
LA_XZ_FN void la_lzip_stream_decode(const uint8_t *src, uint64_t src_off, uint64_t src_lim, uint32_t lim_status, uint8_t *dst, uint64_t cap,
    uint32_t cap_status, uint32_t dict_size, uint16_t *probs, la_xz_lzma *lz, la_lzip_result *res)
{
	uint64_t p = src_off, pos = 0;
	uint32_t ended = 0;
	lz->lc = 3; lz->lp = 0; lz->pb = 2;
	la_xz_lzma_reset(lz, probs);
	uint32_t st = la_xz_lzma_run(lz, probs, src, &p, src_lim, 0, lim_status, dst, &pos, cap, 0, 0, la_xz_dict_cap(dict_size), 1, cap_status,
	    &ended);
	if (st == LA_ST_XZ_DATA || st == LA_ST_XZ_LZMA)
		st = LA_ST_LZIP_DATA;
	res->status = st;
	res->crc32 = 0;
	res->out_len = pos;
	res->consumed = p - src_off;
	res->valid = pos;
}

/* 1: the entry may be decoded: it points inside both buffers and one hash job can carry its bytes */
LA_XZ_FN int la_lzip_entry_ok(const la_lzip_member *m, uint64_t src_bytes, uint64_t dst_total)
{
	if (m->src_off > src_bytes || m->dst_off > dst_total || m->dst_cap > dst_total - m->dst_off || m->dst_cap > LA_XZ_DST_CAP_MAX)
		return 0;
	if (m->src_end != LA_LZIP_UNKNOWN && (m->src_end < m->src_off || m->src_end > src_bytes))
		return 0;
	if (m->data_size != LA_LZIP_UNKNOWN && m->data_size > m->dst_cap)
		return 0;
	return 1;
}

/* The member's stream under its entry's bounds, then what the tentative ends say about a stream that ended well.
 * The CRC is compared by the caller once it has it (la_lzip_crc_verdict). */
LA_XZ_FN void la_lzip_member_decode(const uint8_t *src, uint64_t src_bytes, const la_lzip_member *m, uint8_t *dst, uint16_t *probs,
    la_xz_lzma *lz, la_lzip_result *res)
{
	const int ended = m->src_end != LA_LZIP_UNKNOWN, sized = m->data_size != LA_LZIP_UNKNOWN;
	la_lzip_stream_decode(src, m->src_off, ended ? m->src_end : src_bytes, ended ? (uint32_t)LA_ST_LZIP_SRC_END : (uint32_t)LA_ST_LZIP_TRUNCATED,
	    dst, sized ? m->data_size : m->dst_cap, sized ? (uint32_t)LA_ST_LZIP_SIZE_OVER : (uint32_t)LA_ST_LZIP_OUT_FULL, m->dict_size, probs, lz,
	    res);
	if (res->status == LA_ST_OK && ended && m->src_off + res->consumed != m->src_end)
		res->status = LA_ST_LZIP_EARLY_END;
	if (res->status == LA_ST_OK && sized && res->out_len != m->data_size)
		res->status = LA_ST_LZIP_BAD_SIZE;
}

LA_XZ_FN uint32_t la_lzip_crc_verdict(const la_lzip_member *m, uint32_t status, uint32_t crc)
{
	return status == LA_ST_OK && (m->flags & LA_LZIP_HAS_CRC) && crc != m->crc32 ? (uint32_t)LA_ST_LZIP_BAD_CRC : status;
}

#endif
