/*
 * la_uu_dev.h -- the per-line rules of the uu read filter, stated ONCE: the kernels (la_uu.hip), the CPU stand-in of
 * the tests (tests/mock_gpu/la_gpu_uu_mock.c) and its one-core benchmark all compile this file.  Common subset of C and
 * C++.  The rules are get_line (libarchive/archive_read_support_filter_uu.c:177-209) and the four states of
 * uudecode_filter_read (uu.c:555-713); tests/uu_support.py holds the same rules in Python.
 *
 * Byte classes, as arithmetic in place of the reference's 256-byte tables: ascii[] is 0x20 .. 0x7E plus the two line-end
 * bytes, everything else is a BAD byte; uuchar[] is 0x20 .. 0x60; base64[] is A-Z a-z 0-9 + /, base64num[] their values.
 *
 * Lines.  '\n', "\r\n" and a lone '\r' each end a line (nl = 1, 2, 1); a line is its body and its line end, `len` bytes
 * in all.  A line with a bad byte anywhere in its body is a bad line, whatever else it holds.
 *
 * One line is a FUNCTION over the five states LA_UU_FIND_HEAD, _READ_UU, _UUEND, _READ_BASE64 and _STOP: three bits of
 * next state per state, 15 bits.  STOP maps to STOP.  Beside it the line carries, per live state, why it stops there
 * (LA_UU_R_*) and how many bytes it decodes to: nothing in FIND_HEAD and UUEND, the length character's count in READ_UU,
 * what the groups give in READ_BASE64.  A state that stops decodes nothing.  The record packs all of it into 64 bits:
 *   bits  0..14  next state of states 0..4        bits 27..32  bytes in READ_UU (0..63)
 *   bits 15..26  reason of states 0..3            bits 33..47  bytes in READ_BASE64 (0..24576)
 * The rules per state:
 *   FIND_HEAD    a line of LA_UU_MAX_HEAD_LINE bytes or more stops (R_TOO_LONG).  "begin " with a body of 11 characters
 *                or more, or "begin-base64 " with 18 or more, three octal digits and a space behind it: READ_UU or
 *                READ_BASE64.  Any other line stays.
 *   READ_UU      more than LA_UU_MAX_DATA_LINE bytes stops (R_TOO_LONG).  The first character must be in uuchar[];
 *                l = (c - 0x20) & 0x3f; l above the number of body characters behind it stops (a byte count held
 *                against a character count, as the reference does); l == 0 goes to UUEND; else the line needs
 *                4 (l / 3) + (l % 3 ? l % 3 + 1 : 0) characters of uuchar[] behind the first, and what follows them is
 *                ignored.  Every failure is R_BAD_LINE.
 *   UUEND        exactly the body "end" goes to FIND_HEAD; anything else stops (R_BAD_END).
 *   READ_BASE64  more than LA_UU_MAX_DATA_LINE bytes stops (R_TOO_LONG).  A body that starts with "===" goes to
 *                FIND_HEAD.  Else with p the first position that is not in base64[] (or the body's length): 3 (p / 4)
 *                bytes, plus 1 for p % 4 == 2 and 2 for p % 4 == 3; p % 4 == 1 stops, and so does a character at p that
 *                is not '=' (R_BAD_LINE).  The empty line is legal.
 *   a bad byte   stops every state: R_BAD_BYTE_HEAD in FIND_HEAD (the caller turns it into "ignore the rest" when
 *                anything was decoded), R_BAD_BYTE elsewhere.  Tested first.
 *   no line end  (nl == 0: the last line of the stream) stops FIND_HEAD, READ_UU and READ_BASE64 (R_UNTERMINATED);
 *                UUEND judges it as any other line.  Tested behind the bad byte.
 */
#ifndef LA_UU_DEV_H
#define LA_UU_DEV_H

#include "../../include/la_gpu.h"

#ifndef LA_UU_FN
#define LA_UU_FN static inline
#endif

enum {
	LA_UU_R_NONE = 0,
	LA_UU_R_BAD_BYTE_HEAD,
	LA_UU_R_BAD_BYTE,
	LA_UU_R_BAD_LINE,
	LA_UU_R_BAD_END,
	LA_UU_R_TOO_LONG,
	LA_UU_R_UNTERMINATED
};

LA_UU_FN int la_uu_is_bad(uint32_t c) { return !((c >= 0x20u && c <= 0x7Eu) || c == '\n' || c == '\r'); }
LA_UU_FN int la_uu_is_uuchar(uint32_t c) { return c >= 0x20u && c <= 0x60u; }
LA_UU_FN uint32_t la_uu_dec(uint32_t c) { return (c - 0x20u) & 0x3fu; }
LA_UU_FN int la_uu_is_b64(uint32_t c)
{
	return (c - 'A' < 26u) || (c - 'a' < 26u) || (c - '0' < 10u) || c == '+' || c == '/';
}
LA_UU_FN uint32_t la_uu_b64num(uint32_t c)
{
	return c - 'A' < 26u ? c - 'A' : c - 'a' < 26u ? c - 'a' + 26u : c - '0' < 10u ? c - '0' + 52u : c == '+' ? 62u : 63u;
}

/* 1: position i of src[0, n) ends a line.  A '\r' in the last byte ends one only when the stream ends there. */
LA_UU_FN int la_uu_is_line_end(uint32_t c, int has_next, uint32_t next, int final)
{
	if (c == '\n')
		return 1;
	if (c != '\r')
		return 0;
	return has_next ? next != '\n' : final != 0;
}

/* the identity, and the record's fields */
#define LA_UU_FN_IDENTITY ((uint64_t)(0u | 1u << 3 | 2u << 6 | 3u << 9 | 4u << 12))
LA_UU_FN uint32_t la_uu_rec_next(uint64_t rec, uint32_t state) { return (uint32_t)(rec >> (3u * state)) & 7u; }
LA_UU_FN uint32_t la_uu_rec_reason(uint64_t rec, uint32_t state) { return state < 4u ? (uint32_t)(rec >> (15u + 3u * state)) & 7u : 0u; }
LA_UU_FN uint32_t la_uu_rec_bytes(uint64_t rec, uint32_t state)
{
	return state == LA_UU_READ_UU ? (uint32_t)(rec >> 27) & 0x3fu : state == LA_UU_READ_BASE64 ? (uint32_t)(rec >> 33) & 0x7fffu : 0u;
}
/* first a, then b: the 15 function bits only */
LA_UU_FN uint32_t la_uu_compose(uint32_t a, uint32_t b)
{
	uint32_t f = 0;
	for (uint32_t s = 0; s < 5u; s++)
		f |= ((b >> (3u * ((a >> (3u * s)) & 7u))) & 7u) << (3u * s);
	return f;
}
/* what a stop means to the caller */
LA_UU_FN uint32_t la_uu_reason_status(uint32_t reason, int decoded)
{
	switch (reason) {
	case LA_UU_R_BAD_BYTE_HEAD: return decoded ? LA_ST_UU_IGNORED : LA_ST_UU_BAD_BYTE_HEAD;
	case LA_UU_R_BAD_BYTE:      return LA_ST_UU_BAD_BYTE;
	case LA_UU_R_BAD_LINE:      return LA_ST_UU_BAD_LINE;
	case LA_UU_R_BAD_END:       return LA_ST_UU_BAD_END;
	case LA_UU_R_TOO_LONG:      return LA_ST_UU_TOO_LONG;
	case LA_UU_R_UNTERMINATED:  return LA_ST_UU_UNTERMINATED;
	default:                    return LA_ST_OK;
	}
}

LA_UU_FN int la_uu_has_bad(const uint8_t *p, uint32_t n)
{
	for (uint32_t i = 0; i < n; i++)
		if (la_uu_is_bad(p[i]))
			return 1;
	return 0;
}

/* the record with state s sent to `to`, or stopped for `why` */
LA_UU_FN uint64_t la_uu_rec_go(uint64_t rec, uint32_t s, uint32_t to)
{
	return (rec & ~((uint64_t)7u << (3u * s))) | (uint64_t)to << (3u * s);
}
LA_UU_FN uint64_t la_uu_rec_stop(uint64_t rec, uint32_t s, uint32_t why)
{
	return la_uu_rec_go(rec, s, LA_UU_STOP) | (uint64_t)why << (15u + 3u * s);
}

LA_UU_FN int la_uu_prefix(const uint8_t *b, const char *lit, uint32_t n)
{
	for (uint32_t i = 0; i < n; i++)
		if (b[i] != (uint8_t)lit[i])
			return 0;
	return 1;
}

/* uu.c:565-574: 6 or 13 when the body is a header line, else 0 */
LA_UU_FN uint32_t la_uu_header_kind(const uint8_t *b, uint32_t body)
{
	uint32_t l = 0;
	if (body >= 11u && la_uu_prefix(b, "begin ", 6u))
		l = 6u;
	else if (body >= 18u && la_uu_prefix(b, "begin-base64 ", 13u))
		l = 13u;
	if (l != 0 && b[l] >= '0' && b[l] <= '7' && b[l + 1] >= '0' && b[l + 1] <= '7' && b[l + 2] >= '0' && b[l + 2] <= '7' && b[l + 3] == ' ')
		return l;
	return 0;
}

/* characters a uuencode line of l bytes needs behind its length character */
LA_UU_FN uint32_t la_uu_chars_needed(uint32_t l)
{
	return 4u * (l / 3u) + (l % 3u ? l % 3u + 1u : 0u);
}

/* The record of the line p[0, len), its line end of nl bytes (0: the stream ended first) included; has_bad: a bad byte
 * stands in its body (la_uu_has_bad(p, len - nl), or what the caller knows). */
LA_UU_FN uint64_t la_uu_line_record(const uint8_t *p, uint32_t len, uint32_t nl, int has_bad)
{
	const uint32_t body = len - nl;
	uint64_t rec = LA_UU_FN_IDENTITY;
	uint32_t i;
	if (has_bad) {
		rec = la_uu_rec_stop(rec, LA_UU_FIND_HEAD, LA_UU_R_BAD_BYTE_HEAD);
		rec = la_uu_rec_stop(rec, LA_UU_READ_UU, LA_UU_R_BAD_BYTE);
		rec = la_uu_rec_stop(rec, LA_UU_UUEND, LA_UU_R_BAD_BYTE);
		return la_uu_rec_stop(rec, LA_UU_READ_BASE64, LA_UU_R_BAD_BYTE);
	}
	/* UUEND, uu.c:658-667 */
	if (body == 3u && p[0] == 'e' && p[1] == 'n' && p[2] == 'd')
		rec = la_uu_rec_go(rec, LA_UU_UUEND, LA_UU_FIND_HEAD);
	else
		rec = la_uu_rec_stop(rec, LA_UU_UUEND, LA_UU_R_BAD_END);
	if (nl == 0) {
		rec = la_uu_rec_stop(rec, LA_UU_FIND_HEAD, LA_UU_R_UNTERMINATED);
		rec = la_uu_rec_stop(rec, LA_UU_READ_UU, LA_UU_R_UNTERMINATED);
		return la_uu_rec_stop(rec, LA_UU_READ_BASE64, LA_UU_R_UNTERMINATED);
	}
	/* FIND_HEAD, uu.c:557-602 */
	if (len >= LA_UU_MAX_HEAD_LINE)
		rec = la_uu_rec_stop(rec, LA_UU_FIND_HEAD, LA_UU_R_TOO_LONG);
	else {
		const uint32_t kind = la_uu_header_kind(p, body);
		if (kind)
			rec = la_uu_rec_go(rec, LA_UU_FIND_HEAD, kind == 6u ? LA_UU_READ_UU : LA_UU_READ_BASE64);
	}
	if (len > LA_UU_MAX_DATA_LINE) {
		rec = la_uu_rec_stop(rec, LA_UU_READ_UU, LA_UU_R_TOO_LONG);
		return la_uu_rec_stop(rec, LA_UU_READ_BASE64, LA_UU_R_TOO_LONG);
	}
	/* READ_UU, uu.c:603-657 */
	{
		const uint32_t first = body ? p[0] : 0u;	/* (0 is not in uuchar[]) */
		const uint32_t l = la_uu_dec(first), need = la_uu_chars_needed(l);
		int ok = la_uu_is_uuchar(first) && l <= body - 1u && need <= body - 1u;
		if (ok && l != 0)
			for (i = 1; i <= need; i++)
				ok &= la_uu_is_uuchar(p[i]);
		if (!ok)
			rec = la_uu_rec_stop(rec, LA_UU_READ_UU, LA_UU_R_BAD_LINE);
		else if (l == 0)
			rec = la_uu_rec_go(rec, LA_UU_READ_UU, LA_UU_UUEND);
		else
			rec |= (uint64_t)l << 27;
	}
	/* READ_BASE64, uu.c:668-712 */
	if (body >= 3u && p[0] == '=' && p[1] == '=' && p[2] == '=')
		return la_uu_rec_go(rec, LA_UU_READ_BASE64, LA_UU_FIND_HEAD);
	i = 0;
	while (i < body && la_uu_is_b64(p[i]))
		i++;
	{
		const uint32_t stopper = i < body ? p[i] : (uint32_t)'=';	/* (the body's end stops the groups as '=' does) */
		if ((i & 3u) == 1u || stopper != (uint32_t)'=')
			return la_uu_rec_stop(rec, LA_UU_READ_BASE64, LA_UU_R_BAD_LINE);
	}
	return rec | (uint64_t)(3u * (i >> 2) + ((i & 3u) ? (i & 3u) - 1u : 0u)) << 33;
}

/* n bytes of a uuencode line that passed: p is the line (its length character first) */
LA_UU_FN void la_uu_decode_uu(const uint8_t *p, uint32_t n, uint8_t *out)
{
	const uint8_t *b = p + 1;
	while (n > 0) {
		uint32_t v = la_uu_dec(b[0]) << 18 | la_uu_dec(b[1]) << 12;
		*out++ = (uint8_t)(v >> 16);
		if (--n == 0)
			break;
		v |= la_uu_dec(b[2]) << 6;
		*out++ = (uint8_t)(v >> 8);
		if (--n == 0)
			break;
		v |= la_uu_dec(b[3]);
		*out++ = (uint8_t)v;
		--n;
		b += 4;
	}
}

/* n bytes of a base64 line that passed */
LA_UU_FN void la_uu_decode_b64(const uint8_t *b, uint32_t n, uint8_t *out)
{
	while (n > 0) {
		uint32_t v = la_uu_b64num(b[0]) << 18 | la_uu_b64num(b[1]) << 12;
		*out++ = (uint8_t)(v >> 16);
		if (--n == 0)
			break;
		v |= la_uu_b64num(b[2]) << 6;
		*out++ = (uint8_t)(v >> 8);
		if (--n == 0)
			break;
		v |= la_uu_b64num(b[3]);
		*out++ = (uint8_t)v;
		--n;
		b += 4;
	}
}

LA_UU_FN void la_uu_decode_line(const uint8_t *p, uint32_t state, uint32_t n, uint8_t *out)
{
	if (state == LA_UU_READ_UU)
		la_uu_decode_uu(p, n, out);
	else
		la_uu_decode_b64(p, n, out);
}

#endif
