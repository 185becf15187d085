/*
 * la_gpu_uu_mock.c -- TEST INFRASTRUCTURE: a CPU stand-in for la_gpu_uu_decode as include/la_gpu.h words it, so that
 * the host side (la_filter_uu.c: bidder, windows, the carried tail line, verdicts, read_header) is tested without a GPU.
 *
 * The per-line rules are NOT restated here: this file compiles libarchive_amd/csrc/la_uu_dev.h, the header the kernels
 * compile, and walks the window's lines one after the other where the device scans.  The tests also call the entry
 * directly, with host pointers, and la_uu_rules_line to hold the header against the Python oracle line by line.
 */
#include "../../include/la_gpu.h"
#include <string.h>

#include "../../libarchive_amd/csrc/la_uu_dev.h"

uint64_t la_gpu_uu_workspace_bytes(uint64_t src_bytes) { (void)src_bytes; return 0; }

/* One line under one state: the record of the header, its next state, reason and byte count; decodes into out when the
 * line produces bytes.  Returns the record. */
uint64_t la_uu_rules_line(const uint8_t *p, uint32_t len, uint32_t nl, uint32_t state, uint32_t *next, uint32_t *reason, uint32_t *bytes,
    uint8_t *out)
{
	const uint64_t rec = la_uu_line_record(p, len, nl, la_uu_has_bad(p, len - nl));
	*next = la_uu_rec_next(rec, state);
	*reason = la_uu_rec_reason(rec, state);
	*bytes = la_uu_rec_bytes(rec, state);
	if (*bytes && out)
		la_uu_decode_line(p, state, *bytes, out);
	return rec;
}

/* the walk alone, over host pointers (the one-core benchmark calls it too) */
void la_uu_rules_walk(const uint8_t *src, uint64_t n, int final, la_uu_state in, uint8_t *dst, la_uu_result *r)
{
	uint64_t pos = 0, out = 0;
	uint32_t state = in.state;
	memset(r, 0, sizeof(*r));
	while (pos < n) {
		/* the line from pos on: up to the first byte that ends one */
		uint64_t e = pos;
		while (e < n && !la_uu_is_line_end(src[e], e + 1 < n, e + 1 < n ? src[e + 1] : 0, final))
			e++;
		uint32_t nl = 0;
		if (e < n) {
			nl = src[e] == '\n' && e > pos && src[e - 1] == '\r' ? 2u : 1u;
			e++;
		} else if (!final)
			break;
		const uint32_t len = (uint32_t)(e - pos);
		const uint64_t rec = la_uu_line_record(src + pos, len, nl, la_uu_has_bad(src + pos, len - nl));
		const uint32_t next = la_uu_rec_next(rec, state);
		if (next == LA_UU_STOP) {
			r->status = la_uu_reason_status(la_uu_rec_reason(rec, state), in.decoded || out != 0);
			state = LA_UU_STOP;
			break;
		}
		const uint32_t bytes = la_uu_rec_bytes(rec, state);
		if (bytes)
			la_uu_decode_line(src + pos, state, bytes, dst + out);
		out += bytes;
		if (state == LA_UU_FIND_HEAD && next != LA_UU_FIND_HEAD) {
			r->n_headers++;
			r->head_off = pos;
			r->head_len = len;
		}
		state = next;
		pos = e;
	}
	r->state = state;
	r->decoded = in.decoded || out != 0;
	r->out_len = out;
	r->consumed = r->stop_off = pos;
}

int la_gpu_uu_decode(la_gpu_ctx *c, const la_uu_batch *bt)
{
	(void)c;
	if (!bt || bt->reserved || !bt->d_result || bt->src_bytes > LA_UU_MAX_SRC_BYTES || bt->in.state > LA_UU_READ_BASE64)
		return LA_ERR_ARG;
	if (bt->src_bytes && (!bt->d_src || !bt->d_dst || bt->dst_cap < bt->src_bytes))
		return LA_ERR_ARG;
	la_uu_rules_walk(bt->d_src, bt->src_bytes, bt->final != 0, bt->in, bt->d_dst, bt->d_result);
	return LA_OK;
}
