/*
 * la_gpu_zip_mock.c -- TEST INFRASTRUCTURE: la_gpu_zip_compress of include/la_gpu.h on the CPU, through zlib, beside
 * la_gpu_mock.c (which has the rest of the ABI; "device" memory is host memory there).  It keeps the
 * call's contract -- layout, gaps left alone, results, errors -- not the device's bytes: a deflated segment is one
 * raw-deflate stream with a Z_SYNC_FLUSH behind every chunk and 03 00 where the entry ends, so matches may cross
 * chunks and a chunk may cost a few bytes more than on the device.  Its bound is its own.
 *
 * LA_MOCK_ZIP_FAIL_CALL=n makes the n-th call (from 1, counted while the variable is set and since
 * la_gpu_zip_mock_reset()) fail as a device call would.
 */
#include "../../include/la_gpu.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <zlib.h>

struct la_gpu_ctx { char err[64]; };	/* la_gpu_mock.c's */

static unsigned long zip_calls;
void la_gpu_zip_mock_reset(void) { zip_calls = 0; }

uint64_t la_gpu_zip_compress_workspace_bytes(uint64_t s, uint32_t n, uint32_t c) { (void)s; (void)n; (void)c; return 0; }

uint64_t la_gpu_zip_compress_bound(uint64_t src_bytes, uint32_t n_segs, uint32_t chunk, uint64_t gap_bytes_total)
{
	if (chunk == 0)
		return 0;
	/* zlib: 5 bytes per stored block of at most 16 KiB or so, 5 per flush marker, a few bits of block header */
	return src_bytes + src_bytes / 1024 * 8 + ((src_bytes + chunk - 1) / chunk + n_segs) * 32u + gap_bytes_total + 64u;
}

int la_gpu_zip_compress(la_gpu_ctx *c, const la_zipc_batch *bt)
{
	if (!c || !bt || !bt->d_out_bytes || (bt->n_segs && (!bt->d_segs || !bt->d_results || !bt->d_out)) || (bt->src_bytes && !bt->d_src))
		return LA_ERR_ARG;
	if (bt->chunk_bytes == 0 || bt->chunk_bytes > 49152u || bt->options > LA_GZC_STORED || bt->reserved != 0)
		return LA_ERR_ARG;
	const char *fail = getenv("LA_MOCK_ZIP_FAIL_CALL");
	if (fail && ++zip_calls == strtoul(fail, NULL, 10)) {
		snprintf(c->err, sizeof(c->err), "mock: injected failure of call %lu", zip_calls);
		return LA_ERR_HIP;
	}
	for (uint32_t i = 0; i < bt->n_segs; i++) {
		const la_zipc_seg *g = &bt->d_segs[i];
		if ((g->flags & ~(LA_ZIPC_LAST | LA_ZIPC_STORE)) || g->reserved || g->src_len >= 0x80000000u || g->src_off > bt->src_bytes ||
		    g->src_len > bt->src_bytes - g->src_off)
			return LA_ERR_ARG;
	}
	uint64_t at = 0;
	for (uint32_t i = 0; i < bt->n_segs; i++) {
		const la_zipc_seg *g = &bt->d_segs[i];
		const uint8_t *in = g->src_len ? bt->d_src + g->src_off : (const uint8_t *)"";
		la_zipc_result *r = &bt->d_results[i];
		at += g->gap_before;
		r->out_off = at;
		r->crc32 = (uint32_t)crc32(g->crc_seed, in, g->src_len);
		uint64_t len = 0;
		if (g->flags & LA_ZIPC_STORE) {
			len = g->src_len;
			if (at + len <= bt->out_cap)
				memcpy(bt->d_out + at, in, g->src_len);
		} else {
			z_stream z;
			memset(&z, 0, sizeof(z));
			if (deflateInit2(&z, bt->options == LA_GZC_STORED ? 0 : 6, Z_DEFLATED, -15, 8,
			    bt->options == LA_GZC_FIXED ? Z_FIXED : Z_DEFAULT_STRATEGY) != Z_OK)
				return LA_ERR_NOMEM;
			uint8_t sink[256];
			for (uint32_t done = 0; done < g->src_len; ) {
				const uint32_t n = g->src_len - done < bt->chunk_bytes ? g->src_len - done : bt->chunk_bytes;
				z.next_in = (Bytef *)(uintptr_t)(in + done); z.avail_in = n;
				do {	/* what does not fit is counted and dropped */
					const int fits = at + len < bt->out_cap;
					z.next_out = fits ? bt->d_out + at + len : sink;
					z.avail_out = fits ? (uInt)(bt->out_cap - at - len < 0x10000 ? bt->out_cap - at - len : 0x10000) : (uInt)sizeof(sink);
					const uInt room = z.avail_out;
					deflate(&z, Z_SYNC_FLUSH);
					len += room - z.avail_out;
				} while (z.avail_out == 0);
				done += n;
			}
			deflateEnd(&z);
			if (g->flags & LA_ZIPC_LAST) {
				if (at + len + 2 <= bt->out_cap) {
					bt->d_out[at + len] = 0x03;
					bt->d_out[at + len + 1] = 0x00;
				}
				len += 2;
			}
		}
		r->out_len = (uint32_t)len;
		at += len + g->gap_after;
	}
	*bt->d_out_bytes = at;
	return LA_OK;
}
