/*
 * la_gpu_lzip_mock.c -- TEST INFRASTRUCTURE: a CPU stand-in for la_gpu_lzip_scan and la_gpu_lzip_decode as
 * include/la_gpu.h words them, so that the host side (la_filter_lzip.c: the chain of members, windows, held-back bytes,
 * verdicts) is tested without a GPU.  Linked beside la_gpu_mock.c.
 *
 * The decode rules are NOT restated here: this file compiles libarchive_amd/csrc/la_lzip_dev.h (and through it
 * la_xz_dev.h's symbol loop), the headers the kernel compiles, one member after the other.  What the kernel adds around
 * the header (the refused entry, the CRC into the result) is repeated below in the kernel's order.  CRC32 is zlib's.
 * The tests also call la_gpu_lzip_decode here directly, with host pointers, to hold the rules against liblzma.
 */
#include "../../include/la_gpu.h"
#include <stdlib.h>
#include <string.h>
#include <zlib.h>

#define LA_XZ_FN static inline
#include "../../libarchive_amd/csrc/la_lzip_dev.h"

uint64_t la_gpu_lzip_workspace_bytes(uint32_t n) { (void)n; return 0; }

int la_gpu_lzip_scan(la_gpu_ctx *c, const uint8_t *d_src, uint64_t src_bytes, uint64_t *d_offs, uint32_t cap, uint32_t *d_count)
{
	(void)c;
	if (!d_count || (src_bytes && !d_src) || (cap && !d_offs))
		return LA_ERR_ARG;
	uint64_t count = 0;
	for (uint64_t i = 0; i + 6 <= src_bytes; i++) {
		if (!la_lzip_header_shape(d_src + i))
			continue;
		if (count < cap)
			d_offs[count] = i;
		count++;
	}
	*d_count = count > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)count;
	return LA_OK;
}

int la_gpu_lzip_decode(la_gpu_ctx *c, const la_lzip_batch *bt)
{
	(void)c;
	if (!bt || bt->reserved || (bt->n && (!bt->d_members || !bt->d_results || !bt->d_dst || (bt->src_bytes && !bt->d_src))))
		return LA_ERR_ARG;
	uint16_t *probs = malloc(sizeof(uint16_t) * LA_LZIP_PROBS);
	if (!probs)
		return LA_ERR_NOMEM;
	for (uint32_t b = 0; b < bt->n; b++) {
		const la_lzip_member m = bt->d_members[b];
		la_lzip_result r;
		la_xz_lzma lz;
		memset(&r, 0, sizeof(r));
		if (!la_lzip_entry_ok(&m, bt->src_bytes, bt->dst_cap)) {
			r.status = LA_ST_LZIP_REFUSED;
			bt->d_results[b] = r;
			continue;
		}
		uint8_t *out = bt->d_dst + m.dst_off;
		la_lzip_member_decode(bt->d_src, bt->src_bytes, &m, out, probs, &lz, &r);
		r.crc32 = (uint32_t)crc32(0, out, (uInt)r.out_len);
		r.status = la_lzip_crc_verdict(&m, r.status, r.crc32);
		bt->d_results[b] = r;
	}
	free(probs);
	return LA_OK;
}
