/*
 * la_gpu_lzop_mock.c -- TEST INFRASTRUCTURE: a CPU stand-in for la_gpu_lzop_decode and la_gpu_adler32_many as
 * include/la_gpu.h words them, so that the host side (la_filter_lzop.c: the walk over headers and block infos, windows,
 * verdicts) is tested without a GPU.  Linked beside la_gpu_mock.c.
 *
 * The LZO1X rules are NOT restated here: this file compiles libarchive_amd/csrc/la_lzo_dev.h, the header the kernel
 * compiles, with its plain hooks, one block after the other.  What the kernel adds around the header (the refused
 * entry, the two sums and their order) is repeated below in the kernel's order.  CRC32 and Adler-32 are zlib's.  The
 * tests also call la_gpu_lzop_decode here directly, with host pointers, to hold the rules against the Python decoder.
 */
#include "../../include/la_gpu.h"
#include <string.h>
#include <zlib.h>

#include "../../libarchive_amd/csrc/la_lzo_dev.h"

uint64_t la_gpu_lzop_workspace_bytes(uint32_t n) { (void)n; return 0; }

/* the header's decoder alone, for tests/test_lzo_rules.py (the ABI below refuses what a container cannot hold) */
uint32_t la_lzo_rules_decode(const uint8_t *src, uint32_t src_len, uint8_t *dst, uint32_t dst_len, uint32_t *out_len, uint32_t *consumed)
{
	la_lzo_io io = { src, dst };
	return la_lzo1x_decode(&io, src_len, dst_len, out_len, consumed);
}

int la_gpu_adler32_many(la_gpu_ctx *c, const uint8_t *d_base, const la_hash_job *d_jobs, uint32_t n, uint32_t *d_out)
{
	(void)c;
	if (n && (!d_base || !d_jobs || !d_out))
		return LA_ERR_ARG;
	for (uint32_t i = 0; i < n; i++)
		d_out[i] = (uint32_t)adler32(d_jobs[i].seed, d_base + d_jobs[i].off, d_jobs[i].len);
	return LA_OK;
}

static uint32_t sum_of(uint32_t kind, const uint8_t *p, uint32_t n)
{
	return kind == LA_LZOP_SUM_CRC ? (uint32_t)crc32(0, p, n) : (uint32_t)adler32(1, p, n);
}

int la_gpu_lzop_decode(la_gpu_ctx *c, const la_lzop_batch *bt)
{
	(void)c;
	if (!bt || bt->reserved || (bt->n && (!bt->d_blocks || !bt->d_results || !bt->d_dst || (bt->src_bytes && !bt->d_src))))
		return LA_ERR_ARG;
	for (uint32_t b = 0; b < bt->n; b++) {
		const la_lzop_block k = bt->d_blocks[b];
		la_lzop_result r;
		memset(&r, 0, sizeof(r));
		if (!la_lzop_entry_ok(&k, bt->src_bytes, bt->dst_cap)) {
			r.status = LA_ST_LZOP_REFUSED;
			bt->d_results[b] = r;
			continue;
		}
		const uint8_t *s = bt->d_src + k.src_off;
		uint8_t *d = bt->d_dst + k.dst_off;
		const uint32_t ckind = la_lzop_sum_kind(k.flags, 0), ukind = la_lzop_sum_kind(k.flags, 1);
		if (ckind != LA_LZOP_SUM_NONE) {
			r.sum_c = sum_of(ckind, s, k.src_len);
			if (r.sum_c != k.sum_c)
				r.status = LA_ST_LZOP_BAD_SUM_C;
		}
		if (r.status == LA_ST_OK && k.src_len == k.dst_len) {
			memcpy(d, s, k.src_len);
			r.out_len = r.consumed = k.src_len;
		} else if (r.status == LA_ST_OK) {
			la_lzo_io io = { s, d };
			r.status = la_lzo1x_decode(&io, k.src_len, k.dst_len, &r.out_len, &r.consumed);
			if (r.status == LA_ST_OK && ukind != LA_LZOP_SUM_NONE) {
				r.sum_u = sum_of(ukind, d, k.dst_len);
				if (r.sum_u != k.sum_u)
					r.status = LA_ST_LZOP_BAD_SUM_U;
			}
		}
		bt->d_results[b] = r;
	}
	return LA_OK;
}
