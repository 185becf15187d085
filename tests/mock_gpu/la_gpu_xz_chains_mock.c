/*
 * la_gpu_xz_chains_mock.c -- TEST INFRASTRUCTURE: a CPU stand-in for la_gpu_xz_decode as include/la_gpu.h words it,
 * the chain table (LA_XZ_BATCH_CHAINS) included, so that the host side (la_filter_xz.c, with and without LA_XZ_CHAINS=1)
 * is tested without a GPU: a batch without the table is decoded as it stands.  Linked beside la_gpu_mock.c.
 *
 * Neither the decode rules nor the filters are restated here: this file compiles libarchive_amd/csrc/la_xz_dev.h and
 * la_xz_filters_dev.h, the headers the kernels compile, one block after the other, in the kernels' order: decode, the
 * chain undone over the bytes there are (out_len, which on a failure counts the valid bytes), then sizes and check.
 */
#include "../../include/la_gpu.h"
#include <stdlib.h>
#include <string.h>
#include <zlib.h>

#define LA_XZ_FN static inline
#include "../../libarchive_amd/csrc/la_xz_dev.h"
#include "../../libarchive_amd/csrc/la_xz_filters_dev.h"

uint64_t la_gpu_xz_workspace_bytes(uint32_t n) { (void)n; return 0; }

int la_gpu_xz_decode(la_gpu_ctx *c, const la_xz_batch *bt)
{
	static uint64_t table[256];
	(void)c;
	if (!bt || (bt->reserved & ~LA_XZ_BATCH_CHAINS) || (bt->n && (!bt->d_blocks || !bt->d_results || !bt->d_dst || (bt->src_bytes && !bt->d_src))))
		return LA_ERR_ARG;
	const la_xz_chain *chains = (bt->reserved & LA_XZ_BATCH_CHAINS) ? (const la_xz_chain *)(bt->d_blocks + bt->n) : NULL;
	if (table[1] == 0)
		for (uint32_t i = 0; i < 256; i++)
			table[i] = la_xz_crc64_entry(i);
	uint16_t *probs = malloc(sizeof(uint16_t) * LA_XZ_PROBS_MAX);
	if (!probs)
		return LA_ERR_NOMEM;
	for (uint32_t b = 0; b < bt->n; b++) {
		const la_xz_block blk = bt->d_blocks[b];
		la_xz_result r;
		la_xz_lzma lz;
		memset(&r, 0, sizeof(r));
		if (blk.src_off > bt->src_bytes || blk.dst_off > bt->dst_cap || blk.dst_cap > bt->dst_cap - blk.dst_off ||
		    blk.dst_cap > LA_XZ_DST_CAP_MAX || (blk.uncomp_size != LA_XZ_UNKNOWN && blk.uncomp_size > blk.dst_cap) ||
		    (chains && !la_xz_chain_valid(&chains[b]))) {
			r.status = LA_ST_XZ_SIZE;
			bt->d_results[b] = r;
			continue;
		}
		uint64_t lim = bt->src_bytes;
		uint32_t lim_status = LA_ST_XZ_TRUNCATED;
		if (blk.comp_size != LA_XZ_UNKNOWN && blk.comp_size <= bt->src_bytes - blk.src_off) {
			lim = blk.src_off + blk.comp_size;
			lim_status = LA_ST_XZ_SIZE;
		}
		const int sized = blk.uncomp_size != LA_XZ_UNKNOWN;
		uint8_t *out = bt->d_dst + blk.dst_off;
		la_xz_block_decode(bt->d_src, blk.src_off, lim, lim_status, out, sized ? blk.uncomp_size : blk.dst_cap,
		    sized ? (uint32_t)LA_ST_XZ_SIZE : (uint32_t)LA_ST_XZ_OUT_FULL, blk.dict_size, probs, &lz, &r);
		if (r.status == LA_ST_OK && !la_xz_sizes_agree(&blk, &r))
			r.status = LA_ST_XZ_SIZE;
		if (chains)
			la_xz_unchain_serial(&chains[b], out, r.status == LA_ST_OK ? r.out_len : r.valid);
		if (r.status == LA_ST_OK) {
			uint8_t have[64];
			int supported = 1;
			memset(have, 0, sizeof(have));
			if (blk.check_id == 1u) {
				const uint32_t v = (uint32_t)crc32(0, out, (uInt)r.out_len);
				for (int i = 0; i < 4; i++) have[i] = (uint8_t)(v >> (8 * i));
			} else if (blk.check_id == 4u) {
				/* in two halves, so that the combine arithmetic of the kernel runs here too */
				const uint64_t h = r.out_len / 2;
				const uint64_t v = la_xz_crc64_mul(la_xz_crc64_shift(r.out_len - h), la_xz_crc64(table, out, h, 0)) ^
				    la_xz_crc64(table, out + h, r.out_len - h, 0);
				for (int i = 0; i < 8; i++) have[i] = (uint8_t)(v >> (8 * i));
			} else if (blk.check_id == 10u) {
				la_xz_sha256_all(out, r.out_len, have);
			} else if (blk.check_id != 0u) {
				supported = 0;
			}
			r.status = la_xz_block_tail(bt->d_src, bt->src_bytes, blk.src_off, r.consumed, blk.check_id, have, supported);
		}
		bt->d_results[b] = r;
	}
	free(probs);
	return LA_OK;
}
