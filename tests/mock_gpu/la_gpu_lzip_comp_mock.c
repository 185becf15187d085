/*
 * la_gpu_lzip_comp_mock.c -- TEST INFRASTRUCTURE: a CPU stand-in for la_gpu_lzip_compress as include/la_gpu.h words it,
 * so that the lzip write filter's host side (host/la_write_lzip.c) and the encoder's rules are tested without a GPU.
 * "Device" pointers are host pointers, as in la_gpu_mock.c.
 *
 * The rules are NOT restated here: this file compiles libarchive_amd/csrc/la_lzip_enc_dev.h (over la_xz_enc_dev.h), the
 * header the kernels compile, with the header's defaults: the 64 lanes of a step are walked in a loop, all reads before
 * any write, so the bytes are the device's.  What the kernels add around the header (the slot per member, the CRC32
 * combined from 64 segments, who writes header and trailer) is repeated below in the kernels' order.
 *
 * la_lzc_mock_events(out, reset) reads the event counters of the header's hook (LA_XZC_EV_* and LA_LZC_EV_MARKER), for
 * tests/test_lzip_encode_rules.py.
 */
#include "../../include/la_gpu.h"
#include <stdlib.h>
#include <string.h>

static uint64_t lzc_events[32];
#define LA_XZ_FN static inline
#define LA_XZC_EVENT(kind) (lzc_events[(kind)]++)
#include "../../libarchive_amd/csrc/la_lzip_enc_dev.h"

uint32_t la_lzc_mock_events(uint64_t *out, int reset)
{
	for (int i = 0; i < LA_LZC_EV_COUNT; i++) {
		if (out)
			out[i] = lzc_events[i];
		if (reset)
			lzc_events[i] = 0;
	}
	return LA_LZC_EV_COUNT;
}

uint64_t la_gpu_lzip_compress_member_bytes(uint32_t level) { return la_lzc_member_bytes(level); }
uint64_t la_gpu_lzip_compress_workspace_bytes(uint64_t src_bytes, uint32_t level) { (void)src_bytes; (void)level; return 0; }
uint64_t la_gpu_lzip_compress_bound(uint64_t src_bytes, uint32_t level) { return level <= 9u ? la_lzc_bound(src_bytes, level) : 0u; }

struct sink { uint8_t *p; uint64_t cap, n; };
static void put(struct sink *s, const uint8_t *b, uint64_t n)
{
	for (uint64_t i = 0; i < n; i++, s->n++)
		if (s->n < s->cap)
			s->p[s->n] = b[i];
}

/* the member's CRC32 as the kernel takes it: 64 segments, combined by x^(8 n) mod P */
static uint32_t member_crc(const uint32_t *table, const uint8_t *src, uint32_t n)
{
	const uint32_t seg = (n + 63u) / 64u, sh = la_lzc_crc32_shift(seg);
	uint32_t acc = 0;
	for (uint32_t j = 0; j < 64u && (j == 0 || seg * j < n); j++) {
		const uint32_t f = seg * j < n ? seg * j : n, l = n - f < seg ? n - f : seg;
		const uint32_t c = la_lzc_crc32(table, src + f, l, 0);
		acc = j ? la_lzc_crc32_mul(l == seg ? sh : la_lzc_crc32_shift(l), acc) ^ c : c;
	}
	return acc;
}

int la_gpu_lzip_compress(la_gpu_ctx *c, const la_lzc_batch *bt)
{
	static uint32_t table[256];
	if (!c || !bt || !bt->d_out_bytes || (bt->src_bytes && !bt->d_src) || (bt->out_cap && !bt->d_out))
		return LA_ERR_ARG;
	if (bt->level > 9u || bt->flags != 0u || bt->src_bytes > LA_LZC_MAX_SRC_BYTES)
		return LA_ERR_ARG;
	if (table[1] == 0)
		for (uint32_t i = 0; i < 256; i++)
			table[i] = la_lzc_crc32_entry(i);
	const uint32_t m = la_lzc_member_bytes(bt->level), slot_bytes = (uint32_t)la_lzc_slot_bytes(m);
	const uint64_t members = la_lzc_members(bt->src_bytes, bt->level);
	uint16_t *probs = malloc(sizeof(uint16_t) * LA_XZC_PROBS);
	uint32_t *tab = malloc(sizeof(uint32_t) * LA_XZC_TAB);
	uint8_t *slot = malloc(slot_bytes);
	if (!probs || !tab || !slot) {
		free(probs); free(tab); free(slot);
		return LA_ERR_NOMEM;
	}
	struct sink s = { bt->d_out, bt->out_cap, 0 };
	for (uint64_t k = 0; k < members; k++) {
		const uint64_t off = k * m;
		const uint32_t n = bt->src_bytes - off < m ? (uint32_t)(bt->src_bytes - off) : m;
		const uint8_t *src = n ? bt->d_src + off : (const uint8_t *)"";
		uint32_t m_len[64], m_cand[64];
		uint8_t h[LA_LZC_TRAILER_BYTES];
		const uint32_t stream = la_lzc_member(src, n, probs, tab, m_len, m_cand, slot, slot_bytes);
		la_lzc_header(h, bt->level);
		put(&s, h, LA_LZC_HEADER_BYTES);
		put(&s, slot, stream < slot_bytes ? stream : slot_bytes);
		s.n += stream < slot_bytes ? 0u : stream - slot_bytes;
		la_lzc_trailer(h, member_crc(table, src, n), n, stream);
		put(&s, h, LA_LZC_TRAILER_BYTES);
	}
	*bt->d_out_bytes = s.n;
	free(probs); free(tab); free(slot);
	return LA_OK;
}
