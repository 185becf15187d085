/*
 * la_gpu_lzop_comp_mock.c -- TEST INFRASTRUCTURE: a CPU stand-in for la_gpu_lzop_compress as include/la_gpu.h words it,
 * so that the lzop write filter's host side (host/la_write_lzop.c) and the encoder's rules are tested without a GPU.
 * "Device" pointers are host pointers, as in la_gpu_mock.c.
 *
 * How a sequence becomes bytes is NOT restated here: this file compiles libarchive_amd/csrc/la_lzo_enc_dev.h, the header
 * the kernel compiles, with its plain hooks.  The MATCHER is this file's own: a plain serial greedy one over a table of
 * the last position of every four bytes, limited to the format's longest distance.  It need not find the device's
 * matches (the wave matcher's table collisions are resolved in hardware order), so the bytes are not the device's; what
 * the kernels add around the header (the slot of a block's own size, stored when the stream reaches it, the three info
 * words) is repeated below in the kernels' order.  Adler-32 is zlib's.
 *
 * la_lzo_rules_encode() is the emitter alone over a given sequence list, for tests/test_lzo_encode_rules.py.
 */
#include "../../include/la_gpu.h"
#include <stdlib.h>
#include <string.h>
#include <zlib.h>

#include "../../libarchive_amd/csrc/la_lzo_enc_dev.h"

#define HASH_BITS 13

/* seqs: n_seqs triples (literals, distance, length); the bytes behind the last match are the block's last literals.
 * Returns the stream's size; nothing is stored at or behind cap.  0xFFFFFFFF: the list does not fit the block or holds
 * a match the format cannot code. */
uint32_t la_lzo_rules_encode(const uint8_t *plain, uint32_t n, const uint32_t *seqs, uint32_t n_seqs, uint8_t *out, uint32_t cap)
{
	la_lzoe_io io = { plain, out, cap };
	la_lzoe_state st;
	uint32_t ip = 0;
	la_lzoe_begin(&st);
	for (uint32_t i = 0; i < n_seqs; i++) {
		const uint32_t lit = seqs[3 * i], dist = seqs[3 * i + 1], len = seqs[3 * i + 2];
		if (lit > n - ip || len < 3u || len > n - ip - lit || dist == 0 || dist > LA_LZOE_MAX_DIST || dist > ip + lit)
			return 0xFFFFFFFFu;
		la_lzoe_seq(&io, &st, ip, lit, dist, len);
		ip += lit + len;
	}
	return la_lzoe_end(&io, &st, ip, n - ip);
}

uint32_t la_lzo_rules_worst(uint32_t n) { return la_lzoe_worst(n); }

/* one block into its slot; returns the stream's size (counted behind `cap`) */
static uint32_t block_stream(const uint8_t *in, uint32_t n, uint8_t *slot, uint32_t cap, uint32_t *tab)
{
	la_lzoe_io io = { in, slot, cap };
	la_lzoe_state st;
	uint32_t anchor = 0, p = 1;
	la_lzoe_begin(&st);
	memset(tab, 0xFF, sizeof(uint32_t) << HASH_BITS);
	if (n >= 4u) {
		uint32_t v0;
		memcpy(&v0, in, 4);
		tab[(v0 * 2654435761u) >> (32 - HASH_BITS)] = 0;
	}
	while (n >= 4u && p <= n - 4u) {
		uint32_t v, c = 0;
		memcpy(&v, in + p, 4);
		const uint32_t h = (v * 2654435761u) >> (32 - HASH_BITS);
		const uint32_t cand = tab[h];
		tab[h] = p;
		if (cand == 0xFFFFFFFFu || p - cand > LA_LZOE_MAX_DIST || (memcpy(&c, in + cand, 4), c != v)) {
			p++;
			continue;
		}
		uint32_t len = 4;
		while (p + len < n && in[p + len] == in[cand + len])
			len++;
		la_lzoe_seq(&io, &st, anchor, p - anchor, p - cand, len);
		p += len;
		anchor = p;
	}
	return la_lzoe_end(&io, &st, anchor, n - anchor);
}

uint64_t la_gpu_lzop_compress_workspace_bytes(uint64_t src_bytes, uint32_t block_size) { (void)src_bytes; (void)block_size; return 0; }
uint64_t la_gpu_lzop_compress_bound(uint64_t src_bytes, uint32_t block_size)
{
	return block_size ? src_bytes + 12u * ((src_bytes + block_size - 1) / block_size) : 0u;
}

struct sink { uint8_t *p; uint64_t cap, n; };
static void put(struct sink *s, const uint8_t *b, uint64_t n)
{
	for (uint64_t i = 0; i < n; i++, s->n++)
		if (s->n < s->cap)
			s->p[s->n] = b[i];
}

static void be32(uint8_t *p, uint32_t v)
{
	p[0] = (uint8_t)(v >> 24); p[1] = (uint8_t)(v >> 16); p[2] = (uint8_t)(v >> 8); p[3] = (uint8_t)v;
}

int la_gpu_lzop_compress(la_gpu_ctx *c, const la_lzopc_batch *bt)
{
	if (!c || !bt || !bt->d_out_bytes || (bt->src_bytes && !bt->d_src) || (bt->out_cap && !bt->d_out))
		return LA_ERR_ARG;
	if (bt->block_size < 1u || bt->block_size > LA_LZOPC_BLOCK_BYTES)
		return LA_ERR_ARG;
	const uint32_t slot_bytes = la_lzoe_slot_bytes(bt->block_size);
	uint32_t *tab = malloc(sizeof(uint32_t) << HASH_BITS);
	uint8_t *slot = malloc(slot_bytes);
	if (!tab || !slot) {
		free(tab); free(slot);
		return LA_ERR_NOMEM;
	}
	struct sink s = { bt->d_out, bt->out_cap, bt->lead_bytes };	/* the gap is the caller's */
	for (uint64_t off = 0; off < bt->src_bytes; off += bt->block_size) {
		const uint32_t n = bt->src_bytes - off < bt->block_size ? (uint32_t)(bt->src_bytes - off) : bt->block_size;
		const uint8_t *in = bt->d_src + off;
		const uint32_t stream = block_stream(in, n, slot, n, tab);
		const int stored = stream >= n;
		uint8_t info[12];
		be32(info, n);
		be32(info + 4, stored ? n : stream);
		be32(info + 8, (uint32_t)adler32(1, in, n));
		put(&s, info, 12);
		put(&s, stored ? in : slot, stored ? n : stream);
	}
	*bt->d_out_bytes = s.n;
	free(tab); free(slot);
	return LA_OK;
}
