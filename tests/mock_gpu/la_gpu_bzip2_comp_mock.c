/*
 * la_gpu_bzip2_comp_mock.c -- TEST INFRASTRUCTURE: a CPU stand-in for la_gpu_bzip2_compress over the real libbz2, so
 * that the bzip2 write filter's host side (windows, FIRST / LAST, the state carried between calls, the empty stream)
 * is tested without a device.  "Device" pointers are host pointers, as in la_gpu_mock.c.
 *
 * The same contract as the device: the input is cut every la_gpu_bzip2_compress_block_bytes(level) bytes; per cut ONE
 * BZ2_bzCompressInit(level) / BZ_FINISH stream, which holds exactly one block because the cut fits libbz2's block
 * limit; its 4-byte header is stripped, its trailer is found by trying the 0..7 pad bits for the end magic followed by
 * the block's own CRC, and the block's bits are appended behind the pending bits of the state.
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/la_gpu.h"

/* bzlib.h is not installed with the runtime library: the few declarations used */
typedef struct {
	char *next_in; unsigned int avail_in, total_in_lo32, total_in_hi32;
	char *next_out; unsigned int avail_out, total_out_lo32, total_out_hi32;
	void *state; void *(*bzalloc)(void *, int, int); void (*bzfree)(void *, void *); void *opaque;
} bzc_stream;
int BZ2_bzCompressInit(bzc_stream *, int blockSize100k, int verbosity, int workFactor);
int BZ2_bzCompress(bzc_stream *, int action);
int BZ2_bzCompressEnd(bzc_stream *);
#define BZC_FINISH 2
#define BZC_STREAM_END 4

uint32_t la_gpu_bzip2_compress_block_bytes(uint32_t level)
{
	return level >= 1 && level <= 9 ? 4u * ((100000u * level - 19u) / 5u) : 0u;
}
uint64_t la_gpu_bzip2_compress_workspace_bytes(uint64_t s, uint32_t l) { (void)s; (void)l; return 0; }
uint32_t la_gpu_bzip2_compress_sort_rounds(la_gpu_ctx *c) { (void)c; return 0; }
static uint64_t cut_cap(uint64_t n) { return n + n / 100u + 700u; }	/* libbz2's own worst case, with room to spare */
uint64_t la_gpu_bzip2_compress_bound(uint64_t src_bytes, uint32_t level)
{
	const uint32_t bb = la_gpu_bzip2_compress_block_bytes(level);
	if (bb == 0)
		return 0;
	return (src_bytes / bb) * cut_cap(bb) + cut_cap(src_bytes % bb) + 32u;
}

struct bitw { uint8_t *p; uint64_t bit; };
static void put_bit(struct bitw *w, unsigned b)
{
	if ((w->bit & 7u) == 0)
		w->p[w->bit >> 3] = 0;
	if (b)
		w->p[w->bit >> 3] |= (uint8_t)(0x80u >> (w->bit & 7u));
	w->bit++;
}
static void put_bits(struct bitw *w, uint64_t v, unsigned n)
{
	while (n--)
		put_bit(w, (unsigned)(v >> n) & 1u);
}
static uint64_t get_bits(const uint8_t *p, uint64_t bit, unsigned n)
{
	uint64_t v = 0;
	for (unsigned k = 0; k < n; k++, bit++)
		v = (v << 1) | ((p[bit >> 3] >> (7u - (bit & 7u))) & 1u);
	return v;
}

int la_gpu_bzip2_compress(la_gpu_ctx *c, const la_bz2c_batch *bt)
{
	if (!c || !bt || !bt->d_out_bytes || !bt->d_state || (bt->src_bytes && !bt->d_src) || (bt->out_cap && !bt->d_out))
		return LA_ERR_ARG;
	if (bt->level < 1 || bt->level > 9 || (bt->flags & ~(LA_BZ2C_FIRST | LA_BZ2C_LAST)) || bt->src_bytes > LA_BZ2C_MAX_SRC_BYTES)
		return LA_ERR_ARG;
	const uint32_t bb = la_gpu_bzip2_compress_block_bytes(bt->level);
	la_bz2c_state st = *bt->d_state;
	struct bitw w;
	w.p = malloc(la_gpu_bzip2_compress_bound(bt->src_bytes, bt->level) + 64u);
	uint8_t *one = malloc(cut_cap(bb));
	if (!w.p || !one) {
		free(w.p); free(one);
		return LA_ERR_NOMEM;
	}
	w.bit = 0;
	if (bt->flags & LA_BZ2C_FIRST) {
		memset(&st, 0, sizeof(st));
		put_bits(&w, ((uint64_t)'B' << 24) | ('Z' << 16) | ('h' << 8) | ('0' + bt->level), 32);
	} else {
		put_bits(&w, (st.bits & 0xFFu) >> (8u - (st.nbits & 7u)), st.nbits & 7u);
	}
	int rc = LA_OK;
	for (uint64_t o = 0; o < bt->src_bytes && rc == LA_OK; o += bb) {
		const uint64_t len = bt->src_bytes - o < bb ? bt->src_bytes - o : bb;
		bzc_stream s;
		memset(&s, 0, sizeof(s));
		if (BZ2_bzCompressInit(&s, (int)bt->level, 0, 0) != 0) { rc = LA_ERR_NOMEM; break; }
		s.next_in = (char *)(uintptr_t)(bt->d_src + o); s.avail_in = (unsigned)len;
		s.next_out = (char *)one; s.avail_out = (unsigned)cut_cap(bb);
		const int r = BZ2_bzCompress(&s, BZC_FINISH);
		const uint64_t n = cut_cap(bb) - s.avail_out;
		BZ2_bzCompressEnd(&s);
		if (r != BZC_STREAM_END || n < 14u) { rc = LA_ERR_ARG; break; }
		const uint32_t crc = (uint32_t)get_bits(one, 32u + 48u, 32);
		uint64_t end = 0;
		for (unsigned pad = 0; pad < 8u && end == 0; pad++) {
			const uint64_t at = 8u * n - pad - 80u;
			if (get_bits(one, at, 48) == 0x177245385090ull && (uint32_t)get_bits(one, at + 48u, 32) == crc)
				end = at;
		}
		if (end == 0 || get_bits(one, 32, 48) != 0x314159265359ull) { rc = LA_ERR_ARG; break; }	/* (not exactly one block) */
		for (uint64_t b = 32; b < end; b++)
			put_bit(&w, (unsigned)get_bits(one, b, 1));
		st.crc = ((st.crc << 1) | (st.crc >> 31)) ^ crc;
	}
	if (rc == LA_OK) {
		uint64_t bytes;
		if (bt->flags & LA_BZ2C_LAST) {
			put_bits(&w, 0x177245385090ull, 48);
			put_bits(&w, st.crc, 32);
			while (w.bit & 7u)
				put_bit(&w, 0);
			bytes = w.bit >> 3;
			memset(&st, 0, sizeof(st));
		} else {
			bytes = w.bit >> 3;
			st.nbits = (uint32_t)(w.bit & 7u);
			st.bits = st.nbits ? w.p[bytes] : 0u;
		}
		*bt->d_out_bytes = bytes;
		if (bt->out_cap)
			memcpy(bt->d_out, w.p, bytes < bt->out_cap ? bytes : bt->out_cap);
		if (bytes <= bt->out_cap)	/* as the device: a piece that did not fit leaves the state alone */
			*bt->d_state = st;
	}
	free(w.p); free(one);
	return rc;
}
