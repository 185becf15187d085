/*
 * la_bzip2.hip -- bzip2 on the device: the marker scan and the two-phase block decode behind la_gpu_bzip2_scan /
 * la_gpu_bzip2_decode (include/la_gpu.h).  Replaces what bzip2_filter_read gets from libbz2's BZ2_bzDecompress
 * (libarchive/archive_read_support_filter_bzip2.c:214-332).
 *
 * A block is the parallel unit: one workgroup of 256 threads per candidate, one workspace slot per candidate.
 *   measure  thread 0 reads the header, the symbol map, the code lengths and the selectors and walks the Huffman
 *            symbols (inverse MTF, RUNA/RUNB) -- one serial chain per block, as in libbz2, and the checks are libbz2's
 *            in libbz2's order, because what is reported for damaged input depends on which check fires first;
 *            then the whole workgroup: the BWT vector by a counting sort over 32 lanes' chunks, the chase from 255
 *            evenly spaced starts and the origin, the stitch, the pre-RLE bytes, the run-length function per chunk.
 *   walk     one thread confirms candidates in stream order and packs their offsets.
 *   emit     one thread per 256 pre-RLE bytes expands its runs and takes the CRC of what it wrote; the workgroup
 *            combines the 256 CRCs (GF(2), MSB-first polynomial 0x04C11DB7).
 *   verify   one thread folds the partial CRCs per block, compares, folds the combined CRC per stream.
 * No kernel waits on another workgroup; every loop is bounded by the source end, the slot capacity (>= nblock), the
 * selector count or a fixed table size.
 */
#include "la_dev.h"

#define BZ_TPB        256
#define BZ_MAX_SEL    18002
#define BZ_GROUPS     6
#define BZ_ALPHA      258
#define BZ_CHUNK      256u	/* pre-RLE bytes per emit thread */
#define BZ_STARTS     255u	/* evenly spaced chase starts; id BZ_STARTS is the origin */
#define BZ_STITCH_CAP 1024u
#define BZ_SORT_LANES 32u
#define BZ_POLY       0x04C11DB7u
#define BZ_MAGIC_BLOCK 0x314159265359ull
#define BZ_MAGIC_END   0x177245385090ull
#define BZ_ST_OVER    0xFFu	/* internal: more symbols than the slot holds (the walk turns it into a data error) */

struct bz_info {	/* front of a slot */
	uint32_t status;
	uint32_t nblock;
	uint32_t orig_ptr;
	uint32_t stored_crc;
	uint64_t end_bit;
	uint64_t out_len;
	uint32_t nchunks;
	uint32_t end_run;	/* 1 + the count libbz2 makes up when the block ends on four equal bytes (see the measure kernel), else 0 */
	uint32_t pad[6];
};

struct bz_slot {
	bz_info *info;
	uint32_t *tt;		/* [cap] next << 8 | byte */
	uint8_t *pre;		/* [cap] the block before its run-length expansion */
	uint32_t *chunk_off;	/* [nch + 1] output offset of each chunk of BZ_CHUNK pre-RLE bytes */
	uint8_t *chunk_state;	/* [nch] run state at the chunk's first byte */
	uint2 *part;		/* [ceil(nch / 256)] (raw crc, bytes) of 256 chunks */
};

struct bz_ws {
	la_bz2_state *walk;	/* what the measure walk ended with */
	la_bz2_state *in;	/* state_in as given to MEASURE */
	uint8_t *slots;
	uint64_t slot_bytes;
	uint32_t cap;
};

static uint32_t bz_cap(uint32_t level) { return 100000u * level; }
static uint32_t bz_nch(uint32_t cap) { return (cap + BZ_CHUNK - 1) / BZ_CHUNK; }

static __host__ __device__ void bz_slot_carve(bz_slot *s, uint8_t *base, uint32_t cap, uint64_t *bytes)
{
	const uint32_t nch = (cap + BZ_CHUNK - 1) / BZ_CHUNK;
	uint64_t off = 0;
	s->info = (bz_info *)(base + off); off += sizeof(bz_info);
	s->tt = (uint32_t *)(base + off); off += (uint64_t)cap * 4;
	s->chunk_off = (uint32_t *)(base + off); off += ((uint64_t)nch + 1) * 4;
	off = (off + 7) & ~7ull;
	s->part = (uint2 *)(base + off); off += (uint64_t)((nch + 255) / 256) * 8;
	s->pre = base + off; off += cap;
	s->chunk_state = base + off; off += nch;
	*bytes = (off + 255) & ~255ull;
}

static uint64_t bz_ws_carve(bz_ws *w, uint8_t *base, uint32_t n, uint32_t level)
{
	la_carve cv = { base, 0 };
	w->walk = cv.take<la_bz2_state>(1, 64);
	w->in = cv.take<la_bz2_state>(1, 64);
	bz_slot s;
	w->cap = bz_cap(level);
	bz_slot_carve(&s, nullptr, w->cap, &w->slot_bytes);
	w->slots = cv.take<uint8_t>((uint64_t)n * w->slot_bytes, 256);
	return cv.off;
}

uint64_t la_bzip2_workspace_bytes(uint32_t n, uint32_t level)
{
	bz_ws w;
	return bz_ws_carve(&w, nullptr, n, level);
}

uint32_t la_bzip2_max_blocks(uint32_t level)
{
	bz_ws w;
	bz_ws_carve(&w, nullptr, 1, level);
	const uint64_t k = ((uint64_t)2 << 30) / w.slot_bytes;
	return (uint32_t)(k > 4096 ? 4096 : k);
}

/* ------------------------------------------------------------------ marker scan */

/* the 8 bytes at byte i (0 .. 15) of a thread's span, big-endian, from the three words that cover 24 bytes */
__device__ __forceinline__ uint64_t bz_win(uint64_t w0, uint64_t w1, uint64_t w2, uint32_t i)
{
	const uint64_t a = i < 8 ? w0 : w1, b = i < 8 ? w1 : w2;
	const uint32_t s = (i & 7) * 8;
	return s ? (a << s) | (b >> (64 - s)) : a;
}

__device__ __forceinline__ uint64_t bz_be64(const uint8_t *src, uint64_t at, uint64_t n)
{
	uint64_t v = 0;
	if (at + 8 <= n) {
		__builtin_memcpy(&v, src + at, 8);
		return __builtin_bswap64(v);
	}
	for (uint32_t k = 0; k < 8; k++)
		v = (v << 8) | (at + k < n ? src[at + k] : 0u);
	return v;
}

/* each thread takes 16 bytes (128 bit positions) and the 7 bytes of overhang a 48-bit pattern at phase 7 needs.
 * write == 0: counts[t] = matches; write == 1: the matches go to out[offs[t] ...) in ascending order */
__global__ __launch_bounds__(BZ_TPB) void bz2_scan_kernel(const uint8_t *__restrict__ src, uint64_t n, uint64_t nthreads,
    uint32_t *__restrict__ counts, const uint64_t *__restrict__ offs, la_bz2_cand *__restrict__ out, uint32_t cap, uint32_t *d_count, int write)
{
	const uint64_t t = (uint64_t)blockIdx.x * BZ_TPB + threadIdx.x;
	if (t >= nthreads)
		return;
	const uint64_t base = t * 16;
	const uint64_t w0 = bz_be64(src, base, n), w1 = bz_be64(src, base + 8, n), w2 = bz_be64(src, base + 16, n);
	uint32_t cnt = 0;
	uint64_t o = write ? offs[t] : 0;
	for (uint32_t i = 0; i < 16 && base + i < n; i++) {
		const uint64_t w = bz_win(w0, w1, w2, i);
		for (uint32_t ph = 0; ph < 8; ph++) {
			const uint64_t v = (w >> (16 - ph)) & 0xFFFFFFFFFFFFull;
			if (v != BZ_MAGIC_BLOCK && v != BZ_MAGIC_END)
				continue;
			const uint64_t bit = (base + i) * 8 + ph;
			if (bit + 48 > n * 8)
				continue;
			if (write && o + cnt < cap) {
				la_bz2_cand c;
				c.bit_off = bit; c.kind = v == BZ_MAGIC_BLOCK ? LA_BZ2_KIND_BLOCK : LA_BZ2_KIND_END; c.reserved = 0;
				out[o + cnt] = c;
			}
			cnt++;
		}
	}
	if (!write)
		counts[t] = cnt;
	else if (t == 0) {
		const uint64_t tot = offs[nthreads];
		*d_count = tot > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)tot;
	}
}

uint64_t la_bzip2_scan_ws_bytes(uint64_t src_bytes)
{
	const uint64_t nt = (src_bytes + 15) / 16;
	return ((nt * 4 + 255) & ~255ull) + (((nt + 1) * 8 + 255) & ~255ull) + la_scan_scratch_bytes((uint32_t)nt) + 256;
}

void la_launch_bzip2_scan(hipStream_t s, const uint8_t *d_src, uint64_t src_bytes, la_bz2_cand *d_cands, uint32_t cap,
    uint32_t *d_count, uint8_t *ws)
{
	const uint64_t nt = (src_bytes + 15) / 16;
	if (nt == 0) {
		(void)hipMemsetAsync(d_count, 0, 4, s);
		return;
	}
	la_carve cv = { ws, 0 };
	uint32_t *counts = cv.take<uint32_t>(nt, 256);
	uint64_t *offs = cv.take<uint64_t>(nt + 1, 256);
	void *scratch = cv.take<uint8_t>(la_scan_scratch_bytes((uint32_t)nt), 256);
	const uint32_t grid = (uint32_t)((nt + BZ_TPB - 1) / BZ_TPB);
	hipLaunchKernelGGL(bz2_scan_kernel, dim3(grid), dim3(BZ_TPB), 0, s, d_src, src_bytes, nt, counts, (const uint64_t *)offs, d_cands, cap, d_count, 0);
	la_launch_scan_u32(s, counts, (uint32_t)nt, offs, scratch);
	hipLaunchKernelGGL(bz2_scan_kernel, dim3(grid), dim3(BZ_TPB), 0, s, d_src, src_bytes, nt, counts, (const uint64_t *)offs, d_cands, cap, d_count, 1);
}

/* ------------------------------------------------------------------ bit reader (one thread, MSB first) */

struct bz_bits {
	const uint8_t *src;
	uint64_t nbytes;
	uint64_t pos;		/* next bit */
	uint64_t cbyte;		/* the cached 8 bytes start here */
	uint64_t cw;
	int over;		/* a read passed the end of the source */
};

__device__ __forceinline__ uint32_t bz_get(bz_bits &B, uint32_t n)	/* n <= 24 */
{
	if (B.pos + n > B.nbytes * 8) {
		B.over = 1;
		return 0;
	}
	const uint64_t by = B.pos >> 3;
	if (by < B.cbyte || B.pos + n > (B.cbyte + 8) * 8) {
		B.cbyte = by;
		B.cw = bz_be64(B.src, by, B.nbytes);
	}
	const uint32_t sh = 64u - (uint32_t)(B.pos - B.cbyte * 8) - n;
	const uint32_t v = (uint32_t)(B.cw >> sh) & ((1u << n) - 1u);
	B.pos += n;
	return v;
}

__device__ __forceinline__ uint32_t bz_peek20(bz_bits &B)	/* the next 20 bits, zeros beyond the source */
{
	const uint64_t by = B.pos >> 3;
	if (by < B.cbyte || B.pos + 20 > (B.cbyte + 8) * 8) {
		B.cbyte = by;
		B.cw = bz_be64(B.src, by, B.nbytes);
	}
	return (uint32_t)(B.cw >> (44u - (uint32_t)(B.pos - B.cbyte * 8))) & 0xFFFFFu;
}

/* LDS of the measure kernel.  The selectors are dead once the symbols are walked, the sort's counters live after. */
struct bz_lds {
	union {
		uint8_t selector[BZ_MAX_SEL];
		uint32_t hist[256 * BZ_SORT_LANES];	/* [value][lane] */
	};
	int32_t limit[BZ_GROUPS][23], base[BZ_GROUPS][23];
	uint16_t perm[BZ_GROUPS][BZ_ALPHA];
	uint8_t len[BZ_GROUPS][BZ_ALPHA];
	int32_t minlen[BZ_GROUPS];
	uint32_t unzftab[256];
	uint8_t seq2unseq[256], yy[256];
	uint32_t seg_len[BZ_STARTS + 1];
	uint16_t seg_next[BZ_STARTS + 1];
	uint16_t lst_seg[BZ_STITCH_CAP];
	uint32_t lst_off[BZ_STITCH_CAP];
	uint32_t fn_out[BZ_TPB][5];
	uint8_t fn_end[BZ_TPB][5];
	uint32_t th_off[BZ_TPB];
	uint8_t th_state[BZ_TPB];
	uint32_t nblock, status, orig_ptr, lst_n, serial, beyond;
};

#define BZ_FAIL(st_) do { L.status = (st_); L.nblock = nblock; return; } while (0)
#define BZ_GET(var_, n_) do { (var_) = bz_get(B, (n_)); if (B.over) BZ_FAIL(LA_ST_BZ2_TRUNCATED); } while (0)

/* decompress.c's BZ2_decompress for one block, from behind the magic to the end-of-block symbol: the same reads and the
 * same checks in the same order.  cap stands in for nblockMAX (the walk knows the stream's level and compares again). */
__device__ void bz_entropy(bz_lds &L, bz_bits &B, bz_info *info, uint32_t *tt, uint32_t cap)
{
	uint32_t nblock = 0, v;
	BZ_GET(v, 16); uint32_t crc = v << 16; BZ_GET(v, 16); crc |= v;
	info->stored_crc = crc;
	BZ_GET(v, 1);
	if (v) BZ_FAIL(LA_ST_BZ2_RANDOMISED);
	BZ_GET(v, 24);
	L.orig_ptr = v;
	/* symbol map */
	uint32_t used16, ninuse = 0;
	BZ_GET(used16, 16);
	for (uint32_t i = 0; i < 16; i++)
		if (used16 & (0x8000u >> i)) {
			BZ_GET(v, 16);
			for (uint32_t j = 0; j < 16; j++)
				if (v & (0x8000u >> j))
					L.seq2unseq[ninuse++] = (uint8_t)(i * 16 + j);
		}
	if (ninuse == 0) BZ_FAIL(LA_ST_BZ2_DATA);
	const uint32_t alpha = ninuse + 2;
	uint32_t ngroups, nsel;
	BZ_GET(ngroups, 3);
	if (ngroups < 2 || ngroups > BZ_GROUPS) BZ_FAIL(LA_ST_BZ2_DATA);
	BZ_GET(nsel, 15);
	if (nsel < 1) BZ_FAIL(LA_ST_BZ2_DATA);
	for (uint32_t i = 0; i < nsel; i++) {
		uint32_t j = 0;
		for (;;) {
			BZ_GET(v, 1);
			if (v == 0) break;
			if (++j >= ngroups) BZ_FAIL(LA_ST_BZ2_DATA);
		}
		if (i < BZ_MAX_SEL)	/* libbz2 1.0.8 reads and drops the selectors beyond its table */
			L.selector[i] = (uint8_t)j;
	}
	if (nsel > BZ_MAX_SEL)
		nsel = BZ_MAX_SEL;
	{
		uint8_t pos[BZ_GROUPS];
		for (uint32_t k = 0; k < ngroups; k++) pos[k] = (uint8_t)k;
		for (uint32_t i = 0; i < nsel; i++) {
			uint32_t k = L.selector[i];
			const uint8_t tmp = pos[k];
			while (k > 0) { pos[k] = pos[k - 1]; k--; }
			pos[0] = tmp;
			L.selector[i] = tmp;
		}
	}
	for (uint32_t t = 0; t < ngroups; t++) {
		int32_t curr;
		BZ_GET(v, 5); curr = (int32_t)v;
		for (uint32_t i = 0; i < alpha; i++) {
			for (;;) {
				if (curr < 1 || curr > 20) BZ_FAIL(LA_ST_BZ2_DATA);
				BZ_GET(v, 1);
				if (v == 0) break;
				BZ_GET(v, 1);
				curr += v == 0 ? 1 : -1;
			}
			L.len[t][i] = (uint8_t)curr;
		}
	}
	for (uint32_t t = 0; t < ngroups; t++) {	/* BZ2_hbCreateDecodeTables */
		int32_t mn = 32, mx = 0;
		for (uint32_t i = 0; i < alpha; i++) {
			if (L.len[t][i] > mx) mx = L.len[t][i];
			if (L.len[t][i] < mn) mn = L.len[t][i];
		}
		uint32_t pp = 0;
		for (int32_t i = mn; i <= mx; i++)
			for (uint32_t j = 0; j < alpha; j++)
				if (L.len[t][j] == i) L.perm[t][pp++] = (uint16_t)j;
		int32_t *bs = L.base[t], *lm = L.limit[t];
		for (int i = 0; i < 23; i++) { bs[i] = 0; lm[i] = 0; }
		for (uint32_t i = 0; i < alpha; i++) bs[L.len[t][i] + 1]++;
		for (int i = 1; i < 23; i++) bs[i] += bs[i - 1];
		int32_t vec = 0;
		for (int32_t i = mn; i <= mx; i++) {
			vec += bs[i + 1] - bs[i];
			lm[i] = vec - 1;
			vec <<= 1;
		}
		for (int32_t i = mn + 1; i <= mx; i++)
			bs[i] = ((lm[i - 1] + 1) << 1) - bs[i];
		L.minlen[t] = mn;
	}
	/* the symbols, in groups of 50 */
	const uint32_t eob = ninuse + 1;
	for (uint32_t i = 0; i < 256; i++) { L.unzftab[i] = 0; L.yy[i] = (uint8_t)i; }
	int32_t group_no = -1, group_pos = 0;
	uint32_t g = 0, next_sym;
#define BZ_MTF_VAL() do {                                                                  \
		if (group_pos == 0) {                                                      \
			group_no++;                                                        \
			if (group_no >= (int32_t)nsel) BZ_FAIL(LA_ST_BZ2_DATA);            \
			group_pos = 50;                                                    \
			g = L.selector[group_no];                                          \
		}                                                                          \
		group_pos--;                                                               \
		/* libbz2 reads minLen bits, then one bit at a time while the code is above limit[zn]; the same from one     \
		 * look at the next 20 bits (zeros behind the source's end, which the length test never lets count) */    \
		int32_t zn = L.minlen[g], zvec;                                            \
		const uint32_t pk = bz_peek20(B);                                          \
		for (;;) {                                                                 \
			if (B.pos + (uint32_t)zn > B.nbytes * 8) BZ_FAIL(LA_ST_BZ2_TRUNCATED); \
			if (zn > 20) BZ_FAIL(LA_ST_BZ2_DATA);                              \
			zvec = (int32_t)(pk >> (20 - zn));                                 \
			if (zvec <= L.limit[g][zn]) break;                                 \
			zn++;                                                              \
		}                                                                          \
		B.pos += (uint32_t)zn;                                                     \
		if (zvec - L.base[g][zn] < 0 || zvec - L.base[g][zn] >= BZ_ALPHA) BZ_FAIL(LA_ST_BZ2_DATA); \
		next_sym = L.perm[g][zvec - L.base[g][zn]];                                \
	} while (0)
	BZ_MTF_VAL();
	for (;;) {
		if (next_sym == eob)
			break;
		if (next_sym <= 1) {	/* RUNA / RUNB */
			int32_t es = -1, N = 1;
			do {
				if (N >= 2 * 1024 * 1024) BZ_FAIL(LA_ST_BZ2_DATA);
				es += next_sym == 0 ? N : 2 * N;
				N *= 2;
				BZ_MTF_VAL();
			} while (next_sym <= 1);
			es++;
			const uint8_t uc = L.seq2unseq[L.yy[0]];
			L.unzftab[uc] += (uint32_t)es;
			while (es > 0) {
				if (nblock >= cap) BZ_FAIL(BZ_ST_OVER);
				tt[nblock++] = uc;
				es--;
			}
			continue;
		}
		if (nblock >= cap) BZ_FAIL(BZ_ST_OVER);
		{
			uint32_t nn = next_sym - 1;
			const uint8_t uc = L.yy[nn];
			while (nn > 0) { L.yy[nn] = L.yy[nn - 1]; nn--; }
			L.yy[0] = uc;
			const uint8_t b = L.seq2unseq[uc];
			L.unzftab[b]++;
			tt[nblock++] = b;
		}
		BZ_MTF_VAL();
	}
#undef BZ_MTF_VAL
	L.nblock = nblock;
	L.status = L.orig_ptr >= nblock ? LA_ST_BZ2_DATA : LA_ST_OK;
}

/* the run-length machine over "equals the previous byte": 0 fresh (behind a count byte or at the block's start), 1 .. 3
 * equal bytes so far, 4 = four equal bytes seen, this byte is a count */
__device__ __forceinline__ uint32_t bz_rle_step(uint32_t st, uint32_t b, uint32_t prev, uint32_t *out)
{
	if (st == 4) { *out += b; return 0; }
	*out += 1;
	if (st == 0 || b != prev) return 1;
	return st + 1;
}

__global__ __launch_bounds__(BZ_TPB) void bz2_measure_kernel(const uint8_t *__restrict__ src, uint64_t src_bytes,
    const la_bz2_cand *__restrict__ cands, uint32_t n, uint8_t *slots, uint64_t slot_bytes, uint32_t cap, uint32_t options)
{
	__shared__ bz_lds L;
	const uint32_t tid = threadIdx.x;
	const uint32_t k = blockIdx.x;
	if (k >= n)
		return;
	bz_slot S;
	uint64_t sb;
	bz_slot_carve(&S, slots + (uint64_t)k * slot_bytes, cap, &sb);
	const la_bz2_cand c = cands[k];
	if (tid == 0) {
		L.status = LA_ST_BZ2_REFUTED; L.nblock = 0; L.orig_ptr = 0; L.serial = 0;
		S.info->stored_crc = 0; S.info->end_bit = c.bit_off; S.info->out_len = 0; S.info->nchunks = 0;
		if (c.kind == LA_BZ2_KIND_BLOCK && c.bit_off + 48 <= src_bytes * 8) {
			bz_bits B = { src, src_bytes, c.bit_off + 48, ~0ull, 0, 0 };
			bz_entropy(L, B, S.info, S.tt, cap);
			S.info->end_bit = B.pos;
		}
		S.info->status = L.status; S.info->nblock = L.nblock; S.info->orig_ptr = L.orig_ptr;
	}
	__syncthreads();
	if (L.status != LA_ST_OK)
		return;
	const uint32_t nblock = L.nblock;	/* 1 .. cap */
	uint32_t *tt = S.tt;
	/* --- the vector: tt[cftab[byte_i]++] |= i << 8 as a stable counting sort, BZ_SORT_LANES chunks of the column --- */
	for (uint32_t i = tid; i < 256 * BZ_SORT_LANES; i += BZ_TPB)
		L.hist[i] = 0;
	__syncthreads();
	const uint32_t cs = (nblock + BZ_SORT_LANES - 1) / BZ_SORT_LANES;
	if (tid < BZ_SORT_LANES) {
		const uint32_t lo = tid * cs, hi = lo + cs < nblock ? lo + cs : nblock;
		for (uint32_t i = lo; i < hi; i++)
			L.hist[(tt[i] & 0xFFu) * BZ_SORT_LANES + tid]++;
	}
	__syncthreads();
	{	/* thread v: where value v starts (sum of the counts below it), then the chunks' shares in order */
		uint32_t below = 0;
		for (uint32_t u = 0; u < tid; u++)
			below += L.unzftab[u];
		for (uint32_t l = 0; l < BZ_SORT_LANES; l++) {
			const uint32_t h = L.hist[tid * BZ_SORT_LANES + l];
			L.hist[tid * BZ_SORT_LANES + l] = below;
			below += h;
		}
	}
	__syncthreads();
	if (tid < BZ_SORT_LANES) {
		const uint32_t lo = tid * cs, hi = lo + cs < nblock ? lo + cs : nblock;
		for (uint32_t i = lo; i < hi; i++) {
			const uint32_t p = L.hist[(tt[i] & 0xFFu) * BZ_SORT_LANES + tid]++;
			if (p < nblock)	/* (always: the counts are those of this very column).  One writer per p, and the low byte,
					 * which other lanes read meanwhile, does not change: a plain store, visible to the workgroup
					 * behind the barrier */
				tt[p] = (tt[p] & 0xFFu) | (i << 8);
		}
	}
	__threadfence_block();
	__syncthreads();
	/* --- the chase.  out[k] = tt[p_k] & 0xff, p_0 = tt[origPtr] >> 8, p_(k+1) = tt[p_k] >> 8: nblock dependent loads.
	 * Chased instead from every multiple of `stride` and from p_0 at once, each chain up to the next multiple; the
	 * segments are then laid down in link order from the origin.  tt is a permutation whatever the data, but not
	 * always ONE cycle (periodic input, damage): a chain is cut at nblock steps, the origin's cycle is laid down as
	 * often as it takes, and a list that overflows goes to the serial chase. --- */
	const uint32_t p0 = tt[L.orig_ptr] >> 8;
	const uint32_t stride = (nblock + BZ_STARTS - 1) / BZ_STARTS;
	if (!(options & LA_BZ2_OPT_SERIAL_CHASE)) {
		const uint32_t start = tid == BZ_STARTS ? p0 : tid * stride;
		uint32_t len = 0, p = start;
		if (start < nblock) {
			do {
				p = tt[p] >> 8;
				len++;
			} while (p % stride != 0 && len < nblock);
		}
		L.seg_len[tid] = len;
		L.seg_next[tid] = (uint16_t)(p / stride);
		__syncthreads();
		if (tid == 0) {
			uint32_t off = 0, seg = BZ_STARTS, cnt = 0;
			while (off < nblock) {
				if (cnt == BZ_STITCH_CAP || L.seg_len[seg] == 0) { L.serial = 1; break; }
				L.lst_seg[cnt] = (uint16_t)seg;
				L.lst_off[cnt] = off;
				cnt++;
				off += L.seg_len[seg];
				seg = L.seg_next[seg];
				if (seg >= BZ_STARTS) { L.serial = off < nblock; break; }	/* (a multiple of stride below nblock is below BZ_STARTS * stride) */
			}
			L.lst_n = cnt;
		}
		__syncthreads();
		if (!L.serial)
			for (uint32_t e = tid; e < L.lst_n; e += BZ_TPB) {
				const uint32_t seg = L.lst_seg[e], off = L.lst_off[e];
				uint32_t m = L.seg_len[seg];
				if (m > nblock - off) m = nblock - off;
				uint32_t q = seg == BZ_STARTS ? p0 : seg * stride;
				for (uint32_t i = 0; i < m; i++) {
					const uint32_t w = tt[q];
					S.pre[off + i] = (uint8_t)w;
					q = w >> 8;
				}
				if (e + 1 == L.lst_n)
					L.beyond = tt[q] & 0xFFu;	/* the byte the chain gives behind the block's last */
			}
	} else if (tid == 0)
		L.serial = 1;
	__syncthreads();
	if (L.serial && tid == 0) {
		uint32_t q = p0;
		for (uint32_t i = 0; i < nblock; i++) {
			const uint32_t w = tt[q];
			S.pre[i] = (uint8_t)w;
			q = w >> 8;
		}
		L.beyond = tt[q] & 0xFFu;
	}
	__threadfence_block();
	__syncthreads();
	/* --- length of the run-length expansion.  Whether a byte is data or a count depends on everything in front of it
	 * (in bbbbaaaaa the first a is a count), so each thread takes a contiguous range of chunks through all five states
	 * at once, thread 0 composes the 256 functions, and a second pass with the now known state writes each chunk's
	 * state and offset for the emit kernel. --- */
	const uint32_t nch = (nblock + BZ_CHUNK - 1) / BZ_CHUNK;
	const uint32_t cpt = (nch + BZ_TPB - 1) / BZ_TPB;
	const uint32_t lo = tid * cpt * BZ_CHUNK < nblock ? tid * cpt * BZ_CHUNK : nblock;
	const uint32_t hi = (uint64_t)(tid + 1) * cpt * BZ_CHUNK < nblock ? (tid + 1) * cpt * BZ_CHUNK : nblock;
	{
		uint32_t st[5] = { 0, 1, 2, 3, 4 }, out[5] = { 0, 0, 0, 0, 0 };
		uint32_t prev = lo ? S.pre[lo - 1] : 0;
		for (uint32_t i = lo; i < hi; i++) {
			const uint32_t b = S.pre[i];
#pragma unroll
			for (int s = 0; s < 5; s++)
				st[s] = bz_rle_step(st[s], b, prev, &out[s]);
			prev = b;
		}
		for (int s = 0; s < 5; s++) { L.fn_out[tid][s] = out[s]; L.fn_end[tid][s] = (uint8_t)st[s]; }
	}
	__syncthreads();
	if (tid == 0) {
		uint32_t st = 0;
		uint64_t off = 0;
		for (uint32_t t = 0; t < BZ_TPB; t++) {
			L.th_state[t] = (uint8_t)st;
			L.th_off[t] = (uint32_t)off;
			off += L.fn_out[t][st];
			st = L.fn_end[t][st];
		}
		/* A block that ends on four equal bytes has no count byte behind them.  libbz2 reads one all the same
		 * (bzlib.c, unRLE_obuf_to_output_FAST: the count and the byte behind it are fetched without a look at the
		 * block's end), takes the byte the chain gives there, emits that many more copies and only then finds
		 * nblock_used past the end: a data error, but behind bytes the reference may already have handed out.  So the
		 * made-up run is part of what this block emits, and the verify kernel fails the block. */
		S.info->end_run = 0;
		if (st == 4) {
			S.info->end_run = 1 + L.beyond;
			off += L.beyond;
		}
		/* 255 + 4 bytes out of every 5: below 2^32 for every nblock a slot holds */
		S.info->out_len = off;
		S.info->nchunks = nch;
		S.chunk_off[nch] = (uint32_t)off;
	}
	__syncthreads();
	{
		uint32_t st = L.th_state[tid], out = L.th_off[tid];
		uint32_t prev = lo ? S.pre[lo - 1] : 0;
		for (uint32_t i = lo; i < hi; i++) {
			if ((i % BZ_CHUNK) == 0) {
				S.chunk_off[i / BZ_CHUNK] = out;
				S.chunk_state[i / BZ_CHUNK] = (uint8_t)st;
			}
			const uint32_t b = S.pre[i];
			st = bz_rle_step(st, b, prev, &out);
			prev = b;
		}
	}
}

/* ------------------------------------------------------------------ the walk */

__device__ uint32_t bz_be32_at(const uint8_t *src, uint64_t src_bytes, uint64_t bit)	/* caller: bit + 32 inside */
{
	bz_bits B = { src, src_bytes, bit, ~0ull, 0, 0 };
	const uint32_t hi = bz_get(B, 16);
	return hi << 16 | bz_get(B, 16);
}

__global__ void bz2_walk_kernel(const uint8_t *__restrict__ src, uint64_t src_bytes, const la_bz2_cand *__restrict__ cands,
    uint32_t n, const uint8_t *slots, uint64_t slot_bytes, uint32_t slot_level, la_bz2_state in, la_bz2_result *results,
    la_bz2_state *walk, la_bz2_state *in_copy, la_bz2_state *out)
{
	if (threadIdx.x != 0 || blockIdx.x != 0)
		return;
	la_bz2_result refuted;
	refuted.status = LA_ST_BZ2_REFUTED; refuted.level = 0; refuted.out_len = 0; refuted.end_bit = 0; refuted.dst_off = 0;
	refuted.crc = 0; refuted.stored_crc = 0;
	for (uint32_t i = 0; i < n; i++)
		results[i] = refuted;
	uint32_t open = in.open, level = in.level, i = 0;
	uint64_t pos = in.start_bit, total = 0;
	la_bz2_state st = in;
	st.stop = LA_BZ2_STOP_TABLE; st.stop_entry = 0xFFFFFFFFu; st.first_bad = 0xFFFFFFFFu; st.reserved = 0;
	for (;;) {
		if (!open) {
			pos = (pos + 7) & ~7ull;
			const uint64_t by = pos >> 3;
			if (by + 14 > src_bytes) { st.stop = LA_BZ2_STOP_SHORT; break; }
			const uint8_t *h = src + by;
			while (i < n && cands[i].bit_off < pos + 32) i++;
			if (h[0] != 'B' || h[1] != 'Z' || h[2] != 'h' || h[3] < '1' || h[3] > '9' || i >= n || cands[i].bit_off != pos + 32) {
				st.stop = LA_BZ2_STOP_BID;
				break;
			}
			if ((uint32_t)(h[3] - '0') > slot_level) { st.stop = LA_BZ2_STOP_LEVEL; break; }
			open = 1; level = h[3] - '0'; st.crc = 0;
			pos += 32;
		}
		while (i < n && cands[i].bit_off < pos) i++;
		if (i >= n || cands[i].bit_off != pos) { st.stop = LA_BZ2_STOP_TABLE; break; }
		la_bz2_result r = refuted;
		r.level = level; r.dst_off = total;
		if (cands[i].kind == LA_BZ2_KIND_BLOCK) {
			const bz_info *info = (const bz_info *)(slots + (uint64_t)i * slot_bytes);
			uint32_t s = info->status;
			/* the level's own bounds (decompress.c: origPtr against 10 + 100000 * level as soon as it is read, nblock
			 * against 100000 * level as it grows): both fire before the block's end, so they win over what came later */
			if (s != LA_ST_BZ2_RANDOMISED && (info->orig_ptr > 10u + 100000u * level || info->nblock > 100000u * level || s == BZ_ST_OVER))
				s = LA_ST_BZ2_DATA;
			r.status = s; r.end_bit = info->end_bit; r.stored_crc = info->stored_crc;
			if (s != LA_ST_OK) {
				results[i] = r;
				st.stop = LA_BZ2_STOP_ENTRY; st.stop_entry = i;
				break;
			}
			r.out_len = info->out_len;
			total += r.out_len;
		} else {
			if (pos + 80 > src_bytes * 8) {
				r.status = LA_ST_BZ2_TRUNCATED; r.end_bit = pos;
				results[i] = r;
				st.stop = LA_BZ2_STOP_ENTRY; st.stop_entry = i;
				break;
			}
			r.status = LA_ST_OK;
			r.stored_crc = bz_be32_at(src, src_bytes, pos + 48);
			r.end_bit = (pos + 80 + 7) & ~7ull;
			open = 0;
		}
		results[i] = r;
		pos = r.end_bit;
		i++;
	}
	st.open = open; st.level = level; st.start_bit = pos; st.total_out = total; st.n_taken = i;
	*walk = st;
	*in_copy = in;
	*out = st;
}

/* ------------------------------------------------------------------ emit */

__device__ __forceinline__ uint32_t bz_mulmod(uint32_t a, uint32_t b)	/* a * b mod P, bit i = coefficient of x^i */
{
	uint32_t r = 0;
	for (int i = 31; i >= 0; i--) {
		r = (r << 1) ^ ((r >> 31) ? BZ_POLY : 0u);
		if ((b >> i) & 1u) r ^= a;
	}
	return r;
}
/* a * x^(8 * bytes) mod P; pw[k] = x^(8 * 2^k) */
__device__ __forceinline__ uint32_t bz_shift_bytes(uint32_t a, uint32_t bytes, const uint32_t *pw)
{
	for (uint32_t k = 0; bytes; k++, bytes >>= 1)
		if (bytes & 1u) a = bz_mulmod(a, pw[k]);
	return a;
}
__device__ __forceinline__ void bz_pow_table(uint32_t *pw)	/* one thread */
{
	pw[0] = 0x100u;
	for (int k = 1; k < 32; k++)
		pw[k] = bz_mulmod(pw[k - 1], pw[k - 1]);
}

/* grid (groups of 256 chunks, entries): thread = one chunk of BZ_CHUNK pre-RLE bytes of one confirmed block */
__global__ __launch_bounds__(BZ_TPB) void bz2_emit_kernel(const la_bz2_result *__restrict__ results, uint32_t n_emit, const uint8_t *slots,
    uint64_t slot_bytes, uint32_t cap, const la_bz2_state *__restrict__ walk, uint8_t *dst, uint64_t dst_cap)
{
	__shared__ uint32_t tab[256], pw[32], r_crc[BZ_TPB], r_len[BZ_TPB];
	const uint32_t tid = threadIdx.x, e = blockIdx.y;
	if (e >= n_emit || e >= walk->n_taken)
		return;
	const la_bz2_result r = results[e];
	if (r.status != LA_ST_OK || r.out_len == 0 || r.dst_off > dst_cap || r.out_len > dst_cap - r.dst_off)
		return;
	bz_slot S;
	uint64_t sb;
	bz_slot_carve(&S, (uint8_t *)slots + (uint64_t)e * slot_bytes, cap, &sb);
	const uint32_t nch = S.info->nchunks, nblock = S.info->nblock;
	if (blockIdx.x * BZ_TPB >= nch)
		return;
	{
		uint32_t c = tid << 24;
		for (int b = 0; b < 8; b++)
			c = (c << 1) ^ ((c >> 31) ? BZ_POLY : 0u);
		tab[tid] = c;
	}
	if (tid == 0)
		bz_pow_table(pw);
	__syncthreads();
	const uint32_t ch = blockIdx.x * BZ_TPB + tid;
	uint32_t crc = 0, len = 0;
	if (ch < nch) {
		const uint32_t lo = ch * BZ_CHUNK, hi = lo + BZ_CHUNK < nblock ? lo + BZ_CHUNK : nblock;
		const uint32_t o0 = S.chunk_off[ch], o1 = S.chunk_off[ch + 1];
		uint32_t st = S.chunk_state[ch], o = o0;
		uint32_t prev = lo ? S.pre[lo - 1] : 0;
		uint8_t *d = dst + r.dst_off;
		for (uint32_t i = lo; i < hi; i++) {
			const uint32_t b = S.pre[i];
			if (st == 4) {
				uint32_t m = b;
				if (m > o1 - o) m = o1 - o;	/* (equal by construction: never past the chunk's own share) */
				for (uint32_t j = 0; j < m; j++) {
					d[o + j] = (uint8_t)prev;
					crc = (crc << 8) ^ tab[(crc >> 24) ^ prev];
				}
				o += m;
				st = 0;
				/* prev stays the run's byte; it is not looked at in state 0 */
			} else {
				if (o < o1) {
					d[o++] = (uint8_t)b;
					crc = (crc << 8) ^ tab[(crc >> 24) ^ b];
				}
				st = (st == 0 || b != prev) ? 1 : st + 1;
				prev = b;
			}
		}
		if (ch + 1 == nch && st == 4) {	/* the count libbz2 makes up behind four equal bytes at the block's end */
			while (o < o1) {
				d[o++] = (uint8_t)prev;
				crc = (crc << 8) ^ tab[(crc >> 24) ^ prev];
			}
		}
		len = o - o0;
	}
	r_crc[tid] = crc; r_len[tid] = len;
	__syncthreads();
	for (uint32_t d = 1; d < BZ_TPB; d <<= 1) {
		if ((tid & (2 * d - 1)) == 0) {
			const uint32_t lb = r_len[tid + d];
			r_crc[tid] = bz_shift_bytes(r_crc[tid], lb, pw) ^ r_crc[tid + d];
			r_len[tid] += lb;
		}
		__syncthreads();
	}
	if (tid == 0)
		S.part[blockIdx.x] = make_uint2(r_crc[0], r_len[0]);
}

/* one thread: block CRCs against their headers, the combined CRC of every stream that ends among the emitted entries,
 * the first failing entry in stream order, the stream state behind the last entry taken */
__global__ void bz2_verify_kernel(const la_bz2_cand *__restrict__ cands, la_bz2_result *results, uint32_t n_emit, const uint8_t *slots, uint64_t slot_bytes, uint32_t cap,
    const la_bz2_state *__restrict__ walk, const la_bz2_state *__restrict__ in, uint64_t dst_cap, la_bz2_state *out)
{
	__shared__ uint32_t pw[32];
	if (threadIdx.x != 0 || blockIdx.x != 0)
		return;
	bz_pow_table(pw);
	const la_bz2_state w = *walk;
	la_bz2_state st = *in;
	st.stop = LA_BZ2_STOP_TABLE; st.stop_entry = 0xFFFFFFFFu; st.first_bad = 0xFFFFFFFFu; st.total_out = 0; st.reserved = 0;
	uint32_t i = 0;
	const uint32_t lim = n_emit < w.n_taken ? n_emit : w.n_taken;
	for (; i < lim; i++) {
		la_bz2_result r = results[i];
		if (r.status == LA_ST_BZ2_REFUTED)
			continue;
		if (!st.open) { st.open = 1; st.level = r.level; st.crc = 0; }
		bz_slot S;
		uint64_t sb;
		bz_slot_carve(&S, (uint8_t *)slots + (uint64_t)i * slot_bytes, cap, &sb);
		if (cands[i].kind == LA_BZ2_KIND_BLOCK) {
			if (r.dst_off > dst_cap || r.out_len > dst_cap - r.dst_off)
				break;	/* not emitted: the caller's budget ends here */
			uint32_t raw = 0, len = 0;
			const uint32_t np = (S.info->nchunks + BZ_TPB - 1) / BZ_TPB;
			for (uint32_t g = 0; g < np; g++) {
				const uint2 p = S.part[g];
				raw = bz_shift_bytes(raw, p.y, pw) ^ p.x;
				len += p.y;
			}
			const uint32_t crc = ~(raw ^ bz_shift_bytes(0xFFFFFFFFu, len, pw));
			results[i].crc = crc;
			st.total_out += r.out_len;
			st.start_bit = r.end_bit;
			if (S.info->end_run || crc != r.stored_crc) {
				results[i].status = S.info->end_run ? LA_ST_BZ2_DATA : LA_ST_BZ2_BAD_CRC;
				st.first_bad = i;
				i++;
				break;
			}
			st.crc = ((st.crc << 1) | (st.crc >> 31)) ^ crc;
		} else {
			results[i].crc = st.crc;
			st.start_bit = r.end_bit;
			if (st.crc != r.stored_crc) {
				results[i].status = LA_ST_BZ2_BAD_CRC;
				st.first_bad = i;
				i++;
				break;
			}
			st.open = 0; st.crc = 0;
		}
	}
	st.n_taken = i;
	if (st.first_bad == 0xFFFFFFFFu && i == w.n_taken) {	/* everything the walk confirmed: its verdict stands */
		st.stop = w.stop; st.stop_entry = w.stop_entry; st.start_bit = w.start_bit; st.open = w.open; st.level = w.level;
	}
	*out = st;
}

void la_launch_bzip2_measure(hipStream_t s, const la_bz2_batch *bt, uint8_t *ws_base)
{
	bz_ws w;
	bz_ws_carve(&w, ws_base, bt->n, bt->slot_level);
	if (bt->n)
		hipLaunchKernelGGL(bz2_measure_kernel, dim3(bt->n), dim3(BZ_TPB), 0, s, bt->d_src, bt->src_bytes, bt->d_cands, bt->n, w.slots,
		    w.slot_bytes, w.cap, bt->options);
}

void la_launch_bzip2_walk(hipStream_t s, const la_bz2_batch *bt, uint8_t *ws_base)
{
	bz_ws w;
	bz_ws_carve(&w, ws_base, bt->n, bt->slot_level);
	hipLaunchKernelGGL(bz2_walk_kernel, dim3(1), dim3(1), 0, s, bt->d_src, bt->src_bytes, bt->d_cands, bt->n, (const uint8_t *)w.slots,
	    w.slot_bytes, bt->slot_level, *bt->state_in, bt->d_results, w.walk, w.in, bt->d_state_out);
}

void la_launch_bzip2_emit(hipStream_t s, const la_bz2_batch *bt, uint8_t *ws_base)
{
	bz_ws w;
	bz_ws_carve(&w, ws_base, bt->n, bt->slot_level);
	const uint32_t ne = bt->n_emit < bt->n ? bt->n_emit : bt->n;
	if (ne)
		hipLaunchKernelGGL(bz2_emit_kernel, dim3((bz_nch(w.cap) + BZ_TPB - 1) / BZ_TPB, ne), dim3(BZ_TPB), 0, s,
		    (const la_bz2_result *)bt->d_results, ne, (const uint8_t *)w.slots, w.slot_bytes, w.cap, (const la_bz2_state *)w.walk,
		    bt->d_dst, bt->dst_cap);
}

void la_launch_bzip2_verify(hipStream_t s, const la_bz2_batch *bt, uint8_t *ws_base)
{
	bz_ws w;
	bz_ws_carve(&w, ws_base, bt->n, bt->slot_level);
	const uint32_t ne = bt->n_emit < bt->n ? bt->n_emit : bt->n;
	hipLaunchKernelGGL(bz2_verify_kernel, dim3(1), dim3(1), 0, s, bt->d_cands, bt->d_results, ne, (const uint8_t *)w.slots, w.slot_bytes,
	    w.cap, (const la_bz2_state *)w.walk, (const la_bz2_state *)w.in, bt->dst_cap, bt->d_state_out);
}
