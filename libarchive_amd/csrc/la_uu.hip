/*
 * la_uu.hip -- uuencode and base64 lines on the device: the launches behind la_gpu_uu_decode.
 *
 * The per-line rules are la_uu_dev.h's; this file finds the lines, resolves their states and moves the bytes.  Every
 * phase is a launch of its own on the caller's stream and no workgroup waits for another: a total over workgroups is
 * always reduce (per workgroup), scan of the summaries (one workgroup), apply (per workgroup).
 *
 *   1  line starts   uu_count_kernel, uu_scan_tiles_kernel, uu_starts_kernel.  A workgroup stages a tile of UU_TILE
 *                    positions through LDS, 16 bytes per lane; position p of [0, src_bytes] is a line start when it is 0
 *                    or the byte in front of it ends a line (la_uu_is_line_end: '\n', or a '\r' that no '\n' follows; a
 *                    '\r' in the window's last byte ends a line only in a final window).  Starts and bad bytes are
 *                    counted per tile, the counts scanned, the starts written to the table.  With M starts there are
 *                    M - 1 whole lines; bytes behind the last start are a line only in a final window (nl = 0).
 *   2  records       uu_records_kernel: one lane per line, UU_LPB lines per workgroup, computes the line's record and
 *                    the workgroup composes the UU_LPB functions into one.  A line of more than UU_LONG_LINE bytes asks
 *                    the tiles' bad-byte counts for the whole tiles it covers.
 *   3  states        uu_scan_fn_kernel gives every workgroup of phase 2 the state in front of it, from the state in
 *                    front of the window; uu_apply_kernel scans the functions inside the workgroup again, so every line
 *                    has its state, its byte count under that state and its output offset inside the workgroup, and
 *                    the first line that enters STOP is an atomic minimum (no line behind it produces a byte: STOP is
 *                    absorbing); uu_scan_bytes_kernel scans the workgroups' byte counts and writes the result record.
 *   4  decode        uu_decode_kernel: the lines of one workgroup of phase 2 are contiguous in the source and in the
 *                    output.  Their source is staged in LDS with 16-byte loads, every lane decodes its line from LDS to
 *                    LDS, and the output leaves as whole 16-byte stores on the output's 16-byte grid (bytes only at the
 *                    two ends, where the neighbours own the rest of the 16).  A workgroup whose lines do not fit
 *                    (UU_SRC_LDS, UU_OUT_LDS: lines of many hundred bytes) decodes them from and to global memory.
 *
 * The number of lines is known on the device only, so the per-line kernels walk their workgroups in a grid-stride loop
 * over a grid sized from src_bytes.  Offsets are 32-bit: src_bytes <= LA_UU_MAX_SRC_BYTES.
 */
#include "la_dev.h"

#define LA_UU_FN __host__ __device__ __forceinline__
#include "la_uu_dev.h"

#define UU_TILE      4096u	/* positions per workgroup of phase 1: 256 lanes x 16 bytes */
#define UU_LPB       256u	/* lines per workgroup of phases 2 to 4 */
#define UU_LONG_LINE 8192u
#define UU_SRC_LDS   24576u
#define UU_OUT_LDS   16384u
#define UU_NO_LINE   0xFFFFFFFFu

struct uu_glob {
	uint32_t n_starts;	/* M */
	uint32_t n_lines;
	uint32_t tail;		/* bytes stand behind the last start */
	uint32_t stop_line;
	uint32_t n_headers;
	uint32_t last_header;	/* line + 1 */
	uint32_t final_state;
	uint32_t pad;
};

struct uu_ws {
	uu_glob *glob;
	uint32_t *tile_cnt, *tile_base, *bad_cnt;
	uint32_t *starts;
	uint64_t *recs;
	uint32_t *blk_fn, *blk_state, *blk_bytes, *blk_base;
};

static uint32_t uu_tiles(uint64_t n) { return (uint32_t)((n + 1u + UU_TILE - 1u) / UU_TILE); }
static uint32_t uu_max_blocks(uint64_t n) { return (uint32_t)((n + 1u) / UU_LPB + 2u); }

static uint64_t uu_carve(uu_ws *w, uint8_t *base, uint64_t n)
{
	la_carve cv = { base, 0 };
	const uint32_t nt = uu_tiles(n), nb = uu_max_blocks(n);
	w->glob = cv.take<uu_glob>(1, 256);
	w->tile_cnt = cv.take<uint32_t>(nt + 1u, 256);
	w->tile_base = cv.take<uint32_t>(nt + 1u, 256);
	w->bad_cnt = cv.take<uint32_t>(nt + 1u, 256);
	w->starts = cv.take<uint32_t>(n + 3u, 256);
	w->recs = cv.take<uint64_t>(n + 2u, 256);
	w->blk_fn = cv.take<uint32_t>(nb, 256);
	w->blk_state = cv.take<uint32_t>(nb, 256);
	w->blk_bytes = cv.take<uint32_t>(nb, 256);
	w->blk_base = cv.take<uint32_t>(nb, 256);
	return cv.off + 256u;
}

uint64_t la_uu_workspace_bytes(uint64_t src_bytes)
{
	uu_ws w;
	return uu_carve(&w, nullptr, src_bytes);
}

/* exclusive scan over the 256 lanes of a workgroup; *total is the sum.  tmp: 256 words of LDS */
__device__ __forceinline__ uint32_t uu_wg_scan_add(uint32_t v, uint32_t *tmp, uint32_t *total)
{
	const uint32_t tid = threadIdx.x;
	tmp[tid] = v;
	__syncthreads();
	for (uint32_t d = 1; d < 256u; d <<= 1) {
		const uint32_t a = tid >= d ? tmp[tid - d] : 0u;
		__syncthreads();
		tmp[tid] += a;
		__syncthreads();
	}
	const uint32_t incl = tmp[tid];
	*total = tmp[255];
	__syncthreads();
	return incl - v;
}

/* inclusive scan of functions under composition, earlier lanes first; *total is the workgroup's function.  Returns the
 * function of the lanes IN FRONT of this one. */
__device__ __forceinline__ uint32_t uu_wg_scan_fn(uint32_t f, uint32_t *tmp, uint32_t *total)
{
	const uint32_t tid = threadIdx.x;
	tmp[tid] = f;
	__syncthreads();
	for (uint32_t d = 1; d < 256u; d <<= 1) {
		const uint32_t a = tid >= d ? tmp[tid - d] : (uint32_t)LA_UU_FN_IDENTITY;
		__syncthreads();
		tmp[tid] = la_uu_compose(a, tmp[tid]);
		__syncthreads();
	}
	const uint32_t before = tid ? tmp[tid - 1] : (uint32_t)LA_UU_FN_IDENTITY;
	*total = tmp[255];
	__syncthreads();
	return before;
}

/* ---- phase 1 ---- */

/* the tile's bytes to lds[16 ..], the byte in front of the tile to lds[15] ('\n' in front of the window: position 0 is a start) */
__device__ __forceinline__ void uu_stage_tile(const uint8_t *__restrict__ src, uint32_t n, uint32_t t0, uint8_t *lds)
{
	const uint32_t tid = threadIdx.x, g = t0 + 16u * tid;
	uint8_t *to = lds + 16u + 16u * tid;
	if (g + 16u <= n && g + 16u > g)
		lds_st16(to, ld_u128(src + g));
	else
		for (uint32_t j = 0; j < 16u; j++)
			to[j] = g + j < n ? src[g + j] : (uint8_t)0;
	if (tid == 0)
		lds[15] = t0 ? src[t0 - 1u] : (uint8_t)'\n';
	__syncthreads();
}

/* bit j: position t0 + 16 tid + j is a line start; *bad: bad bytes among this lane's 16 */
__device__ __forceinline__ uint32_t uu_lane_starts(const uint8_t *lds, uint32_t n, uint32_t t0, int final, uint32_t *bad)
{
	const uint32_t tid = threadIdx.x;
	uint32_t m = 0, nbad = 0, prev = lds[15u + 16u * tid];
	for (uint32_t j = 0; j < 16u; j++) {
		const uint32_t p = t0 + 16u * tid + j;
		if (p > n)
			break;
		const uint32_t c = lds[16u + 16u * tid + j];
		if (la_uu_is_line_end(prev, p < n, c, final))
			m |= 1u << j;
		if (p < n && la_uu_is_bad(c))
			nbad++;
		prev = c;
	}
	*bad = nbad;
	return m;
}

__global__ __launch_bounds__(256) void uu_count_kernel(const uint8_t *__restrict__ src, uint32_t n, int final, uint32_t *__restrict__ tile_cnt,
    uint32_t *__restrict__ bad_cnt)
{
	__shared__ __attribute__((aligned(16))) uint8_t lds[16u + UU_TILE];
	__shared__ uint32_t cnt[2];
	const uint32_t t0 = blockIdx.x * UU_TILE;
	if (threadIdx.x < 2)
		cnt[threadIdx.x] = 0;
	uu_stage_tile(src, n, t0, lds);
	uint32_t bad;
	const uint32_t m = uu_lane_starts(lds, n, t0, final, &bad);
	if (m)
		atomicAdd(&cnt[0], (uint32_t)__builtin_popcount(m));
	if (bad)
		atomicAdd(&cnt[1], bad);
	__syncthreads();
	if (threadIdx.x == 0) {
		tile_cnt[blockIdx.x] = cnt[0];
		bad_cnt[blockIdx.x] = cnt[1];
	}
}

/* exclusive scan of in[0, n) by ONE workgroup of 1024 lanes: a chunk per lane, the lanes' sums by lane 0, the chunks again */
__device__ __forceinline__ uint32_t uu_scan_u32(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, uint32_t n, uint32_t *sums)
{
	const uint32_t tid = threadIdx.x, chunk = (n + 1023u) / 1024u;
	const uint32_t lo = tid * chunk < n ? tid * chunk : n, hi = lo + chunk < n ? lo + chunk : n;
	uint32_t s = 0;
	for (uint32_t i = lo; i < hi; i++)
		s += in[i];
	sums[tid] = s;
	__syncthreads();
	if (tid == 0) {
		uint32_t acc = 0;
		for (uint32_t t = 0; t < 1024u; t++) {
			const uint32_t v = sums[t];
			sums[t] = acc;
			acc += v;
		}
		sums[1024] = acc;
	}
	__syncthreads();
	s = sums[tid];
	for (uint32_t i = lo; i < hi; i++) {
		const uint32_t v = in[i];
		out[i] = s;
		s += v;
	}
	return sums[1024];
}

__global__ __launch_bounds__(1024) void uu_scan_tiles_kernel(const uint32_t *__restrict__ tile_cnt, uint32_t *__restrict__ tile_base, uint32_t nt,
    uu_glob *__restrict__ glob)
{
	__shared__ uint32_t sums[1025];
	const uint32_t total = uu_scan_u32(tile_cnt, tile_base, nt, sums);
	if (threadIdx.x == 0) {
		/* every field of the call's record starts here: nothing is left from the call before */
		glob->n_starts = total;
		glob->n_lines = 0;
		glob->tail = 0;
		glob->stop_line = UU_NO_LINE;
		glob->n_headers = 0;
		glob->last_header = 0;
		glob->final_state = 0;
		glob->pad = 0;
	}
}

__global__ __launch_bounds__(256) void uu_starts_kernel(const uint8_t *__restrict__ src, uint32_t n, int final, const uint32_t *__restrict__ tile_base,
    uint32_t *__restrict__ starts, uu_glob *__restrict__ glob)
{
	__shared__ __attribute__((aligned(16))) uint8_t lds[16u + UU_TILE];
	__shared__ uint32_t tmp[256];
	const uint32_t t0 = blockIdx.x * UU_TILE;
	uu_stage_tile(src, n, t0, lds);
	uint32_t bad, total;
	uint32_t m = uu_lane_starts(lds, n, t0, final, &bad);
	uint32_t at = tile_base[blockIdx.x] + uu_wg_scan_add((uint32_t)__builtin_popcount(m), tmp, &total);
	const uint32_t last = glob->n_starts - 1u;	/* (position 0 is always a start) */
	while (m) {
		const uint32_t j = (uint32_t)__builtin_ctz(m), p = t0 + 16u * threadIdx.x + j;
		m &= m - 1u;
		starts[at] = p;
		if (at == last) {
			const uint32_t tail = p < n;
			glob->tail = tail;
			glob->n_lines = last + (final && tail ? 1u : 0u);
			starts[last + 1u] = n;
		}
		at++;
	}
}

/* ---- phase 2 ---- */

__device__ __forceinline__ uint32_t uu_blocks_of(uint32_t n_lines) { return (n_lines + UU_LPB - 1u) / UU_LPB; }

__device__ __forceinline__ int uu_line_has_bad(const uint8_t *__restrict__ src, uint32_t s, uint32_t e, const uint32_t *__restrict__ bad_cnt)
{
	if (e - s <= UU_LONG_LINE)
		return la_uu_has_bad(src + s, e - s);
	uint32_t i = s;
	while (i < e) {
		if ((i & (UU_TILE - 1u)) == 0 && e - i >= UU_TILE) {
			if (bad_cnt[i / UU_TILE])
				return 1;
			i += UU_TILE;
		} else {
			if (la_uu_is_bad(src[i]))
				return 1;
			i++;
		}
	}
	return 0;
}

__global__ __launch_bounds__(256) void uu_records_kernel(const uint8_t *__restrict__ src, int final, const uint32_t *__restrict__ starts,
    const uint32_t *__restrict__ bad_cnt, const uu_glob *__restrict__ glob, uint64_t *__restrict__ recs, uint32_t *__restrict__ blk_fn)
{
	__shared__ uint32_t tmp[256];
	const uint32_t n_lines = glob->n_lines, nb = uu_blocks_of(n_lines);
	const uint32_t open_tail = final && glob->tail;	/* the last line has no line end */
	for (uint32_t b = blockIdx.x; b < nb; b += gridDim.x) {
		const uint32_t line = b * UU_LPB + threadIdx.x;
		uint64_t rec = LA_UU_FN_IDENTITY;
		if (line < n_lines) {
			const uint32_t s = starts[line], e = starts[line + 1u], len = e - s;
			uint32_t nl = 0;
			if (!(open_tail && line == n_lines - 1u))
				nl = src[e - 1u] == '\n' && len >= 2u && src[e - 2u] == '\r' ? 2u : 1u;
			rec = la_uu_line_record(src + s, len, nl, uu_line_has_bad(src, s, e - nl, bad_cnt));
			recs[line] = rec;
		}
		uint32_t total;
		uu_wg_scan_fn((uint32_t)rec & 0x7fffu, tmp, &total);
		if (threadIdx.x == 0)
			blk_fn[b] = total;
	}
}

/* ---- phase 3 ---- */

__global__ __launch_bounds__(1024) void uu_scan_fn_kernel(const uint32_t *__restrict__ blk_fn, uint32_t *__restrict__ blk_state, uint32_t seed,
    uu_glob *__restrict__ glob)
{
	__shared__ uint32_t fns[1024];
	const uint32_t n = uu_blocks_of(glob->n_lines);
	const uint32_t tid = threadIdx.x, chunk = (n + 1023u) / 1024u;
	const uint32_t lo = tid * chunk < n ? tid * chunk : n, hi = lo + chunk < n ? lo + chunk : n;
	uint32_t f = (uint32_t)LA_UU_FN_IDENTITY;
	for (uint32_t i = lo; i < hi; i++)
		f = la_uu_compose(f, blk_fn[i]);
	fns[tid] = f;
	__syncthreads();
	if (tid == 0) {
		uint32_t st = seed;
		for (uint32_t t = 0; t < 1024u; t++) {
			const uint32_t g = fns[t];
			fns[t] = st;
			st = la_uu_rec_next(g, st);
		}
		glob->final_state = st;
	}
	__syncthreads();
	uint32_t st = fns[tid];
	for (uint32_t i = lo; i < hi; i++) {
		blk_state[i] = st;
		st = la_uu_rec_next(blk_fn[i], st);
	}
}

/* recs[line] becomes: bits 0..31 output offset inside the workgroup, 32..47 bytes, 48..50 state in front, 51..53 the
 * reason the line stops for (in that state) */
__global__ __launch_bounds__(256) void uu_apply_kernel(const uint32_t *__restrict__ blk_state, uu_glob *__restrict__ glob, uint64_t *__restrict__ recs,
    uint32_t *__restrict__ blk_bytes)
{
	__shared__ uint32_t tmp[256];
	const uint32_t n_lines = glob->n_lines, nb = uu_blocks_of(n_lines);
	for (uint32_t b = blockIdx.x; b < nb; b += gridDim.x) {
		const uint32_t line = b * UU_LPB + threadIdx.x;
		const uint64_t rec = line < n_lines ? recs[line] : LA_UU_FN_IDENTITY;
		uint32_t total;
		const uint32_t before = uu_wg_scan_fn((uint32_t)rec & 0x7fffu, tmp, &total);
		const uint32_t st = la_uu_rec_next(before, blk_state[b]);
		const uint32_t nxt = la_uu_rec_next(rec, st);
		const uint32_t bytes = line < n_lines && nxt != LA_UU_STOP ? la_uu_rec_bytes(rec, st) : 0u;
		if (line < n_lines && st != LA_UU_STOP && nxt == LA_UU_STOP)
			atomicMin(&glob->stop_line, line);
		if (line < n_lines && st == LA_UU_FIND_HEAD && (nxt == LA_UU_READ_UU || nxt == LA_UU_READ_BASE64)) {
			atomicAdd(&glob->n_headers, 1u);
			atomicMax(&glob->last_header, line + 1u);
		}
		const uint32_t rel = uu_wg_scan_add(bytes, tmp, &total);
		if (line < n_lines)
			recs[line] = (uint64_t)rel | (uint64_t)bytes << 32 | (uint64_t)st << 48 | (uint64_t)la_uu_rec_reason(rec, st) << 51;
		if (threadIdx.x == 0)
			blk_bytes[b] = total;
	}
}

__global__ __launch_bounds__(1024) void uu_scan_bytes_kernel(const uint32_t *__restrict__ blk_bytes, uint32_t *__restrict__ blk_base,
    const uu_glob *__restrict__ glob, const uint32_t *__restrict__ starts, const uint64_t *__restrict__ recs, uint32_t in_decoded,
    la_uu_result *__restrict__ result)
{
	__shared__ uint32_t sums[1025];
	const uint32_t n_lines = glob->n_lines;
	const uint32_t total = uu_scan_u32(blk_bytes, blk_base, uu_blocks_of(n_lines), sums);
	if (threadIdx.x != 0)
		return;
	la_uu_result r;
	r.out_len = total;
	r.decoded = in_decoded || total != 0;
	r.reserved = 0;
	const uint32_t k = glob->stop_line;
	if (k != UU_NO_LINE) {
		r.status = la_uu_reason_status((uint32_t)(recs[k] >> 51) & 7u, (int)r.decoded);
		r.state = LA_UU_STOP;
		r.consumed = r.stop_off = starts[k];
	} else {
		r.status = LA_ST_OK;
		r.state = glob->final_state;
		r.consumed = r.stop_off = starts[n_lines];
	}
	r.n_headers = glob->n_headers;
	r.head_off = 0;
	r.head_len = 0;
	if (r.n_headers) {
		const uint32_t h = glob->last_header - 1u;
		r.head_off = starts[h];
		r.head_len = starts[h + 1u] - starts[h];
	}
	*result = r;
}

/* ---- phase 4 ---- */

__global__ __launch_bounds__(256) void uu_decode_kernel(const uint8_t *__restrict__ src, uint32_t n, const uint32_t *__restrict__ starts,
    const uint64_t *__restrict__ recs, const uu_glob *__restrict__ glob, const uint32_t *__restrict__ blk_bytes, const uint32_t *__restrict__ blk_base,
    uint8_t *__restrict__ dst)
{
	__shared__ __attribute__((aligned(16))) uint8_t lsrc[UU_SRC_LDS];
	__shared__ __attribute__((aligned(16))) uint8_t lout[UU_OUT_LDS];
	const uint32_t n_lines = glob->n_lines, nb = uu_blocks_of(n_lines), tid = threadIdx.x;
	for (uint32_t b = blockIdx.x; b < nb; b += gridDim.x) {
		const uint32_t ob = blk_bytes[b];
		if (ob == 0)
			continue;
		const uint32_t line0 = b * UU_LPB, cnt = n_lines - line0 < UU_LPB ? n_lines - line0 : UU_LPB;
		const uint32_t line = line0 + tid;
		const uint32_t s0 = starts[line0], s1 = starts[line0 + cnt], a0 = s0 & ~15u;
		const uint32_t o0 = blk_base[b], h = o0 & 15u;
		uint32_t rel = 0, bytes = 0, st = 0, ls = 0;
		if (tid < cnt) {
			const uint64_t rec = recs[line];
			rel = (uint32_t)rec;
			bytes = (uint32_t)(rec >> 32) & 0xffffu;
			st = (uint32_t)(rec >> 48) & 7u;
			ls = starts[line];
		}
		if (s1 - a0 > UU_SRC_LDS || h + ob > UU_OUT_LDS) {
			/* long lines: every byte of [o0, o0 + ob) is one of these lines' */
			if (bytes)
				la_uu_decode_line(src + ls, st, bytes, dst + o0 + rel);
			continue;
		}
		const uint32_t nsrc = (s1 - a0 + 15u) >> 4;
		for (uint32_t c = tid; c < nsrc; c += 256u) {
			const uint32_t g = a0 + 16u * c;
			if (n - g >= 16u)
				lds_st16(lsrc + 16u * c, ld_u128(src + g));
			else
				for (uint32_t j = 0; g + j < n; j++)
					lsrc[16u * c + j] = src[g + j];
		}
		__syncthreads();
		if (bytes)
			la_uu_decode_line(lsrc + (ls - a0), st, bytes, lout + h + rel);
		__syncthreads();
		uint8_t *to = dst + (o0 - h);
		const uint32_t nout = (h + ob + 15u) >> 4;
		for (uint32_t c = tid; c < nout; c += 256u) {
			const uint32_t lo = 16u * c, hi = lo + 16u;
			if (lo >= h && hi <= h + ob) {
				const uint4 v = lds_ld16(lout + lo);
				__builtin_memcpy(to + lo, &v, 16);
			} else
				for (uint32_t j = lo < h ? h : lo; j < hi && j < h + ob; j++)
					to[j] = lout[j];
		}
		__syncthreads();
	}
}

/* the four phases, each on its own so that the API layer can time them */
struct uu_launch {
	uu_ws w;
	uint32_t n, nt, grid;
	int final;
};
static uu_launch uu_plan(const la_uu_batch *bt, uint8_t *ws)
{
	uu_launch L;
	uu_carve(&L.w, ws, bt->src_bytes);
	L.n = (uint32_t)bt->src_bytes;
	L.nt = uu_tiles(L.n);
	L.grid = uu_max_blocks(L.n) < 4096u ? uu_max_blocks(L.n) : 4096u;
	L.final = bt->final != 0;
	return L;
}

void la_launch_uu_lines(hipStream_t s, const la_uu_batch *bt, uint8_t *ws)
{
	const uu_launch L = uu_plan(bt, ws);
	const uu_ws &w = L.w;
	hipLaunchKernelGGL(uu_count_kernel, dim3(L.nt), dim3(256), 0, s, bt->d_src, L.n, L.final, w.tile_cnt, w.bad_cnt);
	hipLaunchKernelGGL(uu_scan_tiles_kernel, dim3(1), dim3(1024), 0, s, (const uint32_t *)w.tile_cnt, w.tile_base, L.nt, w.glob);
	hipLaunchKernelGGL(uu_starts_kernel, dim3(L.nt), dim3(256), 0, s, bt->d_src, L.n, L.final, (const uint32_t *)w.tile_base, w.starts, w.glob);
}

void la_launch_uu_records(hipStream_t s, const la_uu_batch *bt, uint8_t *ws)
{
	const uu_launch L = uu_plan(bt, ws);
	const uu_ws &w = L.w;
	hipLaunchKernelGGL(uu_records_kernel, dim3(L.grid), dim3(256), 0, s, bt->d_src, L.final, (const uint32_t *)w.starts, (const uint32_t *)w.bad_cnt,
	    (const uu_glob *)w.glob, w.recs, w.blk_fn);
}

void la_launch_uu_states(hipStream_t s, const la_uu_batch *bt, uint8_t *ws)
{
	const uu_launch L = uu_plan(bt, ws);
	const uu_ws &w = L.w;
	hipLaunchKernelGGL(uu_scan_fn_kernel, dim3(1), dim3(1024), 0, s, (const uint32_t *)w.blk_fn, w.blk_state, bt->in.state, w.glob);
	hipLaunchKernelGGL(uu_apply_kernel, dim3(L.grid), dim3(256), 0, s, (const uint32_t *)w.blk_state, w.glob, w.recs, w.blk_bytes);
	hipLaunchKernelGGL(uu_scan_bytes_kernel, dim3(1), dim3(1024), 0, s, (const uint32_t *)w.blk_bytes, w.blk_base, (const uu_glob *)w.glob,
	    (const uint32_t *)w.starts, (const uint64_t *)w.recs, bt->in.decoded ? 1u : 0u, bt->d_result);
}

void la_launch_uu_decode(hipStream_t s, const la_uu_batch *bt, uint8_t *ws)
{
	const uu_launch L = uu_plan(bt, ws);
	const uu_ws &w = L.w;
	hipLaunchKernelGGL(uu_decode_kernel, dim3(L.grid), dim3(256), 0, s, bt->d_src, L.n, (const uint32_t *)w.starts, (const uint64_t *)w.recs,
	    (const uu_glob *)w.glob, (const uint32_t *)w.blk_bytes, (const uint32_t *)w.blk_base, bt->d_dst);
}
