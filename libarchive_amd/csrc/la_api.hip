/*
 * la_api.hip -- the extern "C" shim declared in include/la_gpu.h.
 *
 * Owns the HIP context objects (stream, events, workspace) and sequences the
 * kernels of one batch; all arithmetic lives in the kernel files.  No host
 * fallback exists: without a usable gfx950 device la_gpu_open() fails and every
 * caller above it fails loudly.
 */
#include "la_dev.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <new>

#define LA_MAX_SLICES 8
#define LA_GZ_LANES_MIN 8192u	/* members per batch from which the lane-per-member kernel is used (wave-per-member below: 4096 members 12.7 vs 23.8 ms, 16384 members 47.7 vs 26.0 ms) */
#define LA_PROF_MAX_RANGES 64

struct la_gpu_ctx {
	int device;
	hipStream_t own_stream;
	hipStream_t stream;
	hipEvent_t ev0, ev1;
	hipEvent_t mark;
	void *ws;
	uint64_t ws_bytes;
	/* dependency words of the lz4 window blocks (la_lz4_deps.hip), one per sequence-table slot: a buffer of its
	 * own beside the workspace, grown by the decode that needs it (la_gpu_lz4_workspace_bytes is a recorded
	 * public figure and keeps describing ws alone) */
	uint32_t *lz4_deps;
	uint64_t lz4_deps_cap;	/* words */
	/* literal plans of the same blocks, written by the same kernel (la_lz4_lit_chunk_edge): one byte per table slot
	 * entry, lz4_deps_cap bytes, reserved with the words */
	uint8_t *lz4_plan;
	/* second stream + events: block checksums / parse of later slices run beside the
	 * expand kernels of earlier ones */
	hipStream_t aux_stream;
	hipEvent_t slice_ev[LA_MAX_SLICES + 1];
	/* a split last slice (la_lz4_slices.h): one event behind each group's launch, and the frames' hash states between
	 * the passes, one LA_XXH_CARRY_BYTES record per block of the slice; grown like lz4_deps, never cleared */
	hipEvent_t split_ev[LA_LZ4_SPLIT_MAX_GROUPS];
	void *lz4_carry;
	uint64_t lz4_carry_cap;	/* records */
	/* optional timing of the last batch: one (start, stop) event pair per kernel range,
	 * recorded on the stream the kernels run on, summed by name when read */
	int prof_on;
	int prof_n;
	hipEvent_t prof_a[LA_PROF_MAX_RANGES], prof_b[LA_PROF_MAX_RANGES];
	const char *prof_name[LA_PROF_MAX_RANGES];
	char err[256];
};

static void prof_begin(la_gpu_ctx *c) { c->prof_n = 0; }
/* returns a handle to close with prof_close, or -1 */
static int prof_open(la_gpu_ctx *c, const char *name, hipStream_t s)
{
	if (!c->prof_on || c->prof_n >= LA_PROF_MAX_RANGES)
		return -1;
	int h = c->prof_n++;
	c->prof_name[h] = name;
	(void)hipEventRecord(c->prof_a[h], s);
	return h;
}
static void prof_close(la_gpu_ctx *c, int h, hipStream_t s)
{
	if (h >= 0)
		(void)hipEventRecord(c->prof_b[h], s);
}

template <typename Launch>
static void prof_range(la_gpu_ctx *c, const char *name, hipStream_t s, Launch launch)	/* one named range around what launch() queues on s */
{
	const int h = prof_open(c, name, s);
	launch();
	prof_close(c, h, s);
}

#define HIPCHK(ctx, call)                                                              \
	do {                                                                           \
		hipError_t e_ = (call);                                                \
		if (e_ != hipSuccess) {                                                \
			snprintf((ctx)->err, sizeof((ctx)->err), "%s: %s", #call,      \
			    hipGetErrorString(e_));                                    \
			return LA_ERR_HIP;                                             \
		}                                                                      \
	} while (0)

extern "C" {

int la_gpu_abi_version(void) { return LA_GPU_ABI_VERSION; }

int la_gpu_device_count(void)
{
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess)
		return 0;
	return n;
}

int la_gpu_open(int device, la_gpu_ctx **out)
{
	if (!out)
		return LA_ERR_ARG;
	*out = NULL;
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n)
		return LA_ERR_NO_DEVICE;
	la_gpu_ctx *c = new (std::nothrow) la_gpu_ctx();
	if (!c)
		return LA_ERR_NOMEM;
	memset(c, 0, sizeof(*c));
	c->device = device;
	if (hipSetDevice(device) != hipSuccess ||
	    hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess ||
	    hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess ||
	    hipEventCreateWithFlags(&c->mark, hipEventDisableTiming) != hipSuccess) {
		delete c;
		return LA_ERR_NO_DEVICE;
	}
	for (int i = 0; i < LA_PROF_MAX_RANGES; i++) {
		(void)hipEventCreate(&c->prof_a[i]);
		(void)hipEventCreate(&c->prof_b[i]);
	}
	(void)hipStreamCreateWithFlags(&c->aux_stream, hipStreamNonBlocking);
	for (int i = 0; i <= LA_MAX_SLICES; i++)
		(void)hipEventCreateWithFlags(&c->slice_ev[i], hipEventDisableTiming);
	for (uint32_t i = 0; i < LA_LZ4_SPLIT_MAX_GROUPS; i++)
		(void)hipEventCreateWithFlags(&c->split_ev[i], hipEventDisableTiming);
	c->stream = c->own_stream;
	*out = c;
	return LA_OK;
}

void la_gpu_close(la_gpu_ctx *c)
{
	if (!c)
		return;
	(void)hipSetDevice(c->device);
	(void)hipStreamSynchronize(c->stream);
	if (c->ws) (void)hipFree(c->ws);
	if (c->lz4_deps) (void)hipFree(c->lz4_deps);
	if (c->lz4_plan) (void)hipFree(c->lz4_plan);
	if (c->lz4_carry) (void)hipFree(c->lz4_carry);
	(void)hipEventDestroy(c->ev0);
	(void)hipEventDestroy(c->ev1);
	(void)hipEventDestroy(c->mark);
	for (int i = 0; i < LA_PROF_MAX_RANGES; i++) {
		(void)hipEventDestroy(c->prof_a[i]);
		(void)hipEventDestroy(c->prof_b[i]);
	}
	for (int i = 0; i <= LA_MAX_SLICES; i++)
		(void)hipEventDestroy(c->slice_ev[i]);
	for (uint32_t i = 0; i < LA_LZ4_SPLIT_MAX_GROUPS; i++)
		(void)hipEventDestroy(c->split_ev[i]);
	(void)hipStreamSynchronize(c->aux_stream);
	(void)hipStreamDestroy(c->aux_stream);
	(void)hipStreamDestroy(c->own_stream);
	delete c;
}

int la_gpu_set_stream(la_gpu_ctx *c, void *hip_stream)
{
	if (!c) return LA_ERR_ARG;
	c->stream = hip_stream ? (hipStream_t)hip_stream : c->own_stream;
	return LA_OK;
}

int la_gpu_sync(la_gpu_ctx *c)
{
	if (!c) return LA_ERR_ARG;
	HIPCHK(c, hipStreamSynchronize(c->stream));
	return LA_OK;
}

const char *la_gpu_last_error(const la_gpu_ctx *c) { return c ? c->err : "no context"; }

int la_gpu_reserve(la_gpu_ctx *c, uint64_t bytes)
{
	if (!c) return LA_ERR_ARG;
	if (bytes <= c->ws_bytes)
		return LA_OK;
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	if (c->ws) { HIPCHK(c, hipFree(c->ws)); c->ws = NULL; c->ws_bytes = 0; }
	bytes = (bytes + 0xFFFFFull) & ~0xFFFFFull;
	HIPCHK(c, hipMalloc(&c->ws, bytes));
	c->ws_bytes = bytes;
	return LA_OK;
}

int la_gpu_malloc(la_gpu_ctx *c, void **p, uint64_t bytes)
{
	if (!c || !p) return LA_ERR_ARG;
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, hipMalloc(p, bytes ? bytes : 1));
	return LA_OK;
}
int la_gpu_free(la_gpu_ctx *c, void *p)
{
	if (!c) return LA_ERR_ARG;
	if (p) HIPCHK(c, hipFree(p));
	return LA_OK;
}
int la_gpu_malloc_host(la_gpu_ctx *c, void **p, uint64_t bytes)
{
	if (!c || !p) return LA_ERR_ARG;
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, hipHostMalloc(p, bytes ? bytes : 1, hipHostMallocDefault));
	return LA_OK;
}
int la_gpu_free_host(la_gpu_ctx *c, void *p)
{
	if (!c) return LA_ERR_ARG;
	if (p) HIPCHK(c, hipHostFree(p));
	return LA_OK;
}
int la_gpu_memcpy_h2d(la_gpu_ctx *c, void *d, const void *h, uint64_t bytes)
{
	if (!c) return LA_ERR_ARG;
	if (bytes) HIPCHK(c, hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, c->stream));
	return LA_OK;
}
int la_gpu_memcpy_d2h(la_gpu_ctx *c, void *h, const void *d, uint64_t bytes)
{
	if (!c) return LA_ERR_ARG;
	if (bytes) HIPCHK(c, hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, c->stream));
	return LA_OK;
}

int la_gpu_mark(la_gpu_ctx *c)
{
	if (!c) return LA_ERR_ARG;
	HIPCHK(c, hipEventRecord(c->mark, c->stream));
	return LA_OK;
}
int la_gpu_wait_mark(la_gpu_ctx *c)
{
	if (!c) return LA_ERR_ARG;
	HIPCHK(c, hipEventSynchronize(c->mark));
	return LA_OK;
}

int la_gpu_memcpy_d2d(la_gpu_ctx *c, void *d, const void *src_, uint64_t bytes)
{
	if (!c) return LA_ERR_ARG;
	if (bytes) HIPCHK(c, hipMemcpyAsync(d, src_, bytes, hipMemcpyDeviceToDevice, c->stream));
	return LA_OK;
}

int la_gpu_timer_start(la_gpu_ctx *c)
{
	if (!c) return LA_ERR_ARG;
	HIPCHK(c, hipEventRecord(c->ev0, c->stream));
	return LA_OK;
}
int la_gpu_timer_stop(la_gpu_ctx *c, float *ms)
{
	if (!c || !ms) return LA_ERR_ARG;
	HIPCHK(c, hipEventRecord(c->ev1, c->stream));
	HIPCHK(c, hipEventSynchronize(c->ev1));
	HIPCHK(c, hipEventElapsedTime(ms, c->ev0, c->ev1));
	return LA_OK;
}

int la_gpu_profile_enable(la_gpu_ctx *c, int on)
{
	if (!c) return LA_ERR_ARG;
	c->prof_on = on ? 1 : 0;
	c->prof_n = 0;
	return LA_OK;
}

int la_gpu_profile_read(la_gpu_ctx *c, float *ms, const char **names, int cap)
{
	if (!c || !ms) return LA_ERR_ARG;
	if (!c->prof_on || c->prof_n == 0)
		return 0;
	int n = 0;
	for (int i = 0; i < c->prof_n; i++) {
		float t = 0;
		HIPCHK(c, hipEventSynchronize(c->prof_b[i]));
		HIPCHK(c, hipEventElapsedTime(&t, c->prof_a[i], c->prof_b[i]));
		int k = 0;
		for (; k < n; k++)
			if (names && names[k] == c->prof_name[i])
				break;
		if (k == n) {
			if (n >= cap)
				continue;
			if (names) names[n] = c->prof_name[i];
			ms[n] = 0;
			n++;
		}
		ms[k] += t;
	}
	return n;
}

/* ------------------------------------------------------------------ hashes */

int la_gpu_xxh32_many(la_gpu_ctx *c, const uint8_t *d_base, const la_hash_job *d_jobs,
    uint32_t n, uint32_t *d_out)
{
	if (!c || (n && (!d_base || !d_jobs || !d_out))) return LA_ERR_ARG;
	la_launch_xxh32_many(c->stream, d_base, d_jobs, n, d_out);
	HIPCHK(c, hipGetLastError());
	return LA_OK;
}

int la_gpu_crc32_many(la_gpu_ctx *c, const uint8_t *d_base, const la_hash_job *d_jobs,
    uint32_t n, uint32_t *d_out)
{
	if (!c || (n && (!d_base || !d_jobs || !d_out))) return LA_ERR_ARG;
	la_launch_crc32_many(c->stream, d_base, d_jobs, n, d_out);
	HIPCHK(c, hipGetLastError());
	return LA_OK;
}

int la_gpu_adler32_many(la_gpu_ctx *c, const uint8_t *d_base, const la_hash_job *d_jobs,
    uint32_t n, uint32_t *d_out)
{
	if (!c || (n && (!d_base || !d_jobs || !d_out))) return LA_ERR_ARG;
	la_launch_adler32_many(c->stream, d_base, d_jobs, n, d_out);
	HIPCHK(c, hipGetLastError());
	return LA_OK;
}

/* ------------------------------------------------------------------ lz4 */

static uint64_t align_up(uint64_t v, uint64_t a) { return (v + a - 1) & ~(a - 1); }

/* workspace layout of one lz4 batch */
struct lz4_ws {
	uint32_t *nseq;		/* [n] */
	uint32_t *caps;		/* [n] table capacity per block */
	uint32_t *sum_status;	/* [n] block-checksum verdicts (merged into the status at the end) */
	uint32_t *big;		/* [n+1] count + list of blocks with more sequences than one LDS segment holds */
	uint64_t *table_off;	/* [n+1] */
	void *scan;		/* scan scratch */
	la_lz4_seq *table;
	uint64_t table_cap;	/* entries */
	uint64_t total;
};

/* (every field starts on a 256-byte boundary; the total is rounded up likewise, plus 4 KiB of slack) */
static void lz4_ws_carve(lz4_ws *w, uint8_t *base, uint32_t n, uint64_t src_bytes, bool with_table)
{
	la_carve cv = { base, 0 };
	w->nseq = cv.take<uint32_t>(n, 256);
	w->caps = cv.take<uint32_t>(n, 256);
	w->sum_status = cv.take<uint32_t>(n, 256);
	w->big = cv.take<uint32_t>(n + 1, 256);
	w->table_off = cv.take<uint64_t>((uint64_t)n + 1, 256);
	w->scan = cv.take<uint8_t>(la_scan_scratch_bytes(n), 256);
	/* a non-final sequence takes >= 3 payload bytes; slots are rounded up to 8 entries:
	 * sum((src_len/3 + 1 + 7) & ~7) <= src_bytes/3 + 8n */
	w->table_cap = with_table ? src_bytes / 3 + 8ull * n : 0;
	w->table = cv.take<la_lz4_seq>(w->table_cap, 256);
	w->total = align_up(cv.off, 256) + 4096;
}

uint64_t la_gpu_lz4_workspace_bytes(uint32_t n_blocks, uint64_t src_bytes)
{
	lz4_ws w;
	lz4_ws_carve(&w, NULL, n_blocks, src_bytes, true);
	return w.total;
}

/* Room for one dependency word and one byte of literal plan per table slot entry (5 B beside the entry's 8: on the
 * 16 GiB bench shape the table is 20 GB, the words 10 GB and the plans 2.5 GB; a filter's 64 MiB window asks for 90 MB
 * and 22 MB).  Grown like the workspace, never shrunk. */
static int lz4_deps_reserve(la_gpu_ctx *c, uint64_t words)
{
	if (words <= c->lz4_deps_cap)
		return LA_OK;
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	HIPCHK(c, hipStreamSynchronize(c->aux_stream));
	c->lz4_deps_cap = 0;
	if (c->lz4_deps) { HIPCHK(c, hipFree(c->lz4_deps)); c->lz4_deps = NULL; }
	if (c->lz4_plan) { HIPCHK(c, hipFree(c->lz4_plan)); c->lz4_plan = NULL; }
	words = (words + 0x3FFFFull) & ~0x3FFFFull;
	HIPCHK(c, hipMalloc((void **)&c->lz4_deps, words * sizeof(uint32_t)));
	HIPCHK(c, hipMalloc((void **)&c->lz4_plan, words));
	c->lz4_deps_cap = words;
	return LA_OK;
}

/* Room for the hash states of a split last slice (la_lz4_slices.h): 64 B per block of the slice, 4 MiB on the bench
 * shape.  A buffer of its own for the reason lz4_deps has one. */
static int lz4_carry_reserve(la_gpu_ctx *c, uint64_t records)
{
	if (records <= c->lz4_carry_cap)
		return LA_OK;
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	HIPCHK(c, hipStreamSynchronize(c->aux_stream));
	c->lz4_carry_cap = 0;
	if (c->lz4_carry) { HIPCHK(c, hipFree(c->lz4_carry)); c->lz4_carry = NULL; }
	records = (records + 0xFFFull) & ~0xFFFull;
	HIPCHK(c, hipMalloc(&c->lz4_carry, records * LA_XXH_CARRY_BYTES));
	c->lz4_carry_cap = records;
	return LA_OK;
}

/* Group bounds of a split last slice in sixteenths of the period, and whether the passes that run beside a later
 * group use the sixteen-lane form (the last pass always does).  Kept by the step time among (8, 13), (8, 14), (10, 15)
 * and (12), each with both forms: profiles/r32_lz4_last_slice.md, section 5. */
static const uint32_t lz4_split_sixteenths[] = { 8, 13, 16 };
static_assert(sizeof(lz4_split_sixteenths) / sizeof(lz4_split_sixteenths[0]) <= LA_LZ4_SPLIT_MAX_GROUPS, "too many groups");
static const bool lz4_split_row_hidden = false;

/* does a decode of this batch hand the polling kernel dependency words?  (not without tables, not under the
 * cross-check option, not when the in-order kernel expands) */
static bool lz4_uses_deps(const la_lz4_batch *bt)
{
	return !(bt->options & (LA_LZ4_OPT_GENERAL_ONLY | LA_LZ4_OPT_SEARCH_IN_EXPAND)) && bt->n_blocks &&
	    ((bt->options & LA_LZ4_OPT_EXPAND_INORDER) == 0 || !la_lz4_expand_inorder_takes(bt->src_bytes));
}

int la_gpu_lz4_decode(la_gpu_ctx *c, const la_lz4_batch *bt)
{
	if (!c || !bt)
		return LA_ERR_ARG;
	/* (d_dst_off even for an empty batch: the scan writes its one total there) */
	if (!bt->d_dst_off || (bt->n_blocks && (!bt->d_src || !bt->d_blocks || !bt->d_dst || !bt->d_out_len ||
	    !bt->d_block_status)))
		return LA_ERR_ARG;
	if (bt->n_frames && (!bt->d_frames || !bt->d_frame_status))
		return LA_ERR_ARG;
	const bool fast = !(bt->options & LA_LZ4_OPT_GENERAL_ONLY);
	const bool verify = !(bt->options & LA_LZ4_OPT_NO_VERIFY);
	/* the in-order expand kernel runs on request (cross-check); not for images of less than 16 bytes */
	const bool poll = (bt->options & LA_LZ4_OPT_EXPAND_INORDER) == 0 || !la_lz4_expand_inorder_takes(bt->src_bytes);
	lz4_ws w;
	lz4_ws_carve(&w, NULL, bt->n_blocks, bt->src_bytes, fast);
	if (w.total > c->ws_bytes) {
		int rc = la_gpu_reserve(c, w.total);
		if (rc != LA_OK) return rc;
	}
	lz4_ws_carve(&w, (uint8_t *)c->ws, bt->n_blocks, bt->src_bytes, fast);
	const bool with_deps = lz4_uses_deps(bt);
	if (with_deps) {
		int rc = lz4_deps_reserve(c, w.table_cap);
		if (rc != LA_OK) return rc;
	}
	const uint32_t n = bt->n_blocks;
	const uint32_t nsl = (fast && n >= 4u * 8192u) ? 4u : 1u;	/* expand slices */
	/* The last slice by position in the frame (la_lz4_slices.h), where the default window kernel runs and frames are
	 * checked: the frames' chains advance between its launches, and the step waits for the last group's bytes only.
	 * Decided here, from the batch's shape alone, so that the carries are reserved before anything is queued. */
	la_lz4_split split = { 0, 0, 0, 0, { 0 } };
	if (fast && poll && with_deps && verify && bt->n_frames && (nsl == 4 || (bt->options & LA_LZ4_OPT_SPLIT_SMALL))) {
		const uint32_t P = la_lz4_split_period(n, bt->n_frames);
		if (P) {
			const uint32_t first = nsl == 4 ? (uint32_t)((uint64_t)n * 3 / 4) / P * P : 0u;
			la_lz4_split_init(&split, first, n, P, lz4_split_sixteenths,
			    sizeof(lz4_split_sixteenths) / sizeof(lz4_split_sixteenths[0]));
			int rc = lz4_carry_reserve(c, n - first);
			if (rc != LA_OK) return rc;
		}
	}
	hipStream_t sx = c->stream;		/* main stream (the caller's): checksums, expand, summary */
	hipStream_t sp = c->aux_stream;		/* second stream: parse beside the block checksums, frame
						 * checksums beside the expand kernel */
	const la_expand_job xj = {	/* every expand launch below is this job, or a slice of it */ bt->d_src, bt->src_bytes, bt->d_blocks, n, bt->d_dst, bt->dst_cap, bt->d_dst_off,
	    bt->d_out_len, bt->d_block_status, w.nseq, fast ? w.table : NULL, w.table_off,
	    LA_LZ4_LONG_SEQ_BYTES,	/* blocks of few long sequences go to the general kernel (la_dev.h) */
	    with_deps ? c->lz4_deps : NULL, with_deps ? c->lz4_plan : NULL };

	prof_begin(c);
	/* the second stream starts after whatever the caller queued on its stream */
	HIPCHK(c, hipEventRecord(c->slice_ev[LA_MAX_SLICES], sx));
	HIPCHK(c, hipStreamWaitEvent(sp, c->slice_ev[LA_MAX_SLICES], 0));

	/* second stream: token-chain parse (+ sequence tables) of the whole batch.  One lane per
	 * block: it needs the whole table in one launch to fill the chip.  Parsing slice by slice
	 * beside the expand launches was measured and is slower (profiles/r06_parse_pipeline.md):
	 * the parse's small workgroups take every LDS gap a finished expand workgroup leaves, the
	 * expand kernel stands still until they are through, and four partial rounds of the parse
	 * cost 7.2 ms where one launch costs 4.4. */
	if (n)
		HIPCHK(c, hipMemsetAsync(bt->d_block_status, 0, (size_t)n * sizeof(uint32_t), sp));
	if (fast) {
		la_launch_lz4_table_caps(sp, bt->d_blocks, n, w.caps);
		la_launch_scan_u32(sp, w.caps, n, w.table_off, w.scan);
	}
	/* block checksums (into their own verdict array) and the token-chain parse: one fused
	 * kernel that stages the image through LDS and reads it from HBM once; the
	 * first-generation pair of kernels stays selectable as a cross-check */
	if (verify && n)
		HIPCHK(c, hipMemsetAsync(w.sum_status, 0, (size_t)n * sizeof(uint32_t), sp));
	if (bt->options & LA_LZ4_OPT_PARSE_V1) {
		if (verify && n)
			prof_range(c, "lz4_block_sums", sp, [&] { la_launch_lz4_block_sums(sp, bt->d_src, bt->d_blocks, n, w.sum_status); });
		prof_range(c, "lz4_parse", sp, [&] {
			la_launch_lz4_parse(sp, bt->d_src, bt->src_bytes, bt->d_blocks, n, bt->d_out_len, w.nseq,
			    bt->d_block_status, fast ? w.table : NULL, w.table_off, w.table_cap);
		});
	} else {
		prof_range(c, "lz4_parse", sp, [&] {
			la_launch_lz4_parse_staged(sp, bt->d_src, bt->src_bytes, bt->d_blocks, n, bt->d_out_len, w.nseq,
			    bt->d_block_status, verify ? w.sum_status : NULL, fast ? w.table : NULL, w.table_off, w.table_cap);
		});
	}
	HIPCHK(c, hipEventRecord(c->slice_ev[0], sp));

	HIPCHK(c, hipStreamWaitEvent(sx, c->slice_ev[0], 0));
	prof_range(c, "scan", sx, [&] { la_launch_scan_u32(sx, bt->d_out_len, n, bt->d_dst_off, w.scan); });
	/* what each match of a window block waits for, once over the whole table, at eight workgroups per CU (the
	 * window kernel, at two, used to search for it).  In front of the slices, not beside them: with slice i + 1's
	 * share on the second stream beside expand slice i the step took 25.48 ms against 25.37 (three runs each,
	 * profiles/r25_lz4_deps.md) -- two window workgroups leave 3 KiB of a CU's LDS, so the dependency kernel only
	 * ever gets in where an expand workgroup has just left */
	if (with_deps)
		prof_range(c, "lz4_deps", sx, [&] { la_launch_lz4_deps(sx, xj, c->lz4_deps, c->lz4_plan); });

	/* blocks the LDS-window kernel does not take (any size, stored, chains of dependent
	 * blocks) first, over the whole table; then the LDS-window kernel in slices, each
	 * slice's frames hashed on the second stream while the next slice expands.  The last
	 * slice has no next one: where it can (below) it goes out in groups of period positions,
	 *     main stream:    slice 1 | slice 2 | slice 3 | group 0    | group 1 | group 2 | join, merge, summary
	 *     second stream:            hash 1  | hash 2  | hash 3     | pass 0  | pass 1  | pass 2 (lz4_frame_sums_tail)
	 * pass g taking every frame of the slice over the blocks that groups 0 .. g completed, so that the step waits for
	 * the chain over the last group's blocks only.  Every ordering is an event between launches.
	 * (The two launches in front of the slices were also tried on the second stream beside lz4_deps, the merge in
	 * front of the join: 0.08 ms per step, inside the spread of three runs, not kept; profiles/r32_lz4_last_slice.md.) */
	prof_range(c, fast ? "lz4_expand_general" : "lz4_expand", sx, [&] { la_launch_lz4_expand_general(sx, xj, bt->hist_len); });
	if (fast && poll)
		/* eligible blocks with more sequences than one LDS segment: classified on the device, shared out over a
		 * small grid (a no-op launch when there are none).  (The in-order kernel takes blocks of any sequence count.) */
		prof_range(c, "lz4_expand_big", sx, [&] { la_launch_lz4_expand_fast_big(sx, xj, w.big); });
	if (bt->n_frames && !verify)
		HIPCHK(c, hipMemsetAsync(bt->d_frame_status, 0, (size_t)bt->n_frames * sizeof(uint32_t), sx));
	for (uint32_t i = 0; i < nsl; i++) {
		uint32_t first = (uint32_t)((uint64_t)n * i / nsl), last = (uint32_t)((uint64_t)n * (i + 1) / nsl);
		if (split.n_groups) {	/* the split slice starts on a multiple of its period */
			if (i + 2 == nsl)
				last = split.first;
			if (i + 1 == nsl) {
				for (uint32_t g = 0; g < split.n_groups; g++) {
					prof_range(c, "lz4_expand", sx, [&] { la_launch_lz4_expand_fast_group(sx, xj, split, g); });
					HIPCHK(c, hipEventRecord(c->split_ev[g], sx));
					HIPCHK(c, hipStreamWaitEvent(sp, c->split_ev[g], 0));
					const bool tail = g + 1 == split.n_groups;
					/* pass g: every frame over the blocks that groups 0 .. g made ready; the last one is the
					 * stretch the step waits for */
					prof_range(c, tail ? "lz4_frame_sums_tail" : "lz4_frame_sums", sp, [&] {
						la_launch_lz4_frame_sums_split(sp, bt->d_src, bt->d_dst, bt->d_frames, bt->n_frames,
						    bt->d_dst_off, bt->dst_cap, bt->d_frame_status, split, g, c->lz4_carry,
						    bt->d_carry_in, bt->d_carry_out, tail || lz4_split_row_hidden);
					});
				}
				break;
			}
		}
		const la_expand_job sj = xj.slice(first, last - first);
		if (fast)
			prof_range(c, "lz4_expand", sx, [&] { (poll ? la_launch_lz4_expand_fast : la_launch_lz4_expand_inorder)(sx, sj); });
		if (bt->n_frames && verify) {
			HIPCHK(c, hipEventRecord(c->slice_ev[1 + i], sx));
			HIPCHK(c, hipStreamWaitEvent(sp, c->slice_ev[1 + i], 0));
			prof_range(c, "lz4_frame_sums", sp, [&] {
				/* frames that END in this slice: all their blocks are in the slab now */
				la_launch_lz4_frame_sums(sp, bt->d_src, bt->d_dst, bt->d_frames, bt->n_frames,
				    bt->d_dst_off, bt->dst_cap, bt->d_frame_status, i ? first + 1 : 0u, last,
				    bt->d_carry_in, bt->d_carry_out,
				    /* nothing overlaps the last slice's hashes (nor a small batch's): the low-latency form */
				    i + 1 == nsl);
			});
		}
	}
	/* join the second stream */
	HIPCHK(c, hipEventRecord(c->slice_ev[LA_MAX_SLICES - 1], sp));
	HIPCHK(c, hipStreamWaitEvent(sx, c->slice_ev[LA_MAX_SLICES - 1], 0));
	if (verify)
		la_launch_lz4_merge_status(sx, w.sum_status, n, bt->d_block_status);
	if (bt->d_summary)
		prof_range(c, "summary", sx, [&] {
			la_launch_lz4_summary(sx, bt->d_out_len, bt->d_block_status, n, bt->d_frame_status, bt->n_frames, bt->d_dst_off, bt->d_summary);
		});
	HIPCHK(c, hipGetLastError());
	return LA_OK;
}

int la_gpu_lz4_debug_deps(la_gpu_ctx *c, const la_lz4_batch *bt, uint32_t block, uint64_t *seq_out, uint32_t *deps_out,
    uint32_t cap)
{
	if (!c || !bt || block >= bt->n_blocks || (cap && (!seq_out || !deps_out)) || !lz4_uses_deps(bt))
		return LA_ERR_ARG;
	/* the layout the decode carved: the same call on the same shape */
	lz4_ws w;
	lz4_ws_carve(&w, (uint8_t *)c->ws, bt->n_blocks, bt->src_bytes, true);
	if (!c->ws || w.total > c->ws_bytes || w.table_cap > c->lz4_deps_cap)
		return LA_ERR_ARG;
	uint32_t ns = 0;
	uint64_t toff = 0;
	HIPCHK(c, hipMemcpyAsync(&ns, w.nseq + block, sizeof(ns), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(c, hipMemcpyAsync(&toff, w.table_off + block, sizeof(toff), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	if (ns == 0xFFFFFFFFu)
		return 0;
	if (ns > 0x7FFFFFFFu || toff > w.table_cap || ns > w.table_cap - toff)
		return LA_ERR_ARG;
	const uint32_t m = ns < cap ? ns : cap;
	if (m) {
		static_assert(sizeof(la_lz4_seq) == sizeof(uint64_t), "a table entry travels as one 64-bit value");
		HIPCHK(c, hipMemcpyAsync(seq_out, w.table + toff, (size_t)m * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
		HIPCHK(c, hipMemcpyAsync(deps_out, c->lz4_deps + toff, (size_t)m * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
		HIPCHK(c, hipStreamSynchronize(c->stream));
	}
	return (int)ns;
}

int la_gpu_lz4_debug_literal_plan(la_gpu_ctx *c, const la_lz4_batch *bt, uint32_t block, uint16_t *plan_out, uint32_t cap)
{
	if (!c || !bt || block >= bt->n_blocks || (cap && !plan_out) || !lz4_uses_deps(bt))
		return LA_ERR_ARG;
	lz4_ws w;
	lz4_ws_carve(&w, (uint8_t *)c->ws, bt->n_blocks, bt->src_bytes, true);
	if (!c->ws || w.total > c->ws_bytes || w.table_cap > c->lz4_deps_cap || !c->lz4_plan)
		return LA_ERR_ARG;
	la_lz4_block b;
	uint32_t ns = 0, st = 0, olen = 0;
	uint64_t toff[2] = { 0, 0 }, doff = 0;
	HIPCHK(c, hipMemcpyAsync(&b, bt->d_blocks + block, sizeof(b), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(c, hipMemcpyAsync(&ns, w.nseq + block, sizeof(ns), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(c, hipMemcpyAsync(&st, bt->d_block_status + block, sizeof(st), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(c, hipMemcpyAsync(&olen, bt->d_out_len + block, sizeof(olen), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(c, hipMemcpyAsync(&doff, bt->d_dst_off + block, sizeof(doff), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(c, hipMemcpyAsync(toff, w.table_off + block, sizeof(toff), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	/* the dependency kernel's own question.  (The status is the decode's final one: a block that failed behind the
	 * dependency kernel -- a wrong checksum -- had its plan written and answers 0 here all the same.) */
	if (la_lz4_route(b, st, olen, ns, doff, bt->dst_cap, true, LA_LZ4_LONG_SEQ_BYTES) != LA_XR_WINDOW)
		return 0;
	const uint32_t m = la_lz4_plan_entries(b.src_len);
	if (toff[0] > toff[1] || toff[1] > w.table_cap || 2ull * m > toff[1] - toff[0])
		return LA_ERR_ARG;
	const uint32_t take = m < cap ? m : cap;
	if (take) {
		HIPCHK(c, hipMemcpyAsync(plan_out, c->lz4_plan + toff[0], (size_t)take * sizeof(uint16_t), hipMemcpyDeviceToHost, c->stream));
		HIPCHK(c, hipStreamSynchronize(c->stream));
	}
	return (int)m;
}

uint64_t la_gpu_zstd_workspace_bytes(uint32_t n_frames)
{
	return la_zstd_workspace_bytes(n_frames);
}

int la_gpu_zstd_decode(la_gpu_ctx *c, const la_zstd_batch *bt)
{
	if (!c || !bt)
		return LA_ERR_ARG;
	if (bt->n_frames && (!bt->d_src || !bt->d_frames || !bt->d_dst || !bt->d_results))
		return LA_ERR_ARG;
	/* LA_ZSTD_OPT_BLOCK_PARALLEL: the block path in front, its workspace behind the frame kernels'; coordinates are
	 * 32-bit as in the gzip chain, so a longer d_dst goes to the frame kernels whole */
	const bool blocks = (bt->options & LA_ZSTD_OPT_BLOCK_PARALLEL) && bt->n_frames && bt->dst_cap <= 0xFFFFFFFFull;
	const uint64_t ws_frames = (la_zstd_workspace_bytes(bt->n_frames) + 255) & ~255ull;
	const uint64_t need = ws_frames + (blocks ? la_zstd_blocks_workspace_bytes(bt->n_frames, bt->src_bytes, bt->dst_cap) : 0);
	if (need > c->ws_bytes) {
		int rc = la_gpu_reserve(c, need);
		if (rc != LA_OK) return rc;
	}
	prof_begin(c);
	uint8_t *ws_blocks = (uint8_t *)c->ws + ws_frames;
	if (blocks)
		prof_range(c, "zstd_blocks", c->stream, [&] {
			la_launch_zstd_blocks(c->stream, bt->d_src, bt->src_bytes, bt->d_frames, bt->n_frames, bt->d_dst, bt->dst_cap,
			    bt->d_results, ws_blocks, bt->options);
		});
	/* behind it, the frames it handed back (without the option: every frame) */
	prof_range(c, "zstd_frames", c->stream, [&] {
		la_launch_zstd_frames(c->stream, bt->d_src, bt->src_bytes, bt->d_frames, bt->n_frames, bt->d_dst, bt->dst_cap,
		    bt->d_results, (uint8_t *)c->ws, bt->options, blocks ? la_zstd_blocks_todo(ws_blocks) : NULL);
	});
	HIPCHK(c, hipGetLastError());
	return LA_OK;
}

uint32_t la_gpu_bzip2_max_blocks(uint32_t slot_level)
{
	return slot_level >= 1 && slot_level <= 9 ? la_bzip2_max_blocks(slot_level) : 0;
}

uint64_t la_gpu_bzip2_workspace_bytes(uint32_t n, uint32_t slot_level)
{
	return slot_level >= 1 && slot_level <= 9 ? la_bzip2_workspace_bytes(n, slot_level) : 0;
}

int la_gpu_bzip2_scan(la_gpu_ctx *c, const uint8_t *d_src, uint64_t src_bytes, la_bz2_cand *d_cands, uint32_t cand_cap, uint32_t *d_count)
{
	if (!c || !d_count || (src_bytes && !d_src) || (cand_cap && !d_cands) || src_bytes >= ((uint64_t)1 << 35))
		return LA_ERR_ARG;
	const uint64_t need = la_bzip2_scan_ws_bytes(src_bytes);
	if (need > c->ws_bytes) {
		int rc = la_gpu_reserve(c, need);
		if (rc != LA_OK) return rc;
	}
	prof_begin(c);
	prof_range(c, "bz2_scan", c->stream, [&] {
		la_launch_bzip2_scan(c->stream, d_src, src_bytes, d_cands, cand_cap, d_count, (uint8_t *)c->ws);
	});
	HIPCHK(c, hipGetLastError());
	return LA_OK;
}

int la_gpu_bzip2_decode(la_gpu_ctx *c, const la_bz2_batch *bt)
{
	if (!c || !bt || !bt->state_in || !bt->d_state_out || bt->slot_level < 1 || bt->slot_level > 9 || bt->reserved)
		return LA_ERR_ARG;
	if (bt->phase != LA_BZ2_MEASURE && bt->phase != LA_BZ2_EMIT)
		return LA_ERR_ARG;
	if (bt->n > la_bzip2_max_blocks(bt->slot_level) || (bt->n && (!bt->d_cands || !bt->d_results)) || (bt->src_bytes && !bt->d_src))
		return LA_ERR_ARG;
	if (bt->phase == LA_BZ2_EMIT && bt->dst_cap && !bt->d_dst)
		return LA_ERR_ARG;
	const uint64_t need = la_bzip2_workspace_bytes(bt->n, bt->slot_level);
	if (need > c->ws_bytes) {
		if (bt->phase == LA_BZ2_EMIT)
			return LA_ERR_ARG;	/* the workspace of the MEASURE call is gone */
		int rc = la_gpu_reserve(c, need);
		if (rc != LA_OK) return rc;
	}
	prof_begin(c);
	uint8_t *ws = (uint8_t *)c->ws;
	if (bt->phase == LA_BZ2_MEASURE) {
		prof_range(c, "bz2_measure", c->stream, [&] { la_launch_bzip2_measure(c->stream, bt, ws); });
		prof_range(c, "bz2_walk", c->stream, [&] { la_launch_bzip2_walk(c->stream, bt, ws); });
	} else {
		prof_range(c, "bz2_emit", c->stream, [&] { la_launch_bzip2_emit(c->stream, bt, ws); });
		prof_range(c, "bz2_verify", c->stream, [&] { la_launch_bzip2_verify(c->stream, bt, ws); });
	}
	HIPCHK(c, hipGetLastError());
	return LA_OK;
}

uint64_t la_gpu_xz_workspace_bytes(uint32_t n)
{
	return la_xz_workspace_bytes(n);
}

int la_gpu_xz_decode(la_gpu_ctx *c, const la_xz_batch *bt)
{
	if (!c || !bt || (bt->reserved & ~LA_XZ_BATCH_CHAINS))
		return LA_ERR_ARG;
	if (bt->n && (!bt->d_blocks || !bt->d_results || !bt->d_dst || (bt->src_bytes && !bt->d_src)))
		return LA_ERR_ARG;
	const bool chains = (bt->reserved & LA_XZ_BATCH_CHAINS) != 0u;
	/* the filters' scratch (it grows with dst_cap) lies behind the decoder's */
	const uint64_t o_filters = (la_xz_workspace_bytes(bt->n) + 255u) & ~(uint64_t)255u;
	const uint64_t need = o_filters + (chains ? la_xz_unfilter_ws_bytes(bt->n, bt->dst_cap) : 0u);
	if (need > c->ws_bytes) {
		int rc = la_gpu_reserve(c, need);
		if (rc != LA_OK) return rc;
	}
	prof_begin(c);
	uint8_t *ws = (uint8_t *)c->ws;
	prof_range(c, "xz_decode", c->stream, [&] { la_launch_xz_decode(c->stream, bt, ws); });
	if (chains)
		prof_range(c, "xz_unfilter", c->stream, [&] { la_launch_xz_unfilter(c->stream, bt, ws, ws + o_filters); });
	prof_range(c, "xz_verify", c->stream, [&] { la_launch_xz_verify(c->stream, bt, ws); });
	HIPCHK(c, hipGetLastError());
	return LA_OK;
}

uint64_t la_gpu_lzip_workspace_bytes(uint32_t n)
{
	return la_lzip_workspace_bytes(n);
}

int la_gpu_lzip_scan(la_gpu_ctx *c, const uint8_t *d_src, uint64_t src_bytes, uint64_t *d_offs, uint32_t cap, uint32_t *d_count)
{
	if (!c || !d_count || (src_bytes && !d_src) || (cap && !d_offs) || src_bytes >= ((uint64_t)1 << 35))
		return LA_ERR_ARG;
	const uint64_t need = la_lzip_scan_ws_bytes(src_bytes);
	if (need > c->ws_bytes) {
		int rc = la_gpu_reserve(c, need);
		if (rc != LA_OK) return rc;
	}
	prof_begin(c);
	prof_range(c, "lzip_scan", c->stream, [&] {
		la_launch_lzip_scan(c->stream, d_src, src_bytes, d_offs, cap, d_count, (uint8_t *)c->ws);
	});
	HIPCHK(c, hipGetLastError());
	return LA_OK;
}

int la_gpu_lzip_decode(la_gpu_ctx *c, const la_lzip_batch *bt)
{
	if (!c || !bt || bt->reserved)
		return LA_ERR_ARG;
	if (bt->n && (!bt->d_members || !bt->d_results || !bt->d_dst || (bt->src_bytes && !bt->d_src)))
		return LA_ERR_ARG;
	const uint64_t need = la_lzip_workspace_bytes(bt->n);
	if (need > c->ws_bytes) {
		int rc = la_gpu_reserve(c, need);
		if (rc != LA_OK) return rc;
	}
	prof_begin(c);
	prof_range(c, "lzip_decode", c->stream, [&] { la_launch_lzip_decode(c->stream, bt, (uint8_t *)c->ws); });
	HIPCHK(c, hipGetLastError());
	return LA_OK;
}

uint64_t la_gpu_lzop_workspace_bytes(uint32_t n)
{
	return la_lzop_workspace_bytes(n);
}

int la_gpu_lzop_decode(la_gpu_ctx *c, const la_lzop_batch *bt)
{
	if (!c || !bt || bt->reserved)
		return LA_ERR_ARG;
	if (bt->n && (!bt->d_blocks || !bt->d_results || !bt->d_dst || (bt->src_bytes && !bt->d_src)))
		return LA_ERR_ARG;
	const uint64_t need = la_lzop_workspace_bytes(bt->n);
	if (need > c->ws_bytes) {
		int rc = la_gpu_reserve(c, need);
		if (rc != LA_OK) return rc;
	}
	prof_begin(c);
	prof_range(c, "lzop_decode", c->stream, [&] { la_launch_lzop_decode(c->stream, bt, (uint8_t *)c->ws); });
	HIPCHK(c, hipGetLastError());
	return LA_OK;
}

uint64_t la_gpu_uu_workspace_bytes(uint64_t src_bytes)
{
	return src_bytes <= LA_UU_MAX_SRC_BYTES ? la_uu_workspace_bytes(src_bytes) : 0u;
}

int la_gpu_uu_decode(la_gpu_ctx *c, const la_uu_batch *bt)
{
	if (!c || !bt || bt->reserved || !bt->d_result || bt->src_bytes > LA_UU_MAX_SRC_BYTES || bt->in.state > LA_UU_READ_BASE64)
		return LA_ERR_ARG;
	if (bt->src_bytes && (!bt->d_src || !bt->d_dst || bt->dst_cap < bt->src_bytes))
		return LA_ERR_ARG;
	const uint64_t need = la_uu_workspace_bytes(bt->src_bytes);
	if (need > c->ws_bytes) {
		int rc = la_gpu_reserve(c, need);
		if (rc != LA_OK) return rc;
	}
	uint8_t *ws = (uint8_t *)c->ws;
	prof_begin(c);
	prof_range(c, "uu_lines", c->stream, [&] { la_launch_uu_lines(c->stream, bt, ws); });
	prof_range(c, "uu_records", c->stream, [&] { la_launch_uu_records(c->stream, bt, ws); });
	prof_range(c, "uu_states", c->stream, [&] { la_launch_uu_states(c->stream, bt, ws); });
	prof_range(c, "uu_decode", c->stream, [&] { la_launch_uu_decode(c->stream, bt, ws); });
	HIPCHK(c, hipGetLastError());
	return LA_OK;
}

/* workspace of a gzip batch on the lane kernels: their scratch, then (two phases) E and the SEG launch's list; returns its size */
static uint64_t gz_ws_carve(uint8_t *base, uint32_t n, bool two_phase, la_inflate_emit *E, uint32_t **big)
{
	la_carve cv = { base, 0 };
	cv.take<uint8_t>(la_inflate_lanes_scratch_bytes(n), 256);
	if (two_phase) {
		E->lit = cv.take<uint8_t>((uint64_t)n * 65536u, 256);
		E->table = cv.take<la_lz4_seq>((uint64_t)n * LA_INFLATE_MAXSEQ, 256);
		E->blocks = cv.take<la_lz4_block>(n, 256);
		E->out_len = cv.take<uint32_t>(n, 256);
		E->nseq = cv.take<uint32_t>(n, 256);
		E->xstatus = cv.take<uint32_t>(n, 256);
		E->todo = cv.take<uint32_t>(n, 256);
		E->dst_off = cv.take<uint64_t>(n + 1, 256);
		E->table_off = cv.take<uint64_t>(n + 1, 256);
		*big = cv.take<uint32_t>(n + 1, 256);
	}
	return align_up(cv.off, 256);
}

/* workspace of a chain batch (LA_GZ_OPT_CHAIN).  Everything is sized by what the host knows, n and the batch's
 * dst_cap: 4 B of source pointer per byte of capacity, then per piece 4 B of measured length, 8 B of packed offset, the
 * scan's scratch and 24 B of packed member record, and the 256 B control block (no staging copy of the bytes and no
 * match records: the emit pass writes bytes and pointers where they belong) */
struct gz_chain_ws {
	uint32_t *ptr, *len, *ctl;
	uint64_t *packed_off;
	void *scan;
	la_gz_member *packed;
};
static uint64_t gz_chain_carve(uint8_t *base, uint32_t n, uint64_t dst_cap, gz_chain_ws *w)
{
	la_carve cv = { base, 0 };
	w->ctl = cv.take<uint32_t>(LA_CHAIN_CTL_WORDS, 256);
	w->ptr = cv.take<uint32_t>(dst_cap, 256);
	w->len = cv.take<uint32_t>(n, 256);
	w->packed_off = cv.take<uint64_t>((uint64_t)n + 1, 256);
	w->scan = cv.take<uint8_t>(la_scan_scratch_bytes(n), 256);
	w->packed = cv.take<la_gz_member>(n, 256);
	return align_up(cv.off, 256);
}

/* LA_GZ_OPT_CHAIN: measure, scan, emit (la_inflate.hip), pointer jumping and gather (la_inflate_chain.hip), then the
 * CRC32 launch over the packed ranges and the summary */
static int gzip_decode_chain(la_gpu_ctx *c, const la_gz_batch *bt)
{
	hipStream_t s = c->stream;
	const uint32_t n = bt->n_members;
	gz_chain_ws w;
	const uint64_t need = gz_chain_carve(NULL, n, bt->dst_cap, &w);
	if (need > c->ws_bytes) {
		int rc = la_gpu_reserve(c, need);
		if (rc != LA_OK) return rc;
	}
	gz_chain_carve((uint8_t *)c->ws, n, bt->dst_cap, &w);
	const la_inflate_chain C = { w.packed_off, w.ptr, bt->hist_len };
	prof_begin(c);
	prof_range(c, "chain_measure", s, [&] {
		la_launch_inflate_chain(s, bt->d_src, bt->src_bytes, bt->d_members, n, bt->d_dst, bt->dst_cap, bt->d_results, C, false);
	});
	prof_range(c, "chain_scan", s, [&] {
		la_launch_chain_lengths(s, bt->d_results, n, w.len);
		la_launch_scan_u32(s, w.len, n, w.packed_off, w.scan);
	});
	prof_range(c, "chain_emit", s, [&] {
		la_launch_inflate_chain(s, bt->d_src, bt->src_bytes, bt->d_members, n, bt->d_dst, bt->dst_cap, bt->d_results, C, true);
	});
	prof_range(c, "chain_resolve", s, [&] {
		la_launch_chain_resolve(s, bt->d_members, bt->d_results, n, bt->d_dst, bt->dst_cap, C, w.packed, w.ctl);
	});
	prof_range(c, "gz_crc32", s, [&] {
		la_launch_gz_verify(s, bt->d_src, bt->src_bytes, w.packed, n, bt->d_dst, bt->d_results, 2);
	});
	if (bt->d_summary)
		la_launch_gz_summary(s, bt->d_results, n, bt->d_summary);
	HIPCHK(c, hipGetLastError());
	return LA_OK;
}

/* workspace of LA_GZ_OPT_BLOCK_STARTS, a function of src_bytes and dst_cap only: the chain's 4 B of source pointer per byte
 * of capacity; one bit per bit of the source (the quick test's masks); 12 B per tile of LA_FIND_TILE_BYTES; at most
 * src_bytes / 32 + 1024 survivors of 16 B; at most src_bytes / 128 + 64 candidates of 56 B */
struct gz_blocks_ws {
	la_gz_find_ws f;
	uint32_t *ptr, *chain_ctl;
	uint64_t *packed_off;
};
static uint64_t gz_blocks_carve(uint8_t *base, uint64_t src_bytes, uint64_t dst_cap, gz_blocks_ws *w)
{
	la_carve cv = { base, 0 };
	la_gz_find_ws &f = w->f;
	f.tiles = (uint32_t)((src_bytes + LA_FIND_TILE_BYTES - 1) / LA_FIND_TILE_BYTES);
	if (f.tiles == 0) f.tiles = 1;
	f.max_surv = (uint32_t)(src_bytes / 32) + 1024u;
	f.max_cand = (uint32_t)(src_bytes / 128) + 64u;
	const uint32_t scan_n = f.max_surv > f.tiles ? f.max_surv : f.tiles;	/* (and above max_cand) */
	f.ctl = cv.take<uint32_t>(LA_FIND_CTL_WORDS, 256);
	w->chain_ctl = cv.take<uint32_t>(LA_CHAIN_CTL_WORDS, 256);
	w->ptr = cv.take<uint32_t>(dst_cap, 256);
	f.mask = cv.take<uint32_t>((uint64_t)f.tiles * (LA_FIND_TILE_BYTES / 4), 256);
	f.tile_cnt = cv.take<uint32_t>(f.tiles, 256);
	f.tile_off = cv.take<uint64_t>((uint64_t)f.tiles + 1, 256);
	f.surv = cv.take<uint32_t>(f.max_surv, 256);
	f.flag = cv.take<uint32_t>(f.max_surv, 256);
	f.flag_off = cv.take<uint64_t>((uint64_t)f.max_surv + 1, 256);
	f.cand = cv.take<uint32_t>(f.max_cand, 256);
	f.res_all = cv.take<la_gz_result>(f.max_cand, 256);
	f.startc = cv.take<uint32_t>((uint64_t)f.max_cand + 1, 256);
	f.resc = cv.take<la_gz_result>(f.max_cand, 256);
	f.lenc = cv.take<uint32_t>(f.max_cand, 256);
	f.crc = cv.take<uint32_t>(f.max_cand, 256);
	w->packed_off = cv.take<uint64_t>((uint64_t)f.max_cand + 1, 256);
	f.scan = cv.take<uint8_t>(la_scan_scratch_bytes(scan_n), 256);
	return align_up(cv.off, 256);
}

/* LA_GZ_OPT_BLOCK_STARTS: find, measure every candidate, walk (la_inflate_find.hip), then the chain path over the
 * confirmed pieces and the two results (la_hash.hip) */
static int gzip_decode_block_starts(la_gpu_ctx *c, const la_gz_batch *bt)
{
	hipStream_t s = c->stream;
	const uint32_t start_bit = (bt->options >> LA_GZ_OPT_START_BIT_SHIFT) & 7u;
	gz_blocks_ws w;
	const uint64_t need = gz_blocks_carve(NULL, bt->src_bytes, bt->dst_cap, &w);
	if (need > c->ws_bytes) {
		int rc = la_gpu_reserve(c, need);
		if (rc != LA_OK) return rc;
	}
	gz_blocks_carve((uint8_t *)c->ws, bt->src_bytes, bt->dst_cap, &w);
	const la_gz_find_ws &f = w.f;
	const la_inflate_chain all = { w.packed_off, w.ptr, bt->hist_len, f.cand, f.ctl + LA_FIND_N_CAND, f.ctl + LA_FIND_N_CAND };
	const la_inflate_chain confirmed = { w.packed_off, w.ptr, bt->hist_len, f.startc, f.ctl + LA_FIND_N_CONF, f.ctl + LA_FIND_N_TABLE };
	prof_begin(c);
	prof_range(c, "blocks_find", s, [&] {
		la_launch_gz_find(s, bt->d_src, bt->src_bytes, bt->d_members, start_bit, f);
	});
	prof_range(c, "blocks_measure", s, [&] {
		la_launch_inflate_chain_bits(s, bt->d_src, bt->src_bytes, bt->d_members, f.max_cand, bt->d_dst, bt->dst_cap, f.res_all, all, false);
	});
	prof_range(c, "blocks_walk", s, [&] {
		la_launch_gz_walk(s, bt->dst_cap, f);
		la_launch_scan_u32(s, f.lenc, f.max_cand, w.packed_off, f.scan);
	});
	prof_range(c, "chain_emit", s, [&] {
		la_launch_inflate_chain_bits(s, bt->d_src, bt->src_bytes, bt->d_members, f.max_cand, bt->d_dst, bt->dst_cap, f.resc, confirmed, true);
	});
	prof_range(c, "chain_resolve", s, [&] {
		la_launch_chain_resolve_dev(s, bt->d_dst, &bt->d_members->dst_off, w.ptr, bt->hist_len, w.packed_off + f.max_cand, bt->dst_cap,
		    w.chain_ctl);
	});
	prof_range(c, "gz_crc32", s, [&] {
		la_launch_gz_blocks_summary(s, bt->d_dst, bt->d_members, w.packed_off, start_bit, f, bt->d_results);
	});
	if (bt->d_summary)
		la_launch_gz_summary(s, bt->d_results, 1, bt->d_summary);
	HIPCHK(c, hipGetLastError());
	return LA_OK;
}

int la_gpu_gzip_decode(la_gpu_ctx *c, const la_gz_batch *bt)
{
	if (!c || !bt)
		return LA_ERR_ARG;
	if (bt->n_members && (!bt->d_src || !bt->d_members || !bt->d_dst || !bt->d_results))
		return LA_ERR_ARG;
	if (bt->options & LA_GZ_OPT_BLOCK_STARTS) {
		/* one span of one stream, decoded as a chain; bit offsets into the source are 32-bit words */
		if ((bt->options & (LA_GZ_OPT_PIECES | LA_GZ_OPT_CHAIN)) != (LA_GZ_OPT_PIECES | LA_GZ_OPT_CHAIN) ||
		    (bt->options & (LA_GZ_OPT_LANE_KERNEL | LA_GZ_OPT_TWO_PHASE | LA_GZ_OPT_EXPAND_INORDER)) ||
		    bt->n_members != 1 || bt->src_bytes >= (1ull << 29) ||
		    bt->hist_len > 32768u || bt->dst_cap + bt->hist_len > 0xFFFFFFFFull)
			return LA_ERR_ARG;
		return gzip_decode_block_starts(c, bt);
	}
	if (bt->options & LA_GZ_OPT_CHAIN) {
		/* pieces only, the wave kernel only; coordinates of history + range are 32-bit words */
		if (!(bt->options & LA_GZ_OPT_PIECES) ||
		    (bt->options & (LA_GZ_OPT_LANE_KERNEL | LA_GZ_OPT_TWO_PHASE | LA_GZ_OPT_EXPAND_INORDER)) ||
		    bt->hist_len > 32768u || bt->dst_cap + bt->hist_len > 0xFFFFFFFFull)
			return LA_ERR_ARG;
		return gzip_decode_chain(c, bt);
	}
	hipStream_t s = c->stream;
	/* many members: one LANE per member (la_inflate_lanes.hip); few: one wave per member */
	const bool lanes = (bt->n_members >= LA_GZ_LANES_MIN || (bt->options & (LA_GZ_OPT_LANE_KERNEL | LA_GZ_OPT_TWO_PHASE))) &&
	    !(bt->options & LA_GZ_OPT_WAVE_KERNEL);
	/* lanes, two phases (default): entropy decode into literal buffers + sequence tables, then the
	 * LDS-window expand kernel of the lz4 path; LA_GZ_OPT_LANE_KERNEL forces the in-place lane kernel */
	const bool two_phase = lanes && !(bt->options & LA_GZ_OPT_LANE_KERNEL);
	const uint32_t n = bt->n_members;
	const bool pieces = (bt->options & LA_GZ_OPT_PIECES) != 0;	/* (every launch below: the template instance that knows pieces) */
	uint8_t *wsb = NULL;
	la_inflate_emit E = {};
	uint32_t *gz_big = NULL;
	if (lanes) {
		const uint64_t need = gz_ws_carve(NULL, n, two_phase, &E, &gz_big);
		if (need > c->ws_bytes) {
			int rc = la_gpu_reserve(c, need);
			if (rc != LA_OK) return rc;
		}
		wsb = (uint8_t *)c->ws;
		gz_ws_carve(wsb, n, two_phase, &E, &gz_big);
	}
	prof_begin(c);
	if (two_phase) {
		prof_range(c, "inflate_symbols", s, [&] {
			la_launch_inflate_symbols(s, bt->d_src, bt->src_bytes, bt->d_members, n, bt->dst_cap, bt->d_results, wsb, E, pieces);
		});
		const la_expand_job xj = la_inflate_expand_job(E, n, bt->d_dst, bt->dst_cap);
		prof_range(c, "inflate_expand", s, [&] {
			if (!(bt->options & LA_GZ_OPT_EXPAND_INORDER)) {
				la_launch_lz4_expand_fast(s, xj);
				/* members with more matches than one LDS segment of the polling kernel holds */
				la_launch_lz4_expand_fast_big(s, xj, gz_big);
			} else {
				la_launch_lz4_expand_inorder(s, xj);
			}
		});
		/* members the LDS-window kernel cannot take: decoded in place */
		prof_range(c, "inflate", s, [&] {
			la_launch_inflate_lanes(s, bt->d_src, bt->src_bytes, bt->d_members, n, bt->d_dst,
			    bt->dst_cap, bt->d_results, wsb, E.todo, pieces);
		});
	} else {
		prof_range(c, "inflate", s, [&] {
			if (lanes)
				la_launch_inflate_lanes(s, bt->d_src, bt->src_bytes, bt->d_members, n, bt->d_dst,
				    bt->dst_cap, bt->d_results, wsb, NULL, pieces);
			else
				la_launch_inflate(s, bt->d_src, bt->src_bytes, bt->d_members, n, bt->d_dst, bt->dst_cap,
				    bt->d_results, pieces);
		});
	}
	prof_range(c, "gz_crc32", s, [&] {
		la_launch_gz_verify(s, bt->d_src, bt->src_bytes, bt->d_members, bt->n_members, bt->d_dst,
		    bt->d_results, (bt->options & (LA_GZ_OPT_RAW | LA_GZ_OPT_PIECES)) ? 2 : !(bt->options & LA_GZ_OPT_NO_VERIFY));
	});
	if (bt->d_summary)
		la_launch_gz_summary(s, bt->d_results, bt->n_members, bt->d_summary);
	HIPCHK(c, hipGetLastError());
	return LA_OK;
}

/* ------------------------------------------------------------------ compression */

/* the body every compress entry shares once its arguments are checked: workspace, profile range, launch */
extern "C++" template <typename Launch>
static int compress_run(la_gpu_ctx *c, uint64_t need, const char *name, Launch launch)
{
	if (need > c->ws_bytes) {
		int rc = la_gpu_reserve(c, need);
		if (rc != LA_OK) return rc;
	}
	prof_begin(c);
	prof_range(c, name, c->stream, [&] { launch((uint8_t *)c->ws); });
	HIPCHK(c, hipGetLastError());
	return LA_OK;
}

int la_gpu_lz4_compress(la_gpu_ctx *c, const la_lz4c_batch *bt)
{
	if (!c || !bt || !bt->d_out_bytes || (bt->src_bytes && (!bt->d_src || !bt->d_out)))
		return LA_ERR_ARG;
	if (bt->block_size == 0 || bt->block_size > 65536u || bt->blocks_per_frame == 0 ||
	    (uint64_t)bt->block_size * bt->blocks_per_frame > 0x7FFFFFFFull ||
	    (bt->src_bytes + bt->block_size - 1) / bt->block_size > 0xFFFFFFFEull)
		return LA_ERR_ARG;
	return compress_run(c, la_gpu_lz4_compress_workspace_bytes(bt->src_bytes, bt->block_size, bt->blocks_per_frame),
	    "lz4_compress", [&](uint8_t *ws) {
		la_launch_lz4_compress(c->stream, bt->d_src, bt->src_bytes, bt->block_size, bt->blocks_per_frame, bt->flags,
		    bt->d_out, bt->out_cap, bt->d_out_bytes, ws);
	});
}

int la_gpu_gzip_compress(la_gpu_ctx *c, const la_gzc_batch *bt)
{
	if (!c || !bt || !bt->d_out_bytes || (bt->src_bytes && (!bt->d_src || !bt->d_out)))
		return LA_ERR_ARG;
	if (bt->chunk_bytes == 0 || bt->chunk_bytes > 49152u || (bt->src_bytes + bt->chunk_bytes - 1) / bt->chunk_bytes > 0xFFFFFFFEull)
		return LA_ERR_ARG;
	if (bt->options > LA_GZC_STORED || bt->framing > LA_GZC_FRAME_STREAM)
		return LA_ERR_ARG;
	return compress_run(c, la_gzip_compress_ws_bytes(bt->src_bytes, bt->chunk_bytes, bt->options), "gzip_compress", [&](uint8_t *ws) {
		la_launch_gzip_compress(c->stream, bt->d_src, bt->src_bytes, bt->chunk_bytes, bt->mtime, bt->options, bt->framing,
		    bt->d_out, bt->out_cap, bt->d_out_bytes, ws);
	});
}

int la_gpu_zip_compress(la_gpu_ctx *c, const la_zipc_batch *bt)
{
	if (!c || !bt || !bt->d_out_bytes || (bt->n_segs && (!bt->d_segs || !bt->d_results || !bt->d_out)) || (bt->src_bytes && !bt->d_src))
		return LA_ERR_ARG;
	if (bt->chunk_bytes == 0 || bt->chunk_bytes > 49152u || bt->options > LA_GZC_STORED || bt->reserved != 0 ||
	    bt->n_segs >= 0x80000000u ||	/* (a span names its segment in 31 bits; a launch has at most 2^31 - 1 blocks) */
	    (bt->src_bytes + bt->chunk_bytes - 1) / bt->chunk_bytes + bt->n_segs > 0x7FFFFFFFull)
		return LA_ERR_ARG;
	if (bt->n_segs == 0) {
		HIPCHK(c, hipMemsetAsync(bt->d_out_bytes, 0, 8, c->stream));
		return LA_OK;
	}
	const uint64_t need = la_zip_compress_ws_bytes(bt->src_bytes, bt->n_segs, bt->chunk_bytes, bt->options);
	if (need > c->ws_bytes) {
		int rc = la_gpu_reserve(c, need);
		if (rc != LA_OK) return rc;
	}
	uint8_t *ws = (uint8_t *)c->ws;
	prof_begin(c);
	prof_range(c, "zip_spans", c->stream, [&] {
		la_launch_zip_spans(c->stream, bt->src_bytes, bt->d_segs, bt->n_segs, bt->chunk_bytes, bt->options, ws);
	});
	/* the segment table lives on the device: its verdict is the one thing the call waits for, before d_out is touched */
	uint32_t verdict = 0;
	HIPCHK(c, hipMemcpyAsync(&verdict, ws, 4, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	if (verdict != 0)
		return LA_ERR_ARG;
	prof_range(c, "zip_compress", c->stream, [&] {
		la_launch_zip_compress(c->stream, bt->d_src, bt->src_bytes, bt->d_segs, bt->n_segs, bt->chunk_bytes, bt->options,
		    bt->d_out, bt->out_cap, bt->d_results, bt->d_out_bytes, ws);
	});
	HIPCHK(c, hipGetLastError());
	return LA_OK;
}

int la_gpu_zstd_compress(la_gpu_ctx *c, const la_zstdc_batch *bt)
{
	if (!c || !bt || !bt->d_out_bytes || (bt->src_bytes && (!bt->d_src || !bt->d_out)))
		return LA_ERR_ARG;
	if (bt->block_size == 0 || bt->block_size > 131072u || bt->blocks_per_frame == 0 ||
	    (uint64_t)bt->block_size * bt->blocks_per_frame > 0x7FFFFFFFull ||
	    (bt->src_bytes + bt->block_size - 1) / bt->block_size > 0x7FFFFFFEull)
		return LA_ERR_ARG;
	return compress_run(c, la_gpu_zstd_compress_workspace_bytes(bt->src_bytes, bt->block_size, bt->blocks_per_frame),
	    "zstd_compress", [&](uint8_t *ws) {
		la_launch_zstd_compress(c->stream, bt->d_src, bt->src_bytes, bt->block_size, bt->blocks_per_frame, bt->flags,
		    bt->d_out, bt->out_cap, bt->d_out_bytes, ws);
	});
}

#define LA_BZ2C_SRC_MAX LA_BZ2C_MAX_SRC_BYTES	/* positions of the RLE1 bytes (5/4 of the input) are 32-bit */
uint32_t la_gpu_bzip2_compress_block_bytes(uint32_t level)
{
	return level >= 1u && level <= 9u ? la_bzip2_compress_block_bytes(level) : 0u;
}
uint64_t la_gpu_bzip2_compress_workspace_bytes(uint64_t src_bytes, uint32_t level)
{
	return level >= 1u && level <= 9u && src_bytes <= LA_BZ2C_SRC_MAX ? la_bzip2_compress_ws_bytes(src_bytes, level) : 0u;
}
uint64_t la_gpu_bzip2_compress_bound(uint64_t src_bytes, uint32_t level)
{
	return level >= 1u && level <= 9u ? la_bzip2_compress_bound(src_bytes, level) : 0u;
}
struct bz2c_prof { la_gpu_ctx *c; int h; };
static void bz2c_mark(void *cx, const char *name)	/* one profile range per stage of the call */
{
	bz2c_prof *p = (bz2c_prof *)cx;
	if (p->h >= 0)
		prof_close(p->c, p->h, p->c->stream);
	p->h = name ? prof_open(p->c, name, p->c->stream) : -1;
}
int la_gpu_bzip2_compress(la_gpu_ctx *c, const la_bz2c_batch *bt)
{
	if (!c || !bt || !bt->d_out_bytes || !bt->d_state || (bt->src_bytes && !bt->d_src) || (bt->out_cap && !bt->d_out))
		return LA_ERR_ARG;
	if (bt->level < 1u || bt->level > 9u || (bt->flags & ~(LA_BZ2C_FIRST | LA_BZ2C_LAST)) || bt->src_bytes > LA_BZ2C_SRC_MAX)
		return LA_ERR_ARG;
	return compress_run(c, la_bzip2_compress_ws_bytes(bt->src_bytes, bt->level), "bzip2_compress", [&](uint8_t *ws) {
		bz2c_prof pr = { c, -1 };
		const la_stage_hook hook = { bz2c_mark, &pr };
		la_launch_bzip2_compress(c->stream, bt, ws, &hook);
	});
}
uint32_t la_gpu_bzip2_compress_sort_rounds(la_gpu_ctx *c)
{
	return c && c->ws ? la_bzip2_compress_rounds(c->stream, (const uint8_t *)c->ws) : 0u;
}

uint64_t la_gpu_xz_compress_block_bytes(uint32_t level)
{
	return level <= 9u ? LA_XZC_BLOCK_BYTES : 0u;
}
uint64_t la_gpu_xz_compress_workspace_bytes(uint64_t src_bytes)
{
	return src_bytes <= LA_XZC_MAX_SRC_BYTES ? la_xz_compress_ws_bytes(src_bytes) : 0u;
}
uint64_t la_gpu_xz_compress_bound(uint64_t src_bytes, uint32_t level)
{
	return level <= 9u ? la_xz_compress_bound(src_bytes) : 0u;
}
int la_gpu_xz_compress(la_gpu_ctx *c, const la_xzc_batch *bt)
{
	if (!c || !bt || !bt->d_out_bytes || (bt->src_bytes && !bt->d_src) || (bt->out_cap && !bt->d_out))
		return LA_ERR_ARG;
	if (bt->level > 9u || (bt->flags & ~LA_XZC_FIRST) || bt->src_bytes > LA_XZC_MAX_SRC_BYTES)
		return LA_ERR_ARG;
	return compress_run(c, la_xz_compress_ws_bytes(bt->src_bytes), "xz_compress", [&](uint8_t *ws) {
		bz2c_prof pr = { c, -1 };
		const la_stage_hook hook = { bz2c_mark, &pr };
		la_launch_xz_compress(c->stream, bt, ws, &hook);
	});
}

uint64_t la_gpu_lzip_compress_member_bytes(uint32_t level)
{
	return level <= 9u ? la_lzip_compress_member_bytes(level) : 0u;
}
uint64_t la_gpu_lzip_compress_workspace_bytes(uint64_t src_bytes, uint32_t level)
{
	return level <= 9u && src_bytes <= LA_LZC_MAX_SRC_BYTES ? la_lzip_compress_ws_bytes(src_bytes, level) : 0u;
}
uint64_t la_gpu_lzip_compress_bound(uint64_t src_bytes, uint32_t level)
{
	return level <= 9u ? la_lzip_compress_bound(src_bytes, level) : 0u;
}
int la_gpu_lzip_compress(la_gpu_ctx *c, const la_lzc_batch *bt)
{
	if (!c || !bt || !bt->d_out_bytes || (bt->src_bytes && !bt->d_src) || (bt->out_cap && !bt->d_out))
		return LA_ERR_ARG;
	if (bt->level > 9u || bt->flags != 0u || bt->src_bytes > LA_LZC_MAX_SRC_BYTES)
		return LA_ERR_ARG;
	return compress_run(c, la_lzip_compress_ws_bytes(bt->src_bytes, bt->level), "lzip_compress", [&](uint8_t *ws) {
		bz2c_prof pr = { c, -1 };
		const la_stage_hook hook = { bz2c_mark, &pr };
		la_launch_lzip_compress(c->stream, bt, ws, &hook);
	});
}

static bool lzopc_block_size_ok(uint64_t src_bytes, uint32_t block_size)
{
	return block_size >= 1u && block_size <= LA_LZOPC_BLOCK_BYTES && (src_bytes + block_size - 1) / block_size <= 0x7FFFFFFEull;
}
uint64_t la_gpu_lzop_compress_workspace_bytes(uint64_t src_bytes, uint32_t block_size)
{
	return lzopc_block_size_ok(src_bytes, block_size) ? la_lzop_compress_ws_bytes(src_bytes, block_size) : 0u;
}
uint64_t la_gpu_lzop_compress_bound(uint64_t src_bytes, uint32_t block_size)
{
	return block_size ? src_bytes + 12u * ((src_bytes + block_size - 1) / block_size) : 0u;
}
int la_gpu_lzop_compress(la_gpu_ctx *c, const la_lzopc_batch *bt)
{
	if (!c || !bt || !bt->d_out_bytes || (bt->src_bytes && !bt->d_src) || (bt->out_cap && !bt->d_out))
		return LA_ERR_ARG;
	if (!lzopc_block_size_ok(bt->src_bytes, bt->block_size))
		return LA_ERR_ARG;
	return compress_run(c, la_lzop_compress_ws_bytes(bt->src_bytes, bt->block_size), "lzop_compress", [&](uint8_t *ws) {
		la_launch_lzop_compress(c->stream, bt, ws);
	});
}

} /* extern "C" */
