/*
 * lzop_write_main.c -- TEST INFRASTRUCTURE: the lzop write filter's host side and the encoder's rules header under the
 * sanitizers, as a program of its own (host sources, the CPU mocks and this main in one link; see the GNUmakefile).  It
 * writes the shapes of tests/lzop_write_support.py (the block borders, noise, runs, far pairs at both sides of the
 * longest distance, short and long literal runs, several windows) through archive_write_* and reads every image back
 * through the project's own lzop read filter over the decode stand-in (archive_read_*), which compiles the decoder's
 * rules header.  The stand-in's entry is also called with short output buffers inside exactly sized allocations, so a
 * byte stored at or behind out_cap is a finding.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/la_archive.h"
#include "../../include/la_gpu.h"

static int fails;
#define CHECK(x) do { if (!(x)) { fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #x); fails++; } } while (0)

#define M ((size_t)65536)

static uint32_t rnd_state;
static uint8_t rnd(void)
{
	rnd_state = rnd_state * 1664525u + 1013904223u;
	return (uint8_t)(rnd_state >> 24);
}

/* kind 0: compressible letters with runs; 1: noise (stored); 2: one value */
static uint8_t *make_data(size_t n, unsigned seed, int kind)
{
	uint8_t *p = malloc(n ? n : 1);
	rnd_state = seed * 2654435761u + 1u;
	for (size_t i = 0; i < n; i++) {
		const uint8_t r = rnd();
		p[i] = kind == 1 ? r : kind == 2 ? 7 : (uint8_t)("abcdefgh"[r & 7u]);
		if (kind == 0 && (rnd_state >> 8 & 31u) == 0 && i >= 6) { memset(p + i - 6, 'z', 6); }
	}
	return p;
}

/* a run of one value with a 64-byte random marker at 100 and again `dist` behind it */
static uint8_t *make_pair(size_t n, size_t dist)
{
	uint8_t *p = malloc(n);
	memset(p, 'r', n);
	rnd_state = (uint32_t)dist;
	for (size_t i = 0; i < 64; i++)
		p[100 + i] = p[100 + dist + i] = rnd();
	return p;
}

/* runs of one value separated by gaps of random bytes, the gap lengths cycling through `gaps` */
static uint8_t *make_gaps(size_t n, const unsigned *gaps, size_t n_gaps)
{
	uint8_t *p = malloc(n);
	size_t at = 0, k = 0;
	rnd_state = 77u;
	while (at < n) {
		const size_t run = 40 + 37 * (k % 9);
		for (size_t i = 0; i < run && at < n; i++)
			p[at++] = (uint8_t)('A' + k % 5);
		for (size_t i = 0; i < gaps[k % n_gaps] && at < n; i++)
			p[at++] = rnd();
		k++;
	}
	return p;
}

/* returns the close code; *used = bytes written */
static int write_stream(const uint8_t *data, size_t n, size_t piece, const char *level, uint8_t *buf, size_t cap, size_t *used, char *err,
    size_t errn)
{
	struct archive *a = archive_write_new();
	int rc;
	err[0] = '\0';
	CHECK(archive_write_add_filter_lzop(a) == ARCHIVE_OK);
	CHECK(archive_write_set_format_raw(a) == ARCHIVE_OK);
	if (level)
		CHECK(archive_write_set_filter_option(a, "lzop", "compression-level", level) == ARCHIVE_OK);
	CHECK(archive_write_open_memory(a, buf, cap, used) == ARCHIVE_OK);
	CHECK(archive_write_header(a, NULL) == ARCHIVE_OK);
	rc = ARCHIVE_OK;
	for (size_t i = 0; i < n && rc == ARCHIVE_OK; i += piece) {
		const size_t m = n - i < piece ? n - i : piece;
		if (archive_write_data(a, data + i, m) != (ssize_t)m)
			rc = ARCHIVE_FATAL;
	}
	if (rc == ARCHIVE_OK)
		rc = archive_write_close(a);
	if (rc != ARCHIVE_OK && archive_error_string(a))
		snprintf(err, errn, "%s", archive_error_string(a));
	archive_write_free(a);
	return rc;
}

/* the image through archive_read_*: the lzop read filter, the raw format (the empty one for a part without blocks) */
static size_t read_back(const uint8_t *img, size_t used, uint8_t *back, size_t cap)
{
	struct archive *a = archive_read_new();
	struct archive_entry *e;
	size_t got = 0;
	CHECK(archive_read_support_filter_lzop(a) == ARCHIVE_OK);
	CHECK(archive_read_support_format_empty(a) == ARCHIVE_OK);
	CHECK(archive_read_support_format_raw(a) == ARCHIVE_OK);
	CHECK(archive_read_open_memory(a, img, used) == ARCHIVE_OK);
	if (archive_read_next_header(a, &e) == ARCHIVE_OK) {
		CHECK(archive_filter_code(a, 0) == ARCHIVE_FILTER_LZOP && strcmp(archive_filter_name(a, 0), "lzop") == 0);
		for (;;) {
			const ssize_t k = archive_read_data(a, back + got, cap - got);
			CHECK(k >= 0);
			if (k <= 0)
				break;
			got += (size_t)k;
		}
	}
	archive_read_free(a);
	return got;
}

static uint32_t be32(const uint8_t *p)
{
	return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3];
}

/* takes `data`; returns the image's size */
static size_t round_trip(uint8_t *data, size_t n, size_t piece, const char *level)
{
	const size_t blocks = (n + M - 1) / M;
	const size_t cap = 38 + n + 12 * blocks + 4;		/* exactly the promised bound */
	uint8_t *buf = malloc(cap), *back = malloc(n + 64);
	size_t used = 0, at = 38, count = 0;
	char err[256];
	const int lv = level ? level[0] - '0' : 5;
	CHECK(write_stream(data, n, piece ? piece : (n ? n : 1), level, buf, cap, &used, err, sizeof(err)) == ARCHIVE_OK);
	/* header, blocks of the promised cut, the closing word, nothing behind */
	CHECK(used >= 42 && memcmp(buf, "\x89LZO\x00\x0d\x0a\x1a\x0a\x10\x30\x09\x40\x09\x40", 15) == 0);
	CHECK(buf[15] == (lv == 1 ? 2 : lv >= 7 ? 3 : 1) && buf[16] == (lv == 1 ? 1 : lv >= 7 ? lv : 5));
	while (at + 12 <= used && be32(buf + at) != 0) {
		const size_t want = n - count * M < M ? n - count * M : M;
		CHECK(be32(buf + at) == want && be32(buf + at + 4) <= want);
		at += 12 + be32(buf + at + 4);
		count++;
	}
	CHECK(count == blocks && at + 4 == used && be32(buf + at) == 0);
	CHECK(read_back(buf, used, back, n + 64) == n && (n == 0 || memcmp(back, data, n) == 0));
	free(data); free(buf); free(back);
	return used;
}

/* the ABI entry with `cap` bytes of room in an allocation of exactly that size */
static void short_buffer(size_t n, uint32_t block_size, uint32_t lead, int kind)
{
	uint8_t *data = make_data(n, 11, kind);
	const uint64_t bound = lead + la_gpu_lzop_compress_bound(n, block_size);
	uint8_t *whole = calloc(bound ? bound : 1, 1);
	uint64_t need = 0, got = 0;
	la_lzopc_batch bt;
	memset(&bt, 0, sizeof(bt));
	bt.d_src = n ? data : NULL; bt.src_bytes = n; bt.block_size = block_size; bt.lead_bytes = lead;
	bt.d_out = whole; bt.out_cap = bound; bt.d_out_bytes = &need;
	CHECK(la_gpu_lzop_compress((la_gpu_ctx *)&bt, &bt) == LA_OK && need <= bound && need >= lead);
	const uint64_t caps[5] = { 0, 5, lead + 11, lead + 12, need ? need - 1 : 0 };
	for (int i = 0; i < 5; i++) {
		uint8_t *part = calloc(caps[i] ? caps[i] : 1, 1);
		bt.d_out = caps[i] ? part : NULL; bt.out_cap = caps[i]; bt.d_out_bytes = &got;
		CHECK(la_gpu_lzop_compress((la_gpu_ctx *)&bt, &bt) == LA_OK && got == need);
		CHECK(caps[i] == 0 || memcmp(part, whole, caps[i] < need ? caps[i] : need) == 0);
		free(part);
	}
	bt.block_size = 0;
	CHECK(la_gpu_lzop_compress((la_gpu_ctx *)&bt, &bt) == LA_ERR_ARG);
	bt.block_size = 65537;
	CHECK(la_gpu_lzop_compress((la_gpu_ctx *)&bt, &bt) == LA_ERR_ARG);
	free(data); free(whole);
}

int main(void)
{
	setenv("LA_GPU_WRITE_WINDOW_MIB", "1", 1);
	setenv("LA_GPU_BID", "all", 1);
	const size_t window = (size_t)1 << 20;
	static const unsigned trails[4] = { 0, 1, 2, 3 }, lits[8] = { 4, 5, 18, 19, 20, 273, 274, 300 };
	CHECK(round_trip(make_data(0, 1, 0), 0, 0, NULL) == 42);
	CHECK(round_trip(make_data(0, 1, 0), 0, 0, "9") == 42);
	round_trip(make_data(1, 2, 0), 1, 0, "1");
	round_trip(make_data(3, 2, 0), 3, 0, NULL);
	round_trip(make_data(4, 2, 0), 4, 0, NULL);
	round_trip(make_data(M - 1, 2, 0), M - 1, 0, NULL);
	round_trip(make_data(M, 3, 0), M, 4096, NULL);
	round_trip(make_data(M + 1, 3, 0), M + 1, 0, NULL);		/* a one-byte last block */
	round_trip(make_data(3 * M + 5, 4, 0), 3 * M + 5, 1000, "7");
	CHECK(round_trip(make_data(2 * M + M / 2, 6, 1), 2 * M + M / 2, 1000, NULL) == 38 + 2 * M + M / 2 + 36 + 4);	/* noise: stored */
	round_trip(make_data(3 * M, 7, 2), 3 * M, 70000, "2");		/* one value: zero-runs, an overlapping distance */
	round_trip(make_pair(M, 20000), M, 0, NULL);
	round_trip(make_pair(M, 40000), M, 0, NULL);
	round_trip(make_pair(M, 49151), M, 0, NULL);
	round_trip(make_pair(M, 49152), M, 0, NULL);
	round_trip(make_gaps(M, trails, 4), M, 0, NULL);
	round_trip(make_gaps(M + 77, lits, 8), M + 77, 0, NULL);
	{	/* 300 random bytes, then a run: the long first literal run */
		uint8_t *p = make_data(5000, 9, 2), *q = make_data(300, 9, 1);
		memcpy(p, q, 300);
		free(q);
		round_trip(p, 5000, 0, NULL);
	}
	round_trip(make_data(window, 9, 0), window, 4096, NULL);		/* ends on the window boundary */
	round_trip(make_data(window + 1, 9, 0), window + 1, 65536 + 17, NULL);
	round_trip(make_data(3 * window - 5, 5, 0), 3 * window - 5, 99991, "8");	/* three windows */
	short_buffer(0, 65536, 38, 0);
	short_buffer(M + 7, 65536, 0, 0);
	short_buffer(M + 7, 4096, 38, 1);
	short_buffer(5000, 1, 3, 0);
	{	/* the client's buffer is too small */
		uint8_t *data = make_data(200000, 7, 1), buf[100];
		size_t used = 0;
		char err[256];
		CHECK(write_stream(data, 200000, 200000, "1", buf, sizeof(buf), &used, err, sizeof(err)) == ARCHIVE_FATAL);
		CHECK(strcmp(err, "Buffer exhausted") == 0);
		free(data);
	}
	{	/* options */
		struct archive *a = archive_write_new();
		CHECK(archive_write_add_filter_lzop(a) == ARCHIVE_OK);
		CHECK(archive_write_set_filter_option(a, "lzop", "compression-level", "0") == ARCHIVE_FAILED);
		CHECK(archive_write_set_filter_option(a, "lzop", "compression-level", "10") == ARCHIVE_FAILED);
		CHECK(archive_write_set_filter_option(a, "lzop", "compression-level", "a") == ARCHIVE_FAILED);
		CHECK(archive_write_set_filter_option(a, "lzop", "compression-level", NULL) == ARCHIVE_FAILED);
		CHECK(archive_write_set_filter_option(a, "lzop", "threads", "1") == ARCHIVE_FAILED);
		CHECK(archive_write_set_filter_option(a, "lzop", "no-such-option", "1") == ARCHIVE_FAILED);
		CHECK(archive_write_set_filter_option(a, "lzop", "compression-level", "5") == ARCHIVE_OK);
		archive_write_free(a);
	}
	if (fails) {
		fprintf(stderr, "%d checks failed\n", fails);
		return 1;
	}
	puts("lzop write: all shapes round-trip");
	return 0;
}
