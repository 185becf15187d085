/*
 * lzip_write_main.c -- TEST INFRASTRUCTURE: the lzip write filter's host side and the encoder's rules header under the
 * sanitizers, as a program of its own (host sources, the CPU mocks and this main in one link; see the Makefile).  It
 * writes the shapes of tests/lzip_write_support.py (the member borders, noise, runs, the large member, several windows)
 * through archive_write_* and reads every image back through the project's own lzip read filter over the decode
 * stand-in (archive_read_*), which compiles the decoder's rules header.  The stand-in's entry is also called with short
 * output buffers inside exactly sized allocations, so a byte stored at or behind out_cap is a finding.
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

/* kind 0: compressible letters with runs; 1: noise (expands); 2: one value */
static uint8_t *make_data(size_t n, unsigned seed, int kind)
{
	uint8_t *p = malloc(n ? n : 1);
	uint32_t s = seed * 2654435761u + 1u;
	for (size_t i = 0; i < n; i++) {
		s = s * 1664525u + 1013904223u;
		p[i] = kind == 1 ? (uint8_t)(s >> 24) : kind == 2 ? 7 : (uint8_t)("abcdefgh"[(s >> 24) & 7u]);
		if (kind == 0 && (s >> 8 & 31u) == 0 && i >= 6) { memset(p + i - 6, 'z', 6); }
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
	CHECK(archive_write_add_filter_lzip(a) == ARCHIVE_OK);
	CHECK(archive_write_set_format_raw(a) == ARCHIVE_OK);
	if (level)
		CHECK(archive_write_set_filter_option(a, "lzip", "compression-level", level) == ARCHIVE_OK);
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

/* the image through archive_read_*: the lzip read filter, the raw format (the empty one for a member of no data) */
static size_t read_back(const uint8_t *img, size_t used, uint8_t *back, size_t cap)
{
	struct archive *a = archive_read_new();
	struct archive_entry *e;
	size_t got = 0;
	CHECK(archive_read_support_filter_lzip(a) == ARCHIVE_OK);
	CHECK(archive_read_support_format_empty(a) == ARCHIVE_OK);	/* (a member of no data is no raw entry) */
	CHECK(archive_read_support_format_raw(a) == ARCHIVE_OK);
	CHECK(archive_read_open_memory(a, img, used) == ARCHIVE_OK);
	if (archive_read_next_header(a, &e) == ARCHIVE_OK) {
		CHECK(archive_filter_code(a, 0) == ARCHIVE_FILTER_LZIP && strcmp(archive_filter_name(a, 0), "lzip") == 0);
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

static uint64_t le64(const uint8_t *p)
{
	uint64_t v = 0;
	for (int i = 0; i < 8; i++)
		v |= (uint64_t)p[i] << (8 * i);
	return v;
}

static void round_trip(size_t n, size_t piece, const char *level, unsigned seed, int kind)
{
	const size_t unit = level && level[0] >= '7' ? 4 * M : M, members = n ? (n + unit - 1) / unit : 1;
	uint8_t *data = make_data(n, seed, kind);
	const size_t cap = n + n / 20 + 64 * members + 4096;
	uint8_t *buf = malloc(cap), *back = malloc(n + 64);
	size_t used = 0, at = 0, count = 0;
	char err[256];
	CHECK(write_stream(data, n, piece ? piece : (n ? n : 1), level, buf, cap, &used, err, sizeof(err)) == ARCHIVE_OK);
	/* the members chain to the image's end and carry the cut of the data */
	while (at + 26 <= used && memcmp(buf + at, "LZIP\x01", 5) == 0) {
		/* the sizes stand at the member's end: the first end whose trailer names this member's data cut and its own length */
		const size_t want = n - count * unit < unit ? n - count * unit : unit;
		size_t end = at + 26;
		while (end <= used && !(le64(buf + end - 16) == want && le64(buf + end - 8) == end - at))
			end++;
		CHECK(end <= used);
		if (end > used)
			break;
		CHECK(buf[at + 5] == (unit == M ? 0x10 : 0x12));
		at = end;
		count++;
	}
	CHECK(at == used && count == members);
	CHECK(read_back(buf, used, back, n + 64) == n && (n == 0 || memcmp(back, data, n) == 0));
	free(data); free(buf); free(back);
}

/* the ABI entry with `cap` bytes of room in an allocation of exactly that size */
static void short_buffer(size_t n, uint32_t level, int kind)
{
	uint8_t *data = make_data(n, 11, kind);
	const uint64_t bound = la_gpu_lzip_compress_bound(n, level);
	uint8_t *whole = malloc(bound);
	uint64_t need = 0, got = 0;
	la_lzc_batch bt;
	memset(&bt, 0, sizeof(bt));
	bt.d_src = n ? data : NULL; bt.src_bytes = n; bt.level = level;
	bt.d_out = whole; bt.out_cap = bound; bt.d_out_bytes = &need;
	CHECK(la_gpu_lzip_compress((la_gpu_ctx *)&bt, &bt) == LA_OK && need <= bound && need >= 26);
	const uint64_t caps[5] = { 0, 5, 6, 25, need - 1 };
	for (int i = 0; i < 5; i++) {
		uint8_t *part = malloc(caps[i] ? caps[i] : 1);
		bt.d_out = caps[i] ? part : NULL; bt.out_cap = caps[i]; bt.d_out_bytes = &got;
		CHECK(la_gpu_lzip_compress((la_gpu_ctx *)&bt, &bt) == LA_OK && got == need);
		CHECK(caps[i] == 0 || memcmp(part, whole, caps[i]) == 0);
		free(part);
	}
	bt.level = 10;
	CHECK(la_gpu_lzip_compress((la_gpu_ctx *)&bt, &bt) == LA_ERR_ARG);
	bt.level = level; bt.flags = 1;
	CHECK(la_gpu_lzip_compress((la_gpu_ctx *)&bt, &bt) == LA_ERR_ARG);
	free(data); free(whole);
}

int main(void)
{
	setenv("LA_GPU_WRITE_WINDOW_MIB", "1", 1);
	setenv("LA_GPU_BID", "all", 1);
	const size_t window = (size_t)1 << 20;
	round_trip(0, 0, NULL, 1, 0);
	round_trip(0, 0, "9", 1, 0);
	round_trip(1, 0, "0", 2, 0);
	round_trip(M - 1, 0, NULL, 2, 0);
	round_trip(M, 4096, NULL, 3, 0);
	round_trip(M + 1, 0, NULL, 3, 0);			/* a one-byte last member */
	round_trip(3 * M + 5, 1000, "0", 4, 0);
	round_trip(2 * M + 5, 1000, NULL, 6, 1);		/* noise: expands */
	round_trip(3 * M, 70000, "0", 7, 2);			/* one value: long matches split */
	round_trip(4 * M + 1, 65536 + 17, "9", 8, 0);		/* the large member and one byte */
	round_trip(window, 4096, NULL, 9, 0);			/* ends on the window boundary */
	round_trip(3 * window - 5, 99991, "7", 5, 0);		/* three windows */
	short_buffer(0, 6, 0);
	short_buffer(M + 7, 6, 0);
	short_buffer(M + 7, 9, 1);
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
		CHECK(archive_write_add_filter_lzip(a) == ARCHIVE_OK);
		CHECK(archive_write_set_filter_option(a, "lzip", "compression-level", "10") == ARCHIVE_FAILED);
		CHECK(archive_write_set_filter_option(a, "lzip", "compression-level", "a") == ARCHIVE_FAILED);
		CHECK(archive_write_set_filter_option(a, "lzip", "compression-level", NULL) == ARCHIVE_FAILED);
		CHECK(archive_write_set_filter_option(a, "lzip", "threads", "x") == ARCHIVE_FAILED);
		CHECK(archive_write_set_filter_option(a, "lzip", "no-such-option", "1") == ARCHIVE_FAILED);
		CHECK(archive_write_set_filter_option(a, "lzip", "threads", "0") == ARCHIVE_OK);
		CHECK(archive_write_set_filter_option(a, "lzip", "compression-level", "5") == ARCHIVE_OK);
		archive_write_free(a);
	}
	if (fails) {
		fprintf(stderr, "%d checks failed\n", fails);
		return 1;
	}
	puts("lzip write: all shapes round-trip");
	return 0;
}
