/*
 * xz_write_main.c -- TEST INFRASTRUCTURE: the xz write filter's host side and the encoder's rules header under the
 * sanitizers, as a program of its own (host sources, the CPU mocks and this main in one link; see the Makefile).  It
 * writes the shapes of tests/test_host_xz_write_mock.py through archive_write_* and reads every image back through the
 * project's own xz read filter over the decode stand-in (archive_read_*), which compiles the decoder's rules header.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/la_archive.h"
#include "../../include/la_gpu.h"

static int fails;
#define CHECK(x) do { if (!(x)) { fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #x); fails++; } } while (0)

/* kind 0: compressible letters with runs; 1: noise (stored chunks); 2: one value */
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
	CHECK(archive_write_add_filter_xz(a) == ARCHIVE_OK);
	CHECK(archive_write_set_format_raw(a) == ARCHIVE_OK);
	if (level)
		CHECK(archive_write_set_filter_option(a, "xz", "compression-level", level) == ARCHIVE_OK);
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

/* the image through archive_read_*: the xz read filter, the raw format */
static size_t read_back(const uint8_t *img, size_t used, uint8_t *back, size_t cap)
{
	struct archive *a = archive_read_new();
	struct archive_entry *e;
	size_t got = 0;
	CHECK(archive_read_support_filter_xz(a) == ARCHIVE_OK);
	CHECK(archive_read_support_format_raw(a) == ARCHIVE_OK);
	CHECK(archive_read_open_memory(a, img, used) == ARCHIVE_OK);
	if (archive_read_next_header(a, &e) == ARCHIVE_OK) {
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

static void round_trip(size_t n, size_t piece, const char *level, unsigned seed, int kind)
{
	uint8_t *data = make_data(n, seed, kind);
	const size_t cap = n + n / 50 + 4096;
	uint8_t *buf = malloc(cap), *back = malloc(n + 64);
	size_t used = 0;
	char err[256];
	CHECK(write_stream(data, n, piece ? piece : (n ? n : 1), level, buf, cap, &used, err, sizeof(err)) == ARCHIVE_OK);
	CHECK(used >= 32 && memcmp(buf, "\xFD" "7zXZ", 6) == 0 && memcmp(buf + used - 2, "YZ", 2) == 0);
	if (n == 0)
		CHECK(used == 32);
	else
		CHECK(read_back(buf, used, back, n + 64) == n && memcmp(back, data, n) == 0);
	free(data); free(buf); free(back);
}

int main(void)
{
	setenv("LA_GPU_WRITE_WINDOW_MIB", "1", 1);
	setenv("LA_GPU_BID", "all", 1);
	const size_t window = (size_t)1 << 20;
	round_trip(0, 0, NULL, 1, 0);
	round_trip(0, 0, "0", 1, 0);
	round_trip(1, 0, "0", 2, 0);
	round_trip(1, 0, NULL, 2, 0);
	round_trip(window, 4096, "0", 3, 0);		/* ends on the window boundary */
	round_trip(window + 1, 65536 + 17, NULL, 4, 0);
	round_trip(3 * window - 5, 99991, "9", 5, 0);	/* three windows */
	round_trip(2 * 65536 + 5, 1000, NULL, 6, 1);	/* stored chunks */
	round_trip(3 * 65536, 70000, "0", 7, 2);	/* one value: long matches split */
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
		CHECK(archive_write_add_filter_xz(a) == ARCHIVE_OK);
		CHECK(archive_write_set_filter_option(a, "xz", "compression-level", "10") == ARCHIVE_FAILED);
		CHECK(archive_write_set_filter_option(a, "xz", "compression-level", "a") == ARCHIVE_FAILED);
		CHECK(archive_write_set_filter_option(a, "xz", "compression-level", NULL) == ARCHIVE_FAILED);
		CHECK(archive_write_set_filter_option(a, "xz", "threads", "x") == ARCHIVE_FAILED);
		CHECK(archive_write_set_filter_option(a, "xz", "no-such-option", "1") == ARCHIVE_FAILED);
		CHECK(archive_write_set_filter_option(a, "xz", "threads", "0") == ARCHIVE_OK);
		CHECK(archive_write_set_filter_option(a, "xz", "compression-level", "5") == ARCHIVE_OK);
		archive_write_free(a);
	}
	if (fails) {
		fprintf(stderr, "%d checks failed\n", fails);
		return 1;
	}
	puts("xz write: all shapes round-trip");
	return 0;
}
