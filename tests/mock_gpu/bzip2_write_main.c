/*
 * bzip2_write_main.c -- TEST INFRASTRUCTURE: the bzip2 write filter's host side under the sanitizers, as a program of
 * its own (host sources, the CPU mocks and this main in one link; see the Makefile).  It writes the shapes of
 * tests/test_host_bzip2_write_mock.py through archive_write_* and reads every image back with libbz2.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/la_archive.h"
#include "../../include/la_gpu.h"

int BZ2_bzBuffToBuffDecompress(char *dest, unsigned int *destLen, char *source, unsigned int sourceLen, int small, int verbosity);

static int fails;
#define CHECK(x) do { if (!(x)) { fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #x); fails++; } } while (0)

static uint8_t *make_data(size_t n, unsigned seed)
{
	uint8_t *p = malloc(n ? n : 1);
	uint32_t s = seed * 2654435761u + 1u;
	for (size_t i = 0; i < n; i++) {
		s = s * 1664525u + 1013904223u;
		p[i] = (uint8_t)("abcdefgh"[(s >> 24) & 7u]);	/* compressible, not trivial */
		if ((s >> 8 & 31u) == 0 && i >= 6) { memset(p + i - 6, 'z', 6); }
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
	CHECK(archive_write_add_filter_bzip2(a) == ARCHIVE_OK);
	CHECK(archive_write_set_format_raw(a) == ARCHIVE_OK);
	if (level)
		CHECK(archive_write_set_filter_option(a, "bzip2", "compression-level", level) == ARCHIVE_OK);
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

static void round_trip(size_t n, size_t piece, const char *level, unsigned seed)
{
	uint8_t *data = make_data(n, seed);
	const size_t cap = n + n / 50 + 4096;
	uint8_t *buf = malloc(cap), *back = malloc(n + 1);
	size_t used = 0;
	char err[256];
	CHECK(write_stream(data, n, piece ? piece : (n ? n : 1), level, buf, cap, &used, err, sizeof(err)) == ARCHIVE_OK);
	CHECK(used >= 14 && memcmp(buf, "BZh", 3) == 0 && buf[3] == (level && level[0] > '0' ? level[0] : level ? '1' : '9'));
	unsigned int got = (unsigned int)(n + 1);
	CHECK(BZ2_bzBuffToBuffDecompress((char *)back, &got, (char *)buf, (unsigned int)used, 0, 0) == 0);
	CHECK(got == n && memcmp(back, data, n) == 0);
	if (n == 0)
		CHECK(used == 14);
	free(data); free(buf); free(back);
}

int main(void)
{
	setenv("LA_GPU_WRITE_WINDOW_MIB", "1", 1);
	const size_t window = ((size_t)1 << 20) / la_gpu_bzip2_compress_block_bytes(1) * la_gpu_bzip2_compress_block_bytes(1);
	round_trip(0, 0, NULL, 1);
	round_trip(0, 0, "1", 1);
	round_trip(1, 0, "0", 2);
	round_trip(1, 0, NULL, 2);
	round_trip(window, 4096, "1", 3);		/* ends on the window boundary: close() writes the trailer alone */
	round_trip(window + 1, 65536 + 17, "1", 4);
	round_trip(3 * window - 5, 99991, "1", 5);	/* three windows */
	round_trip(300000, 1000, NULL, 6);
	{	/* the client's buffer is too small */
		uint8_t *data = make_data(200000, 7), buf[100];
		size_t used = 0;
		char err[256];
		CHECK(write_stream(data, 200000, 200000, "1", buf, sizeof(buf), &used, err, sizeof(err)) == ARCHIVE_FATAL);
		CHECK(strcmp(err, "Buffer exhausted") == 0);
		free(data);
	}
	{	/* options */
		struct archive *a = archive_write_new();
		CHECK(archive_write_add_filter_bzip2(a) == ARCHIVE_OK);
		CHECK(archive_write_set_filter_option(a, "bzip2", "compression-level", "10") == ARCHIVE_FAILED);
		CHECK(archive_write_set_filter_option(a, "bzip2", "compression-level", "a") == ARCHIVE_FAILED);
		CHECK(archive_write_set_filter_option(a, "bzip2", "compression-level", NULL) == ARCHIVE_FAILED);
		CHECK(archive_write_set_filter_option(a, "bzip2", "no-such-option", "1") == ARCHIVE_FAILED);
		CHECK(archive_write_set_filter_option(a, "bzip2", "compression-level", "5") == ARCHIVE_OK);
		archive_write_free(a);
	}
	if (fails) {
		fprintf(stderr, "%d checks failed\n", fails);
		return 1;
	}
	puts("bzip2 write: all shapes round-trip");
	return 0;
}
