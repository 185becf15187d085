/*
 * la_read_main.c -- TEST INFRASTRUCTURE: a program of its own that reads compressed images of any format through the
 * host side (read core, every read filter) over the CPU mock of the device ABI, for the sanitizer build of the Makefile.
 *
 *   la_read_asan FILE...      every file is one image; prints "rc bytes fnv1a message" per file
 *
 * Each image is read three ways: in one piece, 1000 bytes at a time and 1 byte at a time (the last only below 64 KiB),
 * and the three must agree.
 */
#include "../../include/la_archive.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

void la_gpu_bzip2_mock_release(void);

static int read_image(const unsigned char *img, size_t n, size_t read_size, unsigned long long *bytes, unsigned long long *hash, char *msg, size_t msg_cap)
{
	struct archive *a = archive_read_new();
	struct archive_entry *e;
	int r;
	*bytes = 0; *hash = 1469598103934665603ull; msg[0] = 0;
	archive_read_support_filter_all(a);
	archive_read_support_format_empty(a);
	archive_read_support_format_raw(a);
	r = archive_read_open_memory2(a, img, n, read_size);
	if (r == ARCHIVE_OK)
		r = archive_read_next_header(a, &e);
	if (r == ARCHIVE_OK) {
		const void *p; size_t sz; int64_t off;
		while ((r = archive_read_data_block(a, &p, &sz, &off)) == ARCHIVE_OK) {
			for (size_t i = 0; i < sz; i++)
				*hash = (*hash ^ ((const unsigned char *)p)[i]) * 1099511628211ull;
			*bytes += sz;
		}
	}
	if (r != ARCHIVE_EOF && archive_error_string(a))
		snprintf(msg, msg_cap, "%s", archive_error_string(a));
	archive_read_free(a);
	return r == ARCHIVE_EOF ? 0 : r;
}

int main(int argc, char **argv)
{
	int bad = 0;
	for (int k = 1; k < argc; k++) {
		FILE *f = fopen(argv[k], "rb");
		if (!f) { perror(argv[k]); return 2; }
		fseek(f, 0, SEEK_END);
		const long n = ftell(f);
		fseek(f, 0, SEEK_SET);
		unsigned char *img = malloc(n > 0 ? (size_t)n : 1);
		if (!img || fread(img, 1, (size_t)n, f) != (size_t)n) { fprintf(stderr, "%s: read error\n", argv[k]); return 2; }
		fclose(f);
		unsigned long long b0, h0, b, h;
		char m0[256], m[256];
		const int r0 = read_image(img, (size_t)n, (size_t)n ? (size_t)n : 1, &b0, &h0, m0, sizeof(m0));
		printf("%d %llu %016llx %s\n", r0, b0, h0, m0);
		const size_t sizes[2] = { 1000, 1 };
		for (int s = 0; s < 2; s++) {
			if (sizes[s] == 1 && n > 65536)
				continue;
			const int r = read_image(img, (size_t)n, sizes[s], &b, &h, m, sizeof(m));
			if (r != r0 || b != b0 || h != h0 || strcmp(m, m0) != 0) {
				fprintf(stderr, "%s: read size %zu gives %d %llu %016llx %s\n", argv[k], sizes[s], r, b, h, m);
				bad = 1;
			}
		}
		free(img);
	}
	la_gpu_bzip2_mock_release();
	return bad;
}
