/*
 * zip_write_main.c -- TEST INFRASTRUCTURE: a program of its own that writes a ZIP archive of many small entries to
 * memory through archive_write_* (host sources + the CPU mock of the device), to be built with
 * -fsanitize=address,undefined and run as it is.  Exit status 0 and "ok <entries> <bytes>" mean the archive was
 * written, every call answered as expected and the end record says what was written.
 */
#include "../../include/la_archive.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "%s:%d: %s: %s\n", __FILE__, __LINE__, #x, a && archive_error_string(a) ? archive_error_string(a) : ""); return 1; } } while (0)

int main(int argc, char **argv)
{
	const int n = argc > 1 ? atoi(argv[1]) : 3000;
	const size_t cap = (size_t)n * 1200 + (1u << 20);
	unsigned char *buf = malloc(cap), data[700];
	size_t used = 0;
	struct archive *a = archive_write_new();
	struct archive_entry *e = archive_entry_new();
	CHECK(buf && a && e);
	setenv("LA_GPU_WRITE_WINDOW_MIB", "1", 1);
	CHECK(archive_write_set_format_zip(a) == ARCHIVE_OK);
	CHECK(archive_write_set_format_option(a, "zip", "compression-level", "9") == ARCHIVE_OK);
	CHECK(archive_write_set_format_option(a, "zip", "no-such-option", "1") == ARCHIVE_FAILED);
	CHECK(archive_write_open_memory(a, buf, cap, &used) == ARCHIVE_OK);
	for (int i = 0; i < n; i++) {
		char name[64];
		const size_t len = (size_t)((i * 37) % (int)sizeof(data));
		for (size_t k = 0; k < len; k++)
			data[k] = (unsigned char)("zip writer "[(k + (size_t)i) % 11]);
		archive_entry_clear(e);
		snprintf(name, sizeof(name), "dir%d/file%05d.txt", i % 7, i);
		archive_entry_set_pathname(e, name);
		archive_entry_set_mtime(e, 1700000000 + i, 0);
		archive_entry_set_perm(e, 0644);
		if (i % 50 == 49) {
			archive_entry_set_filetype(e, 0040000);
			archive_entry_set_perm(e, 0755);
		} else {
			archive_entry_set_filetype(e, 0100000);
			if (i % 3)
				archive_entry_set_size(e, (long long)(i % 5 == 0 ? len / 2 : len));	/* some are written past their size */
		}
		CHECK(archive_write_header(a, e) == ARCHIVE_OK);
		if (i % 50 != 49)
			CHECK(archive_write_data(a, data, len) >= 0);
		if (i % 4 == 0)
			CHECK(archive_write_finish_entry(a) == ARCHIVE_OK);
	}
	archive_entry_set_filetype(e, 0120000);
	CHECK(archive_write_header(a, e) == ARCHIVE_FAILED);
	CHECK(archive_write_close(a) == ARCHIVE_OK);
	CHECK(used > 22 && memcmp(buf + used - 22, "PK\005\006", 4) == 0);
	CHECK((buf[used - 12] | buf[used - 11] << 8) == n);
	archive_entry_free(e);
	CHECK(archive_write_free(a) == ARCHIVE_OK);
	a = NULL;
	printf("ok %d %zu\n", n, used);
	free(buf);
	return 0;
}
