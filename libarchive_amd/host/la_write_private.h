/*
 * la_write_private.h -- what the write filters share with the minimal write core of la_write_filters.c: the
 * reference's write-filter vtable (libarchive/archive_write_private.h:46-63) and the two calls a filter makes on it.
 * la_write_zstd.c lives in a file of its own so that the builds that link la_write_filters.c against the CPU mock of
 * today's device ABI do not need la_gpu_zstd_compress.
 */
#ifndef LA_WRITE_PRIVATE_H
#define LA_WRITE_PRIVATE_H

#include <stddef.h>
#include <stdint.h>

#include "la_read_private.h"

struct archive_write_filter {	/* archive_write_private.h:46-63 */
	int64_t bytes_written;
	struct archive *archive;
	struct archive_write_filter *next_filter;
	int (*options)(struct archive_write_filter *, const char *key, const char *value);
	int (*open)(struct archive_write_filter *);
	int (*write)(struct archive_write_filter *, const void *, size_t);
	int (*flush)(struct archive_write_filter *);
	int (*close)(struct archive_write_filter *);
	int (*free)(struct archive_write_filter *);
	void *data;
	const char *name;
	int code;
	int bytes_per_block;
	int bytes_in_last_block;
	int state;
};

struct archive_write_filter *__archive_write_allocate_filter(struct archive *);
int __archive_write_filter(struct archive_write_filter *, const void *, size_t);

#endif /* LA_WRITE_PRIVATE_H */
