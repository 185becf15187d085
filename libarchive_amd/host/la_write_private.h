/*
 * la_write_private.h -- what the write filters share with the minimal write core of la_write_filters.c: the
 * reference's write-filter vtable (libarchive/archive_write_private.h:46-63), the two calls a filter makes on it,
 * and the write window every device-backed filter (lz4, gzip, zstd) is built on.  The lz4 and gzip filters live in
 * la_write_filters.c, the zstd filter, whose option parsing is longer, in la_write_zstd.c.
 */
#ifndef LA_WRITE_PRIVATE_H
#define LA_WRITE_PRIVATE_H

#include <stddef.h>
#include <stdint.h>

#include "la_read_private.h"
#include "../../include/la_gpu.h"

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

/* The write window: write() gathers the input into a pinned window, a full window (LA_GPU_WRITE_WINDOW_MIB, default
 * 64) goes to the device in ONE compress call and the stream bytes come back in one copy.  A filter's private data
 * starts with one (f->data points at it); the filter sets `name`, `bound` and `compress` before la_write_window_open
 * and owns nothing else that needs freeing. */
struct la_write_window {
	const char *name;	/* the filter's, in error strings */
	/* the codec: stream bytes n input bytes can take; one compress call of the window on the device */
	uint64_t (*bound)(struct archive_write_filter *, uint64_t n);
	int (*compress)(struct archive_write_filter *, const struct la_write_window *);
	la_gpu_ctx *gpu;
	uint8_t *win;		/* pinned input window */
	size_t cap, len;
	void *d_in, *d_out, *d_len;	/* device copy of the window, its stream bytes, their count */
	uint8_t *out;		/* pinned copy of the stream bytes */
	uint64_t out_cap;
	int wrote_anything;
};

/* opens the device, sizes the window down to whole `unit`s (at least one) and sets f->write */
int la_write_window_open(struct archive_write_filter *, size_t unit);
/* compresses the window (an empty one too when `force_empty`) and hands the bytes to the next filter */
int la_write_window_flush(struct archive_write_filter *, int force_empty);
/* "<name> GPU data plane: <what> failed: <device error>", ARCHIVE_FATAL */
int la_write_window_fail(struct archive_write_filter *, const char *what);
/* the filter's free(): releases the window and the private data */
int la_write_window_free(struct archive_write_filter *);

#endif /* LA_WRITE_PRIVATE_H */
