/*
 * la_write_private.h -- what the write filters and formats share with the minimal write core of la_write_filters.c:
 * the reference's write-filter vtable (libarchive/archive_write_private.h:46-63), the two calls a filter makes on it,
 * the write handle with the reference's format hooks (:75-125), and the write window everything device-backed (the
 * lz4, gzip and zstd filters, the ZIP format) is built on.  The lz4 and gzip filters and the raw format live in
 * la_write_filters.c, the zstd filter, whose option parsing is longer, in la_write_zstd.c, the ZIP format in
 * la_write_zip.c.
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

struct archive_write {	/* archive_write_private.h:75-125, the members this slice uses */
	struct archive archive;		/* first: the error helpers of la_read_core.c work on it */
	struct archive_write_filter *filter_first, *filter_last;
	/* client */
	uint8_t *mem; size_t mem_cap, *mem_used;
	int fd;
	int opened, closed;
	/* the format, set by archive_write_set_format_XXX() (:110-124); format_init runs at the end of open */
	void *format_data;
	const char *format_name;
	int (*format_init)(struct archive_write *);
	int (*format_options)(struct archive_write *, const char *key, const char *value);
	int (*format_finish_entry)(struct archive_write *);
	int (*format_write_header)(struct archive_write *, struct archive_entry *);
	ssize_t (*format_write_data)(struct archive_write *, const void *buff, size_t);
	int (*format_close)(struct archive_write *);
	int (*format_free)(struct archive_write *);
};

/* what a format writes goes to the first filter of the chain (archive_write.c __archive_write_output) */
int __archive_write_output(struct archive_write *, const void *, size_t);

/* The write window: write() gathers the input into a pinned window, a full window (LA_GPU_WRITE_WINDOW_MIB, default
 * 64) goes to the device in ONE compress call and the stream bytes come back in one copy.  A filter's private data
 * starts with one (f->data points at it); the filter sets `name`, `bound` and `compress` before la_write_window_open
 * and owns nothing else that needs freeing. */
struct la_write_window {
	const char *name;	/* the filter's, in error strings */
	/* the codec: stream bytes n input bytes can take; one compress call of the window on the device */
	uint64_t (*bound)(struct archive_write_filter *, uint64_t n);
	int (*compress)(struct archive_write_filter *, const struct la_write_window *);
	/* optional: called with the `total` stream bytes back in `out`, before they are handed on (the ZIP format writes
	 * its headers into the gaps it asked for); ARCHIVE_OK or what the flush is to return */
	int (*patch)(struct archive_write_filter *, const struct la_write_window *, uint64_t total);
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
