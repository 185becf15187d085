/*
 * la_write_lzip.c -- the lzip WRITE filter on the device data plane (la_gpu_lzip_compress), registered on the write core
 * of la_write_filters.c.
 *
 * Registration and options follow libarchive/archive_write_add_filter_xz.c:202-218 and :371-410 (the reference serves
 * xz, lzma and lzip from one file and one option function): name "lzip", code ARCHIVE_FILTER_LZIP, default level 6;
 * "compression-level" takes exactly one character '0'..'9'; "threads" is parsed as the reference parses it (strtoul; NULL
 * or trailing garbage is ARCHIVE_WARN, 0 is accepted) and is WITHOUT EFFECT: the device codes every member of a window
 * at once, whatever the count.  Any other option or value returns ARCHIVE_WARN, which archive_write_set_filter_option
 * turns into ARCHIVE_FAILED "Undefined option".
 *
 * What differs from the reference by design:
 *   - write() only gathers input into the write window of la_write_private.h; a full window (LA_GPU_WRITE_WINDOW_MIB,
 *     default 64, whole members) goes to la_gpu_lzip_compress() in ONE call, which returns complete members back to back;
 *   - the output is MANY members per archive where the reference writes one: 64 KiB of input each at levels 0..6, 256 KiB
 *     at levels 7..9, with the dictionary byte that covers a member (0x10, 0x12) where the reference writes its preset's
 *     (the shape plzip writes, and the one this project's own reader is fastest on); the bytes are not liblzma's;
 *   - nothing is kept between windows and nothing is patched on the host: a member carries its own sizes and CRC32;
 *   - lzip has no uncompressed member, so the output buffers are sized by the coder's worst case, about seven times
 *     the window (include/la_gpu.h): 448 MiB on the device and as much pinned for the default window;
 *   - an archive without data is one member of no data, as the reference writes, and comes from the device call too.
 */
#include <errno.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "la_read_private.h"
#include "la_write_private.h"
#include "../../include/la_gpu.h"
#include "../../include/la_host.h"

struct lzw_private {
	struct la_write_window w;	/* first */
	int compression_level;
	int threads;			/* parsed, without effect */
};

static int lzw_options(struct archive_write_filter *f, const char *key, const char *value)
{
	struct lzw_private *d = f->data;
	if (strcmp(key, "compression-level") == 0) {
		if (value == NULL || !(value[0] >= '0' && value[0] <= '9') || value[1] != '\0')
			return ARCHIVE_WARN;
		d->compression_level = value[0] - '0';
		return ARCHIVE_OK;
	}
	if (strcmp(key, "threads") == 0) {	/* archive_write_add_filter_xz.c:385-403 */
		char *end;
		if (value == NULL)
			return ARCHIVE_WARN;
		errno = 0;
		d->threads = (int)strtoul(value, &end, 10);
		if (errno != 0 || *end != '\0') {
			d->threads = 1;
			return ARCHIVE_WARN;
		}
		return ARCHIVE_OK;
	}
	return ARCHIVE_WARN;
}

static uint64_t lzw_bound(struct archive_write_filter *f, uint64_t n)
{
	const struct lzw_private *d = f->data;
	return la_gpu_lzip_compress_bound(n, (uint32_t)d->compression_level);
}

static int lzw_compress(struct archive_write_filter *f, const struct la_write_window *w)
{
	const struct lzw_private *d = f->data;
	la_lzc_batch bt;
	memset(&bt, 0, sizeof(bt));
	bt.d_src = w->len ? w->d_in : NULL; bt.src_bytes = w->len;
	bt.level = (uint32_t)d->compression_level;
	bt.d_out = w->d_out; bt.out_cap = w->out_cap; bt.d_out_bytes = w->d_len;
	return la_gpu_lzip_compress(w->gpu, &bt);
}

static int lzw_open(struct archive_write_filter *f)
{
	struct lzw_private *d = f->data;
	const size_t unit = (size_t)la_gpu_lzip_compress_member_bytes((uint32_t)d->compression_level);
	int r = la_write_window_open(f, unit);	/* whole members */
	if (r != ARCHIVE_OK)
		return r;
	if (d->w.cap > LA_LZC_MAX_SRC_BYTES)
		d->w.cap = (size_t)(LA_LZC_MAX_SRC_BYTES / unit * unit);
	return ARCHIVE_OK;
}

static int lzw_close(struct archive_write_filter *f)
{
	struct lzw_private *d = f->data;
	if (d->w.gpu == NULL)
		return ARCHIVE_OK;
	/* nothing written at all: the empty window goes to the device once and comes back as one member of no data */
	return la_write_window_flush(f, !d->w.wrote_anything);
}

int archive_write_add_filter_lzip(struct archive *_a)
{
	struct archive_write_filter *f = __archive_write_allocate_filter(_a);
	struct lzw_private *d = calloc(1, sizeof(*d));
	if (f == NULL || d == NULL) {
		free(d);
		archive_set_error(_a, ENOMEM, "Out of memory");
		return ARCHIVE_FATAL;
	}
	d->w.name = "lzip";
	d->w.bound = lzw_bound;
	d->w.compress = lzw_compress;
	d->compression_level = 6;	/* LZMA_PRESET_DEFAULT, archive_write_add_filter_xz.c:152 */
	d->threads = 1;
	f->data = d;
	f->options = lzw_options;
	f->open = lzw_open;
	f->close = lzw_close;
	f->free = la_write_window_free;
	f->code = ARCHIVE_FILTER_LZIP;
	f->name = "lzip";
	return ARCHIVE_OK;
}
