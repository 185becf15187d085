/*
 * la_write_bzip2.c -- the bzip2 WRITE filter on the device data plane (la_gpu_bzip2_compress), registered on the
 * write core of la_write_filters.c.
 *
 * Registration and options follow libarchive/archive_write_add_filter_bzip2.c:79-145: name "bzip2", code
 * ARCHIVE_FILTER_BZIP2, default level 9; "compression-level" takes exactly one character '0'..'9', 0 meaning 1; any
 * other option or value returns ARCHIVE_WARN, which archive_write_set_filter_option turns into ARCHIVE_FAILED
 * "Undefined option".  Adding the filter always returns ARCHIVE_OK.
 *
 * What differs from the reference by design:
 *   - write() only gathers input into the write window of la_write_private.h; a full window (LA_GPU_WRITE_WINDOW_MIB,
 *     default 64, rounded down to whole blocks) goes to la_gpu_bzip2_compress() in ONE call.  The output is still ONE
 *     stream per archive: the device keeps the stream's pending bits and combined CRC (la_bz2c_state) between the
 *     calls, the first window writes the header, the flush that close() makes writes the trailer;
 *   - blocks are cut at a fixed input size (la_gpu_bzip2_compress_block_bytes) instead of filled to libbz2's limit, and
 *     the tables are fitted differently, so the bytes are not libbz2's; every bzip2 reader returns the input;
 *   - libbz2's workFactor has no counterpart: the device sort's round count does not depend on the data;
 *   - there is no external-program ("bzip2" command) path.
 */
#include <errno.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "la_read_private.h"
#include "la_write_private.h"
#include "../../include/la_gpu.h"
#include "../../include/la_host.h"

struct bz2w_private {
	struct la_write_window w;	/* first */
	int compression_level;
	int closing;			/* the flush in progress is close()'s: it carries LA_BZ2C_LAST */
	void *d_state;			/* la_bz2c_state, device-resident */
};

static int bz2w_options(struct archive_write_filter *f, const char *key, const char *value)
{
	struct bz2w_private *d = f->data;
	if (strcmp(key, "compression-level") == 0) {
		if (value == NULL || !(value[0] >= '0' && value[0] <= '9') || value[1] != '\0')
			return ARCHIVE_WARN;
		d->compression_level = value[0] - '0';
		if (d->compression_level < 1)	/* archive_write_add_filter_bzip2.c:131-135 */
			d->compression_level = 1;
		return ARCHIVE_OK;
	}
	return ARCHIVE_WARN;
}

static uint64_t bz2w_bound(struct archive_write_filter *f, uint64_t n)
{
	const struct bz2w_private *d = f->data;
	return la_gpu_bzip2_compress_bound(n, (uint32_t)d->compression_level);
}

static int bz2w_compress(struct archive_write_filter *f, const struct la_write_window *w)
{
	const struct bz2w_private *d = f->data;
	la_bz2c_batch bt;
	memset(&bt, 0, sizeof(bt));
	bt.d_src = w->len ? w->d_in : NULL; bt.src_bytes = w->len;
	bt.level = (uint32_t)d->compression_level;
	bt.flags = (w->wrote_anything ? 0u : LA_BZ2C_FIRST) | (d->closing ? LA_BZ2C_LAST : 0u);
	bt.d_state = d->d_state;
	bt.d_out = w->d_out; bt.out_cap = w->out_cap; bt.d_out_bytes = w->d_len;
	return la_gpu_bzip2_compress(w->gpu, &bt);
}

static int bz2w_open(struct archive_write_filter *f)
{
	struct bz2w_private *d = f->data;
	const size_t unit = la_gpu_bzip2_compress_block_bytes((uint32_t)d->compression_level);
	int r = la_write_window_open(f, unit);	/* whole blocks */
	if (r != ARCHIVE_OK)
		return r;
	/* one compress call takes at most LA_BZ2C_MAX_SRC_BYTES: a larger LA_GPU_WRITE_WINDOW_MIB gives windows of that
	 * many whole blocks (the pinned buffer is the size that was asked for; its tail stays unused) */
	if (d->w.cap > LA_BZ2C_MAX_SRC_BYTES)
		d->w.cap = (size_t)(LA_BZ2C_MAX_SRC_BYTES / unit * unit);
	if (la_gpu_malloc(d->w.gpu, &d->d_state, sizeof(la_bz2c_state)) != LA_OK)
		return la_write_window_fail(f, "device allocation");
	return ARCHIVE_OK;
}

static int bz2w_close(struct archive_write_filter *f)
{
	struct bz2w_private *d = f->data;
	if (d->w.gpu == NULL)
		return ARCHIVE_OK;
	/* always one more call: it carries LAST, with the rest of the data, with nothing when the data ended on a window
	 * boundary (the trailer alone behind the pending bits), or as the 14-byte empty stream when nothing was written */
	d->closing = 1;
	return la_write_window_flush(f, 1);
}

static int bz2w_free(struct archive_write_filter *f)
{
	struct bz2w_private *d = f->data;
	if (d && d->w.gpu && d->d_state) {
		la_gpu_sync(d->w.gpu);
		la_gpu_free(d->w.gpu, d->d_state);
		d->d_state = NULL;
	}
	return la_write_window_free(f);
}

int archive_write_add_filter_bzip2(struct archive *_a)
{
	struct archive_write_filter *f = __archive_write_allocate_filter(_a);
	struct bz2w_private *d = calloc(1, sizeof(*d));
	if (f == NULL || d == NULL) {
		free(d);
		archive_set_error(_a, ENOMEM, "Out of memory");
		return ARCHIVE_FATAL;
	}
	d->w.name = "bzip2";
	d->w.bound = bz2w_bound;
	d->w.compress = bz2w_compress;
	d->compression_level = 9;	/* archive_write_add_filter_bzip2.c:94 */
	f->data = d;
	f->options = bz2w_options;
	f->open = bz2w_open;
	f->close = bz2w_close;
	f->free = bz2w_free;
	f->code = ARCHIVE_FILTER_BZIP2;
	f->name = "bzip2";
	return ARCHIVE_OK;
}
