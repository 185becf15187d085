/*
 * la_write_filters.c -- the lz4 and gzip WRITE filters on the device data plane, with the
 * small slice of libarchive's write side they need to stand alone.
 *
 * The filter keeps the reference's write-filter vtable and registration
 * (libarchive/archive_write_private.h:46-63 `struct archive_write_filter` {options, open, write,
 * flush, close, free, data, name, code}; archive_write_add_filter_lz4.c:94-149: name "lz4", code
 * ARCHIVE_FILTER_LZ4, defaults stream-checksum on / block-checksum off / block-size 7, options
 * :154-201) so that inside libarchive (-DLA_IN_LIBARCHIVE is not wired for this file yet) it is
 * the same kind of source-level swap as the read filters.  What differs by design:
 *   - write() only gathers input into a pinned window; a full window (LA_GPU_WRITE_WINDOW_MIB,
 *     default 64) goes to la_gpu_lz4_compress() in ONE call and the frames come back in one copy;
 *   - the stream is a sequence of frames of sixteen 64 KiB blocks, not one frame: a frame's content
 *     checksum is one serial XXH32 chain, sixteen-block frames keep thousands of chains in flight
 *     on the device (every lz4 reader, the reference's included, reads concatenated frames:
 *     archive_read_support_filter_lz4.c:328-364).  "block-size" 4..7 is accepted, blocks are 64 KiB;
 *   - "block-dependence" is refused (the device compresses independent blocks);
 *     "compression-level" 1..9 is accepted and means the one level the device has.
 *
 * The gzip filter (archive_write_add_filter_gzip.c:98-137 registration: name "gzip", code ARCHIVE_FILTER_GZIP,
 * options "compression-level" and "timestamp" :142-167) works the same way on la_gpu_gzip_compress(): the stream
 * is a sequence of members of at most 48 KiB of input each, every one with the BGZF-compatible size subfield, so
 * that the read side indexes them without searching (every gzip reader reads concatenated members:
 * archive_read_support_filter_gzip.c:340-365).  "compression-level" 0..9 selects what the device has: 0 stored
 * blocks (what zlib's level 0 writes), 1 fixed Huffman codes (the fast level), 2..9 and the default 6 the smallest
 * of a dynamic-Huffman, a fixed-Huffman and a stored block per chunk (LA_GZC_* in la_gpu.h).  The matcher is the
 * same at every level.
 *   "single-member" (boolean, off by default; not an option of the reference, whose only shape this is) writes what
 * archive_write_add_filter_gzip.c:190-345 writes: ONE member for the whole stream.  open sends the reference's
 * 10-byte header (:201-238); every window goes through la_gpu_gzip_compress() with LA_GZC_FRAME_STREAM, which returns
 * a byte-aligned piece of one raw-deflate stream, its chunks still compressed in parallel, while
 * la_gpu_crc32_many() continues the running CRC32 over the window; close ends the stream with the empty fixed block
 * 03 00 and writes the trailer.  For this repository's read filter such a member is one serial unit, which is why
 * many members stay the default.
 *
 * The write core below is the minimum the filters and formats need outside libarchive: archive_write_new,
 * _add_filter_lz4, _set_format_raw (one entry, data passed through: archive_write_set_format_raw.c),
 * _set_filter_option, _set_format_option, _open_memory / _open_fd, _header, _data, _finish_entry, _close, _free.  A
 * format is the reference's set of hooks on the handle (la_write_private.h); the raw format is one here, the ZIP
 * format another in la_write_zip.c, which this file does not know.  Next to it, the write window that the lz4, gzip
 * and zstd filters and the ZIP format share: each adds its output bound and its one compress call.
 */
#include <errno.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <unistd.h>

#include "la_read_private.h"
#include "la_write_private.h"
#include "../../include/la_gpu.h"
#include "../../include/la_host.h"

/* ------------------------------------------------------------------ minimal write core */

static int client_write(struct archive_write_filter *f, const void *buf, size_t len)
{
	struct archive_write *a = (struct archive_write *)f->archive;
	if (a->mem) {
		if (*a->mem_used + len > a->mem_cap) {
			archive_set_error(&a->archive, ENOMEM, "Buffer exhausted");	/* archive_write_open_memory.c:81-85 */
			return ARCHIVE_FATAL;
		}
		memcpy(a->mem + *a->mem_used, buf, len);
		*a->mem_used += len;
		return ARCHIVE_OK;
	}
	const uint8_t *p = buf;
	while (len) {
		ssize_t w = write(a->fd, p, len);
		if (w <= 0) {
			archive_set_error(&a->archive, errno, "Write error");
			return ARCHIVE_FATAL;
		}
		p += w; len -= (size_t)w;
	}
	return ARCHIVE_OK;
}

struct archive_write_filter *__archive_write_allocate_filter(struct archive *_a)
{
	struct archive_write *a = (struct archive_write *)_a;
	struct archive_write_filter *f = calloc(1, sizeof(*f));
	if (!f)
		return NULL;
	f->archive = _a;
	f->state = 1;	/* ARCHIVE_WRITE_FILTER_STATE_NEW */
	if (a->filter_first == NULL)
		a->filter_first = f;
	else
		a->filter_last->next_filter = f;
	a->filter_last = f;
	return f;
}

int __archive_write_filter(struct archive_write_filter *f, const void *buf, size_t len)
{
	if (len == 0)
		return ARCHIVE_OK;
	if (f == NULL || f->write == NULL)
		return ARCHIVE_FATAL;
	int r = f->write(f, buf, len);
	f->bytes_written += (int64_t)len;
	return r;
}

struct archive *archive_write_new(void)
{
	struct archive_write *a = calloc(1, sizeof(*a));
	if (a) {
		a->archive.state = LA_STATE_NEW;
		a->fd = -1;
	}
	return (struct archive *)a;
}

int __archive_write_output(struct archive_write *a, const void *buf, size_t len)
{
	return __archive_write_filter(a->filter_first, buf, len);
}

/* the raw format (archive_write_set_format_raw.c): one entry, its data passed through; its only state is the
 * number of headers seen */
static int raw_write_header(struct archive_write *a, struct archive_entry *entry)
{
	int *entries = a->format_data;
	(void)entry;
	if ((*entries)++ > 0) {
		archive_set_error(&a->archive, ERANGE, "Raw format only supports one entry per archive");	/* archive_write_set_format_raw.c:80-84 */
		return ARCHIVE_FATAL;
	}
	return ARCHIVE_OK;
}

static ssize_t raw_write_data(struct archive_write *a, const void *buff, size_t s)
{
	int r = __archive_write_output(a, buff, s);
	return r == ARCHIVE_OK ? (ssize_t)s : r;
}

static int raw_free(struct archive_write *a)
{
	free(a->format_data);
	a->format_data = NULL;
	return ARCHIVE_OK;
}

int archive_write_set_format_raw(struct archive *_a)
{
	struct archive_write *a = (struct archive_write *)_a;
	if (a->format_free != NULL)	/* another format was registered (archive_write_set_format_raw.c:54-56) */
		a->format_free(a);
	a->format_data = calloc(1, sizeof(int));
	if (a->format_data == NULL) {
		archive_set_error(_a, ENOMEM, "Can't allocate raw data");
		return ARCHIVE_FATAL;
	}
	a->format_name = "raw";
	a->format_init = NULL;
	a->format_options = NULL;
	a->format_finish_entry = NULL;
	a->format_write_header = raw_write_header;
	a->format_write_data = raw_write_data;
	a->format_close = NULL;
	a->format_free = raw_free;
	_a->archive_format = ARCHIVE_FORMAT_RAW;
	_a->archive_format_name = "raw";
	return ARCHIVE_OK;
}

/* archive_write_set_options.c:38-45, :73-88 with _archive_set_option (archive_options.c:38-72): one option for the
 * format; `m` names it or is NULL */
int archive_write_set_format_option(struct archive *_a, const char *m, const char *o, const char *v)
{
	struct archive_write *a = (struct archive_write *)_a;
	const char *mp = (m != NULL && m[0] != '\0') ? m : NULL;
	const char *op = (o != NULL && o[0] != '\0') ? o : NULL;
	const char *vp = (v != NULL && v[0] != '\0') ? v : NULL;
	int r;
	if (op == NULL && vp == NULL)
		return ARCHIVE_OK;
	if (op == NULL) {
		archive_set_error(_a, ARCHIVE_ERRNO_MISC, "Empty option");
		return ARCHIVE_FAILED;
	}
	if (a->format_name == NULL)
		r = mp == NULL ? ARCHIVE_FAILED : ARCHIVE_WARN - 1;
	else if (mp != NULL && strcmp(mp, a->format_name) != 0)
		r = ARCHIVE_WARN - 1;
	else if (a->format_options == NULL)
		r = ARCHIVE_WARN;
	else
		r = a->format_options(a, op, vp);
	if (r == ARCHIVE_WARN - 1) {
		archive_set_error(_a, ARCHIVE_ERRNO_MISC, "Unknown module name: `%s'", mp);
		return ARCHIVE_FAILED;
	}
	if (r == ARCHIVE_WARN) {
		archive_set_error(_a, ARCHIVE_ERRNO_MISC, "Undefined option: `%s%s%s%s%s%s'", vp ? "" : "!", mp ? mp : "", mp ? ":" : "",
		    op, vp ? "=" : "", vp ? vp : "");
		return ARCHIVE_FAILED;
	}
	return r;
}

int archive_write_set_filter_option(struct archive *_a, const char *m, const char *o, const char *v)
{
	struct archive_write *a = (struct archive_write *)_a;
	int handled = 0;
	for (struct archive_write_filter *f = a->filter_first; f; f = f->next_filter) {
		if (f->options == NULL || (m != NULL && (f->name == NULL || strcmp(f->name, m) != 0)))
			continue;
		int r = f->options(f, o, v);
		if (r == ARCHIVE_FATAL || r == ARCHIVE_FAILED)
			return r;
		if (r == ARCHIVE_OK)
			handled = 1;
	}
	if (!handled) {
		archive_set_error(_a, ARCHIVE_ERRNO_MISC, "Undefined option: `%s%s%s'", m ? m : "", m ? ":" : "", o);
		return ARCHIVE_FAILED;
	}
	return ARCHIVE_OK;
}

static int write_open_common(struct archive_write *a)
{
	/* the client sink is the last "filter" of the chain */
	struct archive_write_filter *sink = __archive_write_allocate_filter(&a->archive);
	if (!sink) {
		archive_set_error(&a->archive, ENOMEM, "Out of memory");
		return ARCHIVE_FATAL;
	}
	sink->write = client_write;
	sink->name = "client";
	for (struct archive_write_filter *f = a->filter_first; f; f = f->next_filter) {
		if (f->open) {
			int r = f->open(f);
			if (r != ARCHIVE_OK)
				return r;
		}
		f->state = 2;	/* OPEN */
	}
	a->opened = 1;
	a->archive.state = LA_STATE_HEADER;
	return a->format_init ? a->format_init(a) : ARCHIVE_OK;	/* archive_write.c archive_write_client_open's last step */
}

int archive_write_open_memory(struct archive *_a, void *buff, size_t size, size_t *used)
{
	struct archive_write *a = (struct archive_write *)_a;
	a->mem = buff; a->mem_cap = size; a->mem_used = used;
	*used = 0;
	return write_open_common(a);
}

int archive_write_open_fd(struct archive *_a, int fd)
{
	struct archive_write *a = (struct archive_write *)_a;
	a->fd = fd;
	return write_open_common(a);
}

int archive_write_finish_entry(struct archive *_a)	/* archive_write.c:798-812 */
{
	struct archive_write *a = (struct archive_write *)_a;
	int ret = ARCHIVE_OK;
	if (_a->state == LA_STATE_DATA && a->format_finish_entry != NULL)
		ret = a->format_finish_entry(a);
	if (_a->state == LA_STATE_DATA)
		_a->state = LA_STATE_HEADER;
	return ret;
}

int archive_write_header(struct archive *_a, struct archive_entry *entry)	/* archive_write.c:734-796 */
{
	struct archive_write *a = (struct archive_write *)_a;
	if (!a->opened || a->format_write_header == NULL) {
		archive_set_error(_a, ARCHIVE_ERRNO_MISC, "No format defined (this slice writes the raw format)");
		return ARCHIVE_FATAL;
	}
	/* "retry" and "fatal" get returned immediately (:751-758) */
	int ret = archive_write_finish_entry(_a);
	if (ret < ARCHIVE_OK && ret != ARCHIVE_WARN)
		return ret;
	const int r2 = a->format_write_header(a, entry);
	if (r2 == ARCHIVE_FAILED || r2 == ARCHIVE_FATAL)
		return r2;
	_a->state = LA_STATE_DATA;
	return r2 < ret ? r2 : ret;
}

ssize_t archive_write_data(struct archive *_a, const void *buff, size_t s)
{
	struct archive_write *a = (struct archive_write *)_a;
	if (!a->opened || _a->state != LA_STATE_DATA || a->format_write_data == NULL) {
		archive_set_error(_a, ARCHIVE_ERRNO_MISC, "archive_write_data before archive_write_header");
		return ARCHIVE_FATAL;
	}
	return a->format_write_data(a, buff, s);
}

int archive_write_close(struct archive *_a)
{
	struct archive_write *a = (struct archive_write *)_a;
	int rc = ARCHIVE_OK;
	if (a->closed || !a->opened)
		return ARCHIVE_OK;
	/* the last entry, then the archive, then the filters (archive_write.c:631-647) */
	if (_a->state == LA_STATE_DATA && a->format_finish_entry != NULL)
		rc = a->format_finish_entry(a);
	if (a->format_close != NULL) {
		int r = a->format_close(a);
		if (r < rc)
			rc = r;
	}
	for (struct archive_write_filter *f = a->filter_first; f; f = f->next_filter) {
		if (f->close) {
			int r = f->close(f);
			if (r < rc)
				rc = r;
		}
		f->state = 4;	/* CLOSED */
	}
	a->closed = 1;
	_a->state = LA_STATE_CLOSED;
	return rc;
}

int archive_write_free(struct archive *_a)
{
	struct archive_write *a = (struct archive_write *)_a;
	if (!a)
		return ARCHIVE_OK;
	int rc = archive_write_close(_a);
	if (a->format_free != NULL)
		a->format_free(a);
	struct archive_write_filter *f = a->filter_first;
	while (f) {
		struct archive_write_filter *n = f->next_filter;
		if (f->free)
			f->free(f);
		free(f);
		f = n;
	}
	free(a);
	return rc;
}

/* ------------------------------------------------------------------ the write window */

int la_write_window_fail(struct archive_write_filter *f, const char *what)
{
	const struct la_write_window *w = f->data;
	archive_set_error(f->archive, ARCHIVE_ERRNO_MISC, "%s GPU data plane: %s failed: %s", w->name, what,
	    w->gpu ? la_gpu_last_error(w->gpu) : "no device");
	return ARCHIVE_FATAL;
}

int la_write_window_flush(struct archive_write_filter *f, int force_empty)
{
	struct la_write_window *w = f->data;
	if (w->len == 0 && !force_empty)
		return ARCHIVE_OK;
	/* buffers for a full window, at first use */
	if (w->d_in == NULL && w->len && la_gpu_malloc(w->gpu, &w->d_in, w->cap) != LA_OK)
		return la_write_window_fail(f, "device allocation");
	if (w->out == NULL) {
		const uint64_t cap = w->bound(f, w->cap);
		void *hp = NULL;
		if ((w->d_out == NULL && la_gpu_malloc(w->gpu, &w->d_out, cap) != LA_OK) || la_gpu_malloc_host(w->gpu, &hp, cap) != LA_OK)
			return la_write_window_fail(f, "output allocation");
		w->out = hp; w->out_cap = cap;
	}
	if (w->d_len == NULL && la_gpu_malloc(w->gpu, &w->d_len, 64) != LA_OK)
		return la_write_window_fail(f, "device allocation");
	uint64_t total = 0;
	if ((w->len && la_gpu_memcpy_h2d(w->gpu, w->d_in, w->win, w->len) != LA_OK) ||
	    w->compress(f, w) != LA_OK ||
	    la_gpu_memcpy_d2h(w->gpu, &total, w->d_len, sizeof(total)) != LA_OK ||
	    la_gpu_sync(w->gpu) != LA_OK)
		return la_write_window_fail(f, "compress");
	if (total > w->out_cap)
		return la_write_window_fail(f, "compress (output bound)");
	if (la_gpu_memcpy_d2h(w->gpu, w->out, w->d_out, total) != LA_OK || la_gpu_sync(w->gpu) != LA_OK)
		return la_write_window_fail(f, "device to host copy");
	w->len = 0;
	w->wrote_anything = 1;
	if (w->patch) {
		int r = w->patch(f, w, total);
		if (r != ARCHIVE_OK)
			return r;
	}
	return __archive_write_filter(f->next_filter, w->out, (size_t)total);
}

static int window_write(struct archive_write_filter *f, const void *buff, size_t length)
{
	struct la_write_window *w = f->data;
	const uint8_t *p = buff;
	while (length) {
		size_t n = w->cap - w->len;
		if (n > length) n = length;
		memcpy(w->win + w->len, p, n);
		w->len += n; p += n; length -= n;
		if (w->len == w->cap) {
			int r = la_write_window_flush(f, 0);
			if (r != ARCHIVE_OK)
				return r;
		}
	}
	return ARCHIVE_OK;
}

int la_write_window_open(struct archive_write_filter *f, size_t unit)
{
	struct la_write_window *w = f->data;
	const char *wm = getenv("LA_GPU_WRITE_WINDOW_MIB");
	if (la_gpu_open(la_env_device(), &w->gpu) != LA_OK) {
		archive_set_error(f->archive, ARCHIVE_ERRNO_MISC,
		    "Can't initialize %s GPU data plane (no usable gfx950 device); no CPU fallback is built", w->name);
		return ARCHIVE_FATAL;
	}
	w->cap = ((size_t)(wm && atoi(wm) > 0 ? atoi(wm) : 64) << 20) / unit * unit;
	if (w->cap == 0)
		w->cap = unit;
	void *hp = NULL;
	if (la_gpu_malloc_host(w->gpu, &hp, w->cap) != LA_OK)
		return la_write_window_fail(f, "pinned window allocation");
	w->win = hp;
	f->write = window_write;
	return ARCHIVE_OK;
}

int la_write_window_free(struct archive_write_filter *f)
{
	struct la_write_window *w = f->data;
	if (w) {
		if (w->gpu) {
			la_gpu_sync(w->gpu);
			if (w->win) la_gpu_free_host(w->gpu, w->win);
			if (w->out) la_gpu_free_host(w->gpu, w->out);
			if (w->d_in) la_gpu_free(w->gpu, w->d_in);
			if (w->d_out) la_gpu_free(w->gpu, w->d_out);
			if (w->d_len) la_gpu_free(w->gpu, w->d_len);
			la_gpu_close(w->gpu);
		}
		free(w);
	}
	f->data = NULL;
	return ARCHIVE_OK;
}

/* ------------------------------------------------------------------ the lz4 write filter */

#define LZ4W_BLOCK 65536u
#define LZ4W_BPF   16u
#define GZW_CHUNK  49152u

struct lz4w_private {	/* archive_write_add_filter_lz4.c:49-68 */
	struct la_write_window w;	/* first */
	int compression_level;
	unsigned block_independence:1, block_checksum:1, stream_checksum:1;
	unsigned block_maximum_size:3;
};

static int lz4w_options(struct archive_write_filter *f, const char *key, const char *value)
{
	struct lz4w_private *d = f->data;
	if (strcmp(key, "compression-level") == 0) {
		if (value == NULL || !(value[0] >= '1' && value[0] <= '9') || value[1] != '\0')
			return ARCHIVE_WARN;
		d->compression_level = value[0] - '0';	/* (the device has one level) */
		return ARCHIVE_OK;
	}
	if (strcmp(key, "stream-checksum") == 0) { d->stream_checksum = value != NULL; return ARCHIVE_OK; }
	if (strcmp(key, "block-checksum") == 0) { d->block_checksum = value != NULL; return ARCHIVE_OK; }
	if (strcmp(key, "block-size") == 0) {
		if (value == NULL || !(value[0] >= '4' && value[0] <= '7') || value[1] != '\0')
			return ARCHIVE_WARN;
		d->block_maximum_size = (unsigned)(value[0] - '0');	/* (accepted; blocks are 64 KiB) */
		return ARCHIVE_OK;
	}
	if (strcmp(key, "block-dependence") == 0) {
		if (value != NULL) {
			archive_set_error(f->archive, ARCHIVE_ERRNO_MISC, "block dependence is not supported by the GPU lz4 writer");
			return ARCHIVE_FAILED;
		}
		return ARCHIVE_OK;
	}
	return ARCHIVE_WARN;
}

static uint64_t lz4w_bound(struct archive_write_filter *f, uint64_t n) { (void)f; return la_gpu_lz4_compress_bound(n, LZ4W_BLOCK, LZ4W_BPF); }

static int lz4w_compress(struct archive_write_filter *f, const struct la_write_window *w)
{
	const struct lz4w_private *d = f->data;
	la_lz4c_batch bt;
	memset(&bt, 0, sizeof(bt));
	bt.d_src = w->d_in; bt.src_bytes = w->len;
	bt.block_size = LZ4W_BLOCK; bt.blocks_per_frame = LZ4W_BPF;
	bt.flags = (d->block_checksum ? LA_LZ4C_BLOCK_SUM : 0) | (d->stream_checksum ? LA_LZ4C_CONTENT_SUM : 0);
	bt.d_out = w->d_out; bt.out_cap = w->out_cap; bt.d_out_bytes = w->d_len;
	return la_gpu_lz4_compress(w->gpu, &bt);
}

static int lz4w_open(struct archive_write_filter *f) { return la_write_window_open(f, 1); }	/* (64 MiB: whole 1 MiB frames) */

static int lz4w_close(struct archive_write_filter *f)
{
	struct lz4w_private *d = f->data;
	if (d->w.gpu == NULL)
		return ARCHIVE_OK;
	int r = la_write_window_flush(f, 0);
	if (r == ARCHIVE_OK && !d->w.wrote_anything) {
		/* nothing was written: one empty frame (header, EndMark, checksum of nothing), as the
		 * reference's close does (archive_write_add_filter_lz4.c:300-330) */
		uint8_t h[15];
		const uint8_t flg = (uint8_t)(0x60 | (d->block_checksum ? 0x10 : 0) | (d->stream_checksum ? 0x04 : 0));
		h[0] = 0x04; h[1] = 0x22; h[2] = 0x4D; h[3] = 0x18; h[4] = flg; h[5] = 0x40;
		h[6] = (uint8_t)(la_archive_xxhash.XXH32(h + 4, 2, 0) >> 8);
		memset(h + 7, 0, 4);
		size_t n = 11;
		if (d->stream_checksum) {
			const uint32_t c = la_archive_xxhash.XXH32("", 0, 0);
			h[11] = (uint8_t)c; h[12] = (uint8_t)(c >> 8); h[13] = (uint8_t)(c >> 16); h[14] = (uint8_t)(c >> 24);
			n = 15;
		}
		r = __archive_write_filter(f->next_filter, h, n);
	}
	return r;
}

int archive_write_add_filter_lz4(struct archive *_a)
{
	struct archive_write_filter *f = __archive_write_allocate_filter(_a);
	struct lz4w_private *d = calloc(1, sizeof(*d));
	if (f == NULL || d == NULL) {
		free(d);
		archive_set_error(_a, ENOMEM, "Out of memory");
		return ARCHIVE_FATAL;
	}
	d->w.name = "lz4";
	d->w.bound = lz4w_bound;
	d->w.compress = lz4w_compress;
	d->compression_level = 1;
	d->block_independence = 1;
	d->block_checksum = 0;
	d->stream_checksum = 1;
	d->block_maximum_size = 7;
	f->data = d;
	f->options = lz4w_options;
	f->open = lz4w_open;
	f->close = lz4w_close;
	f->free = la_write_window_free;
	f->code = ARCHIVE_FILTER_LZ4;
	f->name = "lz4";
	return ARCHIVE_OK;
}

/* ------------------------------------------------------------------ the gzip write filter */

struct gzw_private {	/* archive_write_add_filter_gzip.c:58-60 */
	struct la_write_window w;	/* first */
	int compression_level;
	int timestamp;		/* > 0 writes time(NULL) into the member headers (archive_write_add_filter_gzip.c:213-220) */
	uint32_t mtime;
	int single_member;	/* one member for the whole stream, as the reference writes */
	uint32_t crc;		/* single member: CRC32 and length of the input so far */
	uint64_t total_in;
};

static int gzw_options(struct archive_write_filter *f, const char *key, const char *value)
{
	struct gzw_private *d = f->data;
	if (strcmp(key, "compression-level") == 0) {	/* archive_write_add_filter_gzip.c:147-153 */
		if (value == NULL || !(value[0] >= '0' && value[0] <= '9') || value[1] != '\0')
			return ARCHIVE_WARN;
		d->compression_level = value[0] - '0';	/* gzw_compress turns it into a LA_GZC_* mode */
		return ARCHIVE_OK;
	}
	if (strcmp(key, "timestamp") == 0) {		/* :154-157 */
		d->timestamp = (value == NULL) ? -1 : 1;
		return ARCHIVE_OK;
	}
	if (strcmp(key, "single-member") == 0) {
		d->single_member = value != NULL;
		return ARCHIVE_OK;
	}
	return ARCHIVE_WARN;
}

static uint64_t gzw_bound(struct archive_write_filter *f, uint64_t n) { (void)f; return la_gpu_gzip_compress_bound(n, GZW_CHUNK); }

static int gzw_compress(struct archive_write_filter *f, const struct la_write_window *w)
{
	const struct gzw_private *d = f->data;
	la_gzc_batch bt;
	memset(&bt, 0, sizeof(bt));
	bt.d_src = w->d_in; bt.src_bytes = w->len; bt.chunk_bytes = GZW_CHUNK; bt.mtime = d->mtime;
	bt.d_out = w->d_out; bt.out_cap = w->out_cap; bt.d_out_bytes = w->d_len;
	bt.options = d->compression_level == 0 ? LA_GZC_STORED : (d->compression_level == 1 ? LA_GZC_FIXED : LA_GZC_DYNAMIC);
	bt.framing = d->single_member ? LA_GZC_FRAME_STREAM : LA_GZC_FRAME_MEMBERS;
	return la_gpu_gzip_compress(w->gpu, &bt);
}

/* single member: the window's piece of the deflate stream, and the member's CRC32 continued over the window by one
 * seeded job per call (a job's length is 32 bits: a window of 4 GiB or more takes several).  The job and its result
 * live behind the byte count in d_len (64 bytes): job at 16, result at 32. */
static int gzw_compress_stream(struct archive_write_filter *f, const struct la_write_window *w)
{
	struct gzw_private *d = f->data;
	int rc = gzw_compress(f, w);
	uint8_t *t = w->d_len;
	for (uint64_t at = 0; rc == LA_OK && at < w->len; ) {
		const uint64_t left = w->len - at;
		const la_hash_job job = { at, (uint32_t)(left < 0x80000000u ? left : 0x80000000u), d->crc };
		if ((rc = la_gpu_memcpy_h2d(w->gpu, t + 16, &job, sizeof(job))) != LA_OK ||
		    (rc = la_gpu_crc32_many(w->gpu, w->d_in, (const la_hash_job *)(t + 16), 1, (uint32_t *)(t + 32))) != LA_OK ||
		    (rc = la_gpu_memcpy_d2h(w->gpu, &d->crc, t + 32, sizeof(d->crc))) != LA_OK ||
		    (rc = la_gpu_sync(w->gpu)) != LA_OK)	/* `job` leaves scope; the next one is seeded with d->crc */
			break;
		at += job.len;
	}
	if (rc == LA_OK)
		d->total_in += w->len;
	return rc;
}

static int gzw_open(struct archive_write_filter *f)
{
	struct gzw_private *d = f->data;
	int r = la_write_window_open(f, 1);	/* (not whole 48 KiB chunks: rounding would move member boundaries) */
	if (r == ARCHIVE_OK && d->timestamp >= 0)
		d->mtime = (uint32_t)time(NULL);
	if (r == ARCHIVE_OK && d->single_member) {
		/* the reference's header (archive_write_add_filter_gzip.c:201-238): no flags, XFL 2 at level 9 and 4 at
		 * level 1, OS 3 (Unix) */
		const uint8_t xfl = d->compression_level == 9 ? 2 : (d->compression_level == 1 ? 4 : 0);
		const uint8_t h[10] = { 0x1f, 0x8b, 8, 0, (uint8_t)d->mtime, (uint8_t)(d->mtime >> 8), (uint8_t)(d->mtime >> 16),
		    (uint8_t)(d->mtime >> 24), xfl, 3 };
		d->w.compress = gzw_compress_stream;
		d->crc = 0; d->total_in = 0;
		r = __archive_write_filter(f->next_filter, h, sizeof(h));
	}
	return r;
}

static int gzw_close(struct archive_write_filter *f)
{
	struct gzw_private *d = f->data;
	if (d->w.gpu == NULL)
		return ARCHIVE_OK;
	int r = la_write_window_flush(f, 0);
	if (d->single_member) {
		/* the stream's end and the member's trailer (archive_write_add_filter_gzip.c:309-331): an empty final
		 * fixed block, CRC32 and ISIZE of all the input */
		const uint32_t n = (uint32_t)d->total_in;
		const uint8_t t[10] = { 0x03, 0x00, (uint8_t)d->crc, (uint8_t)(d->crc >> 8), (uint8_t)(d->crc >> 16), (uint8_t)(d->crc >> 24),
		    (uint8_t)n, (uint8_t)(n >> 8), (uint8_t)(n >> 16), (uint8_t)(n >> 24) };
		return r == ARCHIVE_OK ? __archive_write_filter(f->next_filter, t, sizeof(t)) : r;
	}
	if (r == ARCHIVE_OK && !d->w.wrote_anything) {
		/* nothing was written: one member with an empty deflate stream, as zlib's Z_FINISH on no input gives
		 * the reference (header, 03 00, crc 0, isize 0) */
		const uint8_t m[20] = { 0x1f, 0x8b, 8, 0, (uint8_t)d->mtime, (uint8_t)(d->mtime >> 8), (uint8_t)(d->mtime >> 16),
		    (uint8_t)(d->mtime >> 24), 0, 3, 0x03, 0x00, 0, 0, 0, 0, 0, 0, 0, 0 };
		r = __archive_write_filter(f->next_filter, m, sizeof(m));
	}
	return r;
}

int archive_write_add_filter_gzip(struct archive *_a)
{
	struct archive_write_filter *f = __archive_write_allocate_filter(_a);
	struct gzw_private *d = calloc(1, sizeof(*d));
	if (f == NULL || d == NULL) {
		free(d);
		archive_set_error(_a, ENOMEM, "Out of memory");
		return ARCHIVE_FATAL;
	}
	d->w.name = "gzip";
	d->w.bound = gzw_bound;
	d->w.compress = gzw_compress;
	d->compression_level = 6;	/* Z_DEFAULT_COMPRESSION in the reference: dynamic Huffman here */
	f->data = d;
	f->options = gzw_options;
	f->open = gzw_open;
	f->close = gzw_close;
	f->free = la_write_window_free;
	f->code = ARCHIVE_FILTER_GZIP;
	f->name = "gzip";
	return ARCHIVE_OK;
}
