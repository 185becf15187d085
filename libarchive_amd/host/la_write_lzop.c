/*
 * la_write_lzop.c -- the lzop WRITE filter on the device data plane (la_gpu_lzop_compress), registered on the write core
 * of la_write_filters.c.
 *
 * Registration and options follow libarchive/archive_write_add_filter_lzop.c:135-223: name "lzop", code
 * ARCHIVE_FILTER_LZOP, default level 5; "compression-level" takes exactly one character '1'..'9' ('0' is refused, :213).
 * Any other option or value returns ARCHIVE_WARN, which archive_write_set_filter_option turns into ARCHIVE_FAILED
 * "Undefined option".
 *
 * The stream: ONE part per archive, as the reference writes it -- the 38-byte header of its template (:103-132), the
 * blocks, then four zero bytes.  Header: magic; version 0x1030; library and needed versions 0x0940, the template's (the
 * reference overwrites the library version with lzo_version(); no liblzo2 stands behind this writer, so the template's
 * bytes stay); method and level bytes from the reference's table (:231-243): level 1 -> 2 / 1, levels 2..6 -> 1 / 5,
 * levels 7, 8, 9 -> 3 / 7, 8, 9; flags 0x0300000d; mode 0100644; time(NULL) in the low mtime word; no name; Adler-32 over
 * header bytes [9, 34).  Every block: BE32 usize, BE32 csize, BE32 adler32(uncompressed), then the LZO1X stream, or the
 * input itself with csize = usize where the stream is not shorter (:364-381).
 *
 * What differs from the reference by design:
 *   - write() only gathers input into the write window of la_write_private.h; a full window (LA_GPU_WRITE_WINDOW_MIB,
 *     default 64, whole blocks) goes to la_gpu_lzop_compress() in ONE call, which returns complete blocks back to back;
 *   - blocks are LA_LZOPC_BLOCK_BYTES (64 KiB) of input where the reference writes 256 KiB: any size up to 64 MiB is
 *     valid lzop, and 64 KiB is the size the device codes with 16-bit positions and this project's reader is fastest on;
 *   - there is ONE coder: levels 1..9 write the same block bytes, only the header's method and level bytes differ; the
 *     bytes are not liblzo2's;
 *   - the header travels with the first window: that call leaves a gap of 38 bytes in front of its blocks and the patch
 *     hook writes the header into it, so open() writes nothing downstream; nothing is kept between windows;
 *   - an archive without data is header + closing word (42 bytes), a valid empty part, where the reference writes the
 *     bare four zero bytes, which no lzop reader accepts.
 */
#include <errno.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "la_read_private.h"
#include "la_write_private.h"
#include "../../include/la_gpu.h"
#include "../../include/la_host.h"

#define LZOW_HEADER_BYTES 38u

struct lzow_private {
	struct la_write_window w;	/* first */
	int compression_level;
	int header_written;
};

static int lzow_options(struct archive_write_filter *f, const char *key, const char *value)
{
	struct lzow_private *d = f->data;
	if (strcmp(key, "compression-level") == 0) {
		if (value == NULL || !(value[0] >= '1' && value[0] <= '9') || value[1] != '\0')
			return ARCHIVE_WARN;
		d->compression_level = value[0] - '0';
		return ARCHIVE_OK;
	}
	return ARCHIVE_WARN;
}

static void lzow_be32enc(uint8_t *p, uint32_t v)
{
	p[0] = (uint8_t)(v >> 24); p[1] = (uint8_t)(v >> 16); p[2] = (uint8_t)(v >> 8); p[3] = (uint8_t)v;
}

/* make_header, archive_write_add_filter_lzop.c:285-312 */
static void lzow_header(const struct lzow_private *d, uint8_t *h)
{
	static const uint8_t template[LZOW_HEADER_BYTES] = {
		0x89, 0x4c, 0x5a, 0x4f, 0x00, 0x0d, 0x0a, 0x1a, 0x0a,	/* magic */
		0x10, 0x30,		/* lzop version */
		0x09, 0x40,		/* library version */
		0x09, 0x40,		/* version needed */
		1, 5,			/* method, level */
		0x03, 0x00, 0x00, 0x0d,	/* flags: Unix, stdin, stdout, Adler-32 of the uncompressed bytes */
		0x00, 0x00, 0x81, 0xa4,	/* mode */
		0, 0, 0, 0, 0, 0, 0, 0,	/* mtime low, high */
		0,			/* name length */
		0, 0, 0, 0,		/* header checksum */
	};
	const int lv = d->compression_level;
	const int64_t t = (int64_t)time(NULL);
	uint32_t a = 1, b = 0;
	memcpy(h, template, sizeof(template));
	h[15] = (uint8_t)(lv == 1 ? 2 : lv >= 7 ? 3 : 1);
	h[16] = (uint8_t)(lv == 1 ? 1 : lv >= 7 ? lv : 5);
	lzow_be32enc(h + 25, (uint32_t)(t & 0xffffffff));
	lzow_be32enc(h + 29, (uint32_t)((t >> 32) & 0xffffffff));
	for (size_t i = 9; i < 34; i++) {
		a = (a + h[i]) % 65521u;
		b = (b + a) % 65521u;
	}
	lzow_be32enc(h + 34, (b << 16) | a);
}

static uint64_t lzow_bound(struct archive_write_filter *f, uint64_t n)
{
	(void)f;
	return LZOW_HEADER_BYTES + la_gpu_lzop_compress_bound(n, LA_LZOPC_BLOCK_BYTES);
}

static int lzow_compress(struct archive_write_filter *f, const struct la_write_window *w)
{
	const struct lzow_private *d = f->data;
	la_lzopc_batch bt;
	memset(&bt, 0, sizeof(bt));
	bt.d_src = w->len ? w->d_in : NULL; bt.src_bytes = w->len;
	bt.block_size = LA_LZOPC_BLOCK_BYTES;
	bt.lead_bytes = d->header_written ? 0u : LZOW_HEADER_BYTES;
	bt.d_out = w->d_out; bt.out_cap = w->out_cap; bt.d_out_bytes = w->d_len;
	return la_gpu_lzop_compress(w->gpu, &bt);
}

/* the first window's bytes came back with a gap in front: the header goes there */
static int lzow_patch(struct archive_write_filter *f, const struct la_write_window *w, uint64_t total)
{
	struct lzow_private *d = f->data;
	if (d->header_written)
		return ARCHIVE_OK;
	if (total < LZOW_HEADER_BYTES)
		return la_write_window_fail(f, "compress (header gap)");
	lzow_header(d, w->out);
	d->header_written = 1;
	return ARCHIVE_OK;
}

static int lzow_open(struct archive_write_filter *f)
{
	return la_write_window_open(f, LA_LZOPC_BLOCK_BYTES);	/* whole blocks */
}

static int lzow_close(struct archive_write_filter *f)
{
	struct lzow_private *d = f->data;
	static const uint8_t end[4] = { 0, 0, 0, 0 };
	if (d->w.gpu == NULL)
		return ARCHIVE_OK;
	int r = la_write_window_flush(f, 0);
	if (r != ARCHIVE_OK)
		return r;
	if (!d->header_written) {	/* no data: the header is the host's alone */
		uint8_t h[LZOW_HEADER_BYTES];
		lzow_header(d, h);
		d->header_written = 1;
		if ((r = __archive_write_filter(f->next_filter, h, sizeof(h))) != ARCHIVE_OK)
			return r;
	}
	return __archive_write_filter(f->next_filter, end, sizeof(end));
}

int archive_write_add_filter_lzop(struct archive *_a)
{
	struct archive_write_filter *f = __archive_write_allocate_filter(_a);
	struct lzow_private *d = calloc(1, sizeof(*d));
	if (f == NULL || d == NULL) {
		free(d);
		archive_set_error(_a, ENOMEM, "Out of memory");
		return ARCHIVE_FATAL;
	}
	d->w.name = "lzop";
	d->w.bound = lzow_bound;
	d->w.compress = lzow_compress;
	d->w.patch = lzow_patch;
	d->compression_level = 5;	/* archive_write_add_filter_lzop.c:172 */
	f->data = d;
	f->options = lzow_options;
	f->open = lzow_open;
	f->close = lzow_close;
	f->free = la_write_window_free;
	f->code = ARCHIVE_FILTER_LZOP;
	f->name = "lzop";
	return ARCHIVE_OK;
}
