/*
 * la_write_xz.c -- the xz WRITE filter on the device data plane (la_gpu_xz_compress), registered on the write core of
 * la_write_filters.c.
 *
 * Registration and options follow libarchive/archive_write_add_filter_xz.c:238-244 and :371-410: name "xz", code
 * ARCHIVE_FILTER_XZ, default level 6, check CRC64; "compression-level" takes exactly one character '0'..'9'; "threads" is
 * parsed as the reference parses it (strtoul; NULL or trailing garbage is ARCHIVE_WARN, 0 is accepted) and is WITHOUT
 * EFFECT: the device codes every chunk of a window at once, whatever the count.  Any other option or value returns
 * ARCHIVE_WARN, which archive_write_set_filter_option turns into ARCHIVE_FAILED "Undefined option".
 *
 * What differs from the reference by design:
 *   - write() only gathers input into the write window of la_write_private.h; a full window (LA_GPU_WRITE_WINDOW_MIB,
 *     default 64, whole blocks) goes to la_gpu_xz_compress() in ONE call, which returns complete blocks back to back,
 *     the stream header in front of the first window's;
 *   - the output is ONE stream per archive of 1 MiB blocks with both sizes in every block header (the shape a threaded
 *     reader, and this project's own, wants), LZMA2 chunks of 64 KiB each with a state reset; the bytes are not liblzma's;
 *   - the index is kept on the host: the patch hook walks the block headers of the bytes that came back and appends
 *     (unpadded size, uncompressed size) to a list; close() writes index and footer from it;
 *   - an archive without data is the 32-byte stream without a block, written without a device call;
 *   - the lzip write filter, which the reference serves from the same file, is la_write_lzip.c.
 */
#include <errno.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "la_read_private.h"
#include "la_write_private.h"
#include "../../include/la_gpu.h"
#include "../../include/la_host.h"

struct xzw_record { uint64_t unpadded, uncomp; };

struct xzw_private {
	struct la_write_window w;	/* first */
	int compression_level;
	int threads;			/* parsed, without effect */
	struct xzw_record *rec;
	size_t n_rec, cap_rec;
};

static int xzw_options(struct archive_write_filter *f, const char *key, const char *value)
{
	struct xzw_private *d = f->data;
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

static uint64_t xzw_bound(struct archive_write_filter *f, uint64_t n)
{
	const struct xzw_private *d = f->data;
	return la_gpu_xz_compress_bound(n, (uint32_t)d->compression_level);
}

static int xzw_compress(struct archive_write_filter *f, const struct la_write_window *w)
{
	const struct xzw_private *d = f->data;
	la_xzc_batch bt;
	memset(&bt, 0, sizeof(bt));
	bt.d_src = w->len ? w->d_in : NULL; bt.src_bytes = w->len;
	bt.level = (uint32_t)d->compression_level;
	bt.flags = w->wrote_anything ? 0u : LA_XZC_FIRST;
	bt.d_out = w->d_out; bt.out_cap = w->out_cap; bt.d_out_bytes = w->d_len;
	return la_gpu_xz_compress(w->gpu, &bt);
}

/* a variable-length integer of the format (at most 9 bytes); 0: malformed or beyond `lim` */
static size_t xzw_vli_get(const uint8_t *p, size_t lim, uint64_t *v)
{
	*v = 0;
	for (size_t i = 0; i < lim && i < 9; i++) {
		*v |= (uint64_t)(p[i] & 0x7Fu) << (7 * i);
		if (!(p[i] & 0x80u))
			return i + 1;
	}
	return 0;
}

static void xzw_le32enc(uint8_t *p, uint32_t v)
{
	p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24);
}

static size_t xzw_vli_put(uint8_t *p, uint64_t v)
{
	size_t n = 0;
	while (v >= 0x80u) {
		p[n++] = (uint8_t)(v | 0x80u);
		v >>= 7;
	}
	p[n++] = (uint8_t)v;
	return n;
}

/* the walk of la_filter_xz.c over what one call returned: block header (both sizes), data, padding, check */
static int xzw_patch(struct archive_write_filter *f, const struct la_write_window *w, uint64_t total)
{
	struct xzw_private *d = f->data;
	uint64_t p = d->n_rec == 0 ? 12u : 0u;	/* the stream header is in front of the first window's blocks */
	while (p < total) {
		const uint8_t *h = w->out + p;
		uint64_t comp = 0, uncomp = 0;
		size_t hs, a, b;
		if (total - p < 8u || (hs = ((size_t)h[0] + 1u) * 4u) > total - p || (h[1] & 0xC0u) != 0xC0u ||
		    (a = xzw_vli_get(h + 2, hs - 2u, &comp)) == 0 || (b = xzw_vli_get(h + 2 + a, hs - 2u - a, &uncomp)) == 0 ||
		    (uint32_t)la_crc32(0, h, hs - 4u) != archive_le32dec(h + hs - 4u))
			return la_write_window_fail(f, "compress (block header)");
		const uint64_t size = hs + ((comp + 3u) & ~(uint64_t)3u) + 8u;
		if (size > total - p)
			return la_write_window_fail(f, "compress (block size)");
		if (d->n_rec == d->cap_rec) {
			const size_t cap = d->cap_rec ? d->cap_rec * 2u : 256u;
			struct xzw_record *r = realloc(d->rec, cap * sizeof(*r));
			if (r == NULL) {
				archive_set_error(f->archive, ENOMEM, "Out of memory");
				return ARCHIVE_FATAL;
			}
			d->rec = r; d->cap_rec = cap;
		}
		d->rec[d->n_rec].unpadded = hs + comp + 8u;
		d->rec[d->n_rec].uncomp = uncomp;
		d->n_rec++;
		p += size;
	}
	return ARCHIVE_OK;
}

static int xzw_open(struct archive_write_filter *f)
{
	struct xzw_private *d = f->data;
	const size_t unit = (size_t)la_gpu_xz_compress_block_bytes((uint32_t)d->compression_level);
	int r = la_write_window_open(f, unit);	/* whole blocks */
	if (r != ARCHIVE_OK)
		return r;
	if (d->w.cap > LA_XZC_MAX_SRC_BYTES)
		d->w.cap = (size_t)(LA_XZC_MAX_SRC_BYTES / unit * unit);
	return ARCHIVE_OK;
}

static int xzw_close(struct archive_write_filter *f)
{
	struct xzw_private *d = f->data;
	if (d->w.gpu == NULL)
		return ARCHIVE_OK;
	int r = la_write_window_flush(f, 0);
	if (r != ARCHIVE_OK)
		return r;
	if (!d->w.wrote_anything) {	/* no data: the stream header is the host's too */
		static const uint8_t head[12] = { 0xFD, '7', 'z', 'X', 'Z', 0x00, 0x00, 0x04, 0xE6, 0xD6, 0xB4, 0x46 };
		if ((r = __archive_write_filter(f->next_filter, head, sizeof(head))) != ARCHIVE_OK)
			return r;
	}
	/* index: indicator, count, the records, zero padding to four bytes, CRC32; then the footer */
	uint8_t *ix = malloc(1u + 9u + d->n_rec * 18u + 4u + 4u + 12u);
	if (ix == NULL) {
		archive_set_error(f->archive, ENOMEM, "Out of memory");
		return ARCHIVE_FATAL;
	}
	size_t n = 0;
	ix[n++] = 0;
	n += xzw_vli_put(ix + n, d->n_rec);
	for (size_t i = 0; i < d->n_rec; i++) {
		n += xzw_vli_put(ix + n, d->rec[i].unpadded);
		n += xzw_vli_put(ix + n, d->rec[i].uncomp);
	}
	while (n & 3u)
		ix[n++] = 0;
	xzw_le32enc(ix + n, (uint32_t)la_crc32(0, ix, n));
	n += 4;
	uint8_t *ft = ix + n;
	xzw_le32enc(ft + 4, (uint32_t)(n / 4u - 1u));	/* backward size */
	ft[8] = 0x00; ft[9] = 0x04;				/* stream flags: CRC64 */
	xzw_le32enc(ft, (uint32_t)la_crc32(0, ft + 4, 6));
	ft[10] = 'Y'; ft[11] = 'Z';
	r = __archive_write_filter(f->next_filter, ix, n + 12u);
	free(ix);
	return r;
}

static int xzw_free(struct archive_write_filter *f)
{
	struct xzw_private *d = f->data;
	if (d) {
		free(d->rec);
		d->rec = NULL;
	}
	return la_write_window_free(f);
}

int archive_write_add_filter_xz(struct archive *_a)
{
	struct archive_write_filter *f = __archive_write_allocate_filter(_a);
	struct xzw_private *d = calloc(1, sizeof(*d));
	if (f == NULL || d == NULL) {
		free(d);
		archive_set_error(_a, ENOMEM, "Out of memory");
		return ARCHIVE_FATAL;
	}
	d->w.name = "xz";
	d->w.bound = xzw_bound;
	d->w.compress = xzw_compress;
	d->w.patch = xzw_patch;
	d->compression_level = 6;	/* LZMA_PRESET_DEFAULT, archive_write_add_filter_xz.c:152 */
	d->threads = 1;
	f->data = d;
	f->options = xzw_options;
	f->open = xzw_open;
	f->close = xzw_close;
	f->free = xzw_free;
	f->code = ARCHIVE_FILTER_XZ;
	f->name = "xz";
	return ARCHIVE_OK;
}
