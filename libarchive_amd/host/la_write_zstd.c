/*
 * la_write_zstd.c -- the zstd WRITE filter on the device data plane (la_gpu_zstd_compress), registered on the
 * write core of la_write_filters.c.
 *
 * Registration and options follow libarchive/archive_write_add_filter_zstd.c (name "zstd", code ARCHIVE_FILTER_ZSTD,
 * default level 3, a content checksum on every frame as its ZSTD_c_checksumFlag = 1), with the option ranges that
 * filter uses when it is built without libzstd's own bounds: "compression-level" -99..22 (0 and below write raw
 * literals; 1 and 2 are the fast levels: Huffman literals for alphabets up to byte 128, predefined sequence tables; 3
 * and above, the default among them, add LA_ZSTDC_FULL_ALPHABET | LA_ZSTDC_FIT_TABLES: Huffman literals for any
 * alphabet and sequence tables chosen per block, the densest stream the device writes), "threads" >= 0 (accepted, ignored), "frame-per-file"
 * (a no-op: the raw format holds one entry), "min-frame-in" / "min-frame-out" / "min-frame-size" (sizes with k / M /
 * G and an optional B, accepted, ignored), "max-frame-in" / "max-frame-size" >= 1024 (frames hold at most this much
 * input), "max-frame-out" >= 1024 (accepted: frames are bounded by their input only), "long" 10..31 (accepted, no
 * effect: matches never leave a block).  An option the filter does not take returns ARCHIVE_WARN, which
 * archive_write_set_filter_option turns into ARCHIVE_FAILED "Undefined option".
 *
 * What differs from the reference by design:
 *   - write() only gathers input into the write window of la_write_private.h; a full window (LA_GPU_WRITE_WINDOW_MIB,
 *     default 64, rounded down to whole frames) goes to la_gpu_zstd_compress() in ONE call and the frames come back
 *     in one copy;
 *   - the stream is a sequence of small frames, by default ONE 128 KiB block each, not the reference's single frame:
 *     the device read side decodes one frame per wave, so a many-frame stream is the shape it reads fast (and the
 *     shape its default bid policy takes), and every zstd reader reads concatenated frames.  "max-frame-in" n below
 *     128 KiB gives frames of one n-byte block, above it frames of floor(n / 128 KiB) blocks of 128 KiB, at most
 *     128 MiB: a single-segment frame's window is its content size, and 2^27 is the window limit of zstd's
 *     streaming decoders (the reference's reader among them).
 */
#include <errno.h>
#include <inttypes.h>
#include <limits.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "la_read_private.h"
#include "la_write_private.h"
#include "../../include/la_gpu.h"
#include "../../include/la_host.h"

#define ZSTDW_BLOCK      131072u
#define ZSTDW_FRAME_MAX  (128u << 20)

struct zstdw_private {
	struct la_write_window w;	/* first */
	int compression_level;
	int threads, long_distance, frame_per_file;	/* accepted, no effect here */
	uint64_t min_frame_in, min_frame_out, max_frame_in, max_frame_out;
	uint32_t block_size, blocks_per_frame;
};

/* a decimal integer, nothing else (archive_write_add_filter_zstd.c string_to_number) */
static int zstdw_number(const char *s, intmax_t *v)
{
	char *end;
	if (s == NULL || *s == '\0')
		return 0;
	errno = 0;
	*v = strtoimax(s, &end, 10);
	return end != s && *end == '\0' && errno == 0;
}

/* a size: digits, an optional k / M / G, an optional B, no sign (string_to_size of the same file) */
static int zstdw_size(const char *s, uint64_t *v)
{
	char *end;
	unsigned shift = 0;
	if (s == NULL || *s == '\0' || *s == '-')
		return 0;
	errno = 0;
	const uintmax_t n = strtoumax(s, &end, 10);
	if (end == s || errno != 0)
		return 0;
	switch (*end) {
	case 'k': case 'K': shift = 10; end++; break;
	case 'm': case 'M': shift = 20; end++; break;
	case 'g': case 'G': shift = 30; end++; break;
	default: break;
	}
	if (*end == 'b' || *end == 'B')
		end++;
	if (*end != '\0' || n > ((uintmax_t)SIZE_MAX >> shift))
		return 0;
	*v = (uint64_t)n << shift;
	return 1;
}

static int zstdw_options(struct archive_write_filter *f, const char *key, const char *value)
{
	struct zstdw_private *d = f->data;
	intmax_t n;
	uint64_t sz;
	if (strcmp(key, "compression-level") == 0) {
		if (!zstdw_number(value, &n) || n < -99 || n > 22)
			return ARCHIVE_WARN;
		d->compression_level = (int)n;
		return ARCHIVE_OK;
	}
	if (strcmp(key, "threads") == 0) {
		if (!zstdw_number(value, &n) || n < 0 || n > INT_MAX)
			return ARCHIVE_WARN;
		d->threads = (int)n;
		return ARCHIVE_OK;
	}
	if (strcmp(key, "frame-per-file") == 0) {
		d->frame_per_file = 1;
		return ARCHIVE_OK;
	}
	if (strcmp(key, "min-frame-in") == 0) {
		if (!zstdw_size(value, &sz))
			return ARCHIVE_WARN;
		d->min_frame_in = sz;
		return ARCHIVE_OK;
	}
	if (strcmp(key, "min-frame-out") == 0 || strcmp(key, "min-frame-size") == 0) {
		if (!zstdw_size(value, &sz))
			return ARCHIVE_WARN;
		d->min_frame_out = sz;
		return ARCHIVE_OK;
	}
	if (strcmp(key, "max-frame-in") == 0 || strcmp(key, "max-frame-size") == 0) {
		if (!zstdw_size(value, &sz) || sz < 1024)
			return ARCHIVE_WARN;
		d->max_frame_in = sz;
		return ARCHIVE_OK;
	}
	if (strcmp(key, "max-frame-out") == 0) {
		if (!zstdw_size(value, &sz) || sz < 1024)
			return ARCHIVE_WARN;
		d->max_frame_out = sz;
		return ARCHIVE_OK;
	}
	if (strcmp(key, "long") == 0) {
		if (!zstdw_number(value, &n) || n < 10 || n > 31)
			return ARCHIVE_WARN;
		d->long_distance = (int)n;
		return ARCHIVE_OK;
	}
	return ARCHIVE_WARN;
}

static uint64_t zstdw_bound(struct archive_write_filter *f, uint64_t n)
{
	const struct zstdw_private *d = f->data;
	return la_gpu_zstd_compress_bound(n, d->block_size, d->blocks_per_frame);
}

static int zstdw_compress(struct archive_write_filter *f, const struct la_write_window *w)
{
	const struct zstdw_private *d = f->data;
	la_zstdc_batch bt;
	memset(&bt, 0, sizeof(bt));
	bt.d_src = w->d_in; bt.src_bytes = w->len;
	bt.block_size = d->block_size; bt.blocks_per_frame = d->blocks_per_frame;
	bt.flags = LA_ZSTDC_CHECKSUM | (d->compression_level <= 0 ? LA_ZSTDC_RAW_LITERALS :
	    d->compression_level >= 3 ? LA_ZSTDC_FULL_ALPHABET | LA_ZSTDC_FIT_TABLES : 0);
	bt.d_out = w->d_out; bt.out_cap = w->out_cap; bt.d_out_bytes = w->d_len;
	return la_gpu_zstd_compress(w->gpu, &bt);
}

static int zstdw_open(struct archive_write_filter *f)
{
	struct zstdw_private *d = f->data;
	/* frame shape: one 128 KiB block by default; max-frame-in below a block is one smaller block */
	uint64_t fin = d->max_frame_in < ZSTDW_FRAME_MAX ? d->max_frame_in : ZSTDW_FRAME_MAX;
	if (fin < ZSTDW_BLOCK) {
		d->block_size = (uint32_t)fin;
		d->blocks_per_frame = 1;
	} else {
		d->block_size = ZSTDW_BLOCK;
		d->blocks_per_frame = d->max_frame_in == UINT64_MAX ? 1u : (uint32_t)(fin / ZSTDW_BLOCK);
	}
	return la_write_window_open(f, (size_t)d->block_size * d->blocks_per_frame);	/* whole frames */
}

static int zstdw_close(struct archive_write_filter *f)
{
	struct zstdw_private *d = f->data;
	if (d->w.gpu == NULL)
		return ARCHIVE_OK;
	/* nothing written at all: one empty frame (FCS 0, one empty last raw block, the checksum of nothing) */
	return la_write_window_flush(f, !d->w.wrote_anything);
}

int archive_write_add_filter_zstd(struct archive *_a)
{
	struct archive_write_filter *f = __archive_write_allocate_filter(_a);
	struct zstdw_private *d = calloc(1, sizeof(*d));
	if (f == NULL || d == NULL) {
		free(d);
		archive_set_error(_a, ENOMEM, "Out of memory");
		return ARCHIVE_FATAL;
	}
	d->w.name = "zstd";
	d->w.bound = zstdw_bound;
	d->w.compress = zstdw_compress;
	d->compression_level = 3;	/* CLEVEL_DEFAULT in the reference */
	d->max_frame_in = UINT64_MAX;
	d->max_frame_out = UINT64_MAX;
	f->data = d;
	f->options = zstdw_options;
	f->open = zstdw_open;
	f->close = zstdw_close;
	f->free = la_write_window_free;
	f->code = ARCHIVE_FILTER_ZSTD;
	f->name = "zstd";
	return ARCHIVE_OK;
}
