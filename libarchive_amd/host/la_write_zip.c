/*
 * la_write_zip.c -- the ZIP WRITE format on the device data plane: archive_write_set_format_zip.
 *
 * Restates libarchive/archive_write_set_format_zip.c for what this slice's entries can say (regular files and
 * directories with a name, a size or none, an mtime, permission bits): the option table (:338-556), the local file
 * header with its extra fields (:788-1319), the data descriptor and the central directory entry (:2025-2141), the
 * end records (:2144-2214), the path rules (:2242-2307) and the DOS time (archive_time.c:76-122).  What differs by
 * design is where the bytes of an entry are made.  The reference runs deflate() and crc32() on every write, one entry
 * after the other (:1477-1820).  Here entry bytes only gather in the pinned write window the filters use
 * (la_write_private.h, LA_GPU_WRITE_WINDOW_MIB); when the window is full, or at close, ONE la_gpu_zip_compress() call
 * takes every entry, or part of an entry, that lies in it as a table of segments and returns their raw-deflate
 * streams and CRC32s with gaps where this file then writes the local headers and the data descriptors
 * (zipw_patch).  That is possible because the reference already writes every regular file "length at end"
 * (:1051-1052, :1062): the local header carries no CRC and no sizes, so it is known when the entry begins, and the
 * descriptor behind the data takes what the device reports.  An entry larger than a window is several segments,
 * chained by the running CRC32; offsets become known in the patch step, window after window, so nothing seeks.
 *
 * Left out: encryption, methods other than 0 and 8, symbolic links and other file types (ARCHIVE_FAILED before
 * anything is written), and the "ux" uid/gid extra field (:1178-1189) because this slice's entries carry no ids.
 * There is no CPU path: without a gfx950 device archive_write_open fails with the write filters' message.
 */
#include <errno.h>
#include <langinfo.h>
#include <limits.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "la_read_private.h"
#include "la_write_private.h"
#include "../../include/la_gpu.h"
#include "../../include/la_host.h"

#define ZIPW_CHUNK    49152u		/* the gzip write filter's chunk */
#define ZIPW_MAX_SEGS 65536u		/* segments and gap bytes of one device call: what its output buffer is sized for */
#define ZIPW_MAX_GAP  (8u << 20)
#define ZIP_4GB_MAX   0xffffffffLL	/* :89-90 */
#define ZIP_4GB_MAX_UNCOMPRESSED 0xff000000LL
#define ZIP_FLAG_AVOID_ZIP64 1		/* :186-187 */
#define ZIP_FLAG_FORCE_ZIP64 2
#define COMPRESSION_UNSPECIFIED (-1)	/* :95-103 */
#define COMPRESSION_STORE   0
#define COMPRESSION_DEFLATE 8
#define ZIP_ENTRY_FLAG_LENGTH_AT_END (1 << 3)	/* :81-87 */
#define ZIP_ENTRY_FLAG_UTF8_NAME     (1 << 11)
#define DOS_MIN_TIME 0x00210000U	/* archive_time.c:36-37 */
#define DOS_MAX_TIME 0xff9fbf7dU

struct zipw_cdent {	/* what the central directory says of one entry (:1145-1168, :2054-2139) */
	char *name;		/* as written: a directory's ends in '/' */
	uint16_t name_len, version, flags, method;
	uint32_t dos_time, ext_attr, crc;
	int mtime_set;
	int64_t mtime;
	uint64_t comp, unc, offset;
};

struct zipw_seg {	/* the host's side of one la_zipc_seg of the window */
	uint32_t ent;		/* its entry in cd[] */
	uint32_t lh_off, lh_len;	/* the local header in hdrs[], for the segment an entry starts with */
	uint8_t first, last, desc_len;
	uint64_t unc_total;	/* last: the entry's bytes */
};

struct zipw {
	struct la_write_window w;		/* first: la_write_window_* work on it */
	struct archive_write_filter self;	/* the window's handle on the chain: data = this, next_filter = the first filter */
	struct archive_write *a;
	/* options (:338-556) */
	int requested_compression, compression_level, fake_crc, utf8_names;
	unsigned flags;
	/* the window's segments */
	la_zipc_seg *segs;
	la_zipc_result *res;
	struct zipw_seg *info;
	uint32_t n_segs;
	uint64_t gap_total;
	uint8_t *hdrs;
	size_t hdrs_len, hdrs_cap;
	void *d_segs, *d_res;
	int failed;		/* a window could not be written: nothing more is */
	/* the entry between its header and its end */
	int open;
	int64_t limit;		/* bytes it still takes (:1482-1483) */
	uint64_t unc_written;
	/* the entry whose segments are coming back (zipw_patch) */
	uint64_t p_comp;
	uint32_t p_crc;
	uint64_t written_bytes;	/* archive bytes handed to the chain so far */
	struct zipw_cdent *cd;
	size_t n_cd, cap_cd;
};

static void le16(uint8_t *p, unsigned v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); }
static void le32(uint8_t *p, uint32_t v) { le16(p, v & 0xffff); le16(p + 2, v >> 16); }
static void le64(uint8_t *p, uint64_t v) { le32(p, (uint32_t)v); le32(p + 4, (uint32_t)(v >> 32)); }

static uint32_t unix_to_dos(int64_t unix_time)	/* archive_time.c:76-122 */
{
	struct tm tmbuf, *t;
	time_t ut = (time_t)unix_time;
	uint32_t dt = 0;
	t = localtime_r(&ut, &tmbuf);
	if (t != NULL && t->tm_year >= INT_MIN + 80) {
		const int year = t->tm_year - 80;
		if (year & ~0x7f)
			dt = year > 0 ? DOS_MAX_TIME : DOS_MIN_TIME;
		else {
			dt += (uint32_t)(year & 0x7f) << 9;
			dt += (uint32_t)((t->tm_mon + 1) & 0x0f) << 5;
			dt += (uint32_t)(t->tm_mday & 0x1f);
			dt <<= 16;
			dt += (uint32_t)(t->tm_hour & 0x1f) << 11;
			dt += (uint32_t)(t->tm_min & 0x3f) << 5;
			dt += (uint32_t)(t->tm_sec & 0x3e) >> 1;	/* only counting every 2 seconds */
		}
	}
	if (dt > DOS_MAX_TIME)
		dt = DOS_MAX_TIME;
	else if (dt < DOS_MIN_TIME)
		dt = DOS_MIN_TIME;
	return dt;
}

static int zipw_nomem(struct zipw *zip)
{
	zip->failed = 1;	/* tables may be half built: nothing more is written */
	zip->open = 0;
	archive_set_error(&zip->a->archive, ENOMEM, "Can't allocate zip data");
	return ARCHIVE_FATAL;
}

/* ------------------------------------------------------------------ options (:338-556) */

static int zipw_options(struct archive_write *a, const char *key, const char *val)
{
	struct zipw *zip = a->format_data;
	int ret = ARCHIVE_FAILED;

	if (strcmp(key, "compression") == 0) {	/* :345-398 */
		if (val == NULL || val[0] == 0)
			archive_set_error(&a->archive, ARCHIVE_ERRNO_MISC, "%s: compression option needs a compression name", a->format_name);
		else if (strcmp(val, "deflate") == 0) {
			zip->requested_compression = COMPRESSION_DEFLATE;
			ret = ARCHIVE_OK;
		} else if (strcmp(val, "store") == 0) {
			zip->requested_compression = COMPRESSION_STORE;
			ret = ARCHIVE_OK;
		} else if (strcmp(val, "bzip2") == 0 || strcmp(val, "lzma") == 0 || strcmp(val, "xz") == 0 || strcmp(val, "zstd") == 0)
			archive_set_error(&a->archive, ARCHIVE_ERRNO_MISC, "%s compression not supported", val);	/* as built without them */
		return ret;
	}
	if (strcmp(key, "compression-level") == 0) {	/* :399-435 */
		char *endptr;
		if (val == NULL)
			return ARCHIVE_WARN;
		errno = 0;
		zip->compression_level = (short)strtoul(val, &endptr, 10);
		if (errno != 0 || *endptr != '\0' || zip->compression_level < 0 || zip->compression_level > 9) {
			zip->compression_level = 6;
			return ARCHIVE_WARN;
		}
		if (zip->compression_level == 0)
			zip->requested_compression = COMPRESSION_STORE;
		else if (zip->requested_compression == COMPRESSION_UNSPECIFIED)	/* not forcing an already specified method */
			zip->requested_compression = COMPRESSION_DEFLATE;
		return ARCHIVE_OK;
	}
	if (strcmp(key, "threads") == 0) {	/* :436-462; the device has its own idea of parallelism */
		char *endptr;
		if (val == NULL)
			return ARCHIVE_FAILED;
		errno = 0;
		(void)strtoul(val, &endptr, 10);
		if (errno != 0 || *endptr != '\0') {
			archive_set_error(&a->archive, ARCHIVE_ERRNO_MISC, "Illegal value `%s'", val);
			return ARCHIVE_FAILED;
		}
		return ARCHIVE_OK;
	}
	if (strcmp(key, "encryption") == 0) {	/* :463-499, as built without a cipher */
		if (val == NULL)
			ret = ARCHIVE_OK;
		else if (val[0] == '1' || strcmp(val, "traditional") == 0 || strcmp(val, "zipcrypt") == 0 || strcmp(val, "ZipCrypt") == 0 ||
		    strcmp(val, "aes128") == 0 || strcmp(val, "aes256") == 0)
			archive_set_error(&a->archive, ARCHIVE_ERRNO_MISC, "encryption not supported");
		else
			archive_set_error(&a->archive, ARCHIVE_ERRNO_MISC, "%s: unknown encryption '%s'", a->format_name, val);
		return ret;
	}
	if (strcmp(key, "fakecrc32") == 0) {	/* :507-517, FOR TESTING ONLY: every CRC written is 0 */
		zip->fake_crc = !(val == NULL || val[0] == 0);
		return ARCHIVE_OK;
	}
	if (strcmp(key, "hdrcharset") == 0) {	/* :518-534; names are written as they are given, so only UTF-8 can be promised */
		if (val == NULL || val[0] == 0)
			archive_set_error(&a->archive, ARCHIVE_ERRNO_MISC, "%s: hdrcharset option needs a character-set name", a->format_name);
		else if (strcmp(val, "UTF-8") == 0 || strcmp(val, "utf-8") == 0 || strcmp(val, "UTF8") == 0 || strcmp(val, "utf8") == 0) {
			zip->utf8_names = 1;
			ret = ARCHIVE_OK;
		} else {
			archive_set_error(&a->archive, ARCHIVE_ERRNO_MISC, "%s: hdrcharset `%s' is not supported: names are not converted, only UTF-8 can be declared",
			    a->format_name, val);
			ret = ARCHIVE_FATAL;
		}
		return ret;
	}
	if (strcmp(key, "zip64") == 0) {	/* :535-549 */
		if (val != NULL && *val != '\0') {
			zip->flags |= ZIP_FLAG_FORCE_ZIP64;
			zip->flags &= ~(unsigned)ZIP_FLAG_AVOID_ZIP64;
		} else {
			zip->flags &= ~(unsigned)ZIP_FLAG_FORCE_ZIP64;
			zip->flags |= ZIP_FLAG_AVOID_ZIP64;
		}
		return ARCHIVE_OK;
	}
	return ARCHIVE_WARN;	/* not handled here: the option supervisor reports it (:552-555) */
}

/* ------------------------------------------------------------------ the window */

static uint64_t zipw_bound(struct archive_write_filter *f, uint64_t n)
{
	(void)f;
	return la_gpu_zip_compress_bound(n, ZIPW_MAX_SEGS, ZIPW_CHUNK, ZIPW_MAX_GAP);
}

static int zipw_compress(struct archive_write_filter *f, const struct la_write_window *w)
{
	struct zipw *zip = f->data;
	la_zipc_batch bt;
	int rc;
	if ((rc = la_gpu_memcpy_h2d(w->gpu, zip->d_segs, zip->segs, (uint64_t)zip->n_segs * sizeof(la_zipc_seg))) != LA_OK)
		return rc;
	memset(&bt, 0, sizeof(bt));
	bt.d_src = w->d_in; bt.src_bytes = w->len;
	bt.d_segs = zip->d_segs; bt.n_segs = zip->n_segs;
	bt.chunk_bytes = ZIPW_CHUNK;
	/* what the device has for a level, as the gzip write filter maps them: 0 stored blocks, 1 fixed codes, 2..9 dynamic */
	bt.options = zip->compression_level == 0 ? LA_GZC_STORED : (zip->compression_level == 1 ? LA_GZC_FIXED : LA_GZC_DYNAMIC);
	bt.d_out = w->d_out; bt.out_cap = w->out_cap;
	bt.d_results = zip->d_res; bt.d_out_bytes = w->d_len;
	if ((rc = la_gpu_zip_compress(w->gpu, &bt)) != LA_OK)
		return rc;
	return la_gpu_memcpy_d2h(w->gpu, zip->res, zip->d_res, (uint64_t)zip->n_segs * sizeof(la_zipc_result));
}

/* The window's bytes are back: local headers into the gaps in front of the entries that start here, data descriptors
 * (:2025-2052) behind those that end here, and the central directory learns offsets, sizes and CRCs. */
static int zipw_patch(struct archive_write_filter *f, const struct la_write_window *w, uint64_t total)
{
	struct zipw *zip = f->data;
	for (uint32_t i = 0; i < zip->n_segs; i++) {
		const la_zipc_seg *g = &zip->segs[i];
		const la_zipc_result *r = &zip->res[i];
		const struct zipw_seg *s = &zip->info[i];
		struct zipw_cdent *e = &zip->cd[s->ent];
		if (r->out_off < g->gap_before || r->out_off + r->out_len + g->gap_after > total)
			return la_write_window_fail(f, "compress (segment layout)");
		if (s->first) {
			e->offset = zip->written_bytes + r->out_off - g->gap_before;
			memcpy(w->out + r->out_off - g->gap_before, zip->hdrs + s->lh_off, s->lh_len);
			zip->p_comp = 0;
		}
		zip->p_comp += r->out_len;
		zip->p_crc = r->crc32;
		if (!s->last)
			continue;
		e->comp = zip->p_comp;
		e->unc = s->unc_total;
		e->crc = zip->fake_crc ? 0 : zip->p_crc;
		if (s->desc_len) {
			uint8_t *d = w->out + r->out_off + r->out_len;
			memcpy(d, "PK\007\010", 4);
			le32(d + 4, e->crc);
			if (s->desc_len == 24) {
				le64(d + 8, e->comp);
				le64(d + 16, e->unc);
			} else {
				le32(d + 8, (uint32_t)e->comp);
				le32(d + 12, (uint32_t)e->unc);
			}
		}
	}
	zip->written_bytes += total;
	return ARCHIVE_OK;
}

static int zipw_flush(struct zipw *zip)
{
	if (zip->failed)
		return ARCHIVE_FATAL;
	if (zip->n_segs == 0)
		return ARCHIVE_OK;
	if (zip->d_segs == NULL &&
	    (la_gpu_malloc(zip->w.gpu, &zip->d_segs, (uint64_t)ZIPW_MAX_SEGS * sizeof(la_zipc_seg)) != LA_OK ||
	     la_gpu_malloc(zip->w.gpu, &zip->d_res, (uint64_t)ZIPW_MAX_SEGS * sizeof(la_zipc_result)) != LA_OK))
		return la_write_window_fail(&zip->self, "device allocation");
	zip->self.next_filter = zip->a->filter_first;
	int r = la_write_window_flush(&zip->self, 1);
	zip->n_segs = 0;
	zip->gap_total = 0;
	zip->hdrs_len = 0;
	if (r != ARCHIVE_OK) {	/* the archive is broken from here on (the reference's ARCHIVE_STATE_FATAL) */
		zip->failed = 1;
		zip->open = 0;
	}
	return r;
}

/* a new segment at the window's end, after making room for it and `gap` more gap bytes */
static int zipw_new_seg(struct zipw *zip, uint32_t ent, uint32_t gap, struct zipw_seg **info, la_zipc_seg **seg)
{
	if (zip->n_segs == ZIPW_MAX_SEGS || zip->gap_total + gap > ZIPW_MAX_GAP) {
		int r = zipw_flush(zip);
		if (r != ARCHIVE_OK)
			return r;
	}
	*seg = &zip->segs[zip->n_segs];
	*info = &zip->info[zip->n_segs];
	memset(*seg, 0, sizeof(**seg));
	memset(*info, 0, sizeof(**info));
	(*seg)->src_off = zip->w.len;
	(*info)->ent = ent;
	zip->n_segs++;
	zip->gap_total += gap;
	return ARCHIVE_OK;
}

/* ------------------------------------------------------------------ entries */

static int is_all_ascii(const char *p)	/* :776-786 */
{
	for (const unsigned char *pp = (const unsigned char *)p; *pp; pp++)
		if (*pp > 127)
			return 0;
	return 1;
}

static const char *unsupported_type_name(unsigned type)	/* archive_write_set_format.c:83-124 */
{
	switch (type) {
	case AE_IFLNK: return "symbolic links";
	case AE_IFCHR: return "character devices";
	case AE_IFBLK: return "block devices";
	case AE_IFIFO: return "named pipes";
	case 0140000u: return "sockets";
	default: return NULL;
	}
}

static int zipw_header(struct archive_write *a, struct archive_entry *entry)	/* :788-1319 */
{
	struct zipw *zip = a->format_data;
	uint8_t lh[30 + sizeof(entry->pathname) + 1 + 16];
	int version_needed = 10;
#define MIN_VERSION_NEEDED(x) do { if (version_needed < x) { version_needed = x; } } while (0)

	if (zip->failed)
		return ARCHIVE_FATAL;
	if (entry == NULL) {
		archive_set_error(&a->archive, ARCHIVE_ERRNO_MISC, "zip format needs an entry for every header");
		return ARCHIVE_FAILED;
	}
	/* types of entries that are not supported (:805-811; symbolic links too, here) */
	const unsigned type = archive_entry_filetype(entry);
	if (type != AE_IFREG && type != AE_IFDIR) {
		const char *name = unsupported_type_name(type);
		if (name != NULL)
			archive_set_error(&a->archive, ARCHIVE_ERRNO_FILE_FORMAT, "%s: %s format cannot archive %s", archive_entry_pathname(entry), "zip", name);
		else
			archive_set_error(&a->archive, ARCHIVE_ERRNO_FILE_FORMAT, "%s: %s format cannot archive files with mode 0%lo",
			    archive_entry_pathname(entry), "zip", (unsigned long)(type | archive_entry_perm(entry)));
		return ARCHIVE_FAILED;
	}
	const int size_set = type == AE_IFREG && archive_entry_size_is_set(entry);
	const int64_t size = size_set ? archive_entry_size(entry) : 0;	/* only regular files can have size > 0 (:830-832) */
	if (zip->flags & ZIP_FLAG_AVOID_ZIP64) {	/* :813-828 */
		if (size_set && size > ZIP_4GB_MAX) {
			archive_set_error(&a->archive, ARCHIVE_ERRNO_MISC, "Files > 4GB require Zip64 extensions");
			return ARCHIVE_FAILED;
		}
		if (zip->written_bytes + zip->w.len > (uint64_t)ZIP_4GB_MAX) {
			archive_set_error(&a->archive, ARCHIVE_ERRNO_MISC, "Archives > 4GB require Zip64 extensions");
			return ARCHIVE_FAILED;
		}
	}

	/* the name: a directory's ends in '/' (:2242-2307) */
	const char *path = archive_entry_pathname(entry);
	size_t name_len = strlen(path);
	const int add_slash = type == AE_IFDIR && (name_len == 0 || path[name_len - 1] != '/');
	unsigned entry_flags = 0;
	/* a name that is not ASCII is declared UTF-8 when that is what it is said to be (:924-935) */
	if (!is_all_ascii(path) && (zip->utf8_names || strcmp(nl_langinfo(CODESET), "UTF-8") == 0))
		entry_flags |= ZIP_ENTRY_FLAG_UTF8_NAME;

	/* method, flags and the version needed (:938-1117) */
	int method;
	if (type != AE_IFREG) {
		method = COMPRESSION_STORE;
		MIN_VERSION_NEEDED(20);
	} else {
		method = zip->requested_compression == COMPRESSION_UNSPECIFIED ? COMPRESSION_DEFLATE : zip->requested_compression;
		if (method == COMPRESSION_STORE)
			MIN_VERSION_NEEDED(10);
		else {
			switch (zip->compression_level) {	/* :990-1005, :1085-1100 */
			case 1: case 2: entry_flags |= (1 << 1) | (1 << 2); break;	/* super fast */
			case 3: case 4: entry_flags |= 1 << 2; break;			/* fast */
			case 8: case 9: entry_flags |= 1 << 1; break;			/* maximum */
			default: break;
			}
			MIN_VERSION_NEEDED(20);
		}
		if (size_set) {
			/* Zip64 when it is forced, when the file is over 4 GiB, or close to it and compressed (:1044-1049) */
			if ((zip->flags & ZIP_FLAG_FORCE_ZIP64) || size > ZIP_4GB_MAX ||
			    (size > ZIP_4GB_MAX_UNCOMPRESSED && method != COMPRESSION_STORE))
				MIN_VERSION_NEEDED(45);
		} else if ((zip->flags & ZIP_FLAG_AVOID_ZIP64) == 0)
			MIN_VERSION_NEEDED(45);	/* we might use zip64 extensions (:1063-1066) */
		entry_flags |= ZIP_ENTRY_FLAG_LENGTH_AT_END;	/* we may know the size, but never the CRC (:1051-1052, :1062) */
	}

	/* the local header (:1119-1136): CRC and sizes stay zero, the descriptor has them */
	memset(lh, 0, 30);
	memcpy(lh, "PK\003\004", 4);
	le16(lh + 4, (unsigned)version_needed);
	le16(lh + 6, entry_flags);
	le16(lh + 8, (unsigned)method);
	const uint32_t dos_time = unix_to_dos(archive_entry_mtime(entry));
	le32(lh + 10, dos_time);
	le16(lh + 26, (unsigned)(name_len + (size_t)add_slash));
	memcpy(lh + 30, path, name_len);
	if (add_slash)
		lh[30 + name_len++] = '/';
	uint8_t *x = lh + 30 + name_len, *const x0 = x;
	/* extra fields: no "ux" (:1178-1189), this slice's entries have no ids; "UT" with the mtime (:1229-1255) */
	if (archive_entry_mtime_is_set(entry)) {
		memcpy(x, "UT\005\000\001", 5);
		le32(x + 5, (uint32_t)archive_entry_mtime(entry));
		x += 9;
	}
	/* an empty Zip64 field tells readers to expect a 64-bit descriptor (:1257-1273) */
	if (size_set && size > ZIP_4GB_MAX) {
		memcpy(x, "\001\000\000\000", 4);
		x += 4;
	}
	le16(lh + 28, (unsigned)(x - x0));
	const uint32_t lh_len = (uint32_t)(x - lh);

	/* the central directory's record (:1145-1168); finished when the entry's last segment is back */
	if (zip->n_cd == zip->cap_cd) {
		const size_t cap = zip->cap_cd ? zip->cap_cd * 2 : 1024;
		struct zipw_cdent *cd = realloc(zip->cd, cap * sizeof(*cd));
		if (cd == NULL)
			return zipw_nomem(zip);
		zip->cd = cd; zip->cap_cd = cap;
	}
	struct zipw_cdent *e = &zip->cd[zip->n_cd];
	memset(e, 0, sizeof(*e));
	e->name = malloc(name_len + 1);
	if (e->name == NULL)
		return zipw_nomem(zip);
	memcpy(e->name, lh + 30, name_len);
	e->name[name_len] = '\0';
	e->name_len = (uint16_t)name_len;
	e->version = (uint16_t)version_needed; e->flags = (uint16_t)entry_flags; e->method = (uint16_t)method;
	e->dos_time = dos_time;
	e->mtime_set = archive_entry_mtime_is_set(entry); e->mtime = archive_entry_mtime(entry);
	e->ext_attr = (uint32_t)(type | archive_entry_perm(entry)) << 16;	/* following Info-Zip, the mode (:1163-1165) */

	/* the entry's first segment; the descriptor's room is counted now so that the entry's end always fits */
	struct zipw_seg *info;
	la_zipc_seg *seg;
	int r = zipw_new_seg(zip, (uint32_t)zip->n_cd, lh_len + 24u, &info, &seg);
	if (r != ARCHIVE_OK) {
		free(e->name);
		return r;
	}
	zip->n_cd++;
	if (zip->hdrs_len + lh_len > zip->hdrs_cap) {
		const size_t cap = (zip->hdrs_cap ? zip->hdrs_cap * 2 : 65536) + lh_len;
		uint8_t *h = realloc(zip->hdrs, cap);
		if (h == NULL)
			return zipw_nomem(zip);
		zip->hdrs = h; zip->hdrs_cap = cap;
	}
	memcpy(zip->hdrs + zip->hdrs_len, lh, lh_len);
	info->first = 1;
	info->lh_off = (uint32_t)zip->hdrs_len; info->lh_len = lh_len;
	zip->hdrs_len += lh_len;
	seg->gap_before = lh_len;
	seg->flags = method == COMPRESSION_STORE ? LA_ZIPC_STORE : 0;
	zip->unc_written = 0;
	if (type != AE_IFREG) {	/* a directory is over: no data, no descriptor */
		seg->flags |= LA_ZIPC_LAST;
		info->last = 1;
		zip->gap_total -= 24u;
		zip->open = 0;
		zip->limit = 0;
		return ARCHIVE_OK;
	}
	zip->open = 1;
	zip->limit = size_set ? size : INT64_MAX;	/* :836, :960 */
	return ARCHIVE_OK;
#undef MIN_VERSION_NEEDED
}

static ssize_t zipw_data(struct archive_write *a, const void *buff, size_t s)	/* :1477-1486, :1245-1301 */
{
	struct zipw *zip = a->format_data;
	const uint8_t *p = buff;
	if ((int64_t)s > zip->limit)
		s = (size_t)zip->limit;		/* bytes past the size the entry was given are ignored */
	if (s == 0 || !zip->open)
		return 0;
	zip->limit -= (int64_t)s;
	zip->unc_written += s;
	for (size_t left = s; left; ) {
		struct la_write_window *w = &zip->w;
		la_zipc_seg *seg = &zip->segs[zip->n_segs - 1];	/* the open entry's is the window's last */
		size_t n = w->cap - w->len;
		if (n > left)
			n = left;
		if (n > 0x7fffffffu - seg->src_len)
			n = 0x7fffffffu - seg->src_len;
		memcpy(w->win + w->len, p, n);
		w->len += n; seg->src_len += (uint32_t)n; p += n; left -= n;
		if (w->len == w->cap || seg->src_len == 0x7fffffffu) {
			/* the window goes; the entry goes on in the next one, its CRC32 continued from what came back */
			const uint32_t ent = zip->info[zip->n_segs - 1].ent, store = seg->flags & LA_ZIPC_STORE;
			struct zipw_seg *info;
			int r = zipw_flush(zip);
			if (r != ARCHIVE_OK)
				return r;
			if ((r = zipw_new_seg(zip, ent, 24u, &info, &seg)) != ARCHIVE_OK)
				return r;
			seg->crc_seed = zip->p_crc;
			seg->flags = store;
		}
	}
	return (ssize_t)s;
}

static int zipw_finish_entry(struct archive_write *a)	/* :1822-2052: the stream's end and the descriptor */
{
	struct zipw *zip = a->format_data;
	if (!zip->open)
		return ARCHIVE_OK;
	la_zipc_seg *seg = &zip->segs[zip->n_segs - 1];
	struct zipw_seg *info = &zip->info[zip->n_segs - 1];
	/* the 64-bit descriptor when Zip64 is forced or a size passes 4 GiB (:2033-2049).  The compressed size is not known
	 * yet: it is taken as passing when its bound does, which differs from the reference only for an entry within
	 * half a MiB of 4 GiB that does not compress. */
	const uint64_t comp_bound = (info->first ? 0 : zip->p_comp) + la_gpu_zip_compress_bound(seg->src_len, 1, ZIPW_CHUNK, 0);
	info->desc_len = ((zip->flags & ZIP_FLAG_FORCE_ZIP64) || zip->unc_written > (uint64_t)ZIP_4GB_MAX ||
	    comp_bound > (uint64_t)ZIP_4GB_MAX) ? 24 : 16;
	zip->gap_total -= 24u - info->desc_len;
	seg->gap_after = info->desc_len;
	seg->flags |= LA_ZIPC_LAST;
	info->last = 1;
	info->unc_total = zip->unc_written;
	zip->open = 0;
	return ARCHIVE_OK;
}

/* ------------------------------------------------------------------ the archive's end (:2144-2214) */

static int zipw_close(struct archive_write *a)
{
	struct zipw *zip = a->format_data;
	uint8_t buff[64];
	if (zip->w.gpu == NULL)
		return ARCHIVE_OK;	/* open failed */
	int ret = zipw_flush(zip);
	if (ret != ARCHIVE_OK)
		return ret;

	/* the central directory: file header, name, "UT" with the mtime alone, Zip64 field where a value does not fit
	 * (:2054-2139) */
	size_t cd_cap = 0;
	for (size_t i = 0; i < zip->n_cd; i++)
		cd_cap += 46u + zip->cd[i].name_len + 9u + 28u;
	uint8_t *cd = malloc(cd_cap ? cd_cap : 1), *p = cd;
	if (cd == NULL)
		return zipw_nomem(zip);
	for (size_t i = 0; i < zip->n_cd; i++) {
		const struct zipw_cdent *e = &zip->cd[i];
		uint8_t *h = p;
		unsigned version = e->version;
		memset(h, 0, 46);
		memcpy(h, "PK\001\002", 4);
		le16(h + 4, 3 * 256 + e->version);	/* "Made by PKZip 2.0 on Unix." (:1151-1152) */
		le16(h + 8, e->flags);
		le16(h + 10, e->method);
		le32(h + 12, e->dos_time);
		le32(h + 16, e->crc);
		le16(h + 28, e->name_len);
		le32(h + 38, e->ext_attr);
		memcpy(h + 46, e->name, e->name_len);
		p = h + 46 + e->name_len;
		uint8_t *const x0 = p;
		if (e->mtime_set) {
			memcpy(p, "UT\005\000\001", 5);
			le32(p + 5, (uint32_t)e->mtime);
			p += 9;
		}
		if (e->comp >= (uint64_t)ZIP_4GB_MAX || e->unc >= (uint64_t)ZIP_4GB_MAX || e->offset > (uint64_t)ZIP_4GB_MAX) {
			uint8_t *z = p;
			memcpy(z, "\001\000\000\000", 4);
			p += 4;
			if (e->unc >= (uint64_t)ZIP_4GB_MAX) { le64(p, e->unc); p += 8; }
			if (e->comp >= (uint64_t)ZIP_4GB_MAX) { le64(p, e->comp); p += 8; }
			if (e->offset >= (uint64_t)ZIP_4GB_MAX) { le64(p, e->offset); p += 8; }
			le16(z + 2, (unsigned)(p - (z + 4)));
			if (version < 45)
				version = 45;	/* Zip64 means version needs to be set to at least 4.5 */
		}
		le16(h + 6, version);
		le32(h + 20, (uint32_t)(e->comp < (uint64_t)ZIP_4GB_MAX ? e->comp : (uint64_t)ZIP_4GB_MAX));
		le32(h + 24, (uint32_t)(e->unc < (uint64_t)ZIP_4GB_MAX ? e->unc : (uint64_t)ZIP_4GB_MAX));
		le16(h + 30, (unsigned)(p - x0));
		le32(h + 42, (uint32_t)(e->offset < (uint64_t)ZIP_4GB_MAX ? e->offset : (uint64_t)ZIP_4GB_MAX));
	}
	const uint64_t offset_start = zip->written_bytes, cd_bytes = (uint64_t)(p - cd), offset_end = offset_start + cd_bytes;
	ret = __archive_write_output(a, cd, (size_t)cd_bytes);
	free(cd);
	if (ret != ARCHIVE_OK)
		return ARCHIVE_FATAL;
	zip->written_bytes = offset_end;

	/* if central dir info is too large, write Zip64 end-of-cd and its locator (:2165-2196) */
	if (cd_bytes > (uint64_t)ZIP_4GB_MAX || offset_start > (uint64_t)ZIP_4GB_MAX || zip->n_cd > 0xffffUL ||
	    (zip->flags & ZIP_FLAG_FORCE_ZIP64)) {
		memset(buff, 0, 56);
		memcpy(buff, "PK\006\006", 4);
		le64(buff + 4, 44);
		le16(buff + 12, 45);
		le16(buff + 14, 45);
		le64(buff + 24, zip->n_cd);
		le64(buff + 32, zip->n_cd);
		le64(buff + 40, cd_bytes);
		le64(buff + 48, offset_start);
		if (__archive_write_output(a, buff, 56) != ARCHIVE_OK)
			return ARCHIVE_FATAL;
		memset(buff, 0, 20);
		memcpy(buff, "PK\006\007", 4);
		le64(buff + 8, offset_end);
		le32(buff + 16, 1);
		if (__archive_write_output(a, buff, 20) != ARCHIVE_OK)
			return ARCHIVE_FATAL;
		zip->written_bytes += 76;
	}
	/* end of central directory (:2198-2212) */
	memset(buff, 0, sizeof(buff));
	memcpy(buff, "PK\005\006", 4);
	le16(buff + 8, (unsigned)(zip->n_cd < 0xffffU ? zip->n_cd : 0xffffU));
	le16(buff + 10, (unsigned)(zip->n_cd < 0xffffU ? zip->n_cd : 0xffffU));
	le32(buff + 12, (uint32_t)(cd_bytes < (uint64_t)ZIP_4GB_MAX ? cd_bytes : (uint64_t)ZIP_4GB_MAX));
	le32(buff + 16, (uint32_t)(offset_start < (uint64_t)ZIP_4GB_MAX ? offset_start : (uint64_t)ZIP_4GB_MAX));
	if (__archive_write_output(a, buff, 22) != ARCHIVE_OK)
		return ARCHIVE_FATAL;
	zip->written_bytes += 22;
	return ARCHIVE_OK;
}

static int zipw_free(struct archive_write *a)
{
	struct zipw *zip = a->format_data;
	if (zip == NULL)
		return ARCHIVE_OK;
	for (size_t i = 0; i < zip->n_cd; i++)
		free(zip->cd[i].name);
	free(zip->cd);
	free(zip->segs);
	free(zip->res);
	free(zip->info);
	free(zip->hdrs);
	if (zip->w.gpu) {
		la_gpu_sync(zip->w.gpu);
		if (zip->d_segs) la_gpu_free(zip->w.gpu, zip->d_segs);
		if (zip->d_res) la_gpu_free(zip->w.gpu, zip->d_res);
	}
	a->format_data = NULL;
	struct archive_write_filter self = zip->self;	/* (a copy: `self` lies in what is freed) */
	return la_write_window_free(&self);	/* the window, the device, and `zip` itself */
}

/* the end of archive_write_open: the device and the pinned window.  Without a gfx950 device this fails with the
 * write filters' message; there is no CPU path. */
static int zipw_init(struct archive_write *a)
{
	struct zipw *zip = a->format_data;
	return la_write_window_open(&zip->self, 1);
}

int archive_write_set_format_zip(struct archive *_a)	/* :720-774 */
{
	struct archive_write *a = (struct archive_write *)_a;
	if (a->format_free != NULL)	/* another format was already registered */
		a->format_free(a);
	struct zipw *zip = calloc(1, sizeof(*zip));
	if (zip != NULL) {
		zip->segs = calloc(ZIPW_MAX_SEGS, sizeof(*zip->segs));
		zip->res = calloc(ZIPW_MAX_SEGS, sizeof(*zip->res));
		zip->info = calloc(ZIPW_MAX_SEGS, sizeof(*zip->info));
	}
	if (zip == NULL || zip->segs == NULL || zip->res == NULL || zip->info == NULL) {
		if (zip) { free(zip->segs); free(zip->res); free(zip->info); }
		free(zip);
		archive_set_error(_a, ENOMEM, "Can't allocate zip data");
		return ARCHIVE_FATAL;
	}
	zip->a = a;
	zip->requested_compression = COMPRESSION_UNSPECIFIED;	/* "unspecified" lets us choose (:740-744) */
	zip->compression_level = 6;
	zip->w.name = "zip";
	zip->w.bound = zipw_bound;
	zip->w.compress = zipw_compress;
	zip->w.patch = zipw_patch;
	zip->self.archive = _a;
	zip->self.data = zip;
	zip->self.name = "zip";
	a->format_data = zip;
	a->format_name = "zip";
	a->format_init = zipw_init;
	a->format_options = zipw_options;
	a->format_write_header = zipw_header;
	a->format_write_data = zipw_data;
	a->format_finish_entry = zipw_finish_entry;
	a->format_close = zipw_close;
	a->format_free = zipw_free;
	_a->archive_format = ARCHIVE_FORMAT_ZIP;
	_a->archive_format_name = "ZIP";
	return ARCHIVE_OK;
}
