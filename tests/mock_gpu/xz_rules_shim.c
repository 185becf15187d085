/*
 * xz_rules_shim.c -- TEST INFRASTRUCTURE: libarchive_amd/csrc/la_xz_filters_dev.h compiled for the host, for
 * tests/test_xz_unfilter_rules.py.  rules_serial is the header's whole-buffer routine.  rules_parallel runs the
 * formulation of the kernels (la_xz_filters.hip) with the header's pieces, in the kernels' phases, the independent
 * pieces of a phase in DESCENDING order: what a piece reads must not depend on a piece that ran before it.
 *   delta  tiles of `tile` bytes, the rows of a tile in `parts` groups: column sums per tile, exclusive scan over the
 *          tiles, apply with the scanned carry plus the groups in front
 *   x86    the first head of every `sub` bytes from the undecoded bytes, then a walk from each to the first head at or
 *          behind the end of its `sub` bytes
 *   map    one unit at a time
 */
#include <stdlib.h>
#include <string.h>

#include "../../libarchive_amd/csrc/la_xz_filters_dev.h"

void rules_serial(uint32_t id, uint32_t prop, uint8_t *buf, uint64_t n)
{
	la_xz_unfilter_serial(id, prop, buf, n);
}

int rules_valid(uint32_t id, uint32_t prop)
{
	return la_xz_filter_valid(id, prop);
}

int rules_parallel(uint32_t id, uint32_t prop, uint8_t *buf, uint64_t n, uint64_t tile, uint64_t sub, uint32_t parts)
{
	if (id == LA_XZF_DELTA) {
		const uint32_t dist = prop;
		const uint64_t tiles = (n + tile - 1) / tile;
		uint8_t *sums = calloc(tiles ? tiles : 1, 256);
		uint8_t *part = malloc((size_t)parts * 256);
		if (!sums || !part)
			return -1;
		for (uint64_t t = tiles; t-- > 0;) {
			const uint64_t lo = t * tile, hi = lo + tile < n ? lo + tile : n;
			for (uint32_t c = 0; c < dist; c++)
				sums[t * 256 + c] = (uint8_t)la_xz_delta_col_sum(buf, 0, lo, hi, dist, c, 0, la_xz_delta_rows(lo, hi, dist));
		}
		for (uint32_t c = 0; c < dist; c++) {
			uint32_t acc = 0;
			for (uint64_t t = 0; t < tiles; t++) {
				const uint32_t s = sums[t * 256 + c];
				sums[t * 256 + c] = (uint8_t)acc;
				acc += s;
			}
		}
		for (uint64_t t = tiles; t-- > 0;) {
			const uint64_t lo = t * tile, hi = lo + tile < n ? lo + tile : n;
			const uint64_t rows = la_xz_delta_rows(lo, hi, dist), per = (rows + parts - 1) / parts;
			for (uint32_t s = 0; s < parts; s++)
				for (uint32_t c = 0; c < dist; c++)
					part[s * 256 + c] = (uint8_t)la_xz_delta_col_sum(buf, 0, lo, hi, dist, c, s * per, (s + 1) * per < rows ? (s + 1) * per : rows);
			for (uint32_t s = parts; s-- > 0;)
				for (uint32_t c = dist; c-- > 0;) {
					uint32_t carry = sums[t * 256 + c];
					for (uint32_t q = 0; q < s; q++)
						carry += part[q * 256 + c];
					if (s * per < rows)
						la_xz_delta_col_apply(buf, 0, lo, hi, dist, c, s * per, (s + 1) * per < rows ? (s + 1) * per : rows, carry & 0xFF);
				}
		}
		free(sums);
		free(part);
	} else if (id == LA_XZF_X86) {
		const uint64_t subs = (n + sub - 1) / sub;
		uint64_t *head = malloc(sizeof(uint64_t) * (subs ? subs : 1));
		if (!head)
			return -1;
		for (uint64_t k = subs; k-- > 0;)
			head[k] = la_xz_x86_first_head(buf, n, k * sub, (k + 1) * sub < n ? (k + 1) * sub : n);
		for (uint64_t k = subs; k-- > 0;)
			if (head[k] < n)
				la_xz_x86_walk(buf, n, prop, head[k], (k + 1) * sub);
		free(head);
	} else {
		const uint32_t ub = la_xz_unit_bytes(id), us = la_xz_unit_stride(id);
		if (ub == 0 || n < ub)
			return 0;
		for (uint64_t i = (n - ub) / us * us + us; i >= us; i -= us)
			la_xz_unit(id, buf, i - us, prop);
	}
	return 0;
}
