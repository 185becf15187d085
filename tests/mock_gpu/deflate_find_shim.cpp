/* TEST INFRASTRUCTURE: the candidate rule of the finder kernels (libarchive_amd/csrc/la_deflate_find_dev.h) compiled for the
 * host, for tests/test_deflate_find_rules.py and the CPU stand-in of LA_GZ_OPT_BLOCK_STARTS.  Not part of the product. */
#include <stdint.h>
#include <string.h>
#include "../../libarchive_amd/csrc/la_deflate_find_dev.h"

/* the bits [p, p + n) of data[0 .. len), n <= 64, bits behind the end read as 0: what the quick kernel stages */
static uint64_t bits_at(const uint8_t *data, uint64_t len, uint64_t p, uint32_t n)
{
	uint64_t v = 0;
	for (uint32_t k = 0; k < n; k++) {
		const uint64_t q = p + k;
		if ((q >> 3) < len && ((data[q >> 3] >> (q & 7)) & 1))
			v |= 1ull << k;
	}
	return v;
}

extern "C" int deflate_find_quick(const uint8_t *data, uint64_t len, uint64_t p)
{
	const uint32_t need = dfl_find_quick((uint32_t)bits_at(data, len, p, 17), bits_at(data, len, p + 17, 57));
	return need != 0 && p + need <= 8 * len;
}

extern "C" int deflate_find_full(const uint8_t *data, uint64_t len, uint64_t p)
{
	return dfl_find_full(data, p, 8 * len) ? 1 : 0;
}

/* out[p] = 1 (quick) | 2 (full) for every bit position of data; returns the number of full candidates */
extern "C" uint64_t deflate_find_scan(const uint8_t *data, uint64_t len, uint8_t *out)
{
	uint64_t n = 0;
	for (uint64_t p = 0; p < 8 * len; p++) {
		const int q = deflate_find_quick(data, len, p), f = deflate_find_full(data, len, p);
		out[p] = (uint8_t)(q | (f << 1));
		n += (uint64_t)f;
	}
	return n;
}
