/*
 * la_zstd_common.h -- what the zstd decoder (la_zstd.hip) and the zstd compressor (la_zstd_comp.hip) share, written
 * once from RFC 8878: XXH64 (the content checksum is its low 32 bits, 3.1.1), the FSE table spread of 4.1.1, the
 * literal-length / match-length baselines of 3.1.1.3.2.1.1 and the predefined distributions of 3.1.1.3.2.2.
 * Everything is `static`: each translation unit gets its own copy, as when it lived in la_zstd.hip.
 */
#ifndef LA_ZSTD_COMMON_H
#define LA_ZSTD_COMMON_H

#include "la_dev.h"

#define P64_1 11400714785074694791ULL
#define P64_2 14029467366897019727ULL
#define P64_3 1609587929392839161ULL
#define P64_4 9650029242287828579ULL
#define P64_5 2870177450012600261ULL
__device__ static uint64_t rotl64(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
__device__ static uint64_t rd64(const uint8_t *p) { uint64_t v; __builtin_memcpy(&v, p, 8); return v; }
__device__ static uint32_t rd32(const uint8_t *p) { uint32_t v; __builtin_memcpy(&v, p, 4); return v; }
__device__ static uint64_t xxh64_round(uint64_t acc, uint64_t in) { acc += in * P64_2; acc = rotl64(acc, 31); return acc * P64_1; }
__device__ static uint64_t xxh64_merge(uint64_t h, uint64_t v) { v = xxh64_round(0, v); h ^= v; return h * P64_1 + P64_4; }

/* XXH64 (the frame's content checksum is its low 32 bits, RFC 8878 3.1.1) */
__device__ static uint64_t dev_xxh64(const uint8_t *p, size_t len, uint64_t seed)
{
	const uint8_t *end = p + len;
	uint64_t h;
	if (len >= 32) {
		uint64_t v1 = seed + P64_1 + P64_2, v2 = seed + P64_2, v3 = seed, v4 = seed - P64_1;
		do {
			v1 = xxh64_round(v1, rd64(p)); v2 = xxh64_round(v2, rd64(p + 8));
			v3 = xxh64_round(v3, rd64(p + 16)); v4 = xxh64_round(v4, rd64(p + 24));
			p += 32;
		} while (p + 32 <= end);
		h = rotl64(v1, 1) + rotl64(v2, 7) + rotl64(v3, 12) + rotl64(v4, 18);
		h = xxh64_merge(h, v1); h = xxh64_merge(h, v2); h = xxh64_merge(h, v3); h = xxh64_merge(h, v4);
	} else {
		h = seed + P64_5;
	}
	h += (uint64_t)len;
	while (p + 8 <= end) { h ^= xxh64_round(0, rd64(p)); h = rotl64(h, 27) * P64_1 + P64_4; p += 8; }
	if (p + 4 <= end) { h ^= (uint64_t)rd32(p) * P64_1; h = rotl64(h, 23) * P64_2 + P64_3; p += 4; }
	while (p < end) { h ^= (uint64_t)(*p++) * P64_5; h = rotl64(h, 11) * P64_1; }
	h ^= h >> 33; h *= P64_2; h ^= h >> 29; h *= P64_3; h ^= h >> 32;
	return h;
}

__device__ static int highbit(uint32_t v) { int r = -1; while (v) { v >>= 1; r++; } return r; }

/* ---- FSE ---- */
typedef struct { uint8_t sym, nbits; uint16_t base; } fse_ent;
typedef struct { fse_ent e[512]; int al; } fse_tab;

__device__ static int fse_build(fse_tab *t, const int16_t *norm, int n_sym, int al)
{
	const int size = 1 << al;
	uint16_t next[256];
	int high = size - 1;
	t->al = al;
	for (int s = 0; s < n_sym; s++) {
		if (norm[s] == -1) { t->e[high--].sym = (uint8_t)s; next[s] = 1; }
		else next[s] = (uint16_t)norm[s];
	}
	const int step = (size >> 1) + (size >> 3) + 3, mask = size - 1;
	int pos = 0;
	for (int s = 0; s < n_sym; s++)
		for (int i = 0; i < norm[s]; i++) {
			t->e[pos].sym = (uint8_t)s;
			do { pos = (pos + step) & mask; } while (pos > high);
		}
	if (pos != 0) return -1;
	for (int u = 0; u < size; u++) {
		const int s = t->e[u].sym;
		const int nx = next[s]++;
		const int nb = al - highbit((uint32_t)nx);
		t->e[u].nbits = (uint8_t)nb;
		t->e[u].base = (uint16_t)((nx << nb) - size);
	}
	return 0;
}

/* literal-length and match-length codes: baselines and extra bits (RFC 8878 3.1.1.3.2.1.1) */
struct seq_tabs { uint32_t ll_base[36]; uint32_t ml_base[53]; uint8_t ll_bits[36]; uint8_t ml_bits[53]; };
__device__ static const seq_tabs SEQ_TABS = {
	{ 0,1,2,3,4,5,6,7,8,9,10,11,12,13,14,15,16,18,20,22,24,28,32,40,48,64,128,256,512,1024,2048,4096,8192,16384,32768,65536 },
	{ 3,4,5,6,7,8,9,10,11,12,13,14,15,16,17,18,19,20,21,22,23,24,25,26,27,28,29,30,31,32,33,34,35,37,39,41,43,47,51,59,67,83,99,131,259,515,1027,2051,4099,8195,16387,32771,65539 },
	{ 0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,1,1,1,1,2,2,3,3,4,6,7,8,9,10,11,12,13,14,15,16 },
	{ 0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,1,1,1,1,2,2,3,3,4,4,5,7,8,9,10,11,12,13,14,15,16 }
};
__device__ static const int16_t LL_DEF[36] = { 4,3,2,2,2,2,2,2,2,2,2,2,2,1,1,1,2,2,2,2,2,2,2,2,2,3,2,1,1,1,1,1,-1,-1,-1,-1 };
__device__ static const int16_t ML_DEF[53] = { 1,4,3,2,2,2,2,2,2,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,-1,-1,-1,-1,-1,-1,-1 };
__device__ static const int16_t OF_DEF[29] = { 1,1,1,1,1,1,2,2,2,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,-1,-1,-1,-1,-1 };

#endif /* LA_ZSTD_COMMON_H */
