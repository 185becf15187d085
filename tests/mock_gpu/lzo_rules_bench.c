/*
 * lzo_rules_bench.c -- TEST INFRASTRUCTURE: libarchive_amd/csrc/la_lzo_dev.h with its plain hooks on ONE host core,
 * the baseline of tools/measure_lzop.py.  It is NOT liblzo2.
 *
 *   lzo_rules_bench FILE REPS     FILE: [u32 n] then n x [u32 src_len][u32 dst_len][src bytes]; prints
 *                                 "bytes seconds" of the best of REPS passes over all blocks
 */
#include "../../include/la_gpu.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "../../libarchive_amd/csrc/la_lzo_dev.h"

int main(int argc, char **argv)
{
	if (argc < 3) return 2;
	FILE *f = fopen(argv[1], "rb");
	if (!f) { perror(argv[1]); return 2; }
	fseek(f, 0, SEEK_END);
	const long n = ftell(f);
	fseek(f, 0, SEEK_SET);
	uint8_t *img = malloc((size_t)n + 1);
	if (!img || fread(img, 1, (size_t)n, f) != (size_t)n) return 2;
	fclose(f);
	uint32_t nb, max_dst = 0;
	memcpy(&nb, img, 4);
	size_t at = 4;
	for (uint32_t i = 0; i < nb; i++) {
		uint32_t sl, dl;
		memcpy(&sl, img + at, 4); memcpy(&dl, img + at + 4, 4);
		if (dl > max_dst) max_dst = dl;
		at += 8 + sl;
	}
	uint8_t *dst = malloc(max_dst + 1);
	if (!dst) return 2;
	double best = 1e30;
	unsigned long long total = 0;
	for (int rep = 0; rep < atoi(argv[2]); rep++) {
		struct timespec t0, t1;
		clock_gettime(CLOCK_MONOTONIC, &t0);
		total = 0;
		at = 4;
		for (uint32_t i = 0; i < nb; i++) {
			uint32_t sl, dl, out_len, consumed;
			memcpy(&sl, img + at, 4); memcpy(&dl, img + at + 4, 4);
			la_lzo_io io = { img + at + 8, dst };
			if (sl == dl)
				memcpy(dst, img + at + 8, sl);
			else if (la_lzo1x_decode(&io, sl, dl, &out_len, &consumed) != LA_ST_OK) { fprintf(stderr, "block %u failed\n", i); return 1; }
			total += dl;
			at += 8 + sl;
		}
		clock_gettime(CLOCK_MONOTONIC, &t1);
		const double s = (double)(t1.tv_sec - t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - t0.tv_nsec);
		if (s < best) best = s;
	}
	printf("%llu %.6f\n", total, best);
	free(dst); free(img);
	return 0;
}
