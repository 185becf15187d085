/*
 * uu_rules_bench.c -- TEST INFRASTRUCTURE: libarchive_amd/csrc/la_uu_dev.h walked line by line on ONE host core (the
 * stand-in's walk, la_gpu_uu_mock.c), the baseline of tools/measure_uu.py.  It is NOT the reference's filter.
 *
 *   uu_rules_bench FILE REPS     FILE: a uuencoded or base64 stream; prints "decoded_bytes seconds" of the best of REPS
 *                                passes over the whole file as one final window
 */
#include "../../include/la_gpu.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

void la_uu_rules_walk(const uint8_t *src, uint64_t n, int final, la_uu_state in, uint8_t *dst, la_uu_result *r);

int main(int argc, char **argv)
{
	if (argc < 3) return 2;
	FILE *f = fopen(argv[1], "rb");
	if (!f) { perror(argv[1]); return 2; }
	fseek(f, 0, SEEK_END);
	const long n = ftell(f);
	fseek(f, 0, SEEK_SET);
	uint8_t *img = malloc((size_t)n + 1), *dst = malloc((size_t)n + 1);
	if (!img || !dst || fread(img, 1, (size_t)n, f) != (size_t)n) return 2;
	fclose(f);
	double best = 1e30;
	la_uu_result r;
	memset(&r, 0, sizeof(r));
	for (int rep = 0; rep < atoi(argv[2]); rep++) {
		struct timespec t0, t1;
		const la_uu_state in = { LA_UU_FIND_HEAD, 0 };
		clock_gettime(CLOCK_MONOTONIC, &t0);
		la_uu_rules_walk(img, (uint64_t)n, 1, in, dst, &r);
		clock_gettime(CLOCK_MONOTONIC, &t1);
		if (r.status != LA_ST_OK) { fprintf(stderr, "status %u at %llu\n", r.status, (unsigned long long)r.stop_off); return 1; }
		const double s = (double)(t1.tv_sec - t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - t0.tv_nsec);
		if (s < best) best = s;
	}
	printf("%llu %.6f\n", (unsigned long long)r.out_len, best);
	free(dst); free(img);
	return 0;
}
