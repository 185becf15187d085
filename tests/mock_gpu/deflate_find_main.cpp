/* TEST INFRASTRUCTURE: a program of its own for the sanitizers.  Runs the candidate rule (la_deflate_find_dev.h, through
 * deflate_find_shim.cpp) over every bit of every file named on the command line, each in a heap buffer of exactly the
 * file's size, and prints per file: bytes, positions that pass the quick test, candidates, and the sum of the candidate
 * positions.  Not part of the product. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

extern "C" uint64_t deflate_find_scan(const uint8_t *data, uint64_t len, uint8_t *out);

int main(int argc, char **argv)
{
	for (int a = 1; a < argc; a++) {
		FILE *f = fopen(argv[a], "rb");
		if (!f) { perror(argv[a]); return 2; }
		fseek(f, 0, SEEK_END);
		const long size = ftell(f);
		fseek(f, 0, SEEK_SET);
		uint8_t *data = (uint8_t *)malloc(size ? (size_t)size : 1), *out = (uint8_t *)malloc(size ? 8 * (size_t)size : 1);
		if (!data || !out || fread(data, 1, (size_t)size, f) != (size_t)size) { fprintf(stderr, "%s: read failed\n", argv[a]); return 2; }
		fclose(f);
		const uint64_t n = deflate_find_scan(data, (uint64_t)size, out);
		uint64_t quick = 0, sum = 0;
		for (uint64_t p = 0; p < 8 * (uint64_t)size; p++) {
			quick += out[p] & 1u;
			if (out[p] & 2u) {
				sum += p;
				if (!(out[p] & 1u)) { fprintf(stderr, "%s: bit %llu is a candidate the quick test refuses\n", argv[a], (unsigned long long)p); return 1; }
			}
		}
		printf("%ld %llu %llu %llu\n", size, (unsigned long long)quick, (unsigned long long)n, (unsigned long long)sum);
		free(data);
		free(out);
	}
	return 0;
}
