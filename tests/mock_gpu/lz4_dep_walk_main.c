/* TEST INFRASTRUCTURE: a stand-alone program around lz4_dep_walk_shim.c, built by tests/test_lz4_dep_walk_rule.py with
 * -fsanitize=address,undefined: the sweep's position arrays are heap blocks of exactly the size the header asks for
 * (the positions and one look's entries behind them), so a look that read outside it would end the program.  Prints
 * the number of walks compared. */
#include <stdint.h>
#include <stdio.h>

uint32_t dw_sweep_all(uint32_t *what, uint64_t *n_cases);

int main(void)
{
	uint32_t what[8] = { 0 };
	uint64_t n = 0;
	const uint32_t rc = dw_sweep_all(what, &n);
	if (rc) {
		fprintf(stderr, "walk differs: rc %u ns %u q %u bound %u x %u: one-step walk %u, by looks %u\n", rc, what[0], what[1],
		    what[2], what[3], what[4], what[5]);
		return 1;
	}
	printf("%llu\n", (unsigned long long)n);
	return 0;
}
