/* TEST INFRASTRUCTURE: libarchive_amd/csrc/la_lz4_dep_walk.h (the dependency kernel's walk by looks) compiled for the
 * CPU as it stands, under exported names, beside the one-step walk it replaces and a sweep that compares the two.
 * Built by tests/test_lz4_dep_walk_rule.py: as a shared object, and with lz4_dep_walk_main.c under the sanitizers. */
#include <stdlib.h>
#include <string.h>

#include "../../libarchive_amd/csrc/la_lz4_dep_walk.h"

uint32_t dw_cap(void) { return LA_LZ4_WALK_CAP; }
uint32_t dw_look(void) { return LA_LZ4_WALK_LOOK; }
uint32_t dw_walk(const uint16_t *pos, uint32_t q, uint32_t bound, uint32_t x) { return la_lz4_dep_walk(pos, q, bound, x); }

/* the rule as la_lz4_deps.hip had it, and as the search inside the window kernel has it */
uint32_t dw_naive(const uint16_t *pos, uint32_t q, uint32_t bound, uint32_t x)
{
	while (q + 1 < bound && pos[q + 1] <= x)
		q++;
	return q;
}

static uint32_t dw_rnd(uint64_t *s)
{
	*s = *s * 6364136223846793005ull + 1442695040888963407ull;
	return (uint32_t)(*s >> 33);
}

/* One block shape: ns ascending positions (gaps of 0 .. 2 * mean, so equal neighbours occur; with `to_end` the last
 * one is 65535 and the ones in front of it are crowded against it), `garbage` in every entry behind ns.  The array is
 * a heap block of exactly LA_LZ4_WALK_CAP + LA_LZ4_WALK_LOOK entries, what the header asks for: a read outside it is
 * the sanitizer's to report.
 *
 * Starts q and bounds: all of 0 .. ns - 1 and 0 .. ns where ns <= 64; else those within `near` of 0, of ns and of each
 * other (a walk reads nothing in front of q + 1 and nothing at or behind the bound, so what matters is the distance
 * between the two and to the array's ends), and a few in the middle.  x: for every position from q - 1 to q + near + 1
 * and the block's last three, the position itself, one below and one above; 0; 65535; values above 16 bits.
 * Returns 0 and the number of walks compared in *n_cases, or 1 with the failing case in what[0..5]. */
uint32_t dw_sweep(uint32_t ns, uint32_t to_end, uint32_t garbage, uint64_t seed, uint32_t *what, uint64_t *n_cases)
{
	const uint32_t near = 2 * LA_LZ4_WALK_LOOK + 4;
	uint16_t *pos = malloc((LA_LZ4_WALK_CAP + LA_LZ4_WALK_LOOK) * sizeof *pos);
	uint32_t *idx = malloc((4 * near + 80) * sizeof *idx);
	if (!pos || !idx || ns == 0 || ns > LA_LZ4_WALK_CAP)
		return 2;
	for (uint32_t i = 0; i < LA_LZ4_WALK_CAP + LA_LZ4_WALK_LOOK; i++)
		pos[i] = (uint16_t)garbage;
	const uint32_t mean = 65535u / ns;
	uint32_t at = 0;
	for (uint32_t i = 0; i < ns; i++) {
		at += i ? dw_rnd(&seed) % (2 * mean + 1) : dw_rnd(&seed) % 3;
		if (at > 65535u)
			at = 65535u;
		pos[i] = (uint16_t)at;
	}
	if (to_end) {	/* ascending up to 65535: the tail pushed against the end */
		uint32_t v = 65535u;
		for (uint32_t i = ns; i-- > 0 && pos[i] < v; ) {
			pos[i] = (uint16_t)v;
			v -= v ? dw_rnd(&seed) % 3 : 0;
		}
	}
	/* the starts (and, one more, the bounds) */
	uint32_t ni = 0;
	if (ns <= 64) {
		for (uint32_t i = 0; i <= ns; i++)
			idx[ni++] = i;
	} else {
		for (uint32_t i = 0; i < near; i++)
			idx[ni++] = i;
		for (uint32_t i = ns / 2; i < ns / 2 + near; i++)
			idx[ni++] = i;
		idx[ni++] = 2047; idx[ni++] = 2048;
		for (uint32_t i = ns - near; i <= ns; i++)
			idx[ni++] = i;
	}
	uint32_t rc = 0;
	for (uint32_t a = 0; a < ni && !rc; a++) {
		const uint32_t q = idx[a];
		if (q >= ns)
			continue;
		for (uint32_t bound = 0; bound <= ns && !rc; bound++) {
			if (ns > 64 && !(bound < near || bound + near > ns || (bound + near > q && bound < q + 2 * near)))
				continue;
			uint32_t xs[3 * 64 + 8], nx = 0;
			for (uint32_t j = q ? q - 1 : 0; j < ns && j <= q + near + 1; j++) {
				xs[nx++] = pos[j]; xs[nx++] = pos[j] ? pos[j] - 1u : 0u; xs[nx++] = pos[j] + 1u;
			}
			for (uint32_t j = ns > 3 ? ns - 3 : 0; j < ns; j++) {
				xs[nx++] = pos[j]; xs[nx++] = pos[j] ? pos[j] - 1u : 0u; xs[nx++] = pos[j] + 1u;
			}
			xs[nx++] = 0; xs[nx++] = 65535u; xs[nx++] = 65536u; xs[nx++] = 0x7FFFFFFFu; xs[nx++] = 0x80000000u; xs[nx++] = 0xFFFFFFFFu;
			for (uint32_t k = 0; k < nx; k++) {
				const uint32_t want = dw_naive(pos, q, bound, xs[k]), got = la_lz4_dep_walk(pos, q, bound, xs[k]);
				(*n_cases)++;
				if (want != got) {
					what[0] = ns; what[1] = q; what[2] = bound; what[3] = xs[k]; what[4] = want; what[5] = got;
					rc = 1;
					break;
				}
			}
		}
	}
	free(idx);
	free(pos);
	return rc;
}

/* every shape the test asks for: ns = 1 .. 20 and CAP - 3 .. CAP, both kinds of garbage, with and without the tail at 65535 */
uint32_t dw_sweep_all(uint32_t *what, uint64_t *n_cases)
{
	for (uint32_t pass = 0; pass < 2; pass++)
		for (uint32_t ns = pass ? LA_LZ4_WALK_CAP - 3 : 1; ns <= (pass ? LA_LZ4_WALK_CAP : 20); ns++)
			for (uint32_t v = 0; v < 4; v++) {
				const uint32_t rc = dw_sweep(ns, v & 1, (v & 2) ? 0xFFFFu : 0u, 0xD1A0000ull + ns * 4 + v, what, n_cases);
				if (rc)
					return rc;
			}
	return 0;
}
