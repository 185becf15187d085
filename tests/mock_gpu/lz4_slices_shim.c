/* TEST INFRASTRUCTURE: libarchive_amd/csrc/la_lz4_slices.h (the schedule of a split last expand slice) compiled for the
 * CPU as it stands, its inline functions under exported names.  Built by tests/test_lz4_slice_rule.py. */
#include "../../libarchive_amd/csrc/la_lz4_slices.h"

uint32_t sl_period(uint32_t n_blocks, uint32_t n_frames) { return la_lz4_split_period(n_blocks, n_frames); }
void sl_init(la_lz4_split *sp, uint32_t first, uint32_t last, uint32_t period, const uint32_t *sixteenths, uint32_t n)
{
	la_lz4_split_init(sp, first, last, period, sixteenths, n);
}
uint32_t sl_group_blocks(const la_lz4_split *sp, uint32_t g) { return la_lz4_split_group_blocks(sp, g); }
uint32_t sl_grid_x(const la_lz4_split *sp, uint32_t g) { return la_lz4_split_grid_x(sp, g); }
uint32_t sl_grid_y(const la_lz4_split *sp, uint32_t g) { return la_lz4_split_grid_y(sp, g); }
uint32_t sl_block(uint32_t base, uint32_t period, uint32_t x, uint32_t y) { return la_lz4_split_block(base, period, x, y); }
uint32_t sl_ready(uint32_t first, uint32_t period, uint32_t h, uint32_t fb, uint32_t nb)
{
	return la_lz4_split_ready(first, period, h, fb, nb);
}
uint32_t sl_pass_lo(uint32_t first, uint32_t period, uint32_t h_lo, uint32_t fb, uint32_t nb)
{
	return la_lz4_split_pass_lo(first, period, h_lo, fb, nb);
}
uint32_t sl_carry_index(uint32_t first, uint32_t fb, uint32_t nb) { return la_lz4_split_carry_index(first, fb, nb); }
uint32_t sl_max_groups(void) { return LA_LZ4_SPLIT_MAX_GROUPS; }

/* ---- the exhaustive check of one period, against a model that marks blocks group by group ----
 * Every set of up to LA_LZ4_SPLIT_MAX_GROUPS bounds, every offset of `first` inside the period, `layouts` random frame
 * layouts each: frames of 0 .. 3 P + 1 blocks, the first ones in front of `first`, one ending exactly at `first`, one
 * straddling it.  Returns 0, or the number of the check that failed with the case in what[0..7]. */
static uint32_t sl_rnd(uint64_t *s)
{
	*s = *s * 6364136223846793005ull + 1442695040888963407ull;
	return (uint32_t)(*s >> 33);
}

#define SL_MAXB 2048
#define SL_MAXF 64
#define SL_FAIL(code) do { what[0] = P; what[1] = mask; what[2] = off; what[3] = lay; what[4] = g; what[5] = f; return (code); } while (0)

uint32_t sl_check_period(uint32_t P, uint64_t seed, uint32_t layouts, uint32_t *what, uint64_t *n_cases)
{
	static uint8_t group_of[SL_MAXB], seen[SL_MAXB], carry_used[SL_MAXB];
	uint32_t fb[SL_MAXF], nb[SL_MAXF];
	uint32_t g = 0, f = 0, lay = 0, off = 0;
	for (uint32_t mask = 0; mask < (1u << (P - 1)); mask++) {
		if (__builtin_popcount(mask) > (int)LA_LZ4_SPLIT_MAX_GROUPS - 1)
			continue;
		la_lz4_split sp;
		sp.period = P;
		sp.n_groups = 0;
		sp.bound[0] = 0;
		for (uint32_t h = 1; h < P; h++)
			if (mask & (1u << (h - 1)))
				sp.bound[++sp.n_groups] = h;
		sp.bound[++sp.n_groups] = P;
		for (off = 0; off < P; off++)
			for (lay = 0; lay < layouts; lay++) {
				const uint32_t first = 3 * P + off;
				/* the layout: frames in a row from somewhere in front of `first` */
				uint32_t nf = 0, at = first - sl_rnd(&seed) % (2 * P + 1);
				if (at < first) {	/* one frame that ends exactly at `first`, then one that straddles what follows */
					fb[nf] = at; nb[nf] = (first - at) / 2; at += nb[nf++];
					fb[nf] = at; nb[nf] = first - at; at += nb[nf++];
				}
				const uint32_t want = 2 + sl_rnd(&seed) % 6;
				while (nf < want + 2 && nf < SL_MAXF) {
					const uint32_t r = sl_rnd(&seed) % 8;
					fb[nf] = at;
					nb[nf] = r == 0 ? 0 : r == 1 ? P : r == 2 ? 3 * P + 1 : sl_rnd(&seed) % (3 * P + 2);
					if (nf == 2 && at == first && lay % 2)	/* a frame that starts below first and straddles it */
						{ fb[nf] = first - 1 - sl_rnd(&seed) % P; nb[nf] += first - fb[nf]; }
					at = fb[nf] + nb[nf];
					nf++;
				}
				const uint32_t last = at > first ? at : first;
				if (last >= SL_MAXB) SL_FAIL(99);
				sp.first = first;
				sp.last = last;
				(*n_cases)++;
				/* the model */
				for (uint32_t i = first; i < last; i++) {
					const uint32_t r = (i - first) % P;
					uint32_t k = 0;
					while (!(sp.bound[k] <= r && r < sp.bound[k + 1])) k++;
					group_of[i] = (uint8_t)k;
					seen[i] = 0;
					carry_used[i - first] = 0;
				}
				/* 1: the groups partition [first, last), the grids hold exactly the groups */
				uint32_t total = 0;
				for (g = 0; g < sp.n_groups; g++) {
					uint32_t model = 0, hit = 0;
					for (uint32_t i = first; i < last; i++) model += group_of[i] == g;
					if (la_lz4_split_group_blocks(&sp, g) != model) SL_FAIL(1);
					total += model;
					const uint32_t gx = la_lz4_split_grid_x(&sp, g), gy = la_lz4_split_grid_y(&sp, g);
					if (gy != sp.bound[g + 1] - sp.bound[g]) SL_FAIL(2);
					for (uint32_t x = 0; x < gx; x++)
						for (uint32_t y = 0; y < gy; y++) {
							const uint32_t bi = la_lz4_split_block(first + sp.bound[g], P, x, y);
							if (bi < first) SL_FAIL(3);
							if (bi >= last) continue;	/* leaves at the kernel's test */
							if (group_of[bi] != g || seen[bi]) SL_FAIL(4);
							seen[bi] = 1;
							hit++;
						}
					if (hit != model) SL_FAIL(5);
					/* no period without a block of the group at the grid's end */
					if (gx && la_lz4_split_block(first + sp.bound[g], P, gx - 1, 0) >= last) SL_FAIL(6);
					if (!gx && model) SL_FAIL(7);
				}
				if (total != last - first) SL_FAIL(8);
				/* 2 .. 5: the passes of every frame that ends in the slice */
				for (f = 0; f < nf; f++) {
					const uint32_t end = fb[f] + nb[f];
					if (nb[f] == 0 || end <= first)
						continue;
					uint32_t pos = 0;
					for (g = 0; g < sp.n_groups; g++) {
						const uint32_t lo = la_lz4_split_pass_lo(first, P, sp.bound[g], fb[f], nb[f]);
						const uint32_t hi = la_lz4_split_ready(first, P, sp.bound[g + 1], fb[f], nb[f]);
						if (lo != pos || hi < lo || hi > nb[f]) SL_FAIL(10);	/* once, in order */
						for (uint32_t k = lo; k < hi; k++)
							if (fb[f] + k >= first && group_of[fb[f] + k] > g) SL_FAIL(11);	/* nothing outside groups 0 .. g */
						if (hi < nb[f] && !(fb[f] + hi >= first && group_of[fb[f] + hi] > g)) SL_FAIL(12);	/* the whole run */
						pos = hi;
					}
					if (pos != nb[f]) SL_FAIL(13);
					const uint32_t ci = la_lz4_split_carry_index(first, fb[f], nb[f]);
					if (ci >= last - first || carry_used[ci]) SL_FAIL(14);
					carry_used[ci] = 1;
				}
			}
	}
	return 0;
}
