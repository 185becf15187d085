/*
 * la_inflate_chain.hip -- the second step of LA_GZ_OPT_CHAIN (gfx950): the pieces of ONE raw-deflate stream whose
 * matches reach back over their flush points (zlib's Z_SYNC_FLUSH, pigz without -i), built from the source pointers
 * the emit instance of the wave kernel left (la_inflate.hip).
 *
 * What is there when these kernels start.  The packed range is T bytes from the first piece's dst_off; byte i of it
 * has the chain coordinate e = hist_len + i, the hist_len bytes in front of the range have the coordinates below
 * hist_len.  out[i] holds the byte itself where it was a literal or stored, and ptr[i] holds a coordinate:
 *   ptr[i] == e   a ROOT: the byte is there (literal, stored);
 *   ptr[i] <  e   the byte is a copy of the byte at that coordinate (a match named it), which may be a copy again.
 * Coordinates below hist_len are roots too (the caller's bytes), and they have no entry in the table.
 *
 * Pointer jumping.  A pass replaces ptr[i] = p by ptr[p] wherever p is not a root, so the distance a pointer spans
 * doubles per pass: 32 passes resolve any chain inside a 4 GiB range (la_api.hip refuses a longer one).  The passes
 * are launched back to back on the stream; a pass raises its flag when it changed a pointer, and the pass behind it
 * returns at once when that flag is down: no host round trip, no waiting inside a launch, no spin.
 *
 * Why the update in place is safe, with other workgroups writing the table in the same pass and an L1 that may show
 * an older value of a word.  Every value ptr[x] ever holds is an ANCESTOR of x -- the byte at that coordinate is the
 * byte x has to become: true of what the emit pass wrote, and replacing an ancestor p by an ancestor of p keeps it
 * true.  So a read of ptr[p] that returns an older value still returns an ancestor of p, hence of i: the pass stores
 * a correct, merely less advanced, pointer.  A root never changes (ptr[p] == p is stored once, by the emit pass, and
 * no pass touches an entry whose pointer is a root or itself), and a non-root never looks like one (its values are
 * all below its own coordinate), so "is p a root" cannot be misread either.  Words are aligned 32-bit loads and
 * stores, which are not torn.  A pass that changed nothing found every pointer on a root: the table is resolved.
 *
 * The gather then copies out[i] = byte at ptr[i] for the non-roots: it reads only roots and writes only non-roots,
 * so no byte is both read and written in that launch.
 *
 * Per packed output byte, from this code: each jump pass that runs reads 4 B (ptr[i]) and, for a non-root pointer,
 * 4 B more (ptr[p]) and writes at most 4 B; the gather reads 4 B of pointer and, for a non-root, reads 1 B and writes
 * 1 B.  The emit pass in front wrote 4 B of pointer per byte and 1 B per literal / stored byte.
 */
#include "la_dev.h"

#define CHAIN_TPB 256

__global__ __launch_bounds__(CHAIN_TPB) void chain_lengths_kernel(const la_gz_result *__restrict__ results, uint32_t n,
    uint32_t *__restrict__ len)
{
	const uint32_t i = blockIdx.x * CHAIN_TPB + threadIdx.x;
	if (i < n)
		len[i] = results[i].out_len;
}

void la_launch_chain_lengths(hipStream_t s, const la_gz_result *d_results, uint32_t n, uint32_t *d_len)
{
	if (n == 0) return;
	hipLaunchKernelGGL(chain_lengths_kernel, dim3((n + CHAIN_TPB - 1) / CHAIN_TPB), dim3(CHAIN_TPB), 0, s, d_results, n, d_len);
}

/* the member table with the packed places, for the CRC32 launch; and T, the end of the last piece that fits: the
 * scan is monotone, so that is the largest of its values not above dst_cap (ctl[32] was zeroed by the launcher) */
__global__ __launch_bounds__(CHAIN_TPB) void chain_pack_kernel(const la_gz_member *__restrict__ members, uint32_t n,
    const uint64_t *__restrict__ packed_off, uint64_t dst_cap, la_gz_member *__restrict__ packed, uint32_t *ctl)
{
	const uint32_t i = blockIdx.x * CHAIN_TPB + threadIdx.x;
	if (i > n)
		return;
	const uint64_t at = packed_off[i];
	if (at <= dst_cap)
		atomicMax(&ctl[LA_CHAIN_JUMP_PASSES], (uint32_t)at);
	if (i < n) {
		la_gz_member m = members[i];
		m.dst_off = members[0].dst_off + at;
		packed[i] = m;
	}
}

/* one pass of ptr[i] = ptr[ptr[i]]; pass 0 always runs, pass k > 0 only when pass k - 1 changed something */
__global__ __launch_bounds__(CHAIN_TPB) void chain_jump_kernel(uint32_t *ptr, uint32_t hist_len, uint32_t *ctl, uint32_t pass)
{
	if (pass != 0 && ctl[pass - 1] == 0)
		return;
	const uint32_t total = ctl[LA_CHAIN_JUMP_PASSES];
	const uint32_t stride = gridDim.x * CHAIN_TPB;
	uint32_t changed = 0;
	for (uint64_t k = blockIdx.x * CHAIN_TPB + threadIdx.x; k < total; k += stride) {
		const uint32_t i = (uint32_t)k, e = hist_len + i;
		const uint32_t p = ptr[i];
		if (p >= e || p < hist_len)	/* a root itself, or a copy of a byte of the history */
			continue;
		const uint32_t q = ptr[p - hist_len];
		if (q < p) {
			ptr[i] = q;
			changed = 1;
		}
	}
	if (__any(changed) && (threadIdx.x & 63) == 0)
		atomicOr(&ctl[pass], 1u);
}

__global__ __launch_bounds__(CHAIN_TPB) void chain_gather_kernel(const uint32_t *__restrict__ ptr, uint32_t hist_len,
    const uint32_t *__restrict__ ctl, const uint64_t *__restrict__ first_off, uint8_t *dst)
{
	/* the byte of coordinate 0; first_off: where the range starts in dst (the first piece's dst_off on the device), NULL = at dst */
	uint8_t *chain = dst + (first_off ? *first_off : 0) - hist_len;
	const uint32_t total = ctl[LA_CHAIN_JUMP_PASSES];
	const uint32_t stride = gridDim.x * CHAIN_TPB;
	for (uint64_t k = blockIdx.x * CHAIN_TPB + threadIdx.x; k < total; k += stride) {
		const uint32_t i = (uint32_t)k, e = hist_len + i;
		const uint32_t p = ptr[i];
		if (p < e)
			chain[e] = chain[p];
	}
}

void la_launch_chain_resolve(hipStream_t s, const la_gz_member *d_members, const la_gz_result *d_results, uint32_t n,
    uint8_t *d_dst, uint64_t dst_cap, const la_inflate_chain &C, la_gz_member *d_packed, uint32_t *d_ctl)
{
	(void)d_results;
	if (n == 0) return;
	(void)hipMemsetAsync(d_ctl, 0, LA_CHAIN_CTL_WORDS * sizeof(uint32_t), s);
	hipLaunchKernelGGL(chain_pack_kernel, dim3(n / CHAIN_TPB + 1), dim3(CHAIN_TPB), 0, s, d_members, n, C.packed_off,
	    dst_cap, d_packed, d_ctl);
	/* grid-stride over a range whose length only the device knows: sized by the capacity, 4 entries per thread */
	uint64_t blocks = (dst_cap + 4 * CHAIN_TPB - 1) / (4 * CHAIN_TPB);
	if (blocks < 1) blocks = 1;
	if (blocks > 4096) blocks = 4096;
	for (uint32_t pass = 0; pass < LA_CHAIN_JUMP_PASSES; pass++)
		hipLaunchKernelGGL(chain_jump_kernel, dim3((uint32_t)blocks), dim3(CHAIN_TPB), 0, s, C.ptr, C.hist_len, d_ctl, pass);
	hipLaunchKernelGGL(chain_gather_kernel, dim3((uint32_t)blocks), dim3(CHAIN_TPB), 0, s, C.ptr, C.hist_len, d_ctl,
	    &d_members->dst_off, d_dst);
}

/* the length of the packed range from the device (LA_GZ_OPT_BLOCK_STARTS: the end of the scan over the confirmed pieces);
 * a value above the capacity -- there is none: the walk stops in front of the piece that would pass it -- resolves nothing */
__global__ void chain_total_dev_kernel(uint32_t *ctl, const uint64_t *total, uint64_t dst_cap)
{
	ctl[LA_CHAIN_JUMP_PASSES] = *total <= dst_cap ? (uint32_t)*total : 0u;
}

void la_launch_chain_resolve_dev(hipStream_t s, uint8_t *d_dst, const uint64_t *d_first_off, uint32_t *d_ptr, uint32_t hist_len,
    const uint64_t *d_total, uint64_t dst_cap, uint32_t *d_ctl)
{
	(void)hipMemsetAsync(d_ctl, 0, LA_CHAIN_CTL_WORDS * sizeof(uint32_t), s);
	hipLaunchKernelGGL(chain_total_dev_kernel, dim3(1), dim3(1), 0, s, d_ctl, d_total, dst_cap);
	uint64_t blocks = (dst_cap + 4 * CHAIN_TPB - 1) / (4 * CHAIN_TPB);
	if (blocks < 1) blocks = 1;
	if (blocks > 4096) blocks = 4096;
	for (uint32_t pass = 0; pass < LA_CHAIN_JUMP_PASSES; pass++)
		hipLaunchKernelGGL(chain_jump_kernel, dim3((uint32_t)blocks), dim3(CHAIN_TPB), 0, s, d_ptr, hist_len, d_ctl, pass);
	hipLaunchKernelGGL(chain_gather_kernel, dim3((uint32_t)blocks), dim3(CHAIN_TPB), 0, s, d_ptr, hist_len, d_ctl, d_first_off, d_dst);
}

__global__ void chain_total_kernel(uint32_t *ctl, uint32_t total) { ctl[LA_CHAIN_JUMP_PASSES] = total; }

/* the jump passes and the gather for a caller that has the pointers of d_dst[0, total) in d_ptr (coordinate = index,
 * no history): the block path of the zstd decoder (la_zstd_blocks.hip) */
void la_launch_chain_resolve_range(hipStream_t s, uint8_t *d_dst, uint32_t *d_ptr, uint32_t total, uint32_t *d_ctl)
{
	if (total == 0) return;
	(void)hipMemsetAsync(d_ctl, 0, LA_CHAIN_CTL_WORDS * sizeof(uint32_t), s);
	hipLaunchKernelGGL(chain_total_kernel, dim3(1), dim3(1), 0, s, d_ctl, total);
	uint64_t blocks = ((uint64_t)total + 4 * CHAIN_TPB - 1) / (4 * CHAIN_TPB);
	if (blocks > 4096) blocks = 4096;
	for (uint32_t pass = 0; pass < LA_CHAIN_JUMP_PASSES; pass++)
		hipLaunchKernelGGL(chain_jump_kernel, dim3((uint32_t)blocks), dim3(CHAIN_TPB), 0, s, d_ptr, 0u, d_ctl, pass);
	hipLaunchKernelGGL(chain_gather_kernel, dim3((uint32_t)blocks), dim3(CHAIN_TPB), 0, s, d_ptr, 0u, d_ctl,
	    (const uint64_t *)NULL, d_dst);
}
