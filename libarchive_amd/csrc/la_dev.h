/*
 * la_dev.h -- shared device-side helpers and the internal launch interface
 * between the kernel translation units and the C-ABI layer (la_api.hip).
 * gfx950 only: wave = 64 lanes, 160 KiB LDS per CU.
 */
#ifndef LA_DEV_H
#define LA_DEV_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/la_gpu.h"
#include "la_lz4_slices.h"

#define LA_WAVE 64

/* ---- unaligned little-endian loads (gfx950 global memory is byte addressable
 * and the HSA ABI runs with unaligned access enabled; the compiler emits one
 * global_load_dword[x4] for these) ---- */
__device__ __forceinline__ uint32_t ld_u32(const uint8_t *p)
{
	uint32_t v;
	__builtin_memcpy(&v, p, 4);
	return v;
}
__device__ __forceinline__ uint4 ld_u128(const uint8_t *p)
{
	uint4 v;
	__builtin_memcpy(&v, p, 16);
	return v;
}
__device__ __forceinline__ uint32_t rotl32(uint32_t x, int r)
{
	return __builtin_rotateleft32(x, r);
}

/* ---- XXH32 (libarchive/xxhash.c:189-193 constants, :245-291 arithmetic) ---- */
#define XXH_P1 0x9E3779B1u
#define XXH_P2 0x85EBCA77u
#define XXH_P3 0xC2B2AE3Du
#define XXH_P4 0x27D4EB2Fu
#define XXH_P5 0x165667B1u

__device__ __forceinline__ uint32_t xxh_round(uint32_t acc, uint32_t lane)
{
	return rotl32(acc + lane * XXH_P2, 13) * XXH_P1;
}
__device__ __forceinline__ uint32_t xxh_avalanche(uint32_t h)
{
	h ^= h >> 15; h *= XXH_P2;
	h ^= h >> 13; h *= XXH_P3;
	h ^= h >> 16;
	return h;
}
/* one whole hash computed by ONE lane (many-hash kernels run one hash per lane).
 * The stripe loop is unrolled four times so that a lane keeps 64 bytes of loads
 * in flight: per-lane streams are latency bound, not issue bound. */
__device__ __forceinline__ uint32_t xxh32_lane(const uint8_t *p, uint32_t len, uint32_t seed)
{
	const uint8_t *end = p + len;
	uint32_t h;
	if (len >= 16) {
		uint32_t v1 = seed + XXH_P1 + XXH_P2, v2 = seed + XXH_P2, v3 = seed, v4 = seed - XXH_P1;
		while (p + 64 <= end) {
			uint4 a = ld_u128(p), b = ld_u128(p + 16), c = ld_u128(p + 32), d = ld_u128(p + 48);
			v1 = xxh_round(v1, a.x); v2 = xxh_round(v2, a.y); v3 = xxh_round(v3, a.z); v4 = xxh_round(v4, a.w);
			v1 = xxh_round(v1, b.x); v2 = xxh_round(v2, b.y); v3 = xxh_round(v3, b.z); v4 = xxh_round(v4, b.w);
			v1 = xxh_round(v1, c.x); v2 = xxh_round(v2, c.y); v3 = xxh_round(v3, c.z); v4 = xxh_round(v4, c.w);
			v1 = xxh_round(v1, d.x); v2 = xxh_round(v2, d.y); v3 = xxh_round(v3, d.z); v4 = xxh_round(v4, d.w);
			p += 64;
		}
		while (p + 16 <= end) {
			uint4 x = ld_u128(p);
			v1 = xxh_round(v1, x.x);
			v2 = xxh_round(v2, x.y);
			v3 = xxh_round(v3, x.z);
			v4 = xxh_round(v4, x.w);
			p += 16;
		}
		h = rotl32(v1, 1) + rotl32(v2, 7) + rotl32(v3, 12) + rotl32(v4, 18);
	} else {
		h = seed + XXH_P5;
	}
	h += len;
	while (p + 4 <= end) {
		h = rotl32(h + ld_u32(p) * XXH_P3, 17) * XXH_P4;
		p += 4;
	}
	while (p < end) {
		h = rotl32(h + (uint32_t)(*p) * XXH_P5, 11) * XXH_P1;
		p++;
	}
	return xxh_avalanche(h);
}

/* one hash computed by FOUR adjacent lanes (lane j of the quad owns accumulator
 * v(j+1) and reads the j-th dword of every 16-byte stripe, so a quad's load is one
 * contiguous 16 bytes).  Used for the long content-checksum chains, where there
 * are few hashes and each is long.  Result valid in all four lanes. */
__device__ __forceinline__ uint32_t xxh32_quad(const uint8_t *p, uint32_t len, uint32_t seed, int j)
{
	const uint8_t *end = p + len;
	uint32_t h;
	if (len >= 16) {
		uint32_t v = (j == 0) ? seed + XXH_P1 + XXH_P2 : (j == 1) ? seed + XXH_P2 : (j == 2) ? seed : seed - XXH_P1;
		const uint8_t *q = p + 4 * j;
		/* 512 bytes (32 stripes) of loads in flight per quad: the chain itself is short,
		 * the stream must not wait for memory.  (Requesting the next batch before this one is
		 * chained -- software prefetch with a second register set -- made this loop twice as
		 * slow as compiled, 14 vs 7 ms per step; it is kept in the 16-lane form below only.) */
		while (p + 512 <= end) {
			uint32_t x[32];
#pragma unroll
			for (int t = 0; t < 32; t++)
				x[t] = ld_u32(q + 16 * t);
#pragma unroll
			for (int t = 0; t < 32; t++)
				v = xxh_round(v, x[t]);
			p += 512; q += 512;
		}
		while (p + 128 <= end) {
			uint32_t x0 = ld_u32(q), x1 = ld_u32(q + 16), x2 = ld_u32(q + 32), x3 = ld_u32(q + 48);
			uint32_t x4 = ld_u32(q + 64), x5 = ld_u32(q + 80), x6 = ld_u32(q + 96), x7 = ld_u32(q + 112);
			v = xxh_round(v, x0); v = xxh_round(v, x1); v = xxh_round(v, x2); v = xxh_round(v, x3);
			v = xxh_round(v, x4); v = xxh_round(v, x5); v = xxh_round(v, x6); v = xxh_round(v, x7);
			p += 128; q += 128;
		}
		while (p + 16 <= end) {
			v = xxh_round(v, ld_u32(q));
			p += 16; q += 16;
		}
		const int rot = (j == 0) ? 1 : (j == 1) ? 7 : (j == 2) ? 12 : 18;
		uint32_t t = rotl32(v, rot);
		t += __shfl_xor(t, 1, 64);
		t += __shfl_xor(t, 2, 64);
		h = t;
	} else {
		h = seed + XXH_P5;
	}
	h += len;
	while (p + 4 <= end) {
		h = rotl32(h + ld_u32(p) * XXH_P3, 17) * XXH_P4;
		p += 4;
	}
	while (p < end) {
		h = rotl32(h + (uint32_t)(*p) * XXH_P5, 11) * XXH_P1;
		p++;
	}
	return xxh_avalanche(h);
}

/* The same hash by SIXTEEN adjacent lanes (one DPP row).  A single XXH32 accumulator is a serial
 * chain  v = rotl(v + x * P2, 13) * P1  whose two 32-bit multiplies run at quarter rate; in the
 * four-lane form every lane pays both per stripe.  Here lane 4t + j loads dword j of stripe t of
 * each 64-byte group (one coalesced 64-byte load per row), ONE multiply instruction turns all of
 * them into products, and lanes 0..3 (accumulator j) chain over the four stripes pulling the
 * products of the other lanes in with DPP row shifts: one multiply on the chain per stripe
 * instead of two, 29 instead of 62 cycles per stripe.  Only a quarter as many hashes share an
 * instruction, so this form is for hashes nothing else hides (the last slice of a batch, frames
 * that cross batches), not for bulk.  Result valid in lanes 0..3 of the row. */
#define XXH_ROW_BATCH 32
__device__ __forceinline__ uint32_t xxh_chain_step(uint32_t v, uint32_t prod)
{
	return rotl32(v + prod, 13) * XXH_P1;
}
__device__ __forceinline__ uint32_t xxh32_row(const uint8_t *p, uint32_t len, uint32_t seed, int l)
{
	const int j = l & 3;
	const uint8_t *end = p + len;
	uint32_t h;
	if (len >= 16) {
		uint32_t v = (j == 0) ? seed + XXH_P1 + XXH_P2 : (j == 1) ? seed + XXH_P2 : (j == 2) ? seed : seed - XXH_P1;
		const uint8_t *q = p + 4 * l;
		/* XXH_ROW_BATCH groups of four stripes per batch (2 KiB per row); the next batch is
		 * requested before this one is chained, and chaining a batch takes about as long as a
		 * load does */
#define XXH_ROW_CHAIN(xg_)                                                                                        \
		do {                                                                                              \
			const uint32_t pr_ = (xg_) * XXH_P2;                                                      \
			v = xxh_chain_step(v, pr_);                                                               \
			v = xxh_chain_step(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)pr_, 0x104, 0xf, 0xf, false));	/* row_shl:4 */ \
			v = xxh_chain_step(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)pr_, 0x108, 0xf, 0xf, false));	/* row_shl:8 */ \
			v = xxh_chain_step(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)pr_, 0x10c, 0xf, 0xf, false));	/* row_shl:12 */ \
		} while (0)
		if (p + XXH_ROW_BATCH * 64 <= end) {
			uint32_t x[XXH_ROW_BATCH];
#pragma unroll
			for (int g = 0; g < XXH_ROW_BATCH; g++)
				x[g] = ld_u32(q + 64 * g);
			p += XXH_ROW_BATCH * 64; q += XXH_ROW_BATCH * 64;
			while (p + XXH_ROW_BATCH * 64 <= end) {
				uint32_t y[XXH_ROW_BATCH];
#pragma unroll
				for (int g = 0; g < XXH_ROW_BATCH; g++)
					y[g] = ld_u32(q + 64 * g);
#pragma unroll
				for (int g = 0; g < XXH_ROW_BATCH; g++)
					XXH_ROW_CHAIN(x[g]);
#pragma unroll
				for (int g = 0; g < XXH_ROW_BATCH; g++)
					x[g] = y[g];
				p += XXH_ROW_BATCH * 64; q += XXH_ROW_BATCH * 64;
			}
#pragma unroll
			for (int g = 0; g < XXH_ROW_BATCH; g++)
				XXH_ROW_CHAIN(x[g]);
		}
		while (p + 64 <= end) {
			XXH_ROW_CHAIN(ld_u32(q));
			p += 64; q += 64;
		}
#undef XXH_ROW_CHAIN
		while (p + 16 <= end) {	/* fewer than four stripes left: lanes 0..3 on their own */
			v = xxh_round(v, ld_u32(p + 4 * j));
			p += 16;
		}
		const int rot = (j == 0) ? 1 : (j == 1) ? 7 : (j == 2) ? 12 : 18;
		uint32_t t = rotl32(v, rot);
		t += __shfl_xor(t, 1, 64);
		t += __shfl_xor(t, 2, 64);
		h = t;
	} else {
		h = seed + XXH_P5;
	}
	h += len;
	while (p + 4 <= end) {
		h = rotl32(h + ld_u32(p) * XXH_P3, 17) * XXH_P4;
		p += 4;
	}
	while (p < end) {
		h = rotl32(h + (uint32_t)(*p) * XXH_P5, 11) * XXH_P1;
		p++;
	}
	return xxh_avalanche(h);
}

/* 512-byte register window over the compressed payload: lane l holds the
 * aligned dwords at base+4l (w0) and base+256+4l (w1). */
struct src_window {
	const uint8_t *base;	/* 4-byte aligned, wave-uniform */
	const uint8_t *limit;	/* one past the last readable byte of the whole source image */
	uint32_t w0, w1;
};

__device__ __forceinline__ uint32_t win_load(const src_window &W, const uint8_t *p)
{
	/* p is 4-aligned.  A dword that holds at least one byte of the image lies in
	 * the same page as that byte, so loading it whole cannot fault; dwords
	 * entirely past the image are never touched. */
	return (p < W.limit) ? *(const uint32_t *)p : 0u;
}

__device__ __forceinline__ void win_reset(src_window &W, const uint8_t *q, int lane)
{
	W.base = (const uint8_t *)((uintptr_t)q & ~(uintptr_t)3);
	W.w0 = win_load(W, W.base + 4 * lane);
	W.w1 = win_load(W, W.base + 256 + 4 * lane);
}

/* byte at q (wave-uniform address, q >= W.base) */
__device__ __forceinline__ uint32_t win_byte(src_window &W, const uint8_t *q, int lane)
{
	uint32_t d = (uint32_t)(q - W.base);
	if (d >= 256) {
		if (d < 512) {
			W.base += 256;
			W.w0 = W.w1;
			W.w1 = win_load(W, W.base + 256 + 4 * lane);
			d -= 256;
		} else {
			win_reset(W, q, lane);
			d = (uint32_t)(q - W.base);
		}
	}
	uint32_t dw = (uint32_t)__builtin_amdgcn_readlane((int)W.w0, (int)(d >> 2));
	return (dw >> ((d & 3) * 8)) & 0xffu;
}

__device__ __forceinline__ void wave_mem_fence()
{
	/* make this wave's earlier global stores visible to its own later loads
	 * (same CU, same L1): s_waitcnt vmcnt(0) is all the hardware needs */
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
	__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

/* unaligned little-endian dword at q (wave-uniform), served from the window */
__device__ __forceinline__ uint32_t win_u32(src_window &W, const uint8_t *q, int lane)
{
	uint32_t d = (uint32_t)(q - W.base);
	if (d + 4 > 256) {
		if (d < 256) {
			/* straddles the two halves: assemble from bytes (rare) */
			uint32_t v = 0;
			for (int k = 0; k < 4; k++)
				v |= win_byte(W, q + k, lane) << (8 * k);
			return v;
		}
		win_byte(W, q, lane);	/* slides or reloads the window */
		d = (uint32_t)(q - W.base);
	}
	uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)W.w0, (int)(d >> 2));
	uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)W.w0, (int)(((d >> 2) + 1) & 63));
	if ((d >> 2) == 63)
		hi = (uint32_t)__builtin_amdgcn_readlane((int)W.w1, 0);
	return __builtin_amdgcn_alignbyte(hi, lo, d & 3);
}

/* LDS accepts unaligned 2/4/8-byte accesses on gfx950 (the compiler emits
 * ds_read_b64 / ds_write_b64 for these), so window copies move 8 bytes per
 * instruction at any byte address. */
__device__ __forceinline__ uint64_t lds_ld8(const uint8_t *p) { uint64_t v; __builtin_memcpy(&v, p, 8); return v; }
__device__ __forceinline__ void lds_st8(uint8_t *p, uint64_t v) { __builtin_memcpy(p, &v, 8); }
__device__ __forceinline__ void lds_st4(uint8_t *p, uint32_t v) { __builtin_memcpy(p, &v, 4); }
__device__ __forceinline__ uint4 lds_ld16(const uint8_t *p) { uint4 v; __builtin_memcpy(&v, p, 16); return v; }
__device__ __forceinline__ void lds_st16(uint8_t *p, uint4 v) { __builtin_memcpy(p, &v, 16); }
__device__ __forceinline__ void lds_st2(uint8_t *p, uint16_t v) { __builtin_memcpy(p, &v, 2); }

/* store the low n (< 8) bytes of v */
__device__ __forceinline__ void lds_st_tail(uint8_t *p, uint64_t v, uint32_t n)
{
	if (n & 4) { lds_st4(p, (uint32_t)v); p += 4; v >>= 32; }
	if (n & 2) { lds_st2(p, (uint16_t)v); p += 2; v >>= 16; }
	if (n & 1) *p = (uint8_t)v;
}

/* load n (< 8) bytes without touching bytes past p+n */
__device__ __forceinline__ uint64_t lds_ld_tail(const uint8_t *p, uint32_t n)
{
	uint64_t v = 0;
	uint32_t sh = 0;
	if (n & 4) { uint32_t t; __builtin_memcpy(&t, p, 4); v = t; p += 4; sh = 32; }
	if (n & 2) { uint16_t t; __builtin_memcpy(&t, p, 2); v |= (uint64_t)t << sh; p += 2; sh += 16; }
	if (n & 1) v |= (uint64_t)(*p) << sh;
	return v;
}

/* The usual match -- at most 64 bytes, not overlapping its source -- as ONE straight line of predicated DS
 * instructions.  A wave on its own issues an instruction every four or five cycles and pays an instruction-fetch
 * restart for every taken branch, and the matcher's passes are nothing but this copy: what the compiler makes of
 * `if (class) copy piece` is three to eight instructions and up to two branches per piece.  Here a piece is two:
 * exec = ready lanes of the class (both wave-uniform masks, the class masks worked out once per group), then the
 * DS instruction; no branch.  All loads are issued before anything is stored, pieces as in io_copy_exact:
 * 16-byte pieces at 0 / 16 / 32 and one that ENDS with the match, 8 + 8 overlapping below 16 bytes, 4 + 4 below 8,
 * 2 + 1 below 4 (1..3 bytes: only the deflate front end makes these). */
typedef uint32_t io_u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t io_u32x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) uint8_t io_lds_u8;
__device__ __forceinline__ uint32_t io_lds_addr(const uint8_t *p) { return (uint32_t)(uintptr_t)(const io_lds_u8 *)p; }

struct io_cls {		/* lanes of the group by length class, fast lanes only (wave-uniform, one SGPR pair each) */
	uint64_t k16, k32, k48, ke;	/* >= 16, >= 32, >= 48, end piece (length > 16 and not 32 or 48) */
	uint64_t ks, ks8, ks88;		/* < 16 (8-byte load), 8..15, 9..15 */
	uint64_t ks4, ks44, k2, k1;	/* 4..7, 5..7, {2,3}, {1,3} */
};
struct io_adr {		/* per lane: LDS byte addresses and shift counts */
	uint32_t fp, mp;	/* source, destination */
	uint32_t fe, me;	/* + length - 16 */
	uint32_t f8, m8;	/* + length - 8 */
	uint32_t m4, sh4;	/* mp + length - 4, 8 * (length - 4) */
	uint32_t m1, sh1;	/* mp + (length & 2), 8 * (length & 2) */
};

/* one predicated DS instruction: exec = ready lanes of the class, then the instruction (IO_EXP_SKIP_EMPTY: the
 * instruction is jumped over when no lane is left -- a timing experiment, see profiles/r03_inorder_whatif.txt) */
#ifdef IO_EXP_SKIP_EMPTY
#define IO_DS(mask_, ins_, n_) "s_and_b64 exec, %[R], %[" mask_ "]\n\ts_cbranch_execz .Lio" n_ "_%=\n\t" ins_ "\n\t.Lio" n_ "_%=:\n\t"
#else
#define IO_DS(mask_, ins_, n_) "s_and_b64 exec, %[R], %[" mask_ "]\n\t" ins_ "\n\t"
#endif
__device__ __forceinline__ void io_copy_fast(const uint64_t R, const io_cls &K, const io_adr &A)
{
	io_u32x4 v0, v1, v2, vt;
	io_u32x2 a0, at;
	uint64_t sv;
	asm volatile(
	    "s_mov_b64 %[sv], exec\n\t"
	    IO_DS("k16", "ds_read_b128 %[v0], %[fp]", "0")
	    IO_DS("k32", "ds_read_b128 %[v1], %[fp] offset:16", "1")
	    IO_DS("k48", "ds_read_b128 %[v2], %[fp] offset:32", "2")
	    IO_DS("ke", "ds_read_b128 %[vt], %[fe]", "3")
	    IO_DS("ks", "ds_read_b64 %[a0], %[fp]", "4")
	    IO_DS("ks88", "ds_read_b64 %[at], %[f8]", "5")
	    "s_mov_b64 exec, %[sv]\n\t"
	    "s_waitcnt lgkmcnt(0)"
	    : [sv] "=&s"(sv), [v0] "=&v"(v0), [v1] "=&v"(v1), [v2] "=&v"(v2), [vt] "=&v"(vt), [a0] "=&v"(a0), [at] "=&v"(at)
	    : [R] "s"(R), [k16] "s"(K.k16), [k32] "s"(K.k32), [k48] "s"(K.k48), [ke] "s"(K.ke), [ks] "s"(K.ks), [ks88] "s"(K.ks88),
	      [fp] "v"(A.fp), [fe] "v"(A.fe), [f8] "v"(A.f8)
	    : "memory");
	/* (lanes outside a class hold garbage in that class's registers: never stored) */
#ifdef IO_EXP_LOADS_ONLY	/* timing experiment */
	asm volatile("" :: "v"(v0), "v"(v1), "v"(v2), "v"(vt), "v"(a0), "v"(at));
	return;
#endif
	const uint32_t a0lo = a0.x;
	const uint32_t t4 = (uint32_t)((((uint64_t)a0.y << 32) | a0.x) >> (A.sh4 & 63u));
	const uint32_t t1 = a0lo >> (A.sh1 & 31u);
	asm volatile(
	    "s_mov_b64 %[sv], exec\n\t"
	    IO_DS("k16", "ds_write_b128 %[mp], %[v0]", "0")
	    IO_DS("k32", "ds_write_b128 %[mp], %[v1] offset:16", "1")
	    IO_DS("k48", "ds_write_b128 %[mp], %[v2] offset:32", "2")
	    IO_DS("ke", "ds_write_b128 %[me], %[vt]", "3")
	    IO_DS("ks8", "ds_write_b64 %[mp], %[a0]", "4")
	    IO_DS("ks88", "ds_write_b64 %[m8], %[at]", "5")
	    IO_DS("ks4", "ds_write_b32 %[mp], %[a0lo]", "6")
	    IO_DS("ks44", "ds_write_b32 %[m4], %[t4]", "7")
	    IO_DS("k2", "ds_write_b16 %[mp], %[a0lo]", "8")
	    IO_DS("k1", "ds_write_b8 %[m1], %[t1]", "9")
	    "s_mov_b64 exec, %[sv]"
	    : [sv] "=&s"(sv)
	    : [R] "s"(R), [k16] "s"(K.k16), [k32] "s"(K.k32), [k48] "s"(K.k48), [ke] "s"(K.ke), [ks8] "s"(K.ks8), [ks88] "s"(K.ks88),
	      [ks4] "s"(K.ks4), [ks44] "s"(K.ks44), [k2] "s"(K.k2), [k1] "s"(K.k1),
	      [mp] "v"(A.mp), [me] "v"(A.me), [m8] "v"(A.m8), [m4] "v"(A.m4), [m1] "v"(A.m1),
	      [v0] "v"(v0), [v1] "v"(v1), [v2] "v"(v2), [vt] "v"(vt), [a0] "v"(a0), [at] "v"(at), [a0lo] "v"(a0lo), [t4] "v"(t4), [t1] "v"(t1)
	    : "memory");
}
#undef IO_DS

/* Bump carver over a launcher's workspace.  The launcher carves the workspace it is given; its
 * *_workspace_bytes function runs the same carve on a null base and reads the size off `off`. */
struct la_carve {
	uint8_t *base;
	uint64_t off;
	template <typename T> T *take(uint64_t count, uint64_t align = alignof(T))
	{
		off = (off + align - 1) & ~(align - 1);
		T *p = base ? (T *)(void *)(base + off) : nullptr;
		off += count * sizeof(T);
		return p;
	}
};

/* ---- launch interface (definitions live next to their kernels) ---- */

/* la_hash.hip */
void la_launch_xxh32_many(hipStream_t s, const uint8_t *d_base, const la_hash_job *d_jobs,
    uint32_t n, uint32_t *d_out);
void la_launch_crc32_many(hipStream_t s, const uint8_t *d_base, const la_hash_job *d_jobs,
    uint32_t n, uint32_t *d_out);
void la_launch_adler32_many(hipStream_t s, const uint8_t *d_base, const la_hash_job *d_jobs,
    uint32_t n, uint32_t *d_out);
void la_launch_lz4_block_sums(hipStream_t s, const uint8_t *d_src, const la_lz4_block *d_blocks,
    uint32_t n, uint32_t *d_status);
void la_launch_lz4_frame_sums(hipStream_t s, const uint8_t *d_src, const uint8_t *d_dst,
    const la_lz4_frame *d_frames, uint32_t n_frames, const uint64_t *d_dst_off,
    uint64_t dst_cap, uint32_t *d_frame_status, uint32_t end_lo, uint32_t end_hi,
    const void *d_carry_in, void *d_carry_out, int row /* 16 lanes per frame: latency over throughput */);
/* hash pass g of a split last slice (la_lz4_slices.h); d_carries: one LA_XXH_CARRY_BYTES record per block of the slice */
void la_launch_lz4_frame_sums_split(hipStream_t s, const uint8_t *d_src, const uint8_t *d_dst,
    const la_lz4_frame *d_frames, uint32_t n_frames, const uint64_t *d_dst_off, uint64_t dst_cap,
    uint32_t *d_frame_status, const la_lz4_split &sp, uint32_t g, void *d_carries, const void *d_carry_in,
    void *d_carry_out, int row);
void la_launch_lz4_merge_status(hipStream_t s, const uint32_t *d_sum_status, uint32_t n, uint32_t *d_status);

/* la_lz4.hip, la_lz4_fast.hip */
struct la_lz4_seq {	/* one LZ4 sequence, 8 bytes, written by the parse kernel */
	uint16_t lit_src;	/* offset of the first literal inside the block payload */
	uint16_t lit_len;
	uint16_t dst;		/* output offset where the literals go */
	uint16_t off;		/* match offset (0 in a final, literal-only sequence) */
};
/* match length of sequence k = (k+1 < nseq ? seq[k+1].dst : out_len) - (dst + lit_len) */

#define LA_LZ4_FAST_MAXSEQ 4096u	/* sequences per block the LDS-window kernel holds (per segment) */
#define LA_INFLATE_MAXSEQ 12288u	/* table entries per deflate member in the two-phase path (three segments) */

/* blocks that get a table slot (the LDS-window kernels can only take these): compressed, independent,
 * window <= 64 KiB.  Who EXPANDS a block is la_lz4_route's decision, below. */
__host__ __device__ __forceinline__ bool la_lz4_fast_eligible(const la_lz4_block &b)
{
	return !(b.flags & (LA_LZ4B_STORED | LA_LZ4B_DEPENDENT)) && b.dst_cap <= 65536u && b.src_len <= 65536u;
}

/* Blocks made of few, long sequences (long runs, big repeats: on average LA_LZ4_LONG_SEQ_BYTES decoded bytes per
 * sequence or more) go to the wave-wide general kernel even when the LDS-window kernels could take them: one lane per
 * match copies a 64 KiB run at the speed of one lane (10 GB/s on blocks of zeros), the general kernel's wave-wide
 * copies reach 250 GB/s on them (tools/measure_long_matches.py).  thr = 0 switches the routing off (the deflate
 * front end has no general kernel behind it).  Asked by la_lz4_route only. */
#define LA_LZ4_LONG_SEQ_BYTES 512u
__host__ __device__ __forceinline__ bool la_lz4_long_sequences(uint32_t nseq, uint32_t out_len, uint32_t thr)
{
	return thr != 0 && nseq != 0xFFFFFFFFu && (uint64_t)nseq * thr <= out_len;
}

/* Which expand kernel writes a block's bytes: THE place where that is decided.  Every expand kernel and the classify
 * kernel ask with the block's words and act on one answer: the general kernel takes GENERAL, the polling kernel WINDOW
 * or, in its segmented launch, WINDOW_SEG; the in-order kernel, run instead of both, takes both.  Nobody takes NONE.
 * have_tables: the batch was parsed into sequence tables; nseq = 0xFFFFFFFF: no room for this block's table.
 * The in-order kernel alone used to refuse out_len > 64 KiB, nseq == 0 and src_off > src_bytes, blocks the general
 * kernel stood aside for.  Dropped, because a block with a window answer cannot be in such a state: both parse kernels
 * fail a sequence that passes dst_cap (<= 64 KiB if eligible), count every sequence they put in a table, and read zeros
 * beyond the image, which fail (offset 0) or decode to nothing; the deflate front end sends members above 64 KiB
 * elsewhere, closes its table with the last literals, and sets src_off inside its own literal buffer. */
enum la_expand_route { LA_XR_NONE, LA_XR_GENERAL, LA_XR_WINDOW, LA_XR_WINDOW_SEG };
__host__ __device__ __forceinline__ la_expand_route la_lz4_route(const la_lz4_block &b, uint32_t status, uint32_t out_len,
    uint32_t nseq, uint64_t dst_off, uint64_t dst_cap, bool have_tables, uint32_t long_thr)
{
	if (status != LA_ST_OK || out_len == 0 || dst_off + out_len > dst_cap)	/* never write past the slab, whatever the tables say */
		return LA_XR_NONE;
	if (!have_tables || !la_lz4_fast_eligible(b) || la_lz4_long_sequences(nseq, out_len, long_thr) || nseq == 0xFFFFFFFFu)
		return LA_XR_GENERAL;
	return nseq <= LA_LZ4_FAST_MAXSEQ ? LA_XR_WINDOW : LA_XR_WINDOW_SEG;
}

/* A block's words, fetched once: what la_lz4_route is asked with, and where the block's payload, output and table slot
 * lie.  The expand kernels (window, in-order, general) open with la_lz4_load_block_words and route on what it returns
 * (la_lz4_route_words); the dependency kernel, at eight workgroups per CU, gained 0.03 ms of 2.17 from it, short of the
 * margin, and reads its words as before.  Read word by word where la_lz4_route first needs them, every array is a scalar
 * load of its own behind its own wait and branch -- the compiler sinks a load to the test that first asks for it and does not lift it
 * back over a branch: six memory round trips in a row before a kernel has asked for its first payload byte
 * (profiles/r31_lz4_block_words.md).  Here all of them are requested together, and the pin -- an empty asm that takes
 * every word in a scalar register -- keeps them live at one point, so they form one clause behind one wait.
 * The block index must be wave-uniform (a scalar register: blockIdx, or through readfirstlane) and below n: then every
 * index is inside its array, table_off having n + 1 entries (lz4_ws_carve in la_api.hip, la_inflate_emit).  All the
 * arrays are read whatever the block's state, so a launch passes only arrays it was given: TABLE_OFF = false for a
 * kernel that has no table offsets (the general kernel; its nseq words are carved for every batch, and routed on only
 * with have_tables). */
struct la_lz4_block_words {
	uint64_t src_off;
	uint32_t src_len, dst_cap, flags;
	uint32_t block_sum;	/* (nobody asks for it here.  It lies in the 16 bytes that one load fetches with the three words
				 * in front of it; left out of the pin, its register is handed to the next load at once, which then
				 * has to wait for this one: a second round trip) */
	uint32_t status, out_len, nseq;
	uint64_t dst_off, table_off;
};
/* (device only: the host has no scalar registers to pin) */
#if defined(__HIP_DEVICE_COMPILE__)
#define LA_PIN_SCALARS(...) asm volatile("" :: __VA_ARGS__)
__device__ __forceinline__ void la_lz4_pin_block_words(la_lz4_block_words &w)
{
	asm volatile("" : "+s"(w.src_off), "+s"(w.src_len), "+s"(w.dst_cap), "+s"(w.flags), "+s"(w.block_sum), "+s"(w.status), "+s"(w.out_len),
	    "+s"(w.nseq), "+s"(w.dst_off), "+s"(w.table_off));
}
#else
#define LA_PIN_SCALARS(...) do { } while (0)
__device__ __forceinline__ void la_lz4_pin_block_words(la_lz4_block_words &) { }
#endif
/* the value of lane 0 in a scalar register (a no-op on a value that is in one already) */
__device__ __forceinline__ uint32_t la_first_lane(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint64_t la_first_lane(uint64_t v)
{
	return ((uint64_t)la_first_lane((uint32_t)(v >> 32)) << 32) | la_first_lane((uint32_t)v);
}
/* VECTOR_LOADS: the kernel asks again behind its own stores (a loop over blocks), where the compiler loads through the
 * vector path, every lane the same address: the words move to scalar registers by hand, so that the pin holds */
template <bool TABLE_OFF = true, bool VECTOR_LOADS = false>
__device__ __forceinline__ la_lz4_block_words la_lz4_load_block_words(uint32_t bi, const la_lz4_block *blocks,
    const uint32_t *status, const uint32_t *out_len, const uint32_t *nseq, const uint64_t *dst_off, const uint64_t *table_off)
{
	la_lz4_block_words w;
	w.src_off = blocks[bi].src_off;
	w.src_len = blocks[bi].src_len;
	w.dst_cap = blocks[bi].dst_cap;
	w.flags = blocks[bi].flags;
	w.block_sum = blocks[bi].block_sum;
	w.status = status[bi];
	w.out_len = out_len[bi];
	w.nseq = nseq[bi];
	w.dst_off = dst_off[bi];
	w.table_off = TABLE_OFF ? table_off[bi] : 0;
	if (VECTOR_LOADS) {
		w.src_off = la_first_lane(w.src_off); w.src_len = la_first_lane(w.src_len); w.dst_cap = la_first_lane(w.dst_cap);
		w.flags = la_first_lane(w.flags); w.block_sum = la_first_lane(w.block_sum); w.status = la_first_lane(w.status);
		w.out_len = la_first_lane(w.out_len); w.nseq = la_first_lane(w.nseq); w.dst_off = la_first_lane(w.dst_off);
		w.table_off = la_first_lane(w.table_off);
	}
	la_lz4_pin_block_words(w);
	return w;
}
/* la_lz4_route asked with the fetched words (slab_cap: the decoded slab's size, la_lz4_route's dst_cap) */
__device__ __forceinline__ la_expand_route la_lz4_route_words(const la_lz4_block_words &w, uint64_t slab_cap, bool have_tables,
    uint32_t long_thr)
{
	la_lz4_block b;
	b.src_off = w.src_off;
	b.src_len = w.src_len;
	b.dst_cap = w.dst_cap;
	b.flags = w.flags;
	b.block_sum = w.block_sum;
	return la_lz4_route(b, w.status, w.out_len, w.nseq, w.dst_off, slab_cap, have_tables, long_thr);
}

/* What a match of the LDS-window kernel has to wait for: THE place where that is decided.  Literals are all in the window
 * before the first match is copied, so sequence k (output position d, match at mdst = d + lit_len, offset off, mlen match
 * bytes) waits only for earlier MATCHES under its source.  The source is the span min(mlen, off) from mdst - off (an
 * overlapping match reads its own bytes behind that), clipped below d: from d on the bytes are the sequence's own.
 * la_lz4_dep_source: false when nothing in front of the sequence is read (empty match, or a source inside its own literals);
 * else *hi_byte is the last byte that is.  With q the last sequence that starts at or before the source and qe the last
 * one that starts at or before hi_byte, the wait is for the matches of q .. qe, and la_lz4_dep_drops_last says that qe
 * falls out again: a sequence is literals first and match second, so a source that ends before qe's match start
 * (last_mstart = its d + lit_len) touches its literals only.  The word handed to the poll loop is q | count << 16.
 * Asked by the dependency kernel (la_lz4_deps.hip) and by the search inside lz4_expand_fast_kernel. */
__device__ __forceinline__ bool la_lz4_dep_source(uint32_t d, uint32_t mdst, uint32_t off, uint32_t mlen, uint32_t *hi_byte)
{
	const uint32_t s0 = mdst - off;
	if (mlen == 0 || s0 >= d)
		return false;
	const uint32_t span = mlen < off ? mlen : off;
	uint32_t hi = s0 + span - 1;
	if (hi >= d)
		hi = d - 1;
	*hi_byte = hi;
	return true;
}
__device__ __forceinline__ bool la_lz4_dep_drops_last(uint32_t hi_byte, uint32_t last_mstart)
{
	return hi_byte < last_mstart;
}

/* Where phase L of the LDS-window kernel starts in the sequence table: THE place where that is decided.  Phase L gives
 * every 32-byte chunk of a block's payload to one thread, which has to know the first sequence with literal bytes in or
 * behind its chunk.  Positions are relative to the payload's first byte.  With le(k) = lit_src + lit_len the end of
 * sequence k's literal run (le(-1) = 0), the LITERAL PLAN of a block is a chunk index:
 *   entry c, c < ceil(src_len / 32):  the first sequence whose literals end beyond payload offset 32 c, that is the k
 *       with la_lz4_lit_chunk_edge(le(k - 1)) <= c < la_lz4_lit_chunk_edge(le(k)); LA_LZ4_PLAN_NONE when there is none
 *       (chunks behind the last literal byte: a thread there has nothing to place);
 *   one entry behind them:  the number of chunks that hold literals, la_lz4_lit_chunk_edge(le(ns - 1)).
 * A sequence whose run ends in front of the same chunk edge as the run before it is no chunk's entry; one without
 * literals counts with lit_len = 0, its le the place where they would stand.
 * A sequence number is below LA_LZ4_FAST_MAXSEQ = 4096, so 0xFFFF is free for "none".  The entries are 16-bit and lie
 * in a byte buffer of one byte per table slot entry, the block's first one at byte table_off[block] (slots are
 * multiples of eight entries, so that is even): 2 (ceil(src_len / 32) + 1) <= (src_len / 3 + 8) & ~7 for every
 * src_len, checked in tests/test_lz4_literal_plan_rule.py.
 * Asked by the dependency kernel (la_lz4_deps.hip), which writes the plan, and by the window kernel's own chunk index
 * (DEPS = false, la_lz4_fast.hip). */
#define LA_LZ4_PLAN_NONE 0xFFFFu
__host__ __device__ __forceinline__ uint32_t la_lz4_lit_chunk_edge(uint32_t lit_end)
{
	return (lit_end + 31u) >> 5;	/* the chunks [0, edge) begin in front of lit_end */
}
__host__ __device__ __forceinline__ uint32_t la_lz4_plan_entries(uint32_t src_len)
{
	return la_lz4_lit_chunk_edge(src_len) + 1u;
}

/* Which dwords of a payload chunk a literal run stores: THE place where that is decided.  Phase L moves a 32-byte chunk
 * of the payload (from payload offset c0, a multiple of 32) to the window as whole dwords on the chunk's own grid.  A run
 * [ls, le) of a sequence with output position dst stores the dwords [*m0, *mend) of the chunk, the ones that hold at
 * least one of its bytes, and dword m goes to  *w0 + 4 m,  *w0 = w + dst + c0 - ls  with w the window's first byte: a
 * pointer, or an offset (then modulo 2^32: dst + c0 - ls lies up to 31 below zero for a run that starts inside the chunk;
 * a dword the run stores is at most three bytes in front of dst).  False, and nothing written, when no byte of the run
 * lies in the chunk.  The first and the last dword may spill up to three bytes over the run's ends: into the match in
 * front of it or behind it, which is at least four bytes long and is copied later, or into the window's headroom and
 * slack.
 * In a table the lz4 parse kernels wrote two literal runs are at least three payload bytes apart (the match offset and
 * the next token stand between them), so a dword of the grid holds bytes of at most one run: the ranges of a chunk's
 * runs are disjoint and increasing, and a dword has one owner or none.  That is what lets the window kernel pick an
 * owner per dword (DEPS = true) instead of walking the dwords once per run (put(), the other instantiations); both ask
 * here, and tests/lz4_literal_dword_rule.py restates it. */
template <class W>
__host__ __device__ __forceinline__ bool la_lz4_lit_run_dwords(uint32_t ls, uint32_t le, uint32_t dst, uint32_t c0, W w,
    uint32_t *m0, uint32_t *mend, W *w0)
{
	const uint32_t c1 = c0 + 32u;
	const uint32_t lo = ls > c0 ? ls : c0, hi = le < c1 ? le : c1;
	if (hi > lo) {
		*m0 = (lo - c0) >> 2;
		*mend = (hi - c0 + 3) >> 2;
		*w0 = w + dst + c0 - ls;
		return true;
	}
	return false;
}

/* One expand step over a table of blocks: what every expand launch is given.  Host side only: the launchers unpack
 * it into their kernels' (restrict-qualified) arguments. */
struct la_expand_job {
	const uint8_t *src;		/* compressed image (deflate front end: its literal buffers) */
	uint64_t src_bytes;
	const la_lz4_block *blocks;	/* [n] */
	uint32_t n;
	uint8_t *dst;			/* decoded slab */
	uint64_t dst_cap;
	const uint64_t *dst_off;	/* per block, as out_len, status, nseq and table_off */
	const uint32_t *out_len;
	uint32_t *status;
	const uint32_t *nseq;
	const la_lz4_seq *table;	/* NULL: no sequence tables, the general kernel takes every block */
	const uint64_t *table_off;
	uint32_t long_thr;		/* la_lz4_long_sequences */
	const uint32_t *deps;		/* one word per table entry, written by la_launch_lz4_deps for the LA_XR_WINDOW blocks
					 * (la_lz4_dep_source); NULL: the window kernel searches for itself */
	const uint8_t *lit_plan;	/* with deps, by the same launch: the blocks' literal plans (la_lz4_lit_chunk_edge), one byte
					 * per table entry */

	/* blocks first .. first + count - 1: the per-block arrays move; image, slab, table, deps and plan (absolute offsets) stay */
	la_expand_job slice(uint32_t first, uint32_t count) const
	{
		return la_expand_job{ src, src_bytes, blocks + first, count, dst, dst_cap, dst_off + first, out_len + first,
		    status + first, nseq + first, table, table_off + first, long_thr, deps, lit_plan };
	}
};

void la_launch_lz4_table_caps(hipStream_t s, const la_lz4_block *d_blocks, uint32_t n, uint32_t *d_caps);
void la_launch_lz4_parse(hipStream_t s, const uint8_t *d_src, uint64_t src_bytes,
    const la_lz4_block *d_blocks, uint32_t n, uint32_t *d_out_len, uint32_t *d_nseq,
    uint32_t *d_status, la_lz4_seq *d_table /* NULL: measure only */, const uint64_t *d_table_off,
    uint64_t table_cap /* entries */);
/* la_lz4_parse.hip: the same parse fed from an LDS-staged image, block checksums fused in
 * (d_sum_status NULL: no checksums) */
void la_launch_lz4_parse_staged(hipStream_t s, const uint8_t *d_src, uint64_t src_bytes,
    const la_lz4_block *d_blocks, uint32_t n, uint32_t *d_out_len, uint32_t *d_nseq,
    uint32_t *d_status, uint32_t *d_sum_status, la_lz4_seq *d_table, const uint64_t *d_table_off,
    uint64_t table_cap);
void la_launch_lz4_expand_general(hipStream_t s, const la_expand_job &j, uint32_t hist_len);
void la_launch_lz4_expand_fast(hipStream_t s, const la_expand_job &j);
void la_launch_lz4_expand_fast_big(hipStream_t s, const la_expand_job &j, uint32_t *d_big /* n + 1 words */);
/* group g of a split last slice (la_lz4_slices.h): j is the whole batch's job and carries deps and lit_plan */
void la_launch_lz4_expand_fast_group(hipStream_t s, const la_expand_job &j, const la_lz4_split &sp, uint32_t g);
/* la_lz4_deps.hip: the dependency words and the literal plans of the job's LA_XR_WINDOW blocks, for a later
 * la_launch_lz4_expand_fast whose job carries d_deps and d_plan (same table offsets) */
void la_launch_lz4_deps(hipStream_t s, const la_expand_job &j, uint32_t *d_deps, uint8_t *d_plan);

/* la_lz4_inorder.hip: the in-order expand step, run on request as the cross-check of the polling kernel (in-order
 * matcher wave + literal wave + flush wave per 64 KiB LDS window); the same contract, blocks of any sequence count
 * (no _big launch) */
bool la_lz4_expand_inorder_takes(uint64_t src_bytes);	/* false: image too short for it, use the polling kernel */
void la_launch_lz4_expand_inorder(hipStream_t s, const la_expand_job &j);

/* la_zstd.hip */
uint64_t la_zstd_workspace_bytes(uint32_t n_frames);
void la_launch_zstd_frames(hipStream_t s, const uint8_t *d_src, uint64_t src_bytes, const la_zstd_frame *d_frames, uint32_t n,
    uint8_t *d_dst, uint64_t dst_cap, la_zstd_result *d_results, uint8_t *ws, uint32_t options,
    const uint32_t *d_only /* [n] nonzero = decode this frame; NULL = every frame */);
/* la_zstd_blocks.hip: LA_ZSTD_OPT_BLOCK_PARALLEL.  Finishes what frames it can (status, out_len, path = 1) and leaves
 * todo[i] != 0 for the others; d_todo is the first array of the workspace (la_zstd_blocks_todo). */
uint64_t la_zstd_blocks_workspace_bytes(uint32_t n_frames, uint64_t src_bytes, uint64_t dst_cap);
const uint32_t *la_zstd_blocks_todo(const uint8_t *ws);
void la_launch_zstd_blocks(hipStream_t s, const uint8_t *d_src, uint64_t src_bytes, const la_zstd_frame *d_frames, uint32_t n,
    uint8_t *d_dst, uint64_t dst_cap, la_zstd_result *d_results, uint8_t *ws, uint32_t options);

/* la_bzip2.hip */
uint64_t la_bzip2_workspace_bytes(uint32_t n, uint32_t level);
uint32_t la_bzip2_max_blocks(uint32_t level);
uint64_t la_bzip2_scan_ws_bytes(uint64_t src_bytes);
void la_launch_bzip2_scan(hipStream_t s, const uint8_t *d_src, uint64_t src_bytes, la_bz2_cand *d_cands, uint32_t cap,
    uint32_t *d_count, uint8_t *ws);
/* la_gpu_bzip2_decode: MEASURE = measure + walk, EMIT = emit + verify; all four carve the same workspace from (n, slot_level) */
void la_launch_bzip2_measure(hipStream_t s, const la_bz2_batch *bt, uint8_t *ws);
void la_launch_bzip2_walk(hipStream_t s, const la_bz2_batch *bt, uint8_t *ws);
void la_launch_bzip2_emit(hipStream_t s, const la_bz2_batch *bt, uint8_t *ws);
void la_launch_bzip2_verify(hipStream_t s, const la_bz2_batch *bt, uint8_t *ws);

/* la_xz.hip: ws = the CRC32 jobs of the n blocks, then their CRC32s */
uint64_t la_xz_workspace_bytes(uint32_t n);
void la_launch_xz_decode(hipStream_t s, const la_xz_batch *bt, uint8_t *ws);
void la_launch_xz_verify(hipStream_t s, const la_xz_batch *bt, uint8_t *ws);
/* la_lzip.hip */
uint64_t la_lzip_scan_ws_bytes(uint64_t src_bytes);
void la_launch_lzip_scan(hipStream_t s, const uint8_t *d_src, uint64_t src_bytes, uint64_t *d_offs, uint32_t cap, uint32_t *d_count,
    uint8_t *ws);
uint64_t la_lzip_workspace_bytes(uint32_t n);
void la_launch_lzip_decode(hipStream_t s, const la_lzip_batch *bt, uint8_t *ws);

/* la_lzo.hip */
uint64_t la_lzop_workspace_bytes(uint32_t n);
void la_launch_lzop_decode(hipStream_t s, const la_lzop_batch *bt, uint8_t *ws);
/* la_uu.hip: the four phases of la_gpu_uu_decode, in this order, over one workspace carved from src_bytes */
uint64_t la_uu_workspace_bytes(uint64_t src_bytes);
void la_launch_uu_lines(hipStream_t s, const la_uu_batch *bt, uint8_t *ws);
void la_launch_uu_records(hipStream_t s, const la_uu_batch *bt, uint8_t *ws);
void la_launch_uu_states(hipStream_t s, const la_uu_batch *bt, uint8_t *ws);
void la_launch_uu_decode(hipStream_t s, const la_uu_batch *bt, uint8_t *ws);
/* la_xz_filters.hip: the chains behind d_blocks[n] (LA_XZ_BATCH_CHAINS) undone over the decoded bytes; jobs_ws is
 * la_launch_xz_decode's workspace, ws a 256-byte aligned scratch of la_xz_unfilter_ws_bytes() of its own */
uint64_t la_xz_unfilter_ws_bytes(uint32_t n, uint64_t dst_cap);
void la_launch_xz_unfilter(hipStream_t s, const la_xz_batch *bt, uint8_t *jobs_ws, uint8_t *ws);

/* la_bzip2_comp.hip */
uint32_t la_bzip2_compress_block_bytes(uint32_t level);
uint64_t la_bzip2_compress_ws_bytes(uint64_t src_bytes, uint32_t level);
uint64_t la_bzip2_compress_bound(uint64_t src_bytes, uint32_t level);
uint32_t la_bzip2_compress_rounds(hipStream_t s, const uint8_t *ws);
/* mark(cx, name) ends the stage before and begins `name` (NULL: none): the API layer's profile ranges */
struct la_stage_hook { void (*mark)(void *cx, const char *name); void *cx; };
void la_launch_bzip2_compress(hipStream_t s, const la_bz2c_batch *bt, uint8_t *ws, const la_stage_hook *hook);

/* la_xz_comp.hip */
uint64_t la_xz_compress_ws_bytes(uint64_t src_bytes);
uint64_t la_xz_compress_bound(uint64_t src_bytes);
void la_launch_xz_compress(hipStream_t s, const la_xzc_batch *bt, uint8_t *ws, const la_stage_hook *hook);

/* la_lzip_comp.hip */
uint32_t la_lzip_compress_member_bytes(uint32_t level);
uint64_t la_lzip_compress_ws_bytes(uint64_t src_bytes, uint32_t level);
uint64_t la_lzip_compress_bound(uint64_t src_bytes, uint32_t level);
void la_launch_lzip_compress(hipStream_t s, const la_lzc_batch *bt, uint8_t *ws, const la_stage_hook *hook);

/* la_lzo_comp.hip */
uint64_t la_lzop_compress_ws_bytes(uint64_t src_bytes, uint32_t block_size);
void la_launch_lzop_compress(hipStream_t s, const la_lzopc_batch *bt, uint8_t *ws);

/* la_lz4_comp.hip */
void la_launch_lz4_compress(hipStream_t s, const uint8_t *d_src, uint64_t src_bytes, uint32_t block_size,
    uint32_t bpf, uint32_t flags, uint8_t *d_out, uint64_t out_cap, uint64_t *d_out_bytes, uint8_t *ws);

/* la_zstd_comp.hip */
void la_launch_zstd_compress(hipStream_t s, const uint8_t *d_src, uint64_t src_bytes, uint32_t block_size,
    uint32_t bpf, uint32_t flags, uint8_t *d_out, uint64_t out_cap, uint64_t *d_out_bytes, uint8_t *ws);

/* la_deflate_comp.hip */
void la_launch_gzip_compress(hipStream_t s, const uint8_t *d_src, uint64_t src_bytes, uint32_t chunk, uint32_t mtime,
    uint32_t options, uint32_t framing, uint8_t *d_out, uint64_t out_cap, uint64_t *d_out_bytes, uint8_t *ws);	/* LA_GZC_*, LA_GZC_FRAME_* */
uint64_t la_gzip_compress_ws_bytes(uint64_t src_bytes, uint32_t chunk, uint32_t options);	/* LA_GZC_* */
/* la_gpu_zip_compress in two halves: the span table with its checks, whose verdict is the first word of `ws` (0 = the
 * table is good), then everything that writes d_out */
void la_launch_zip_spans(hipStream_t s, uint64_t src_bytes, const la_zipc_seg *d_segs, uint32_t n_segs, uint32_t chunk,
    uint32_t options, uint8_t *ws);
void la_launch_zip_compress(hipStream_t s, const uint8_t *d_src, uint64_t src_bytes, const la_zipc_seg *d_segs, uint32_t n_segs,
    uint32_t chunk, uint32_t options, uint8_t *d_out, uint64_t out_cap, la_zipc_result *d_results, uint64_t *d_out_bytes,
    uint8_t *ws);
uint64_t la_zip_compress_ws_bytes(uint64_t src_bytes, uint32_t n_segs, uint32_t chunk, uint32_t options);

/* la_inflate.hip */
void la_launch_inflate(hipStream_t s, const uint8_t *d_src, uint64_t src_bytes,
    const la_gz_member *d_members, uint32_t n, uint8_t *d_dst, uint64_t dst_cap, la_gz_result *d_results, bool pieces);
/* LA_GZ_OPT_CHAIN: what the emit instance of the wave kernel is given beside the batch (la_inflate.hip) */
struct la_inflate_chain {
	const uint64_t *packed_off;	/* [n + 1] exclusive scan of the measured out_len */
	uint32_t *ptr;			/* one source pointer per packed output byte */
	uint32_t hist_len;
	/* LA_GZ_OPT_BLOCK_STARTS only (la_launch_inflate_chain_bits; the other instances do not read them): piece i starts
	 * at bit starts[i] of the span d_members[0]; *n_starts pieces, a number only the device knows */
	const uint32_t *starts;
	const uint32_t *n_starts;
	const uint32_t *n_table;	/* entries of starts[], *n_starts or one more: where a piece that is not decoded starts */
};
void la_launch_inflate_chain(hipStream_t s, const uint8_t *d_src, uint64_t src_bytes, const la_gz_member *d_members,
    uint32_t n, uint8_t *d_dst, uint64_t dst_cap, la_gz_result *d_results, const la_inflate_chain &C, bool emit);
/* the same two instances for pieces that start at a bit: d_members is ONE span, n_max bounds *C.n_starts (the grid);
 * results: consumed is the BIT the piece ended on, counted from the span's first byte, and the measure instance leaves
 * in crc32 the index of the start a LA_ST_GZ_PIECE_END piece ended on (0xFFFFFFFF: on the end of the span) */
void la_launch_inflate_chain_bits(hipStream_t s, const uint8_t *d_src, uint64_t src_bytes, const la_gz_member *d_span,
    uint32_t n_max, uint8_t *d_dst, uint64_t dst_cap, la_gz_result *d_results, const la_inflate_chain &C, bool emit);
/* la_inflate_find.hip (LA_GZ_OPT_BLOCK_STARTS): the candidate table, the confirming walk, the summary */
struct la_gz_find_ws {
	uint32_t *ctl;		/* LA_FIND_* words */
	uint32_t *mask;		/* one bit per bit position: passed dfl_find_quick */
	uint32_t *tile_cnt;	/* survivors per tile */
	uint64_t *tile_off;	/* [tiles + 1] */
	uint32_t *surv;		/* [max_surv] survivor bit offsets, ascending */
	uint32_t *flag;		/* [max_surv] 1: the survivor passed the full rule */
	uint64_t *flag_off;	/* [max_surv + 1] */
	uint32_t *cand;		/* [max_cand] cand[0] = the caller's start bit, then the candidates behind it, ascending */
	la_gz_result *res_all;	/* [max_cand] measured, per candidate */
	uint32_t *startc;	/* [max_cand + 1] confirmed starts, and behind them the start of the piece that did not fit */
	la_gz_result *resc;	/* [max_cand] results of the confirmed pieces (measure, then emit) */
	uint32_t *lenc;		/* [max_cand] their measured lengths, 0 behind the last */
	uint32_t *crc;		/* [max_cand] CRC32 of each confirmed piece's packed bytes */
	void *scan;
	uint32_t tiles, max_surv, max_cand;
};
enum { LA_FIND_N_SURV = 0, LA_FIND_N_CAND = 1, LA_FIND_N_CONF = 2, LA_FIND_STOP = 3, LA_FIND_STOP_BIT = 4, LA_FIND_N_TABLE = 5, LA_FIND_CTL_WORDS = 64 };
#define LA_FIND_TILE_BYTES 1024u
void la_launch_gz_find(hipStream_t s, const uint8_t *d_src, uint64_t src_bytes, const la_gz_member *d_span, uint32_t start_bit,
    const la_gz_find_ws &W);
void la_launch_gz_walk(hipStream_t s, uint64_t dst_cap, const la_gz_find_ws &W);
/* la_hash.hip: CRC32 of every confirmed piece, then results[0] / results[1] of the call */
void la_launch_gz_blocks_summary(hipStream_t s, const uint8_t *d_dst, const la_gz_member *d_span, const uint64_t *d_packed_off,
    uint32_t start_bit, const la_gz_find_ws &W, la_gz_result *d_results);
/* la_inflate_chain.hip: the jump passes and the gather over a range whose length is *d_total (at most dst_cap) */
void la_launch_chain_resolve_dev(hipStream_t s, uint8_t *d_dst, const uint64_t *d_first_off, uint32_t *d_ptr, uint32_t hist_len,
    const uint64_t *d_total, uint64_t dst_cap, uint32_t *d_ctl);
/* la_inflate_chain.hip: between the two instances (measured lengths as the scan's input), and behind them (packed
 * member table for the CRC32 launch, the pointer-jumping passes, the gather) */
#define LA_CHAIN_JUMP_PASSES 32u
#define LA_CHAIN_CTL_WORDS 64u	/* [0, 32) one "changed" flag per jump pass, [32] bytes of the packed range */
void la_launch_chain_lengths(hipStream_t s, const la_gz_result *d_results, uint32_t n, uint32_t *d_len);
void la_launch_chain_resolve(hipStream_t s, const la_gz_member *d_members, const la_gz_result *d_results, uint32_t n,
    uint8_t *d_dst, uint64_t dst_cap, const la_inflate_chain &C, la_gz_member *d_packed, uint32_t *d_ctl);
/* the same jump passes and gather over a range that starts at d_dst (coordinate 0, no history): total entries of d_ptr */
void la_launch_chain_resolve_range(hipStream_t s, uint8_t *d_dst, uint32_t *d_ptr, uint32_t total, uint32_t *d_ctl);
uint64_t la_inflate_lanes_scratch_bytes(uint32_t n);
/* outputs of the entropy-only launch (la_launch_inflate_symbols): everything
 * lz4_expand_fast_kernel needs to build the members in its LDS window */
struct la_inflate_emit {
	uint8_t *lit;		/* literal bytes, 64 KiB per member */
	la_lz4_seq *table;	/* LA_INFLATE_MAXSEQ entries per member */
	la_lz4_block *blocks;	/* [n] literal buffer as the expand kernel's "payload" */
	uint32_t *out_len;	/* [n] */
	uint32_t *nseq;		/* [n] */
	uint32_t *xstatus;	/* [n] 0 = expand it, else skip (member goes to the in-place kernel) */
	uint32_t *todo;		/* [n] 1 = the in-place kernel must decode this member */
	uint64_t *dst_off;	/* [n+1] */
	uint64_t *table_off;	/* [n+1] */
};
/* the expand step behind the entropy-only launch (no long-sequence routing: no general kernel runs behind it) */
static inline la_expand_job la_inflate_expand_job(const la_inflate_emit &E, uint32_t n, uint8_t *d_dst, uint64_t dst_cap)
{
	return la_expand_job{ E.lit, (uint64_t)n * 65536u, E.blocks, n, d_dst, dst_cap, E.dst_off, E.out_len, E.xstatus,
	    E.nseq, E.table, E.table_off, 0u };
}
void la_launch_inflate_lanes(hipStream_t s, const uint8_t *d_src, uint64_t src_bytes,
    const la_gz_member *d_members, uint32_t n, uint8_t *d_dst, uint64_t dst_cap, la_gz_result *d_results,
    void *d_scratch, const uint32_t *d_only /* NULL: every member */, bool pieces);
void la_launch_inflate_symbols(hipStream_t s, const uint8_t *d_src, uint64_t src_bytes,
    const la_gz_member *d_members, uint32_t n, uint64_t dst_cap, la_gz_result *d_results,
    void *d_scratch, la_inflate_emit E, bool pieces);
void la_launch_gz_verify(hipStream_t s, const uint8_t *d_src, uint64_t src_bytes,
    const la_gz_member *d_members, uint32_t n, const uint8_t *d_dst, la_gz_result *d_results, int verify);
void la_launch_gz_summary(hipStream_t s, const la_gz_result *d_results, uint32_t n, la_batch_summary *d_summary);

/* la_scan.hip */
void la_launch_scan_u32(hipStream_t s, const uint32_t *d_in, uint32_t n, uint64_t *d_out /* n+1 */,
    void *d_scratch);
void la_launch_scan_u32_base(hipStream_t s, const uint32_t *d_in, uint32_t n, uint64_t *d_out, void *d_scratch,
    const uint64_t *d_base);
uint64_t la_scan_scratch_bytes(uint32_t n);
void la_launch_lz4_summary(hipStream_t s, const uint32_t *d_out_len, const uint32_t *d_block_status,
    uint32_t n_blocks, const uint32_t *d_frame_status, uint32_t n_frames,
    const uint64_t *d_dst_off, la_batch_summary *d_summary);

#endif
