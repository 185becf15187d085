/*
 * la_zstd.hip -- Zstandard frame decoder for gfx950, first cut: the data plane of the zstd read filter
 * (SURVEY section 8 f3).  Replaces, for a batch of whole frames per call, what the reference's filter gets from
 * libzstd's ZSTD_decompressStream (libarchive/archive_read_support_filter_zstd.c:171-260): frame header, raw / RLE /
 * compressed blocks (Huffman literals in 1 or 4 streams with direct or FSE-coded weights, FSE sequences with
 * predefined / RLE / described / repeated tables, repeat offsets), and the XXH64 content checksum (RFC 8878).
 *
 * Parallelism in THIS file is across frames: here a frame is one serial chain (every block may reach back into the
 * previous ones, entropy tables and repeat offsets carry over).  That is the shape of pzstd output and of seekable /
 * chunked .zst files; a one-frame .zst runs on one wave here.  LA_ZSTD_OPT_BLOCK_PARALLEL puts la_zstd_blocks.hip in
 * front of these kernels: it decodes the BLOCKS of a frame in parallel and leaves to them (d_only) the frames it hands
 * back.  The bit readers, table readers and the sequence decoder both files use are in la_zstd_common.h.
 *
 *   zstd_frames_wave_kernel (default)  one WAVE per frame.  All 64 lanes run the same decoder on the same frame
 *       (uniform control flow: every lane computes the same header, table and sequence values, so nothing is
 *       broadcast and nothing diverges); the entropy tables live in LDS (10 KiB per wave), the bit streams are read
 *       through a 64-bit register window, and the byte moving is split over the lanes: raw / RLE blocks, literal
 *       runs and matches (an overlapping match reads position k mod offset of the bytes in front of it, so all
 *       its bytes go out at once), the four Huffman streams on four lanes, XXH64's four accumulators on four lanes.
 *       Sequences go 64 at a time: the wave decodes them (uniform, lane j keeps sequence j), then every lane copies its
 *       own literal run, one s_waitcnt vmcnt(0), and the matches follow in ballot rounds (a source that reaches into
 *       the group waits for the lanes whose sequences it touches, found with two lower bounds over the lanes' end
 *       positions; the scheme of la_lz4_wide.hip's in-order path).
 *   zstd_frames_kernel (LA_ZSTD_OPT_LANE_KERNEL)  the first form, one LANE per frame with its tables in an HBM
 *       workspace slot: same results, kept as a cross-check.
 * Measured (tools/measure_zstd.py, profiles/r02_zstd.txt): 16 384 frames of 64 KiB at level 3 decode at 20 GiB/s
 * resident in HBM (lane form: 6.1) against 2.9 GiB/s for libzstd on one host core.  87 % of a frame's cycles go to the
 * uniform 64-sequence decode loop: about 350 instructions per sequence, but ONE dependency chain per wave (state -> LDS
 * table word -> length table -> bit read -> next state); fewer branches changed nothing and moving the chain to the scalar
 * unit (v_readfirstlane, ZSTD_SCALAR) made it slower, and the 10.8 KiB of LDS tables hold a CU to 14 waves.  Next: two or
 * more frames interleaved per wave (independent chains), smaller tables for occupancy.
 */
#include "la_dev.h"
#include "la_zstd_common.h"


template <bool W> __device__ __forceinline__ static int64_t zstd_block(zframe *f, const uint8_t *src, size_t len, uint8_t *dst, size_t dst_pos, size_t dst_cap)
{
	/* ---- literals section ---- */
	zlit_hdr lh;
	if (zstd_lit_header(src, len, lh) < 0) return -1;
	const int64_t lu = zstd_literals<W>(f, src, len, lh, f->lit);
	if (lu < 0) return -1;
	size_t regen = lh.regen;
	const uint8_t *p = src + lu;
	size_t left = len - (size_t)lu;
	/* ---- sequences section ---- */
	if (W) wave_fence();	/* the literals are in the buffer */
	size_t nseq;
	{ const int c = zstd_nseq(p, left, &nseq); if (c < 0) return -1; p += c; left -= (size_t)c; }
	size_t out = dst_pos, lit_pos = 0;
	if (nseq) {
		if (left < 1) return -1;
		const int modes = p[0];
		/* (bits 0-1 are reserved; libzstd 1.4.8 ZSTD_decodeSeqHeaders does not look at them) */
		p += 1; left -= 1;
		int c;
		c = seq_table(&f->ll, &f->have_ll, modes >> 6, p, left, 9, 35, LL_DEF, 36, 6); if (c < 0) return -1; p += c; left -= (size_t)c;
		c = seq_table(&f->of, &f->have_of, (modes >> 4) & 3, p, left, 8, 31, OF_DEF, 29, 5); if (c < 0) return -1; p += c; left -= (size_t)c;
		c = seq_table(&f->ml, &f->have_ml, (modes >> 2) & 3, p, left, 9, 52, ML_DEF, 53, 6); if (c < 0) return -1; p += c; left -= (size_t)c;
		seqdec<rbits> sd;
		sd.pos = (int32_t)rev_init(p, left);
		if (sd.pos < 0) return -1;
		bits_init(sd.rb, p, left);
		sd.pos = unis<W && ZSTD_SCALAR>(sd.pos);
		sd.sl = bits_read<W && ZSTD_SCALAR>(sd.rb, &sd.pos, (unsigned)f->ll.al);
		sd.so = bits_read<W && ZSTD_SCALAR>(sd.rb, &sd.pos, (unsigned)f->of.al);
		sd.sm = bits_read<W && ZSTD_SCALAR>(sd.rb, &sd.pos, (unsigned)f->ml.al);
		if (sd.pos < 0) return -1;
		sd.r0 = uni<W && ZSTD_SCALAR>(f->rep[0]); sd.r1 = uni<W && ZSTD_SCALAR>(f->rep[1]); sd.r2 = uni<W && ZSTD_SCALAR>(f->rep[2]);
		if constexpr (!W) {
			for (size_t i = 0; i < nseq; i++) {
				uint32_t ll, ml, offset, ov;
				if (seq_next<false>(f, sd, i + 1 == nseq, ll, ml, offset, ov) < 0) return -1;
				if (ll > regen - lit_pos) return -1;
				if (out - dst_pos + ll + ml > ZBLOCK_MAX) return -1;
				if (out + ll + ml > dst_cap) return -2;
				dev_copy(dst + out, f->lit + lit_pos, ll); out += ll; lit_pos += ll;
				if (offset > out) return -1;
				t_match<false>(dst, out, offset, ml);
				out += ml;
			}
		} else {
			/* 64 sequences at a time: decoded by the whole wave (uniform), then executed one lane per sequence */
			const uint32_t lane = __lane_id();
			nseq = (size_t)uni64<ZSTD_SCALAR>(nseq); out = (size_t)uni64<ZSTD_SCALAR>(out); regen = (size_t)uni64<ZSTD_SCALAR>(regen);
			dst_cap = (size_t)uni64<ZSTD_SCALAR>(dst_cap); dst_pos = (size_t)uni64<ZSTD_SCALAR>(dst_pos);
			for (size_t base = 0; base < nseq; base += 64) {
				const uint32_t cnt = nseq - base < 64 ? (uint32_t)(nseq - base) : 64u;
				uint32_t my_ll = 0, my_ml = 0, my_off = 1;
				size_t my_out = out, my_lit = 0;
				for (uint32_t j = 0; j < cnt; j++) {
					uint32_t ll, ml, offset, ov;
					if (ZSTD_SCALAR) {	/* loop-carried state back into scalar registers: the compiler cannot prove it uniform across the back edge */
						j = uni<ZSTD_SCALAR>(j);
						sd.pos = unis<ZSTD_SCALAR>(sd.pos); sd.rb.lo = unis<ZSTD_SCALAR>(sd.rb.lo); sd.rb.win = uni64<ZSTD_SCALAR>(sd.rb.win);
						sd.rb.len = uni<ZSTD_SCALAR>(sd.rb.len); sd.rb.src = (const uint8_t *)uni64<ZSTD_SCALAR>((uint64_t)sd.rb.src);
						sd.sl = uni<ZSTD_SCALAR>(sd.sl); sd.sm = uni<ZSTD_SCALAR>(sd.sm); sd.so = uni<ZSTD_SCALAR>(sd.so);
						sd.r0 = uni<ZSTD_SCALAR>(sd.r0); sd.r1 = uni<ZSTD_SCALAR>(sd.r1); sd.r2 = uni<ZSTD_SCALAR>(sd.r2);
						out = (size_t)uni64<ZSTD_SCALAR>(out); lit_pos = (size_t)uni64<ZSTD_SCALAR>(lit_pos);
					}
					if (seq_next<ZSTD_SCALAR>(f, sd, base + j + 1 == nseq, ll, ml, offset, ov) < 0) return -1;
					if (ll > regen - lit_pos) return -1;
					if (out - dst_pos + ll + ml > ZBLOCK_MAX) return -1;
					if (out + ll + ml > dst_cap) return -2;
					if (offset > out + ll) return -1;
					if (lane == j) { my_ll = ll; my_ml = ml; my_off = offset; my_out = out; my_lit = lit_pos; }
					out += (size_t)ll + ml; lit_pos += ll;
				}
				const bool have = lane < cnt;
				/* literal runs: every lane its own */
				{
					const uint8_t *ls = f->lit + my_lit;
					uint8_t *ld = dst + my_out;
					uint32_t i = 0;
					for (; i + 8 <= my_ll; i += 8) { uint64_t v; __builtin_memcpy(&v, ls + i, 8); __builtin_memcpy(ld + i, &v, 8); }
					for (; i < my_ll; i++) ld[i] = ls[i];
				}
				wave_fence();	/* the literals of the group and everything in front of it are in place */
				/* matches: a source that reaches into the group waits for the lanes whose sequences it touches */
				const size_t g0 = (size_t)__shfl((int)(uint32_t)my_out, 0, 64) | ((size_t)__shfl((int)(uint32_t)((uint64_t)my_out >> 32), 0, 64) << 32);
				const size_t mdst = my_out + my_ll;
				const size_t s0 = mdst - my_off;
				const uint32_t span = my_ml < my_off ? my_ml : my_off;
				bool pendm = have && my_ml != 0;
				uint64_t depmask = 0;
				{
					/* ends of the group's sequences relative to its first byte (increasing over the lanes) */
					const uint32_t end = have ? (uint32_t)(mdst + my_ml - g0) : 0xFFFFFFFFu;
					const bool inside = pendm && s0 + span > g0;
					const uint32_t rlo = s0 > g0 ? (uint32_t)(s0 - g0) : 0u;
					const uint32_t rhi = inside ? (uint32_t)(s0 + span - 1 - g0) : 0u;
					uint32_t jlo = 0, jhi = 0;
#pragma unroll
					for (uint32_t bit = 32; bit; bit >>= 1) {
						const uint32_t e_lo = (uint32_t)__shfl((int)end, (int)(jlo + bit - 1u), 64);
						if (e_lo <= rlo) jlo += bit;
						const uint32_t e_hi = (uint32_t)__shfl((int)end, (int)(jhi + bit - 1u), 64);
						if (e_hi <= rhi) jhi += bit;
					}
					if (inside && lane != 0) {
						const uint32_t hi = jhi < lane ? jhi : lane - 1u;	/* own literals are in place */
						if (jlo <= hi) {
							const uint64_t upto = hi >= 63u ? ~0ull : ((1ull << (hi + 1u)) - 1ull);
							depmask = upto & ~((1ull << jlo) - 1ull);
						}
					}
				}
				for (;;) {
					const uint64_t pending = __ballot(pendm);
					if (pending == 0)
						break;
					if (pendm && (depmask & pending) == 0) {
						const uint8_t *ms = dst + s0;
						uint8_t *md = dst + mdst;
						if (my_off >= my_ml) {
							uint32_t i = 0;
							for (; i + 8 <= my_ml; i += 8) { uint64_t v; __builtin_memcpy(&v, ms + i, 8); __builtin_memcpy(md + i, &v, 8); }
							for (; i < my_ml; i++) md[i] = ms[i];
						} else {
							uint32_t m = 0;	/* i mod offset, carried */
							for (uint32_t i = 0; i < my_ml; i++) { md[i] = ms[m]; m = m + 1 == my_off ? 0 : m + 1; }
						}
						pendm = false;
					}
					wave_fence();
				}
			}
		}
		f->rep[0] = sd.r0; f->rep[1] = sd.r1; f->rep[2] = sd.r2;
		if (sd.pos != 0) return -1;	/* (libzstd 1.5 checks the exact end too; 1.4.8 does not) */
	} else if (left != 0) return -1;
	const size_t rest = regen - lit_pos;
	if (out - dst_pos + rest > ZBLOCK_MAX) return -1;
	if (out + rest > dst_cap) return -2;
	t_copy<W>(dst + out, f->lit + lit_pos, rest); out += rest;
	return (int64_t)(out - dst_pos);
}

/* One frame at src (zstd or skippable).  *consumed = its compressed length.  Returns decoded bytes appended at
 * dst + dst_pos, or -1 format error, -2 dst too small, -3 truncated input. */
template <bool W> __device__ __forceinline__ static int64_t zstd_frame(const uint8_t *src, size_t len, uint8_t *dst, size_t dst_pos, size_t dst_cap, size_t *consumed, zframe *fp, uint8_t *litbuf, uint32_t options)
{
	zframe_hdr fh;
	{
		const int64_t r = zstd_frame_header(src, len, fh);
		if (r < 0) return r;
		if (fh.skippable) { *consumed = fh.p; return 0; }
	}
	size_t p = fh.p;
	const uint32_t bmax = fh.bmax;
	const int fcs_len = fh.fcs_len, csum = fh.csum;
	const uint64_t fcs = fh.fcs;
	zframe &f = *fp;
	f.have_huf = f.have_ll = f.have_of = f.have_ml = 0;
	f.rep[0] = 1; f.rep[1] = 4; f.rep[2] = 8;
	f.lit = litbuf;
	size_t out = dst_pos;
	for (;;) {
		if (p + 3 > len) return -3;
		const uint32_t bh = src[p] | ((uint32_t)src[p + 1] << 8) | ((uint32_t)src[p + 2] << 16);
		p += 3;
		const int last = bh & 1, type = (bh >> 1) & 3;
		const uint32_t bsize = bh >> 3;
		if (zstd_block_header_bad(type, bsize, bmax)) return -1;
		if (type == 1) {
			if (p + 1 > len) return -3;
			if (out + bsize > dst_cap) return -2;
			t_fill<W>(dst + out, src[p], bsize); out += bsize; p += 1;
		} else {
			if (p + bsize > len) return -3;
			if (type == 0) {
				if (out + bsize > dst_cap) return -2;
				t_copy<W>(dst + out, src + p, bsize); out += bsize;
			} else {
				const int64_t r = zstd_block<W>(&f, src + p, bsize, dst + dst_pos, out - dst_pos, dst_cap - dst_pos);
				if (r < 0) return r;
				if ((uint64_t)r > bmax) return -1;
				out += (size_t)r;
			}
			p += bsize;
		}
		if (last) break;
	}
	if (fcs_len && (uint64_t)(out - dst_pos) != fcs) return -1;
	if (csum) {
		if (p + 4 > len) return -3;
		if (W) wave_fence();
		if (!(options & LA_ZSTD_OPT_NO_VERIFY) &&
		    (uint32_t)(W ? wave_xxh64(dst + dst_pos, out - dst_pos, 0) : dev_xxh64(dst + dst_pos, out - dst_pos, 0)) != rd32(src + p)) return -4;
		p += 4;
	}
	*consumed = p;
	return (int64_t)(out - dst_pos);
}


#define ZSTD_WS_STRIDE (144u * 1024u)	/* per lane: zframe (tables) + the literals buffer of one block */
#define ZSTD_MAX_LANES 8192u

__global__ __launch_bounds__(64) void zstd_frames_kernel(const uint8_t *__restrict__ src, uint64_t src_bytes,
    const la_zstd_frame *__restrict__ frames, uint32_t n, uint8_t *dst, uint64_t dst_cap, la_zstd_result *results,
    uint8_t *ws, uint32_t lanes, uint32_t options, const uint32_t *__restrict__ d_only)
{
	const uint32_t w = blockIdx.x * 64u + threadIdx.x;
	if (w >= lanes)
		return;
	zframe *fp = (zframe *)(ws + (size_t)w * ZSTD_WS_STRIDE);
	uint8_t *lit = (uint8_t *)fp + 12288;
	for (uint32_t k = 0; k < sizeof(seq_tabs) / 4; k++)
		((uint32_t *)&fp->tabs)[k] = ((const uint32_t *)&SEQ_TABS)[k];
	for (uint32_t i = w; i < n; i += lanes) {
		if (d_only && !d_only[i]) continue;	/* (the block path finished this frame) */
		const la_zstd_frame fr = frames[i];
		la_zstd_result r;
		r.status = LA_ST_ZSTD_CORRUPT; r.path = 0; r.out_len = 0;
		if (fr.src_off <= src_bytes && fr.src_len <= src_bytes - fr.src_off && fr.dst_off <= dst_cap && fr.dst_cap <= dst_cap - fr.dst_off) {
			size_t used = 0;
			const int64_t v = zstd_frame<false>(src + fr.src_off, (size_t)fr.src_len, dst + fr.dst_off, 0, (size_t)fr.dst_cap, &used, fp, lit, options);
			if (v >= 0) {
				r.status = (used == fr.src_len) ? LA_ST_OK : LA_ST_ZSTD_CORRUPT;	/* the host cut the frame here */
				r.out_len = (uint64_t)v;
			} else {
				r.status = v == -2 ? LA_ST_ZSTD_OUT_FULL : v == -3 ? LA_ST_ZSTD_TRUNCATED : v == -4 ? LA_ST_ZSTD_BAD_CHECKSUM :
				    v == -5 ? LA_ST_ZSTD_UNSUPPORTED : v == -6 ? LA_ST_ZSTD_WINDOW : v == -7 ? LA_ST_ZSTD_DICTIONARY : LA_ST_ZSTD_CORRUPT;
			}
		}
		results[i] = r;
	}
}

#define ZSTD_WAVE_WS_STRIDE (132u * 1024u)	/* per wave: the literals buffer of one block (the tables are in LDS) */
#define ZSTD_MAX_WAVES 4096u

/* one WAVE per frame: tables in LDS, uniform decode, lane-parallel byte moving, Huffman streams and XXH64 on four lanes */
__global__ __launch_bounds__(64) void zstd_frames_wave_kernel(const uint8_t *__restrict__ src, uint64_t src_bytes,
    const la_zstd_frame *__restrict__ frames, uint32_t n, uint8_t *dst, uint64_t dst_cap, la_zstd_result *results,
    uint8_t *ws, uint32_t waves, uint32_t options, const uint32_t *__restrict__ d_only)
{
	__shared__ zframe sf;
	for (uint32_t i = threadIdx.x; i < sizeof(seq_tabs) / 4; i += 64)
		((uint32_t *)&sf.tabs)[i] = ((const uint32_t *)&SEQ_TABS)[i];
	__syncthreads();
	const uint32_t w = blockIdx.x;
	uint8_t *lit = ws + (size_t)w * ZSTD_WAVE_WS_STRIDE;
	for (uint32_t i = w; i < n; i += waves) {
		if (d_only && !d_only[i]) continue;	/* (the block path finished this frame) */
		const la_zstd_frame fr = frames[i];
		la_zstd_result r;
		r.status = LA_ST_ZSTD_CORRUPT; r.path = 0; r.out_len = 0;
		if (fr.src_off <= src_bytes && fr.src_len <= src_bytes - fr.src_off && fr.dst_off <= dst_cap && fr.dst_cap <= dst_cap - fr.dst_off) {
			size_t used = 0;
			const int64_t v = zstd_frame<true>(src + fr.src_off, (size_t)fr.src_len, dst + fr.dst_off, 0, (size_t)fr.dst_cap, &used, &sf, lit, options);
			if (v >= 0) {
				r.status = (used == fr.src_len) ? LA_ST_OK : LA_ST_ZSTD_CORRUPT;
				r.out_len = (uint64_t)v;
			} else {
				r.status = v == -2 ? LA_ST_ZSTD_OUT_FULL : v == -3 ? LA_ST_ZSTD_TRUNCATED : v == -4 ? LA_ST_ZSTD_BAD_CHECKSUM :
				    v == -5 ? LA_ST_ZSTD_UNSUPPORTED : v == -6 ? LA_ST_ZSTD_WINDOW : v == -7 ? LA_ST_ZSTD_DICTIONARY : LA_ST_ZSTD_CORRUPT;
			}
		}
		if (threadIdx.x == 0)
			results[i] = r;
		wave_fence();
	}
}

static uint32_t zstd_lanes(uint32_t n) { return n < ZSTD_MAX_LANES ? n : ZSTD_MAX_LANES; }
static uint32_t zstd_waves(uint32_t n) { return n < ZSTD_MAX_WAVES ? n : ZSTD_MAX_WAVES; }

uint64_t la_zstd_workspace_bytes(uint32_t n_frames)
{
	const uint64_t a = (uint64_t)zstd_lanes(n_frames) * ZSTD_WS_STRIDE, b = (uint64_t)zstd_waves(n_frames) * ZSTD_WAVE_WS_STRIDE;
	return a > b ? a : b;
}

void la_launch_zstd_frames(hipStream_t s, const uint8_t *d_src, uint64_t src_bytes, const la_zstd_frame *d_frames, uint32_t n,
    uint8_t *d_dst, uint64_t dst_cap, la_zstd_result *d_results, uint8_t *ws, uint32_t options, const uint32_t *d_only)
{
	if (n == 0) return;
	static_assert(sizeof(zframe) <= 12288, "zframe must fit in front of the literals buffer");
	if (options & LA_ZSTD_OPT_LANE_KERNEL) {
		const uint32_t lanes = zstd_lanes(n);
		hipLaunchKernelGGL(zstd_frames_kernel, dim3((lanes + 63u) / 64u), dim3(64), 0, s, d_src, src_bytes, d_frames, n, d_dst, dst_cap,
		    d_results, ws, lanes, options, d_only);
	} else {
		const uint32_t waves = zstd_waves(n);
		hipLaunchKernelGGL(zstd_frames_wave_kernel, dim3(waves), dim3(64), 0, s, d_src, src_bytes, d_frames, n, d_dst, dst_cap,
		    d_results, ws, waves, options, d_only);
	}
}
