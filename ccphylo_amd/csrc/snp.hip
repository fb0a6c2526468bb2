// snp.hip -- all-pairs SNP distances on gfx950 (the `ccphylo dist` hot loop).
//
// Reference: fsacmp.c:552 fsacmp (count of included positions where the
// 2-bit codes differ), fsacmp.c:587 fsacmpair (same over inc_i & inc_j, plus
// the number of compared positions), driven by fsacmpthrd.c:108 cmpFsaThrd /
// :261 cmpairFsaThrd which store nFactor*dist (resp. the A7 epilogue) into
// LT cell (i, j).
//
// Data layout in HBM ("bit planes"): for taxon t and 32-position word w,
//   hi[t][w] = high code bits, lo[t][w] = low code bits, MSB = first position
// (the include-mask bit order of fsacmp.c:200).  Non-pair mode pre-applies
// the global include mask to both planes, so a pair's count is
//   sum_w popc((hi_a ^ hi_b) | (lo_a ^ lo_b))        -- 3 VALU ops / 32 nt
// (v_xor, v_bitop3, v_bcnt with accumulate).
// Pair mode keeps each taxon's mask m beside its planes:
//   d += popc(((hi_a ^ hi_b) | (lo_a ^ lo_b)) & m_a & m_b), n += popc(m_a & m_b).
// Two kernel families compute it:
//   - the default, k_snp_mfma3 (non-pair) / k_snp_mfma2_pair: the count as an
//     exact MX-fp4 dot product on the matrix cores (each code a +-1
//     tetrahedron vector, dist = (3 L - dot) / 4), 256x256 pair tiles,
//     MFMA-bound; k_snp_mfma3 stages its chunks by LDS-DMA and interleaves
//     the plane-to-fp4 spreads with the MFMAs, k_snp_mfma2 (CCG_DIST_GLDS=0)
//     is the register-staged form it replaced;
//   - k_snp_tile / k_snp_tile_pair (CCG_DIST_MFMA=0): the popcount form
//     above, VALU-integer-bound, 128x128 pair tiles, 8x8 pairs per thread in
//     registers; k_snp_mfma / k_snp_mfma_pair (CCG_DIST_MFMA=1) are the first
//     matrix-core form on the same 128x128 tiles.  These are the independent
//     side of the bit-for-bit tests.
// All stage chunks of a few words of the two row panels through LDS, and every
// kernel is one template over SPLIT (split-K: word slices, exact u32 counts,
// a finish kernel) and BAND (the A panel gathers one rank's owned rows of the
// row-sharded layout, rows stored at Shard::off).  On the host, snp_launch
// routes a matrix to snp_launch_mfma2 (256x256 tiles) or snp_launch_tile128;
// both take their work from tile_range and their slices from plan_split.
#include <cstring>
#include <vector>
#include <type_traits>
#include "ccg_internal.h"
#include "ccg_shard_layout.h"

#define TILE 128
#define KC 16          // words per LDS chunk (non-pair)
#define KCP 8          // words per LDS chunk (pair)
#define RS 130         // LDS row stride in 8-byte units: 16-byte aligned, 2-way write conflicts at most
#define RSP 130        // pair: stride in 16-byte units

// (a ^ b) | c in one v_bitop3_b32 (truth table 0xBE, checked on gfx950 by
// tools/micro/bitop3_check.hip): a word pair costs xor + bitop3 + bcnt
__device__ __forceinline__ uint32_t xor_or(uint32_t a, uint32_t b, uint32_t c) {
	return __builtin_amdgcn_bitop3_b32(a, b, c, 0xBE);
}

__device__ __forceinline__ uint32_t compress_even(uint64_t x) {
	x &= 0x5555555555555555ull;
	x = (x | (x >> 1)) & 0x3333333333333333ull;
	x = (x | (x >> 2)) & 0x0F0F0F0F0F0F0F0Full;
	x = (x | (x >> 4)) & 0x00FF00FF00FF00FFull;
	x = (x | (x >> 8)) & 0x0000FFFF0000FFFFull;
	x = (x | (x >> 16)) & 0x00000000FFFFFFFFull;
	return (uint32_t) x;
}

// qseq2nibble word (position p at bits 63-2p..62-2p) -> (hi, lo) planes.
// Non-pair mode may compact the words: plane word w holds alignment word
// widx[w] (the words the global mask does not exclude entirely, in order), so
// W32 is then their count; widx = NULL keeps every word.
__global__ void k_planes(const uint64_t *__restrict__ seqs, const uint32_t *__restrict__ incs, int n, int stride,
                         int W32, int Wp, int pair, uint2 *__restrict__ out2, uint4 *__restrict__ out4,
                         const int *__restrict__ widx) {
	// grid-stride: n * Wp exceeds 2^32 work-items at config sizes (50k x 5M)
	const long long total = (long long) n * Wp;
	for(long long e = (long long) blockIdx.x * blockDim.x + threadIdx.x; e < total;
	    e += (long long) gridDim.x * blockDim.x) {
		const int t = (int) (e / Wp), w = (int) (e % Wp);
		uint32_t hi = 0, lo = 0, m = 0;
		if(w < W32) {
			const int ws = widx ? widx[w] : w;
			uint64_t x = seqs[(size_t) t * stride + ws];
			hi = compress_even(x >> 1);
			lo = compress_even(x);
			m = pair ? incs[(size_t) t * stride + ws] : incs[ws];
		}
		if(pair) {
			out4[e] = make_uint4(hi, lo, m, 0);
		} else {
			out2[e] = make_uint2(hi & m, lo & m);
		}
	}
}

__global__ void k_popsum(const uint32_t *__restrict__ inc, int W32, int *out) {
	int s = 0;
	for(int w = threadIdx.x; w < W32; w += blockDim.x) s += __popc(inc[w]);
	for(int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
	__shared__ int ws[16];
	if((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = s;
	__syncthreads();
	if(threadIdx.x == 0) {
		int t = 0;
		for(int k = 0; k < (int) (blockDim.x >> 6); ++k) t += ws[k];
		*out = t;
	}
}

// linear tile index -> (I, J), I >= J, row-major over the lower triangle
__device__ __forceinline__ void tile_ij(long long t, int &I, int &J) {
	long long r = (long long) ((sqrt(8.0 * (double) t + 1.0) - 1.0) * 0.5);
	while(r * (r + 1) / 2 > t) --r;
	while((r + 1) * (r + 2) / 2 <= t) ++r;
	I = (int) r;
	J = (int) (t - r * (r + 1) / 2);
}

// tile t of a rank's band list (tile_range): panel I = last with pfx[I] <= t, J = t - pfx[I]
__device__ __forceinline__ void band_ij(const long long *__restrict__ pfx, int npanels, long long t, int &I, int &J) {
	int lo = 0, hi = npanels - 1;
	while(lo < hi) {
		const int mid = (lo + hi + 1) >> 1;
		if(pfx[mid] <= t) lo = mid; else hi = mid - 1;
	}
	I = lo;
	J = (int) (t - pfx[lo]);
}

// the row a band A panel stages for the rank's L-th owned row (row l of panel
// I: L = I * edge + l); owned rows past n stage row 0 and are never stored
__device__ __forceinline__ long long band_row(const Shard &sh, long long L, int n) {
	const long long r = sh.global_row(L);
	return r < n ? r : 0;
}

// XCD-aware tile order: workgroups are dispatched round-robin over the 8
// XCDs, so give XCD x a contiguous run of row-major tiles (tiles (I, J),
// (I, J+1), ... share the I panel in that XCD's L2).  Bijective on [0, cnt).
__device__ __forceinline__ long long xcd_tile(long long b, long long cnt) {
	const long long x = b & 7, k = b >> 3, q = cnt >> 3, r = cnt & 7;
	return x < r ? x * (q + 1) + k : r * (q + 1) + (x - r) * q + k;
}

// Non-pair tiles: double-buffered KC-word chunks of both 128-row panels; the
// next chunk's global loads are in flight while the current one is consumed
// from LDS, one barrier per chunk.  Work item = (tile, word slice): with
// S > 1 slices (split-K, so small tile counts still fill the chip) the
// partial counts are summed exactly with u32 atomics into `cnt` and
// k_snp_finish writes D.  BAND: the tiles of one rank of the row-sharded
// layout (ccg_shard.h): tile item / S of the rank's list (pfx), the A panel
// gathers the rank's owned rows, so a rank computes only its own rows and
// writes them at Shard::off, where ccg_tree_shard_dev reads them (SURVEY 8(d)
// config 5); split-K counts are then indexed by the rank's local element.
template <int ET, bool SPLIT, bool BAND>
__global__ __launch_bounds__(256, 2) void k_snp_tile(const uint2 *__restrict__ P, int Wp, int n, long long t0,
                                                     long long items, int S, int Wk, double nFactor, double bs,
                                                     typename Elem<ET>::T *__restrict__ D, long long rowBegin,
                                                     long long rowEnd, unsigned *__restrict__ cnt, long long cbase,
                                                     const long long *__restrict__ pfx, int npanels, int rank,
                                                     int world) {
	__shared__ __attribute__((aligned(16))) uint2 As[2][KC * RS];
	__shared__ __attribute__((aligned(16))) uint2 Bs[2][KC * RS];
	int I, J;
	const long long item = t0 + xcd_tile(blockIdx.x, items);
	if(BAND) band_ij(pfx, npanels, item / S, I, J);
	else tile_ij(item / S, I, J);
	const Shard sh{rank, world};
	const int wb = (int) (item % S) * Wk, we = wb + Wk < Wp ? wb + Wk : Wp;
	const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
	// A-panel row l: Ap + arow(l) * Wp, the panel's own row l or (BAND) the rank's owned row I * TILE + l
	const uint2 *Ap = P + (BAND ? 0 : (size_t) I * TILE * Wp) + wb;
	const uint2 *Bp = P + (size_t) J * TILE * Wp + wb;
	const int Wl = we - wb;   // words of this slice (a multiple of KC)
	uint32_t acc[8][8];
#pragma unroll
	for(int a = 0; a < 8; ++a)
#pragma unroll
		for(int c = 0; c < 8; ++c) acc[a][c] = 0;
	// this thread's staging slots: rows e>>3, word pairs 2*(e&7), e = q*256 + tid
	uint4 va[4], vb[4];
	long long ar[4];
#pragma unroll
	for(int q = 0; q < 4; ++q) {
		const int e = q * 256 + threadIdx.x, row = e >> 3, wp = e & 7;
		ar[q] = BAND ? band_row(sh, (long long) I * TILE + row, n) : row;
		va[q] = *(const uint4 *) (Ap + (size_t) ar[q] * Wp + 2 * wp);
		vb[q] = *(const uint4 *) (Bp + (size_t) row * Wp + 2 * wp);
	}
#pragma unroll
	for(int q = 0; q < 4; ++q) {
		const int e = q * 256 + threadIdx.x, row = e >> 3, wp = e & 7;
		As[0][(2 * wp) * RS + row] = make_uint2(va[q].x, va[q].y);
		As[0][(2 * wp + 1) * RS + row] = make_uint2(va[q].z, va[q].w);
		Bs[0][(2 * wp) * RS + row] = make_uint2(vb[q].x, vb[q].y);
		Bs[0][(2 * wp + 1) * RS + row] = make_uint2(vb[q].z, vb[q].w);
	}
	__syncthreads();
	int buf = 0;
	for(int w0 = 0; w0 < Wl; w0 += KC, buf ^= 1) {
		const bool more = w0 + KC < Wl;
		if(more) {
#pragma unroll
			for(int q = 0; q < 4; ++q) {
				const int e = q * 256 + threadIdx.x, row = e >> 3, wp = e & 7;
				va[q] = *(const uint4 *) (Ap + (size_t) ar[q] * Wp + w0 + KC + 2 * wp);
				vb[q] = *(const uint4 *) (Bp + (size_t) row * Wp + w0 + KC + 2 * wp);
			}
		}
		const uint2 *Ac = As[buf], *Bc = Bs[buf];
#pragma unroll 1
		for(int w = 0; w < KC; ++w) {
			uint4 a[4], b[4];
#pragma unroll
			for(int q = 0; q < 4; ++q) {
				a[q] = *(const uint4 *) &Ac[w * RS + 2 * ty + 32 * q];
				b[q] = *(const uint4 *) &Bc[w * RS + 2 * tx + 32 * q];
			}
#pragma unroll
			for(int qa = 0; qa < 4; ++qa) {
#pragma unroll
				for(int qb = 0; qb < 4; ++qb) {
					acc[2 * qa][2 * qb] += __popc(xor_or(a[qa].x, b[qb].x, a[qa].y ^ b[qb].y));
					acc[2 * qa][2 * qb + 1] += __popc(xor_or(a[qa].x, b[qb].z, a[qa].y ^ b[qb].w));
					acc[2 * qa + 1][2 * qb] += __popc(xor_or(a[qa].z, b[qb].x, a[qa].w ^ b[qb].y));
					acc[2 * qa + 1][2 * qb + 1] += __popc(xor_or(a[qa].z, b[qb].z, a[qa].w ^ b[qb].w));
				}
			}
		}
		if(more) {
			uint2 *An = As[buf ^ 1], *Bn = Bs[buf ^ 1];
#pragma unroll
			for(int q = 0; q < 4; ++q) {
				const int e = q * 256 + threadIdx.x, row = e >> 3, wp = e & 7;
				An[(2 * wp) * RS + row] = make_uint2(va[q].x, va[q].y);
				An[(2 * wp + 1) * RS + row] = make_uint2(va[q].z, va[q].w);
				Bn[(2 * wp) * RS + row] = make_uint2(vb[q].x, vb[q].y);
				Bn[(2 * wp + 1) * RS + row] = make_uint2(vb[q].z, vb[q].w);
			}
		}
		__syncthreads();
	}
	// epilogue: D[i][j] = nFactor * dist (fsacmpthrd.c:247-255), j < i only
#pragma unroll
	for(int a = 0; a < 8; ++a) {
		const long long L = (long long) I * TILE + 2 * ty + 32 * (a >> 1) + (a & 1), i = BAND ? sh.global_row(L) : L;
		if(i >= n || (!BAND && (i < rowBegin || i >= rowEnd))) continue;
		const long long base = BAND ? sh.off(i) : tri(i);
#pragma unroll
		for(int c = 0; c < 8; ++c) {
			long long j = (long long) J * TILE + 2 * tx + 32 * (c >> 1) + (c & 1);
			if(j < i) {
				if(SPLIT) {
					atomicAdd(&cnt[base + j - cbase], acc[a][c]);
				} else {
					double v = nFactor * (double) acc[a][c];
					D[base + j] = Elem<ET>::put(v, 0.5, bs);
				}
			}
		}
	}
}

// ------------------------------------------------------------------ MFMA tiles (non-pair)
// fsacmp's count as a dot product on the matrix cores, exactly.  A 2-bit code
// (hi, lo) becomes the tetrahedron vector (s_hi, s_lo, s_hi s_lo) of +-1
// (s = 1 - 2 bit): equal codes dot to 3, different ones to -1, so over the
// L positions of a word slice (padding and the pre-masked positions are code
// 0 in every row: "equal")  dist = (3 L - dot) / 4.  The three components are
// MX-fp4 operands of v_mfma_scale_f32_32x32x64_f8f6f4 (e2m1 +1 = 0x2,
// -1 = 0xA, unit scales); f32 accumulation of the +-1 products is exact while
// |dot| <= 3 L < 2^24 (the host splits K beyond that).  A lane's operand for
// one 32x32x64 step is one 32-position plane word expanded to 32 nibbles
// (tools/micro/mfma_fp4: row = lane & 31, and A's (lane, nibble) meets B's
// (lane, nibble), so any fixed spread of the word's bits over the nibbles
// works if both panels use it): dword q holds bits q, q+4, ..., q+28 at the
// nibbles' sign bits, (x << (3 - q)) & 0x88888888 | 0x22222222, 2 VALU ops.
// Block = 4 waves on a 128x128 pair tile, each wave 64x64 (2x2 MFMA tiles,
// 3 components x 2 words of 32 positions per step); raw words staged through
// LDS as in k_snp_tile (double-buffered KC-word chunks, XCD-contiguous tile
// order, split-K over word slices).
typedef int v8i_t __attribute__((ext_vector_type(8)));
typedef float v16f_t __attribute__((ext_vector_type(16)));
#define MFMA_FP4 4
#define MFMA_SCALE1 127
#define MFMA_KMAX 174762   // words per slice: 3 * 32 * Wk < 2^24
#ifndef MFMA_UNROLL
#define MFMA_UNROLL 2
#endif
// k_snp_mfma's LDS chunk (words) and blocks per CU: 8-word chunks keep a
// block's double-buffered panels at 33 KB, so 3 blocks fit a CU's LDS
#ifndef KCM
#define KCM 8
#endif
#ifndef MFMA_BLOCKS
#define MFMA_BLOCKS 3
#endif
#define QS (TILE * KCM / 2 / 256)   // uint4 staged per thread per panel

// (a & b) | c in one v_bitop3_b32 (truth table 0xEA in xor_or's convention)
__device__ __forceinline__ uint32_t and_or(uint32_t a, uint32_t b, uint32_t c) {
	return __builtin_amdgcn_bitop3_b32(a, b, c, 0xEA);
}

__device__ __forceinline__ v8i_t fp4_spread(uint32_t x) {
	v8i_t v;
	v[0] = (int) and_or(x << 3, 0x88888888u, 0x22222222u);
	v[1] = (int) and_or(x << 2, 0x88888888u, 0x22222222u);
	v[2] = (int) and_or(x << 1, 0x88888888u, 0x22222222u);
	v[3] = (int) and_or(x, 0x88888888u, 0x22222222u);
	v[4] = v[5] = v[6] = v[7] = 0;
	return v;
}

template <int ET, bool SPLIT, bool BAND>
__global__ __launch_bounds__(256, MFMA_BLOCKS) void k_snp_mfma(const uint2 *__restrict__ P, int Wp, int n, long long t0,
                                                     long long items, int S, int Wk, double nFactor, double bs,
                                                     typename Elem<ET>::T *__restrict__ D, long long rowBegin,
                                                     long long rowEnd, unsigned *__restrict__ cnt, long long cbase,
                                                     const long long *__restrict__ pfx, int npanels, int rank,
                                                     int world) {
	__shared__ __attribute__((aligned(16))) uint2 As[2][KCM * RS];
	__shared__ __attribute__((aligned(16))) uint2 Bs[2][KCM * RS];
	int I, J;
	const long long item = t0 + xcd_tile(blockIdx.x, items);
	if(BAND) band_ij(pfx, npanels, item / S, I, J);
	else tile_ij(item / S, I, J);
	const Shard sh{rank, world};
	const int wb = (int) (item % S) * Wk, we = wb + Wk < Wp ? wb + Wk : Wp;
	const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
	const int wr = wid >> 1, wc = wid & 1;   // this wave's 64x64 quarter
	const uint2 *Ap = P + (BAND ? 0 : (size_t) I * TILE * Wp) + wb;   // row l at Ap + arow(l) * Wp, as k_snp_tile
	const uint2 *Bp = P + (size_t) J * TILE * Wp + wb;
	const int Wl = we - wb;   // words of this slice (a multiple of KC)
	v16f_t acc[2][2];
#pragma unroll
	for(int a = 0; a < 2; ++a)
#pragma unroll
		for(int c = 0; c < 2; ++c)
#pragma unroll
			for(int r = 0; r < 16; ++r) acc[a][c][r] = 0.0f;
	uint4 va[QS], vb[QS];
	long long ar[QS];
#pragma unroll
	for(int q = 0; q < QS; ++q) {
		const int e = q * 256 + threadIdx.x, row = e / (KCM / 2), wp = e % (KCM / 2);
		ar[q] = BAND ? band_row(sh, (long long) I * TILE + row, n) : row;
		va[q] = *(const uint4 *) (Ap + (size_t) ar[q] * Wp + 2 * wp);
		vb[q] = *(const uint4 *) (Bp + (size_t) row * Wp + 2 * wp);
	}
#pragma unroll
	for(int q = 0; q < QS; ++q) {
		const int e = q * 256 + threadIdx.x, row = e / (KCM / 2), wp = e % (KCM / 2);
		As[0][(2 * wp) * RS + row] = make_uint2(va[q].x, va[q].y);
		As[0][(2 * wp + 1) * RS + row] = make_uint2(va[q].z, va[q].w);
		Bs[0][(2 * wp) * RS + row] = make_uint2(vb[q].x, vb[q].y);
		Bs[0][(2 * wp + 1) * RS + row] = make_uint2(vb[q].z, vb[q].w);
	}
	__syncthreads();
	const int h = lane >> 5, l32 = lane & 31;
	const int ra0 = 64 * wr + l32, rb0 = 64 * wc + l32;
	int buf = 0;
	for(int w0 = 0; w0 < Wl; w0 += KCM, buf ^= 1) {
		const bool more = w0 + KCM < Wl;
		if(more) {
#pragma unroll
			for(int q = 0; q < QS; ++q) {
				const int e = q * 256 + threadIdx.x, row = e / (KCM / 2), wp = e % (KCM / 2);
				va[q] = *(const uint4 *) (Ap + (size_t) ar[q] * Wp + w0 + KCM + 2 * wp);
				vb[q] = *(const uint4 *) (Bp + (size_t) row * Wp + w0 + KCM + 2 * wp);
			}
		}
		const uint2 *Ac = As[buf], *Bc = Bs[buf];
#pragma unroll MFMA_UNROLL
		for(int s = 0; s < KCM / 2; ++s) {
			const int w = 2 * s + h;   // this lane's word: its half of the step's 64 positions
			uint2 a[2], b[2];
#pragma unroll
			for(int t = 0; t < 2; ++t) {
				a[t] = Ac[w * RS + ra0 + 32 * t];
				b[t] = Bc[w * RS + rb0 + 32 * t];
			}
#pragma unroll
			for(int comp = 0; comp < 3; ++comp) {
				v8i_t fa[2], fb[2];
#pragma unroll
				for(int t = 0; t < 2; ++t) {
					fa[t] = fp4_spread(comp == 0 ? a[t].x : comp == 1 ? a[t].y : a[t].x ^ a[t].y);
					fb[t] = fp4_spread(comp == 0 ? b[t].x : comp == 1 ? b[t].y : b[t].x ^ b[t].y);
				}
#pragma unroll
				for(int ta = 0; ta < 2; ++ta)
#pragma unroll
					for(int tb = 0; tb < 2; ++tb)
						acc[ta][tb] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(
						    fa[ta], fb[tb], acc[ta][tb], MFMA_FP4, MFMA_FP4, 0, MFMA_SCALE1, 0, MFMA_SCALE1);
			}
		}
		if(more) {
			uint2 *An = As[buf ^ 1], *Bn = Bs[buf ^ 1];
#pragma unroll
			for(int q = 0; q < QS; ++q) {
				const int e = q * 256 + threadIdx.x, row = e / (KCM / 2), wp = e % (KCM / 2);
				An[(2 * wp) * RS + row] = make_uint2(va[q].x, va[q].y);
				An[(2 * wp + 1) * RS + row] = make_uint2(va[q].z, va[q].w);
				Bn[(2 * wp) * RS + row] = make_uint2(vb[q].x, vb[q].y);
				Bn[(2 * wp + 1) * RS + row] = make_uint2(vb[q].z, vb[q].w);
			}
		}
		__syncthreads();
	}
	// epilogue: C/D of 32x32 (col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5));
	// dist = (3 L - dot) / 4 over the slice's L = 32 Wl positions
	const int L3 = 3 * 32 * Wl;
#pragma unroll
	for(int ta = 0; ta < 2; ++ta) {
#pragma unroll
		for(int r = 0; r < 16; ++r) {
			const long long L = (long long) I * TILE + 64 * wr + 32 * ta + (r & 3) + 8 * (r >> 2) + 4 * h;
			const long long i = BAND ? sh.global_row(L) : L;
			if(i >= n || (!BAND && (i < rowBegin || i >= rowEnd))) continue;
			const long long base = BAND ? sh.off(i) : tri(i);
#pragma unroll
			for(int tb = 0; tb < 2; ++tb) {
				const long long j = (long long) J * TILE + 64 * wc + 32 * tb + l32;
				if(j < i) {
					const unsigned d = (unsigned) ((L3 - (int) acc[ta][tb][r]) >> 2);
					if(SPLIT) {
						atomicAdd(&cnt[base + j - cbase], d);
					} else {
						const double v = nFactor * (double) d;
						D[base + j] = Elem<ET>::put(v, 0.5, bs);
					}
				}
			}
		}
	}
}

// ------------------------------------------------------------------ MFMA, 256 x 256 tiles
// k_snp_mfma2: the same exact MX-fp4 form on 256 x 256 pair tiles, one block of
// 4 waves per CU, each wave 128 x 128 (4 x 4 MFMA tiles, 256 accumulator
// VGPRs).  Per 64-position step a lane spreads its 4 A and 4 B plane words
// once per component and feeds 16 MFMAs with them (k_snp_mfma: 4 spreads per
// 4 MFMAs), and the third component (hi ^ lo) comes from the first two
// spreads in one v_bitop3 per dword ((a ^ b) | 0x22222222: the sign bits
// xor, the 0x2 exponent bits cancel and are set again), so the VALU work per
// MFMA drops about 3x and each staged panel byte feeds twice the position
// pairs (half the panel traffic into the CUs).  BAND: the A panel gathers
// one rank's owned rows of the band layout (as k_snp_tile), D indexed by
// Shard::off.  SPLIT: word slice item % S of Wk words, exact u32 counts.
#define TILE2 256
#define KC2 8                          // words per LDS chunk (the default; KC2L with CCG_DIST_KC=16)
#define KC2L 16
#define RS2 260                        // LDS row stride (uint2): 16-byte aligned rows of 256 + pad

// Super-tile order of the LT's 256 x 256 tiles (CCG_DIST_ORDER=1): super-rows
// of 4 panel rows; inside one, column chunks of 8 panels (4 x 8 = 32 tiles,
// one XCD's 32 CUs at a time under xcd_tile), row-major inside a chunk, then
// the diagonal remainder J in [8F, I] row-major.  A super-row starts at the
// same tile index as in row-major order (T(P) = 4P (4P + 1) / 2), so the
// row-major row of t names its super-row; a super-row cut by the last panel
// row Ihi (the end of the range) stays row-major.  The 32 tiles an XCD runs
// together then read 4 A + 8 B panels (row-major: 1 + 32), in step along K.
__device__ __forceinline__ void tile_ij_super(long long t, long long Ihi, int &I, int &J) {
	int r, c;
	tile_ij(t, r, c);
	const long long P = r >> 2, I0 = 4 * P;
	if(I0 + 3 > Ihi) {
		I = r;
		J = c;
		return;
	}
	const long long u = t - I0 * (I0 + 1) / 2, F = P >> 1;   // F full chunks: J < 8F <= I0
	if(u < 32 * F) {
		const int v = (int) (u & 31);
		I = (int) I0 + (v >> 3);
		J = 8 * (int) (u >> 5) + (v & 7);
		return;
	}
	long long w = u - 32 * F;
	int i = (int) I0;
	while(w >= i - 8 * F + 1) {
		w -= i - 8 * F + 1;
		++i;
	}
	I = i;
	J = (int) (8 * F + w);
}

__device__ __forceinline__ v8i_t fp4_xor_spread(const v8i_t &a, const v8i_t &b) {
	v8i_t v;
#pragma unroll
	for(int q = 0; q < 4; ++q) v[q] = (int) xor_or((uint32_t) a[q], (uint32_t) b[q], 0x22222222u);
	v[4] = v[5] = v[6] = v[7] = 0;
	return v;
}

// fp4_spread and fp4_xor_spread in two halves (dwords 0, 1: 4 / 2 VALU; dwords
// 2, 3: 3 / 2 VALU), for k_snp_mfma3's one half per MFMA gap
__device__ __forceinline__ void fp4_spread_half(v8i_t &v, uint32_t x, int hf) {
	if(hf == 0) {
		v[0] = (int) and_or(x << 3, 0x88888888u, 0x22222222u);
		v[1] = (int) and_or(x << 2, 0x88888888u, 0x22222222u);
		v[4] = v[5] = v[6] = v[7] = 0;
	} else {
		v[2] = (int) and_or(x << 1, 0x88888888u, 0x22222222u);
		v[3] = (int) and_or(x, 0x88888888u, 0x22222222u);
	}
}

__device__ __forceinline__ void fp4_xor_spread_half(v8i_t &v, const v8i_t &a, const v8i_t &b, int hf) {
	if(hf == 0) v[4] = v[5] = v[6] = v[7] = 0;
#pragma unroll
	for(int q = 2 * hf; q < 2 * hf + 2; ++q) v[q] = (int) xor_or((uint32_t) a[q], (uint32_t) b[q], 0x22222222u);
}

template <int ET, bool SPLIT, bool BAND, int KCW = KC2>
__global__ __launch_bounds__(256, 1) void k_snp_mfma2(const uint2 *__restrict__ P, int Wp, int n, long long t0,
                                                      long long items, int S, int Wk, double nFactor, double bs,
                                                      typename Elem<ET>::T *__restrict__ D, long long rowBegin,
                                                      long long rowEnd, unsigned *__restrict__ cnt, long long cbase,
                                                      const long long *__restrict__ pfx, int npanels, int rank,
                                                      int world, int sorder) {
	constexpr int QS2 = TILE2 * KCW / 2 / 256, WPR = KCW / 2;   // uint4 staged per thread per panel; per row
	__shared__ __attribute__((aligned(16))) uint2 As[2][KCW * RS2];
	__shared__ __attribute__((aligned(16))) uint2 Bs[2][KCW * RS2];
	const long long item = t0 + xcd_tile(blockIdx.x, items), t = SPLIT ? item / S : item;
	int I, J;
	if(BAND) {   // tile t of the rank's list: panel I = last with pfx[I] <= t, J = t - pfx[I]
		int lo = 0, hi = npanels - 1;
		while(lo < hi) {
			const int mid = (lo + hi + 1) >> 1;
			if(pfx[mid] <= t) lo = mid; else hi = mid - 1;
		}
		I = lo;
		J = (int) (t - pfx[lo]);
	} else if(sorder) {
		tile_ij_super(t, (rowEnd - 1) / TILE2, I, J);
	} else {
		tile_ij(t, I, J);
	}
	const int wb = SPLIT ? (int) (item % S) * Wk : 0;
	const int Wl = SPLIT ? (wb + Wk < Wp ? Wk : Wp - wb) : Wp;
	const Shard sh{rank, world};
	// the A panel's row l: I * TILE2 + l, or the rank's owned row of that local
	// index (rows past n stage row 0 and are never stored)
	const auto arow = [&](int l) -> long long {
		const long long L = (long long) I * TILE2 + l;
		if(!BAND) return L;
		const long long lb = L / SB, r = (lb * world + rank) * SB + (L - lb * SB);
		return r < n ? r : 0;
	};
	const uint2 *Bp = P + (size_t) J * TILE2 * Wp + wb;
	long long ar[QS2];
	uint4 va[QS2], vb[QS2];
#pragma unroll
	for(int q = 0; q < QS2; ++q) {
		const int e = q * 256 + threadIdx.x, row = e / WPR, wp = e % WPR;
		ar[q] = arow(row);
		va[q] = *(const uint4 *) (P + (size_t) ar[q] * Wp + wb + 2 * wp);
		vb[q] = *(const uint4 *) (Bp + (size_t) row * Wp + 2 * wp);
	}
#pragma unroll
	for(int q = 0; q < QS2; ++q) {
		const int e = q * 256 + threadIdx.x, row = e / WPR, wp = e % WPR;
		As[0][(2 * wp) * RS2 + row] = make_uint2(va[q].x, va[q].y);
		As[0][(2 * wp + 1) * RS2 + row] = make_uint2(va[q].z, va[q].w);
		Bs[0][(2 * wp) * RS2 + row] = make_uint2(vb[q].x, vb[q].y);
		Bs[0][(2 * wp + 1) * RS2 + row] = make_uint2(vb[q].z, vb[q].w);
	}
	__syncthreads();
	const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
	const int wr = wid >> 1, wc = wid & 1;
	const int h = lane >> 5, l32 = lane & 31;
	const int ra0 = 128 * wr + l32, rb0 = 128 * wc + l32;
	v16f_t acc[4][4];
#pragma unroll
	for(int a = 0; a < 4; ++a)
#pragma unroll
		for(int c = 0; c < 4; ++c)
#pragma unroll
			for(int r = 0; r < 16; ++r) acc[a][c][r] = 0.0f;
	int buf = 0;
	for(int w0 = 0; w0 < Wl; w0 += KCW, buf ^= 1) {
		const bool more = w0 + KCW < Wl;
		if(more) {
#pragma unroll
			for(int q = 0; q < QS2; ++q) {
				const int e = q * 256 + threadIdx.x, row = e / WPR, wp = e % WPR;
				va[q] = *(const uint4 *) (P + (size_t) ar[q] * Wp + wb + w0 + KCW + 2 * wp);
				vb[q] = *(const uint4 *) (Bp + (size_t) row * Wp + w0 + KCW + 2 * wp);
			}
		}
		const uint2 *Ac = As[buf], *Bc = Bs[buf];
#pragma unroll
		for(int s = 0; s < KCW / 2; ++s) {
			const int w = 2 * s + h;   // this lane's word: its half of the step's 64 positions
			uint2 a[4], b[4];
#pragma unroll
			for(int x = 0; x < 4; ++x) {
				a[x] = Ac[w * RS2 + ra0 + 32 * x];
				b[x] = Bc[w * RS2 + rb0 + 32 * x];
			}
			v8i_t f0[4], g0[4], f1[4], g1[4];
#pragma unroll
			for(int x = 0; x < 4; ++x) {
				f0[x] = fp4_spread(a[x].x);
				g0[x] = fp4_spread(b[x].x);
			}
#pragma unroll
			for(int ta = 0; ta < 4; ++ta)
#pragma unroll
				for(int tb = 0; tb < 4; ++tb)
					acc[ta][tb] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(
					    f0[ta], g0[tb], acc[ta][tb], MFMA_FP4, MFMA_FP4, 0, MFMA_SCALE1, 0, MFMA_SCALE1);
#pragma unroll
			for(int x = 0; x < 4; ++x) {
				f1[x] = fp4_spread(a[x].y);
				g1[x] = fp4_spread(b[x].y);
			}
#pragma unroll
			for(int ta = 0; ta < 4; ++ta)
#pragma unroll
				for(int tb = 0; tb < 4; ++tb)
					acc[ta][tb] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(
					    f1[ta], g1[tb], acc[ta][tb], MFMA_FP4, MFMA_FP4, 0, MFMA_SCALE1, 0, MFMA_SCALE1);
#pragma unroll
			for(int x = 0; x < 4; ++x) {
				f0[x] = fp4_xor_spread(f0[x], f1[x]);
				g0[x] = fp4_xor_spread(g0[x], g1[x]);
			}
#pragma unroll
			for(int ta = 0; ta < 4; ++ta)
#pragma unroll
				for(int tb = 0; tb < 4; ++tb)
					acc[ta][tb] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(
					    f0[ta], g0[tb], acc[ta][tb], MFMA_FP4, MFMA_FP4, 0, MFMA_SCALE1, 0, MFMA_SCALE1);
		}
		if(more) {
			uint2 *An = As[buf ^ 1], *Bn = Bs[buf ^ 1];
#pragma unroll
			for(int q = 0; q < QS2; ++q) {
				const int e = q * 256 + threadIdx.x, row = e / WPR, wp = e % WPR;
				An[(2 * wp) * RS2 + row] = make_uint2(va[q].x, va[q].y);
				An[(2 * wp + 1) * RS2 + row] = make_uint2(va[q].z, va[q].w);
				Bn[(2 * wp) * RS2 + row] = make_uint2(vb[q].x, vb[q].y);
				Bn[(2 * wp + 1) * RS2 + row] = make_uint2(vb[q].z, vb[q].w);
			}
		}
		__syncthreads();
	}
	// epilogue: C/D of 32x32 (col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5));
	// dist = (3 L - dot) / 4 over the slice's L = 32 Wl positions
	const int L3 = 3 * 32 * Wl;
#pragma unroll
	for(int ta = 0; ta < 4; ++ta) {
#pragma unroll
		for(int r = 0; r < 16; ++r) {
			const int l = 128 * wr + 32 * ta + (r & 3) + 8 * (r >> 2) + 4 * h;
			const long long L = (long long) I * TILE2 + l;
			long long i = L;
			if(BAND) {
				const long long lb = L / SB;
				i = (lb * world + rank) * SB + (L - lb * SB);
			}
			if(i >= n || (!BAND && (i < rowBegin || i >= rowEnd))) continue;
			const long long base = BAND ? sh.off(i) : tri(i);
#pragma unroll
			for(int tb = 0; tb < 4; ++tb) {
				const long long j = (long long) J * TILE2 + 128 * wc + 32 * tb + l32;
				if(j < i) {
					const unsigned d = (unsigned) ((L3 - (int) acc[ta][tb][r]) >> 2);
					if(SPLIT) {
						atomicAdd(&cnt[base + j - cbase], d);
					} else {
						const double v = nFactor * (double) d;
						D[base + j] = Elem<ET>::put(v, 0.5, bs);
					}
				}
			}
		}
	}
}

// ------------------------------------------------------------------ MFMA, 256 x 256 tiles, LDS-DMA staged
// k_snp_mfma3: k_snp_mfma2's tile, its MX-fp4 steps and its epilogue, with the
// panels staged by global_load_lds (no VGPR staging, no ds_write) through
// NST3 stages of LDS, so that NST3 - 2 chunks stay in flight across each
// barrier (cdna_hip_programming.md, "Pipelining across barriers": counted
// vmcnt, raw s_barrier).  At one block per CU and 512 VGPRs the round-4/5
// kernel had one chunk of register staging in flight and waited for it
// before every barrier.  LDS image, one array: [stage][panel][slice][row] of
// 16 bytes (two plane words of one row), so one wave-instruction (64 lanes x
// 16 B, lane-linear) writes 64 consecutive rows of one slice, and a step's
// 8-byte reads (row ra0 + 32x, word 2s + h) are 512 contiguous bytes per
// wave.  Wave w stages slice w of both panels: 4 + 4 instructions per chunk.
#define NST3 4
#define KC3 8
// CCG_DIST_STAMPS (the Makefile's `stamps` target, a diagnostic engine loaded
// through CCPHYLO_AMD_ENGINE): k_snp_mfma3 stamps s_memtime around the parts
// of each chunk of its main loop and sums the differences per part; lane 0 of
// waves 0 and 3 store the sums to a buffer of their own, [item][wave][8]:
// steps 0, 1, 2, step 3 up to the counted wait, the wait and the barrier,
// component 1 of step 3, the rest of step 3, the chunks summed.
// The stamps fence the schedule (sched_barrier) and drain the LDS reads in
// flight, so the shares are the record, not the run time.  The normal build
// holds no stamp.
#ifdef CCG_DIST_STAMPS
#define ST3_SLOTS 8
__device__ unsigned long long *ccg_dist_stamp_buf;
__device__ long long ccg_dist_stamp_item0;
#define ST3(K)                                                                              \
	do {                                                                                    \
		unsigned long long tn_;                                                             \
		__builtin_amdgcn_sched_barrier(0);                                                  \
		asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(tn_)::"memory");         \
		__builtin_amdgcn_sched_barrier(0);                                                  \
		if((K) >= 0) stamp_sum[(K) < 0 ? 0 : (K)] += tn_ - stamp_prev;                      \
		stamp_prev = tn_;                                                                   \
	} while(0)
#else
#define ST3(K)
#endif
template <int ET, bool SPLIT, bool BAND>
__global__ __launch_bounds__(256, 1) void k_snp_mfma3(const uint2 *__restrict__ P, int Wp, int n, long long t0,
                                                      long long items, int S, int Wk, double nFactor, double bs,
                                                      typename Elem<ET>::T *__restrict__ D, long long rowBegin,
                                                      long long rowEnd, unsigned *__restrict__ cnt, long long cbase,
                                                      const long long *__restrict__ pfx, int npanels, int rank,
                                                      int world, int sorder) {
	constexpr int NSL = KC3 / 2;   // 16-byte slices per chunk (one per wave)
	static_assert(NSL == 4, "one slice per wave");
	__shared__ __attribute__((aligned(16))) uint4 L[NST3 * 2 * NSL * TILE2];   // 128 KB
	const long long item = t0 + xcd_tile(blockIdx.x, items), t = SPLIT ? item / S : item;
	int I, J;
	if(BAND) {
		int lo = 0, hi = npanels - 1;
		while(lo < hi) {
			const int mid = (lo + hi + 1) >> 1;
			if(pfx[mid] <= t) lo = mid; else hi = mid - 1;
		}
		I = lo;
		J = (int) (t - pfx[lo]);
	} else if(sorder) {
		tile_ij_super(t, (rowEnd - 1) / TILE2, I, J);
	} else {
		tile_ij(t, I, J);
	}
	const int wb = SPLIT ? (int) (item % S) * Wk : 0;
	const int Wl = SPLIT ? (wb + Wk < Wp ? Wk : Wp - wb) : Wp;
	const Shard sh{rank, world};
	const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
	// this lane's staging sources: rows q 64 + lane of both panels, words 2 wid, 2 wid + 1 of each chunk
	const uint2 *srcA[4], *srcB[4];
#pragma unroll
	for(int q = 0; q < 4; ++q) {
		const long long Lr = (long long) I * TILE2 + q * 64 + lane;
		long long r = Lr;
		if(BAND) {
			const long long lb = Lr / SB;
			r = (lb * world + rank) * SB + (Lr - lb * SB);
			r = r < n ? r : 0;   // rows past n stage row 0 and are never stored
		}
		srcA[q] = P + (size_t) r * Wp + wb + 2 * wid;
		srcB[q] = P + ((size_t) J * TILE2 + q * 64 + lane) * Wp + wb + 2 * wid;
	}
	const int nch = Wl / KC3;
	// one LDS-DMA wave-instruction (64 lanes x 16 B, lane-linear at the
	// wave-uniform LDS byte address lds): in inline asm, so that the compiler
	// does not drain vmcnt(0) before every ds_read of the array (it cannot
	// tell the stages apart); the counted waits below order the reads
	const unsigned lbase = (unsigned) (uintptr_t) (__attribute__((address_space(3))) uint4 *) L;
	auto glds = [&](const uint2 *src, unsigned lds) {
		unsigned keep;
		asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
		             : "=&s"(keep)
		             : "v"(src), "s"(lds)
		             : "memory");
	};
	// this wave's slice of stage 0, panel A, in an SGPR: a piece's LDS address is scalar arithmetic on it
	const unsigned lwave = (unsigned) __builtin_amdgcn_readfirstlane((int) (lbase + (unsigned) (wid * TILE2 * 16)));
	auto issue1 = [&](int c, int i) {   // piece i of chunk c's 8 (rows 64 (i / 2) .. + 63 of panel i % 2) into stage c % NST3
		const int st = c % NST3, w0 = c * KC3, q = i >> 1, p = i & 1;
		glds((p ? srcB[q] : srcA[q]) + w0, lwave + (unsigned) ((((st * 2 + p) * NSL) * TILE2 + q * 64) * 16));
	};
	auto issue = [&](int c) {
#pragma unroll
		for(int i = 0; i < 8; ++i) issue1(c, i);
	};
	const int wr = wid >> 1, wc = wid & 1;
	const int h = lane >> 5, l32 = lane & 31;
	const int ra0 = 128 * wr + l32, rb0 = 128 * wc + l32;
	v16f_t acc[4][4];
#pragma unroll
	for(int ta = 0; ta < 4; ++ta)
#pragma unroll
		for(int tb = 0; tb < 4; ++tb)
#pragma unroll
			for(int r = 0; r < 16; ++r) acc[ta][tb][r] = 0.0f;
	// chunk c landed for every wave: this wave's counted wait (the later chunks
	// stay in flight), then the raw barrier
	auto land = [&](int c) {
		const int ahead = nch - 1 - c < NST3 - 2 ? nch - 1 - c : NST3 - 2;
		if(ahead >= 2) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
		else if(ahead == 1) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
		else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
		asm volatile("" ::: "memory");
		__builtin_amdgcn_s_barrier();
		asm volatile("" ::: "memory");
	};
	// step gs (64 positions): word 2 (gs % 4) + h of chunk gs / 4, rows ra0 + 32 x / rb0 + 32 x
	auto rd1 = [&](int gs, int p, uint2 (&v)[4]) {   // panel p (0: A, 1: B)
		const int st = (gs >> 2) % NST3, sl = gs & 3;
		const uint2 *Pc = (const uint2 *) &L[((st * 2 + p) * NSL + sl) * TILE2];
#pragma unroll
		for(int x = 0; x < 4; ++x) v[x] = Pc[((p ? rb0 : ra0) + 32 * x) * 2 + h];
	};
	auto rd = [&](int gs, uint2 (&a)[4], uint2 (&b)[4]) {
		rd1(gs, 0, a);
		rd1(gs, 1, b);
	};
#define MF3(TA, TB, F, G)                                                                                         \
	acc[TA][TB] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(F, G, acc[TA][TB], MFMA_FP4, MFMA_FP4, 0, MFMA_SCALE1, \
	                                                              0, MFMA_SCALE1)
	for(int c = 0; c < NST3 - 1 && c < nch; ++c) issue(c);
	land(0);
	uint2 a[4], b[4];
	v8i_t f0[4], g0[4];
	rd(0, a, b);
#pragma unroll
	for(int x = 0; x < 4; ++x) {
		f0[x] = fp4_spread(a[x].x);
		g0[x] = fp4_spread(b[x].x);
	}
#ifdef CCG_DIST_STAMPS
	unsigned long long stamp_sum[ST3_SLOTS] = {0, 0, 0, 0, 0, 0, 0, 0}, stamp_prev = 0;
#endif
	// Each component's 16 MFMAs carry the VALU work of the next component, so
	// the matrix pipe does not idle while a wave spreads (k_snp_mfma2: 16 MFMAs,
	// then the spreads; ~60% MFMA busy, profiles/r06_dist_clock.json):
	//   comp 0 (f0, g0) + the spreads of lo (f1, g1)
	//   comp 1 (f1, g1) + the xors (x0, y0), the next step's LDS reads
	//   comp 2 (x0, y0) + the next step's spreads of hi (f0, g0)
	// and two of the 8 DMA pieces of chunk c + NST3 - 1 in each of chunk c's four
	// steps (PC3 / PK3 below)
	// The order is written out gap by gap and fenced: one MFMA, half a spread
	// (4 or 3 VALU) or half an xor (2 VALU), then sched_barrier(0), so no gap
	// holds more than 4 VALU (5 with a piece's address add) and the compiler
	// cannot gather them (tools/micro/mfma_valu: up to 5 hide beside an MFMA).
	// The operands are made in the order the next component reads them
	// (ORD: f[0], g[0..3], f[1..3]), each at least 3 MFMAs before its reader.
	// A chunk's last step waits for the next chunk (counted vmcnt + barrier)
	// between comp 0 and comp 1, fenced on both sides, so that step's reads
	// follow the barrier.
	// The ring's pieces.  Chunk x lives in stage x % NST3.  Iteration c of the
	// steady loop issues the pieces of chunk c + NST3 - 1 into the stage of
	// chunk c - 1: free, because every wave passed the barrier in chunk c - 1's
	// last step, and each had consumed its last LDS reads of that chunk (the
	// .y words of step 4 c - 1, spread in that step's comp 0) before it arrived
	// there.  Two pieces per step, in gaps that carry no LDS read, never in
	// adjacent gaps, so that the four waves' 1-KiB pieces do not queue behind
	// each other (all 8 in one component ran at the CU's LDS-DMA rate, ~120
	// cycles a piece).  Step 3's two go before the counted wait: at that wait
	// chunks c + 1, c + 2 and c + 3 are outstanding, 24 pieces issued in that
	// order, so vmcnt(16) is exactly "chunk c + 1 landed".  The prologue issues
	// chunks 0 .. NST3 - 2 only.  The steady loop ends with c = nch - NST3 + 1:
	// the second copy starts with chunks c + 1 .. nch - 1 outstanding, which is
	// what land()'s run-time count assumes.
#define GAP3() __builtin_amdgcn_sched_barrier(0)
	// PC3(s, i) / PK3(s, i): the component and the gap of piece 2 s + i in step s of a chunk: component 1's
	// gaps 5 and 11 (its gaps 0 and 1 carry the LDS reads); in step 3 component 0's, before the wait
#define PC3(S, I) ((S) == 3 ? 0 : 1)
#define PK3(S, I) ((I) ? 11 : 5)
	// OPEN: 0 = no chunk opens here; 1 = the next chunk opens, nothing left to
	// issue (the last NST3 - 2 opens of a tile); 2 = it opens in the steady loop:
	// 2 chunks stay in flight (vmcnt(16), known at compile time).
	// ISS: -1, or this step's index in its chunk: it issues pieces 2 ISS, 2 ISS + 1
	auto step = [&](auto OPEN, auto MORE, auto ISS, int gs) {
		constexpr int open = decltype(OPEN)::value;
		constexpr bool more = decltype(MORE)::value;
		constexpr int iss = decltype(ISS)::value;
		const int ci = (gs >> 2) + NST3 - 1;   // iss >= 0: the chunk whose pieces 2 iss, 2 iss + 1 this step issues
		v8i_t f1[4], g1[4], x0[4], y0[4];
#pragma unroll
		for(int k = 0; k < 16; ++k) {
			MF3(k >> 2, k & 3, f0[k >> 2], g0[k & 3]);
			const int j = k >> 1;   // operand j of ORD
			if(j == 0 || j > 4) fp4_spread_half(f1[j ? j - 4 : 0], a[j ? j - 4 : 0].y, k & 1);
			else fp4_spread_half(g1[j - 1], b[j - 1].y, k & 1);
			if(iss >= 0 && PC3(iss, 0) == 0 && k == PK3(iss, 0)) issue1(ci, 2 * iss);
			if(iss >= 0 && PC3(iss, 1) == 0 && k == PK3(iss, 1)) issue1(ci, 2 * iss + 1);
			GAP3();
		}
		const int cn = (gs + 1) >> 2;   // open: the next step opens chunk cn
		if(open) {
			ST3(3);
			GAP3();
			if(open == 2) {
				asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
				asm volatile("" ::: "memory");
				__builtin_amdgcn_s_barrier();
				asm volatile("" ::: "memory");
			} else {
				land(cn);
			}
			GAP3();
			ST3(4);
		}
		uint2 an[4], bn[4];
#pragma unroll
		for(int k = 0; k < 16; ++k) {
			MF3(k >> 2, k & 3, f1[k >> 2], g1[k & 3]);
			const int j = k >> 1;
			if(j == 0 || j > 4) fp4_xor_spread_half(x0[j ? j - 4 : 0], f0[j ? j - 4 : 0], f1[j ? j - 4 : 0], k & 1);
			else fp4_xor_spread_half(y0[j - 1], g0[j - 1], g1[j - 1], k & 1);
			if(more && k == 0) rd1(gs + 1, 0, an);   // the next step's LDS reads, behind the barrier: A, then B
			if(more && k == 1) rd1(gs + 1, 1, bn);
			if(iss >= 0 && PC3(iss, 0) == 1 && k == PK3(iss, 0)) issue1(ci, 2 * iss);
			if(iss >= 0 && PC3(iss, 1) == 1 && k == PK3(iss, 1)) issue1(ci, 2 * iss + 1);
			GAP3();
		}
		if(open == 2) ST3(5);
#pragma unroll
		for(int k = 0; k < 16; ++k) {
			MF3(k >> 2, k & 3, x0[k >> 2], y0[k & 3]);
			if(more) {
				const int j = k >> 1;
				if(j == 0 || j > 4) fp4_spread_half(f0[j ? j - 4 : 0], an[j ? j - 4 : 0].x, k & 1);
				else fp4_spread_half(g0[j - 1], bn[j - 1].x, k & 1);
			}
			if(iss >= 0 && PC3(iss, 0) == 2 && k == PK3(iss, 0)) issue1(ci, 2 * iss);
			if(iss >= 0 && PC3(iss, 1) == 2 && k == PK3(iss, 1)) issue1(ci, 2 * iss + 1);
			GAP3();
		}
		if(more) {
#pragma unroll
			for(int x = 0; x < 4; ++x) {
				a[x] = an[x];
				b[x] = bn[x];
			}
		}
	};
	typedef std::integral_constant<int, 0> O0;
	typedef std::integral_constant<int, 1> O1;
	typedef std::integral_constant<int, 2> O2;
	typedef std::integral_constant<int, -1> NI;
	typedef std::true_type MT;
	ST3(-1);
	int c = 0;
	for(; c + NST3 - 1 < nch; ++c) {   // 4 steps, each issues 2 pieces of chunk c + NST3 - 1; the last one opens chunk c + 1
		step(O0(), MT(), std::integral_constant<int, 0>(), 4 * c + 0);
		ST3(0);
		step(O0(), MT(), std::integral_constant<int, 1>(), 4 * c + 1);
		ST3(1);
		step(O0(), MT(), std::integral_constant<int, 2>(), 4 * c + 2);
		ST3(2);
		step(O2(), MT(), std::integral_constant<int, 3>(), 4 * c + 3);
		ST3(6);
	}
	for(; c + 1 < nch; ++c) {   // the chunks with nothing left to issue, but the last
		step(O0(), MT(), NI(), 4 * c + 0);
		step(O0(), MT(), NI(), 4 * c + 1);
		step(O0(), MT(), NI(), 4 * c + 2);
		step(O1(), MT(), NI(), 4 * c + 3);
	}
#ifdef CCG_DIST_STAMPS
	if(ccg_dist_stamp_buf && lane == 0 && (wid == 0 || wid == 3)) {
		stamp_sum[7] = nch > NST3 - 1 ? nch - (NST3 - 1) : 0;
		unsigned long long *sb =
		    ccg_dist_stamp_buf + ((t0 - ccg_dist_stamp_item0 + blockIdx.x) * 2 + (wid ? 1 : 0)) * ST3_SLOTS;
		for(int k = 0; k < ST3_SLOTS; ++k) sb[k] = stamp_sum[k];
	}
#endif
	{   // the last chunk
		const int g = 4 * (nch - 1);
		step(O0(), MT(), NI(), g + 0);
		step(O0(), MT(), NI(), g + 1);
		step(O0(), MT(), NI(), g + 2);
		step(O0(), std::false_type(), NI(), g + 3);
	}
#undef MF3
#undef GAP3
#undef PC3
#undef PK3
	// epilogue: k_snp_mfma2's
	const int L3 = 3 * 32 * Wl;
#pragma unroll
	for(int ta = 0; ta < 4; ++ta) {
#pragma unroll
		for(int r = 0; r < 16; ++r) {
			const int l = 128 * wr + 32 * ta + (r & 3) + 8 * (r >> 2) + 4 * h;
			const long long Lr = (long long) I * TILE2 + l;
			long long i = Lr;
			if(BAND) {
				const long long lb = Lr / SB;
				i = (lb * world + rank) * SB + (Lr - lb * SB);
			}
			if(i >= n || (!BAND && (i < rowBegin || i >= rowEnd))) continue;
			const long long base = BAND ? sh.off(i) : tri(i);
#pragma unroll
			for(int tb = 0; tb < 4; ++tb) {
				const long long j = (long long) J * TILE2 + 128 * wc + 32 * tb + l32;
				if(j < i) {
					const unsigned d = (unsigned) ((L3 - (int) acc[ta][tb][r]) >> 2);
					if(SPLIT) {
						atomicAdd(&cnt[base + j - cbase], d);
					} else {
						const double v = nFactor * (double) d;
						D[base + j] = Elem<ET>::put(v, 0.5, bs);
					}
				}
			}
		}
	}
}

// split-K epilogue: D[f] = nFactor * count (fsacmpthrd.c:247-255)
template <int ET>
__global__ void k_snp_finish(const unsigned *__restrict__ cnt, long long cbase, long long f0, long long f1,
                             double nFactor, double bs, typename Elem<ET>::T *__restrict__ D) {
	for(long long f = f0 + (long long) blockIdx.x * blockDim.x + threadIdx.x; f < f1;
	    f += (long long) gridDim.x * blockDim.x) {
		D[f] = Elem<ET>::put(nFactor * (double) cnt[f - cbase], 0.5, bs);
	}
}

// A7 epilogue (fsacmpthrd.c:420-475) for one pair
template <int ET>
__device__ __forceinline__ void pair_store(typename Elem<ET>::T *D, typename Elem<ET>::T *N, long long f, uint32_t dist,
                                           uint32_t inc, unsigned norm, unsigned minLength, double bs) {
	typedef typename Elem<ET>::T T;
	if(ET == 8) {
		double v;
		if(minLength <= inc) {
			v = norm ? (double) ((unsigned long long) dist * norm) / inc : (double) dist;
		} else {
			v = -1.0;
		}
		D[f] = (T) v;
		if(N) N[f] = (T) (double) inc;
	} else if(ET == 4) {
		float v;
		if(minLength <= inc) {
			if(norm) {
				v = (float) ((unsigned long long) dist * norm);
				v = v / (float) inc;
			} else {
				v = (float) dist;
			}
		} else {
			v = -1.0f;
		}
		D[f] = (T) v;
		if(N) N[f] = (T) (float) inc;
	} else {
		double v;
		if(minLength <= inc) {
			v = norm ? ((double) ((unsigned long long) dist * norm) * bs + 0.5) / inc : (double) dist * bs + 0.5;
		} else {
			v = -1.0 * bs + 0;
		}
		D[f] = (T) cvt_i32_x86(v);
		if(N) N[f] = (T) cvt_i32_x86(inc * bs + 0.5);
	}
}

// Pair tiles: as k_snp_tile, with each taxon's mask beside its planes
// (uint4 {hi, lo, m, 0} per word): double-buffered KCP-word chunks of both
// 128-row panels, XCD-contiguous tile order, and split-K over word slices when
// the tiles do not fill the chip (exact u32 atomics of dist and n, then
// k_snp_pair_finish applies the A7 epilogue).  BAND as in k_snp_tile (no N).
template <int ET, bool SPLIT, bool BAND>
__global__ __launch_bounds__(256, 2) void k_snp_tile_pair(const uint4 *__restrict__ P, int Wp, int n, long long t0,
                                                          long long items, int S, int Wk, unsigned norm,
                                                          unsigned minLength, double bs,
                                                          typename Elem<ET>::T *__restrict__ D,
                                                          typename Elem<ET>::T *__restrict__ Nm, long long rowBegin,
                                                          long long rowEnd, unsigned *__restrict__ cd,
                                                          unsigned *__restrict__ cn, long long cbase,
                                                          const long long *__restrict__ pfx, int npanels, int rank,
                                                          int world) {
	__shared__ __attribute__((aligned(16))) uint4 As[2][KCP * RSP];
	__shared__ __attribute__((aligned(16))) uint4 Bs[2][KCP * RSP];
	int I, J;
	const long long item = t0 + xcd_tile(blockIdx.x, items);
	if(BAND) band_ij(pfx, npanels, item / S, I, J);
	else tile_ij(item / S, I, J);
	const Shard sh{rank, world};
	const int wb = (int) (item % S) * Wk, we = wb + Wk < Wp ? wb + Wk : Wp;
	const int Wl = we - wb;   // a multiple of KCP
	const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
	const uint4 *Aq[4];
#pragma unroll
	for(int q = 0; q < 4; ++q) {
		const long long L = (long long) I * TILE + ((q * 256 + threadIdx.x) >> 3);
		Aq[q] = P + (size_t) (BAND ? band_row(sh, L, n) : L) * Wp + wb;
	}
	const uint4 *Bp = P + (size_t) J * TILE * Wp + wb;
	uint32_t ad[8][8], an[8][8];
#pragma unroll
	for(int a = 0; a < 8; ++a)
#pragma unroll
		for(int c = 0; c < 8; ++c) {
			ad[a][c] = 0;
			an[a][c] = 0;
		}
	uint4 va[4], vb[4];
#pragma unroll
	for(int q = 0; q < 4; ++q) {
		const int e = q * 256 + threadIdx.x, row = e >> 3, wp = e & 7;
		va[q] = Aq[q][wp];
		vb[q] = Bp[(size_t) row * Wp + wp];
	}
#pragma unroll
	for(int q = 0; q < 4; ++q) {
		const int e = q * 256 + threadIdx.x, row = e >> 3, wp = e & 7;
		As[0][wp * RSP + row] = va[q];
		Bs[0][wp * RSP + row] = vb[q];
	}
	__syncthreads();
	int buf = 0;
	for(int w0 = 0; w0 < Wl; w0 += KCP, buf ^= 1) {
		const bool more = w0 + KCP < Wl;
		if(more) {
#pragma unroll
			for(int q = 0; q < 4; ++q) {
				const int e = q * 256 + threadIdx.x, row = e >> 3, wp = e & 7;
				va[q] = Aq[q][w0 + KCP + wp];
				vb[q] = Bp[(size_t) row * Wp + w0 + KCP + wp];
			}
		}
		const uint4 *Ac = As[buf], *Bc = Bs[buf];
#pragma unroll 1
		for(int w = 0; w < KCP; ++w) {
			uint4 a[8], b[8];
#pragma unroll
			for(int q = 0; q < 4; ++q) {
				a[2 * q] = Ac[w * RSP + 2 * ty + 32 * q];
				a[2 * q + 1] = Ac[w * RSP + 2 * ty + 32 * q + 1];
				b[2 * q] = Bc[w * RSP + 2 * tx + 32 * q];
				b[2 * q + 1] = Bc[w * RSP + 2 * tx + 32 * q + 1];
			}
#pragma unroll
			for(int x = 0; x < 8; ++x) {
#pragma unroll
				for(int y = 0; y < 8; ++y) {
					const uint32_t m = a[x].z & b[y].z;
					ad[x][y] += __popc(xor_or(a[x].x, b[y].x, a[x].y ^ b[y].y) & m);
					an[x][y] += __popc(m);
				}
			}
		}
		if(more) {
			uint4 *An = As[buf ^ 1], *Bn = Bs[buf ^ 1];
#pragma unroll
			for(int q = 0; q < 4; ++q) {
				const int e = q * 256 + threadIdx.x, row = e >> 3, wp = e & 7;
				An[wp * RSP + row] = va[q];
				Bn[wp * RSP + row] = vb[q];
			}
		}
		__syncthreads();
	}
#pragma unroll
	for(int a = 0; a < 8; ++a) {
		const int l = 2 * ty + 32 * (a >> 1) + (a & 1);
		const long long L = (long long) I * TILE + l, i = BAND ? sh.global_row(L) : L;
		if(i >= n || (!BAND && (i < rowBegin || i >= rowEnd))) continue;
		const long long base = BAND ? sh.off(i) : tri(i);
#pragma unroll
		for(int c = 0; c < 8; ++c) {
			long long j = (long long) J * TILE + 2 * tx + 32 * (c >> 1) + (c & 1);
			if(j < i) {
				if(SPLIT) {
					atomicAdd(&cd[base + j - cbase], ad[a][c]);
					atomicAdd(&cn[base + j - cbase], an[a][c]);
				} else {
					pair_store<ET>(D, Nm, base + j, ad[a][c], an[a][c], norm, minLength, bs);
				}
			}
		}
	}
}

// Pair mode (fsacmpair fsacmp.c:587: dist and n over inc_a & inc_b) on the
// matrix cores: each component nibble is zeroed where the row's mask bit is
// 0, so over the positions both rows include, equal codes dot to 3 and
// different ones to -1 (dot = 3 n - 4 dist), and a fourth component, the
// mask itself (+1 / 0), dots to n = popc(m_a & m_b).  Same tiles, staging
// (uint4 {hi, lo, m, 0} words, KCP-word chunks) and split-K as
// k_snp_tile_pair; exact while 3 L < 2^24 per slice.
// one pair-mode operand: component comp (0 hi, 1 lo, 2 hi ^ lo: masked +-1;
// 3: the mask as +1 / 0) of a lane's word, from its mask spread mq
__device__ __forceinline__ v8i_t fp4_pair_comp(uint32_t hi, uint32_t lo, const uint32_t (&mq)[4], int comp) {
	v8i_t v;
#pragma unroll
	for(int q = 0; q < 4; ++q) {
		if(comp == 3) {
			v[q] = (int) (mq[q] >> 2);   // +1.0 where included
		} else {
			const uint32_t x = comp == 0 ? hi : comp == 1 ? lo : hi ^ lo;
			const uint32_t xs = q < 3 ? x << (3 - q) : x;
			const uint32_t mf = mq[q] | (mq[q] >> 1) | (mq[q] >> 2) | (mq[q] >> 3);   // 0xF where included
			v[q] = (int) (((xs & 0x88888888u) | 0x22222222u) & mf);
		}
	}
	v[4] = v[5] = v[6] = v[7] = 0;
	return v;
}

template <int ET, bool SPLIT, bool BAND>
__global__ __launch_bounds__(256, 2) void k_snp_mfma_pair(const uint4 *__restrict__ P, int Wp, int n, long long t0,
                                                          long long items, int S, int Wk, unsigned norm,
                                                          unsigned minLength, double bs,
                                                          typename Elem<ET>::T *__restrict__ D,
                                                          typename Elem<ET>::T *__restrict__ Nm, long long rowBegin,
                                                          long long rowEnd, unsigned *__restrict__ cd,
                                                          unsigned *__restrict__ cn, long long cbase,
                                                          const long long *__restrict__ pfx, int npanels, int rank,
                                                          int world) {
	__shared__ __attribute__((aligned(16))) uint4 As[2][KCP * RSP];
	__shared__ __attribute__((aligned(16))) uint4 Bs[2][KCP * RSP];
	int I, J;
	const long long item = t0 + xcd_tile(blockIdx.x, items);
	if(BAND) band_ij(pfx, npanels, item / S, I, J);
	else tile_ij(item / S, I, J);
	const Shard sh{rank, world};
	const int wb = (int) (item % S) * Wk, we = wb + Wk < Wp ? wb + Wk : Wp;
	const int Wl = we - wb;   // a multiple of KCP
	const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
	const int wr = wid >> 1, wc = wid & 1;
	const uint4 *Aq[4];
#pragma unroll
	for(int q = 0; q < 4; ++q) {
		const long long L = (long long) I * TILE + ((q * 256 + threadIdx.x) >> 3);
		Aq[q] = P + (size_t) (BAND ? band_row(sh, L, n) : L) * Wp + wb;
	}
	const uint4 *Bp = P + (size_t) J * TILE * Wp + wb;
	v16f_t acc[2][2], accn[2][2];
#pragma unroll
	for(int a = 0; a < 2; ++a)
#pragma unroll
		for(int c = 0; c < 2; ++c)
#pragma unroll
			for(int r = 0; r < 16; ++r) acc[a][c][r] = accn[a][c][r] = 0.0f;
	uint4 va[4], vb[4];
#pragma unroll
	for(int q = 0; q < 4; ++q) {
		const int e = q * 256 + threadIdx.x, row = e >> 3, wp = e & 7;
		va[q] = Aq[q][wp];
		vb[q] = Bp[(size_t) row * Wp + wp];
	}
#pragma unroll
	for(int q = 0; q < 4; ++q) {
		const int e = q * 256 + threadIdx.x, row = e >> 3, wp = e & 7;
		As[0][wp * RSP + row] = va[q];
		Bs[0][wp * RSP + row] = vb[q];
	}
	__syncthreads();
	const int h = lane >> 5, l32 = lane & 31;
	const int ra0 = 64 * wr + l32, rb0 = 64 * wc + l32;
	int buf = 0;
	for(int w0 = 0; w0 < Wl; w0 += KCP, buf ^= 1) {
		const bool more = w0 + KCP < Wl;
		if(more) {
#pragma unroll
			for(int q = 0; q < 4; ++q) {
				const int e = q * 256 + threadIdx.x, row = e >> 3, wp = e & 7;
				va[q] = Aq[q][w0 + KCP + wp];
				vb[q] = Bp[(size_t) row * Wp + w0 + KCP + wp];
			}
		}
		const uint4 *Ac = As[buf], *Bc = Bs[buf];
#pragma unroll 1
		for(int s = 0; s < KCP / 2; ++s) {
			const int w = 2 * s + h;
			uint4 a[2], b[2];
			uint32_t ma[2][4], mb[2][4];
#pragma unroll
			for(int t = 0; t < 2; ++t) {
				a[t] = Ac[w * RSP + ra0 + 32 * t];
				b[t] = Bc[w * RSP + rb0 + 32 * t];
#pragma unroll
				for(int q = 0; q < 4; ++q) {
					ma[t][q] = (q < 3 ? a[t].z << (3 - q) : a[t].z) & 0x88888888u;
					mb[t][q] = (q < 3 ? b[t].z << (3 - q) : b[t].z) & 0x88888888u;
				}
			}
#pragma unroll
			for(int comp = 0; comp < 4; ++comp) {
				v8i_t fa[2], fb[2];
#pragma unroll
				for(int t = 0; t < 2; ++t) {
					fa[t] = fp4_pair_comp(a[t].x, a[t].y, ma[t], comp);
					fb[t] = fp4_pair_comp(b[t].x, b[t].y, mb[t], comp);
				}
#pragma unroll
				for(int ta = 0; ta < 2; ++ta)
#pragma unroll
					for(int tb = 0; tb < 2; ++tb) {
						if(comp < 3)
							acc[ta][tb] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(
							    fa[ta], fb[tb], acc[ta][tb], MFMA_FP4, MFMA_FP4, 0, MFMA_SCALE1, 0, MFMA_SCALE1);
						else
							accn[ta][tb] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(
							    fa[ta], fb[tb], accn[ta][tb], MFMA_FP4, MFMA_FP4, 0, MFMA_SCALE1, 0, MFMA_SCALE1);
					}
			}
		}
		if(more) {
			uint4 *An = As[buf ^ 1], *Bn = Bs[buf ^ 1];
#pragma unroll
			for(int q = 0; q < 4; ++q) {
				const int e = q * 256 + threadIdx.x, row = e >> 3, wp = e & 7;
				An[wp * RSP + row] = va[q];
				Bn[wp * RSP + row] = vb[q];
			}
		}
		__syncthreads();
	}
#pragma unroll
	for(int ta = 0; ta < 2; ++ta) {
#pragma unroll
		for(int r = 0; r < 16; ++r) {
			const long long L = (long long) I * TILE + 64 * wr + 32 * ta + (r & 3) + 8 * (r >> 2) + 4 * h;
			const long long i = BAND ? sh.global_row(L) : L;
			if(i >= n || (!BAND && (i < rowBegin || i >= rowEnd))) continue;
			const long long base = BAND ? sh.off(i) : tri(i);
#pragma unroll
			for(int tb = 0; tb < 2; ++tb) {
				const long long j = (long long) J * TILE + 64 * wc + 32 * tb + l32;
				if(j < i) {
					const int nn = (int) accn[ta][tb][r];
					const unsigned d = (unsigned) ((3 * nn - (int) acc[ta][tb][r]) >> 2);
					if(SPLIT) {
						atomicAdd(&cd[base + j - cbase], d);
						atomicAdd(&cn[base + j - cbase], (unsigned) nn);
					} else {
						pair_store<ET>(D, Nm, base + j, d, (uint32_t) nn, norm, minLength, bs);
					}
				}
			}
		}
	}
}

// k_snp_mfma2_pair: pair mode on k_snp_mfma2's 256 x 256 tiles.  The mask
// enters the nibble's exponent instead of being and-ed in afterwards: a
// component nibble is (sign << 3) | (m << 1), +-1.0 where the row includes the
// position and +-0.0 where it does not, so one mask spread per word (the 0x2
// bits, itself the fourth operand: +1 / 0) serves all four components; hi and
// lo cost one and_or per dword on top of it and hi ^ lo one xor_or
// ((a ^ b) | msp: the shared exponent bits cancel and are set again).  Two
// accumulator sets (dot, n) per 32 x 32 tile, so a wave takes 128 x 64 and a
// block of 4 waves one column half of a 256 x 256 tile (items = 2 per tile):
// each step spreads 4 A and 2 B words (25 VALU each) for 32 MFMAs, against
// k_snp_mfma_pair's 384 VALU for 16.  Staging as k_snp_mfma2 with uint4
// {hi, lo, m, 0} words (99 KB of LDS at 8 words per chunk, one block per
// CU); BAND and SPLIT as k_snp_mfma2.
__device__ __forceinline__ v8i_t pair2_mask(uint32_t m) {
	v8i_t v;
	v[0] = (int) ((m << 1) & 0x22222222u);
	v[1] = (int) (m & 0x22222222u);
	v[2] = (int) ((m >> 1) & 0x22222222u);
	v[3] = (int) ((m >> 2) & 0x22222222u);
	v[4] = v[5] = v[6] = v[7] = 0;
	return v;
}

__device__ __forceinline__ v8i_t pair2_comp(uint32_t x, const v8i_t &m) {
	v8i_t v;
	v[0] = (int) and_or(x << 3, 0x88888888u, (uint32_t) m[0]);
	v[1] = (int) and_or(x << 2, 0x88888888u, (uint32_t) m[1]);
	v[2] = (int) and_or(x << 1, 0x88888888u, (uint32_t) m[2]);
	v[3] = (int) and_or(x, 0x88888888u, (uint32_t) m[3]);
	v[4] = v[5] = v[6] = v[7] = 0;
	return v;
}

__device__ __forceinline__ v8i_t pair2_xor(const v8i_t &h, const v8i_t &l, const v8i_t &m) {
	v8i_t v;
#pragma unroll
	for(int q = 0; q < 4; ++q) v[q] = (int) xor_or((uint32_t) h[q], (uint32_t) l[q], (uint32_t) m[q]);
	v[4] = v[5] = v[6] = v[7] = 0;
	return v;
}

#define RS2P 258   // pair LDS row strides (uint4): 256 A rows, 128 B rows, + pad
#define RS2B 130
template <int ET, bool SPLIT, bool BAND>
__global__ __launch_bounds__(256, 1) void k_snp_mfma2_pair(const uint4 *__restrict__ P, int Wp, int n, long long t0,
                                                           long long items, int S, int Wk, unsigned norm,
                                                           unsigned minLength, double bs,
                                                           typename Elem<ET>::T *__restrict__ D,
                                                           typename Elem<ET>::T *__restrict__ Nm, long long rowBegin,
                                                           long long rowEnd, unsigned *__restrict__ cd,
                                                           unsigned *__restrict__ cn, long long cbase,
                                                           const long long *__restrict__ pfx, int npanels, int rank,
                                                           int world) {
	constexpr int QA = TILE2 * KC2 / 256, QB = QA / 2;   // uint4 staged per thread: A panel, B half panel
	__shared__ __attribute__((aligned(16))) uint4 As[2][KC2 * RS2P];
	__shared__ __attribute__((aligned(16))) uint4 Bs[2][KC2 * RS2B];
	const long long item = t0 + xcd_tile(blockIdx.x, items), th = SPLIT ? item / S : item, t = th >> 1;
	const int half = (int) (th & 1);   // the tile's column half: B rows J * 256 + 128 half + [0, 128)
	int I, J;
	if(BAND) {
		int lo = 0, hi = npanels - 1;
		while(lo < hi) {
			const int mid = (lo + hi + 1) >> 1;
			if(pfx[mid] <= t) lo = mid; else hi = mid - 1;
		}
		I = lo;
		J = (int) (t - pfx[lo]);
	} else {
		tile_ij(t, I, J);
	}
	const int wb = SPLIT ? (int) (item % S) * Wk : 0;
	const int Wl = SPLIT ? (wb + Wk < Wp ? Wk : Wp - wb) : Wp;
	const auto arow = [&](int l) -> long long {
		const long long L = (long long) I * TILE2 + l;
		if(!BAND) return L;
		const long long lb = L / SB, r = (lb * world + rank) * SB + (L - lb * SB);
		return r < n ? r : 0;
	};
	const uint4 *Bp = P + ((size_t) J * TILE2 + 128 * half) * Wp + wb;
	const uint4 *Ap[QA];
	// (staging registers in arrays of 4 uint4: a larger array is left in scratch)
	// (staging registers as native 4-dword vectors: HIP's uint4 struct copies
	// become memcpys that keep the arrays in scratch)
	typedef unsigned u4v __attribute__((ext_vector_type(4)));
	u4v vaa[4], vab[4], vb[4];
	static_assert(QA == 8 && QB == 4, "staging registers: A in two arrays of 4, B in one");
	u4v *As4 = (u4v *) &As[0][0], *Bs4 = (u4v *) &Bs[0][0];
	const int srow = threadIdx.x / KC2, swp = threadIdx.x % KC2;   // staged element q: row srow + 32 q, word swp
#pragma unroll
	for(int q = 0; q < QA; ++q) Ap[q] = P + (size_t) arow(srow + 32 * q) * Wp + wb + swp;
#pragma unroll
	for(int q = 0; q < 4; ++q) {
		vaa[q] = *(const u4v *) Ap[q];
		vab[q] = *(const u4v *) Ap[q + 4];
	}
	Bp += (size_t) srow * Wp + swp;
#pragma unroll
	for(int q = 0; q < QB; ++q) vb[q] = *(const u4v *) (Bp + (size_t) 32 * q * Wp);
#pragma unroll
	for(int q = 0; q < 4; ++q) {
		As4[swp * RS2P + srow + 32 * q] = vaa[q];
		As4[swp * RS2P + srow + 32 * (q + 4)] = vab[q];
	}
#pragma unroll
	for(int q = 0; q < QB; ++q) Bs4[swp * RS2B + srow + 32 * q] = vb[q];
	__syncthreads();
	const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
	const int wr = wid >> 1, wc = wid & 1;
	const int h = lane >> 5, l32 = lane & 31;
	const int ra0 = 128 * wr + l32, rb0 = 64 * wc + l32;
	v16f_t acc[4][2], accn[4][2];
#pragma unroll
	for(int a = 0; a < 4; ++a)
#pragma unroll
		for(int c = 0; c < 2; ++c)
#pragma unroll
			for(int r = 0; r < 16; ++r) acc[a][c][r] = accn[a][c][r] = 0.0f;
	int buf = 0;
	for(int w0 = 0; w0 < Wl; w0 += KC2, buf ^= 1) {
		const bool more = w0 + KC2 < Wl;
		if(more) {
#pragma unroll
			for(int q = 0; q < 4; ++q) {
				vaa[q] = *(const u4v *) (Ap[q] + w0 + KC2);
				vab[q] = *(const u4v *) (Ap[q + 4] + w0 + KC2);
			}
#pragma unroll
			for(int q = 0; q < QB; ++q) vb[q] = *(const u4v *) (Bp + (size_t) 32 * q * Wp + w0 + KC2);
		}
		const uint4 *Ac = As[buf], *Bc = Bs[buf];
#pragma unroll
		for(int s = 0; s < KC2 / 2; ++s) {
			const int w = 2 * s + h;
			uint4 av[4], bv[2];
			v8i_t am[4], ah[4], al[4], bm[2], bh[2], bl[2];
#pragma unroll
			for(int x = 0; x < 4; ++x) {
				av[x] = Ac[w * RS2P + ra0 + 32 * x];
				am[x] = pair2_mask(av[x].z);
			}
#pragma unroll
			for(int y = 0; y < 2; ++y) {
				bv[y] = Bc[w * RS2B + rb0 + 32 * y];
				bm[y] = pair2_mask(bv[y].z);
			}
#pragma unroll
			for(int ta = 0; ta < 4; ++ta)
#pragma unroll
				for(int tb = 0; tb < 2; ++tb)
					accn[ta][tb] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(
					    am[ta], bm[tb], accn[ta][tb], MFMA_FP4, MFMA_FP4, 0, MFMA_SCALE1, 0, MFMA_SCALE1);
#pragma unroll
			for(int x = 0; x < 4; ++x) ah[x] = pair2_comp(av[x].x, am[x]);
#pragma unroll
			for(int y = 0; y < 2; ++y) bh[y] = pair2_comp(bv[y].x, bm[y]);
#pragma unroll
			for(int ta = 0; ta < 4; ++ta)
#pragma unroll
				for(int tb = 0; tb < 2; ++tb)
					acc[ta][tb] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(
					    ah[ta], bh[tb], acc[ta][tb], MFMA_FP4, MFMA_FP4, 0, MFMA_SCALE1, 0, MFMA_SCALE1);
#pragma unroll
			for(int x = 0; x < 4; ++x) al[x] = pair2_comp(av[x].y, am[x]);
#pragma unroll
			for(int y = 0; y < 2; ++y) bl[y] = pair2_comp(bv[y].y, bm[y]);
#pragma unroll
			for(int ta = 0; ta < 4; ++ta)
#pragma unroll
				for(int tb = 0; tb < 2; ++tb)
					acc[ta][tb] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(
					    al[ta], bl[tb], acc[ta][tb], MFMA_FP4, MFMA_FP4, 0, MFMA_SCALE1, 0, MFMA_SCALE1);
#pragma unroll
			for(int x = 0; x < 4; ++x) ah[x] = pair2_xor(ah[x], al[x], am[x]);
#pragma unroll
			for(int y = 0; y < 2; ++y) bh[y] = pair2_xor(bh[y], bl[y], bm[y]);
#pragma unroll
			for(int ta = 0; ta < 4; ++ta)
#pragma unroll
				for(int tb = 0; tb < 2; ++tb)
					acc[ta][tb] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(
					    ah[ta], bh[tb], acc[ta][tb], MFMA_FP4, MFMA_FP4, 0, MFMA_SCALE1, 0, MFMA_SCALE1);
		}
		if(more) {
			u4v *An = (u4v *) As[buf ^ 1], *Bn = (u4v *) Bs[buf ^ 1];
#pragma unroll
			for(int q = 0; q < 4; ++q) {
				An[swp * RS2P + srow + 32 * q] = vaa[q];
				An[swp * RS2P + srow + 32 * (q + 4)] = vab[q];
			}
#pragma unroll
			for(int q = 0; q < QB; ++q) Bn[swp * RS2B + srow + 32 * q] = vb[q];
		}
		__syncthreads();
	}
	// epilogue as k_snp_mfma2 (C/D row (r & 3) + 8 (r >> 2) + 4 h, column l32)
#pragma unroll
	for(int ta = 0; ta < 4; ++ta) {
#pragma unroll
		for(int r = 0; r < 16; ++r) {
			const long long L = (long long) I * TILE2 + 128 * wr + 32 * ta + (r & 3) + 8 * (r >> 2) + 4 * h;
			long long i = L;
			if(BAND) {
				const long long lb = L / SB;
				i = (lb * world + rank) * SB + (L - lb * SB);
			}
			if(i >= n || (!BAND && (i < rowBegin || i >= rowEnd))) continue;
			const long long base = BAND ? Shard{rank, world}.off(i) : tri(i);
#pragma unroll
			for(int tb = 0; tb < 2; ++tb) {
				const long long j = (long long) J * TILE2 + 128 * half + 64 * wc + 32 * tb + l32;
				if(j < i) {
					const int nn = (int) accn[ta][tb][r];
					const unsigned d = (unsigned) ((3 * nn - (int) acc[ta][tb][r]) >> 2);
					if(SPLIT) {
						atomicAdd(&cd[base + j - cbase], d);
						atomicAdd(&cn[base + j - cbase], (unsigned) nn);
					} else {
						pair_store<ET>(D, Nm, base + j, d, (uint32_t) nn, norm, minLength, bs);
					}
				}
			}
		}
	}
}

// split-K epilogue of pair mode: the A7 store of the summed (dist, n)
template <int ET>
__global__ void k_snp_pair_finish(const unsigned *__restrict__ cd, const unsigned *__restrict__ cn, long long f0,
                                  long long f1, unsigned norm, unsigned minLength, double bs,
                                  typename Elem<ET>::T *__restrict__ D, typename Elem<ET>::T *__restrict__ Nm) {
	for(long long f = f0 + (long long) blockIdx.x * blockDim.x + threadIdx.x; f < f1;
	    f += (long long) gridDim.x * blockDim.x) {
		pair_store<ET>(D, Nm, f, cd[f - f0], cn[f - f0], norm, minLength, bs);
	}
}

// ------------------------------------------------- pair mode with -P > 0
// maskProxi (fsacmp.c:355-485) followed by fsacmpair (fsacmp.c:587).  The
// reference walks the pair's SNPs (inc_i & inc_j set, codes differ) from the
// last position down; its counter i stands for position p + 1 (the "label"),
// and with lastSNP starting at len + proxi it clears include bits
// [label, lastSNP] whenever lastSNP - label <= proxi, then lastSNP = label.
// The cleared set is therefore the union of the closed intervals between
// consecutive labels (plus the sentinel len + proxi) that are at most proxi
// apart, and the pair's (dist, n) are the unmasked counts minus the counts
// over that union.  Consecutive intervals share one end point, which is
// added back once when both sides qualify.
//
// One wave per pair, 64 words per step (one per lane, coalesced): a max-scan
// of the lanes' highest labels gives every lane the label below its first
// SNP; a second scan over (label, qualified) carries whether that label's
// own lower gap qualified.  Interval counts re-read the (cached) words they
// cover.  The sequential dependency of maskProxi is only between consecutive
// SNPs, so the result is exact and independent of the lane split.
__device__ __forceinline__ int wave_scan_max_incl(int v, int lane) {
#pragma unroll
	for(int o = 1; o < 64; o <<= 1) {
		int t = __shfl_up(v, o, 64);
		if(lane >= o) v = v > t ? v : t;
	}
	return v;
}

// positions [s, e] (clipped to the W32 counted words) of pair rows A, B
__device__ __forceinline__ void range_counts(const uint4 *__restrict__ A, const uint4 *__restrict__ B, int W32, int s,
                                             int e, uint32_t &cm, uint32_t &cd) {
	cm = cd = 0;
	if(e > 32 * W32 - 1) e = 32 * W32 - 1;
	for(int w = s >> 5; w <= (e >> 5) && s <= e; ++w) {
		const int ks = w == (s >> 5) ? (s & 31) : 0, ke = w == (e >> 5) ? (e & 31) : 31;
		const uint32_t msk = (0xFFFFFFFFu >> ks) & (0xFFFFFFFFu << (31 - ke));
		const uint4 a = A[w], b = B[w];
		const uint32_t m = a.z & b.z & msk;
		cm += __popc(m);
		cd += __popc(xor_or(a.x, b.x, a.y ^ b.y) & m);
	}
}

template <int ET>
__global__ __launch_bounds__(256) void k_snp_pair_proxi(const uint4 *__restrict__ P, int Wp, int W32, int len, int proxi,
                                                        long long f0, long long f1, unsigned norm, unsigned minLength,
                                                        double bs, typename Elem<ET>::T *__restrict__ D,
                                                        typename Elem<ET>::T *__restrict__ Nm) {
	const int lane = threadIdx.x & 63;
	const long long stride = (long long) gridDim.x * 4;
	for(long long f = f0 + (long long) blockIdx.x * 4 + (threadIdx.x >> 6); f < f1; f += stride) {
		long long i = (long long) ((1.0 + sqrt(1.0 + 8.0 * (double) f)) * 0.5);
		while(tri(i) > f) --i;
		while(tri(i + 1) <= f) ++i;
		const long long j = f - tri(i);
		const uint4 *A = P + (size_t) i * Wp, *B = P + (size_t) j * Wp;
		int dist = 0, cnt = 0;
		int cL = -1, cQ = 0;                 // highest label so far, and whether its lower gap qualified
		for(int w0 = 0; w0 < W32; w0 += 64) {
			const int w = w0 + lane;
			uint32_t m = 0, d = 0;
			if(w < W32) {
				const uint4 a = A[w], b = B[w];
				m = a.z & b.z;
				d = xor_or(a.x, b.x, a.y ^ b.y) & m;
			}
			cnt += __popc(m);
			dist += __popc(d);
			// bit 31 - k <-> position 32w + k; label = position + 1
			const int hiL = d ? 32 * w + 32 - (__ffs(d)) + 1 : -1;
			int incl = wave_scan_max_incl(hiL, lane);
			int prevL = __shfl_up(incl, 1, 64);
			if(lane == 0) prevL = -1;
			if(cL > prevL) prevL = cL;
			// q of each own label: gap to the label below <= proxi
			int qhi = 0;
			{
				int prev = prevL;
				for(uint32_t x = d; x;) {
					const int k = __clz(x);
					x &= ~(0x80000000u >> k);
					const int cur = 32 * w + k + 1;
					qhi = prev >= 0 && cur - prev <= proxi;
					prev = cur;
				}
			}
			const int packed = hiL >= 0 ? 2 * hiL + qhi : -1;
			const int incl2 = wave_scan_max_incl(packed, lane);
			int prevP = __shfl_up(incl2, 1, 64);
			if(lane == 0) prevP = -1;
			const int cP = cL >= 0 ? 2 * cL + cQ : -1;
			if(cP > prevP) prevP = cP;
			// subtract the qualifying intervals ending at this lane's labels
			{
				int prev = prevL, qprev = prevP >= 0 ? (prevP & 1) : 0;
				for(uint32_t x = d; x;) {
					const int k = __clz(x);
					x &= ~(0x80000000u >> k);
					const int cur = 32 * w + k + 1;
					const int qc = prev >= 0 && cur - prev <= proxi;
					if(qc) {
						uint32_t rm, rd;
						range_counts(A, B, W32, prev, cur, rm, rd);
						cnt -= rm;
						dist -= rd;
						if(qprev) {
							range_counts(A, B, W32, prev, prev, rm, rd);
							cnt += rm;
							dist += rd;
						}
					}
					prev = cur;
					qprev = qc;
				}
			}
			const int top = __shfl(incl2, 63, 64);
			if(top >= 0 && (top >> 1) > cL) {
				cL = top >> 1;
				cQ = top & 1;
			}
		}
		// the highest SNP against the sentinel lastSNP = len + proxi (fsacmp.c:367)
		if(lane == 0 && cL >= 0 && (long long) len + proxi - cL <= proxi) {
			uint32_t rm, rd;
			const long long e = (long long) len + proxi;
			range_counts(A, B, W32, cL, e < 32LL * W32 ? (int) e : 32 * W32 - 1, rm, rd);
			cnt -= rm;
			dist -= rd;
			if(cQ) {
				range_counts(A, B, W32, cL, cL, rm, rd);
				cnt += rm;
				dist += rd;
			}
		}
#pragma unroll
		for(int o = 32; o > 0; o >>= 1) {
			dist += __shfl_xor(dist, o, 64);
			cnt += __shfl_xor(cnt, o, 64);
		}
		if(lane == 0) pair_store<ET>(D, Nm, f, (uint32_t) dist, (uint32_t) cnt, norm, minLength, bs);
	}
}

// ------------------------------------------------------------------ host
static inline long long cdivll(long long a, long long b) { return (a + b - 1) / b; }

// The work of one launch: tiles [t_begin, t_end) of edge `tile` and the output
// elements [f0, f1) they fill.  world == 0: the tiles touching the LT rows
// [rb, re).  world > 0: one rank's rows of the band layout in its own order,
// as npanels panels of `tile` owned rows, each against the column tiles below
// its last row (those with a cell j < i); pfx prefix-sums the tiles per panel,
// so that a launch spans many panels and fills the chip (band_ij finds a tile
// in its device copy d_pfx).  A rank that owns no row has no panel.
struct TileRange {
	long long t_begin = 0, t_end = 0, f0 = 0, f1 = 0;
	int npanels = 0;
	std::vector<long long> pfx;   // lives until the launcher has synchronised the copy
	DevMem d_pfx;
};

static int tile_range(ccg_ctx *ctx, long long n, long long rb, long long re, int rank, int world, int tile,
                      TileRange *tr) {
	if(world == 0) {
		const long long Ilo = rb / tile, Ihi = (re - 1) / tile;
		tr->t_begin = Ilo * (Ilo + 1) / 2;
		tr->t_end = (Ihi + 1) * (Ihi + 2) / 2;
		tr->f0 = tri(rb);
		tr->f1 = tri(re);
		return CCG_OK;
	}
	const Shard sh{rank, world};
	const long long nb = cdivll(n, SB);
	long long nloc = 0;   // owned rows below n
	if(rank < nb) {
		const long long owned = (nb - 1 - rank) / world + 1, last = (owned - 1) * world + rank;
		nloc = (owned - 1) * SB + (n - last * SB < SB ? n - last * SB : SB);
	}
	const int np = (int) cdivll(nloc, tile);
	if(np == 0) return CCG_OK;
	tr->pfx.assign(np + 1, 0);
	for(long long I = 0; I < np; ++I) {
		const long long Lmax = ((I + 1) * tile < nloc ? (I + 1) * tile : nloc) - 1;   // the panel's last owned row
		tr->pfx[I + 1] = tr->pfx[I] + cdivll(sh.global_row(Lmax), tile);
	}
	const size_t pb = (size_t) (np + 1) * sizeof(long long);
	CCG_TRY(tr->d_pfx.alloc(pb));
	CCG_CHECK(hipMemcpyAsync(tr->d_pfx.p, tr->pfx.data(), pb, hipMemcpyHostToDevice, ctx->stream));
	tr->npanels = np;
	tr->t_end = tr->pfx[np];
	tr->f1 = ccg_shard_elems(n, rank, world);
	return CCG_OK;
}

// Split-K: when `tiles` tiles do not fill the chip's `slots` resident blocks 16
// times over (so the tail round of blocks is small), each tile's Wp words are
// cut into S slices of Wk words, a multiple of the kernel's kc-word chunk; a
// slice keeps >= 4 chunks.  kmax > 0: and Wk <= kmax (the f32-exact slice of
// the MFMA forms), however many tiles there are.  CCG_DIST_SLICES=S (S >= 1, a
// diagnostic knob) takes the place of the fill-the-chip choice: S slices, at
// most one per chunk (no 4-chunk floor), then the same rounding and clamp, so
// a test picks the chunks a slice gets whatever the device's CU count.  The
// plan is kept in the context (ccg_last_dist_plan).
struct SplitPlan {
	int S, Wk;
};

static SplitPlan plan_split(ccg_ctx *ctx, long long tiles, long long slots, int Wp, int kc, int kmax) {
	const int chunks = Wp / kc;
	const char *fse = getenv("CCG_DIST_SLICES");
	const int forced = fse ? atoi(fse) : 0;
	int S = 1;
	if(forced >= 1) {
		S = forced < chunks ? forced : chunks;
	} else if(tiles < 16 * slots) {
		S = (int) cdivll(16 * slots, tiles);
		if(S > chunks / 4) S = chunks / 4;
		if(S < 1) S = 1;
	}
	int Wk = (int) cdivll(chunks, S) * kc;
	if(kmax && Wk > kmax) Wk = (kmax / kc) * kc;
	ctx->dist_slices = (int) cdivll(Wp, Wk);
	ctx->dist_slice_words = Wk;
	return SplitPlan{ctx->dist_slices, Wk};
}

// the kernels' SPLIT and BAND template arguments from two runtime values:
// f(std::bool_constant<SPLIT>(), std::bool_constant<BAND>())
template <class F>
static void with_split_band(bool split, bool band, F &&f) {
	if(split && band) f(std::true_type(), std::true_type());
	else if(split) f(std::true_type(), std::false_type());
	else if(band) f(std::false_type(), std::true_type());
	else f(std::false_type(), std::false_type());
}

// the zeroed u32 split-K counts of a launcher (pair mode: dist counts, then n counts)
static int alloc_counts(ccg_ctx *ctx, size_t elems, DevMem &cnt) {
	CCG_TRY(cnt.alloc(elems * sizeof(unsigned)));
	CCG_CHECK(hipMemsetAsync(cnt.p, 0, elems * sizeof(unsigned), ctx->stream));
	return CCG_OK;
}

// the split-K epilogue over the elements [f0, f1) (fsacmpthrd.c:247-255, resp. A7)
template <int ET>
static hipError_t launch_finish(ccg_ctx *ctx, const ccg_snp_args *a, const unsigned *cnt, long long f0, long long f1,
                                double nFactor, typename Elem<ET>::T *D, typename Elem<ET>::T *N) {
	const long long g = cdivll(f1 - f0, 256);
	const unsigned grid = (unsigned) (g < 65536 ? g : 65536);
	if(a->pair)
		k_snp_pair_finish<ET><<<grid, 256, 0, ctx->stream>>>(cnt, cnt + (f1 - f0), f0, f1, a->norm, a->minLength,
		                                                     a->byteScale, D, N);
	else k_snp_finish<ET><<<grid, 256, 0, ctx->stream>>>(cnt, f0, f0, f1, nFactor, a->byteScale, D);
	return hipGetLastError();
}

// k_snp_mfma3 / k_snp_mfma2 / k_snp_mfma2_pair over the LT rows [rb, re)
// (world == 0) or over one rank's rows of the band layout (world > 0, rb = 0,
// re = n), with split-K over word slices when the tiles do not fill the chip
// (one block per CU) or a row exceeds the f32-exact slice, counts finished by
// k_snp_finish / k_snp_pair_finish
template <int ET, bool PAIR>
static int snp_launch_mfma2(ccg_ctx *ctx, const ccg_snp_args *a, const void *planes, int Wp, double nFactor, void *D,
                            void *N, long long rb, long long re, int rank, int world) {
	typedef typename Elem<ET>::T T;
	const long long n = a->n;
	hipDeviceProp_t prop;
	CCG_CHECK(hipGetDeviceProperties(&prop, ctx->device));
	TileRange tr;
	const int trc = tile_range(ctx, n, rb, re, rank, world, TILE2, &tr);
	if(trc != CCG_OK || (world > 0 && tr.npanels == 0)) return trc;
	// pair mode: items are tile column halves
	const long long t_begin = tr.t_begin * (PAIR ? 2 : 1), t_end = tr.t_end * (PAIR ? 2 : 1), f0 = tr.f0, f1 = tr.f1;
	// words per LDS chunk (CCG_DIST_KC=16: half the barriers, 133 KB of LDS)
	// and the tile order (CCG_DIST_ORDER=1: super-tiles, whole LT ranges from
	// a super-row start only)
	const char *kce = getenv("CCG_DIST_KC"), *ore = getenv("CCG_DIST_ORDER");
	const int kc = !PAIR && kce && atoi(kce) == KC2L && Wp % KC2L == 0 ? KC2L : KC2;
	// the LDS-DMA staged kernel (CCG_DIST_GLDS=0: k_snp_mfma2)
	const char *gle = getenv("CCG_DIST_GLDS");
	const bool glds = !PAIR && !(gle && atoi(gle) == 0) && kc == KC3;
	const int sorder = !PAIR && world == 0 && ore && atoi(ore) == 1 && (rb / TILE2) % 4 == 0;
	const SplitPlan plan = plan_split(ctx, t_end - t_begin, prop.multiProcessorCount, Wp, kc, MFMA_KMAX);   // one block per CU
	const int S = plan.S, Wk = plan.Wk;
	const long long batch = 1 << 16;
	T *Nn = world > 0 ? NULL : (T *) N;
	DevMem counts;   // (with tr.d_pfx and the stamps: freed once `idle` below has waited for the launches)
#ifdef CCG_DIST_STAMPS
	// the stamp sums of k_snp_mfma3, appended to the file CCG_DIST_STAMPS_OUT names (tools/dist_stamps.py reads it)
	DevMem stamps;
#endif
	StreamSync idle(ctx->stream);
#ifdef CCG_DIST_STAMPS
	const char *sto = getenv("CCG_DIST_STAMPS_OUT");
	const size_t stn = (size_t) (t_end - t_begin) * S * 2 * ST3_SLOTS;
	const long long st_item0 = t_begin * S;
	if(glds && sto) {
		CCG_TRY(stamps.alloc(stn * sizeof(unsigned long long)));
		CCG_CHECK(hipMemsetAsync(stamps.p, 0, stn * sizeof(unsigned long long), ctx->stream));
	}
	unsigned long long *const d_st = stamps.as<unsigned long long>();
	CCG_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(ccg_dist_stamp_buf), &d_st, sizeof(d_st)));
	CCG_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(ccg_dist_stamp_item0), &st_item0, sizeof(st_item0)));
#endif
	if(S > 1) CCG_TRY(alloc_counts(ctx, (size_t) (f1 - f0) * (PAIR ? 2 : 1), counts));
	unsigned *const cnt = counts.as<unsigned>();
	const long long *const d_pfx = tr.d_pfx.as<long long>();
	for(long long t = t_begin * S; t < t_end * S; t += batch) {
		const long long items = t_end * S - t < batch ? t_end * S - t : batch;
		with_split_band(S > 1, world > 0, [&](auto SP, auto BD) {
			constexpr bool sp = decltype(SP)::value, bd = decltype(BD)::value;
			const uint2 *pl = (const uint2 *) planes;
			if(PAIR)
				k_snp_mfma2_pair<ET, sp, bd><<<(unsigned) items, 256, 0, ctx->stream>>>(
				    (const uint4 *) planes, Wp, (int) n, t, items, S, Wk, a->norm, a->minLength, a->byteScale, (T *) D, Nn,
				    rb, re, cnt, cnt ? cnt + (f1 - f0) : NULL, f0, d_pfx, tr.npanels, rank, world);
			else if(glds)   // KC3-word chunks, LDS-DMA staged
				k_snp_mfma3<ET, sp, bd><<<(unsigned) items, 256, 0, ctx->stream>>>(
				    pl, Wp, (int) n, t, items, S, Wk, nFactor, a->byteScale, (T *) D, rb, re, cnt, f0, d_pfx, tr.npanels,
				    rank, world, sorder);
			else if(kc == KC2L)
				k_snp_mfma2<ET, sp, bd, KC2L><<<(unsigned) items, 256, 0, ctx->stream>>>(
				    pl, Wp, (int) n, t, items, S, Wk, nFactor, a->byteScale, (T *) D, rb, re, cnt, f0, d_pfx, tr.npanels,
				    rank, world, sorder);
			else
				k_snp_mfma2<ET, sp, bd, KC2><<<(unsigned) items, 256, 0, ctx->stream>>>(
				    pl, Wp, (int) n, t, items, S, Wk, nFactor, a->byteScale, (T *) D, rb, re, cnt, f0, d_pfx, tr.npanels,
				    rank, world, sorder);
		});
		CCG_CHECK(hipGetLastError());
	}
	if(S > 1) CCG_CHECK(launch_finish<ET>(ctx, a, cnt, f0, f1, nFactor, (T *) D, Nn));
	CCG_CHECK(hipStreamSynchronize(ctx->stream));
#ifdef CCG_DIST_STAMPS
	if(d_st) {
		std::vector<unsigned long long> hs(stn);
		CCG_CHECK(hipMemcpy(hs.data(), d_st, stn * sizeof(unsigned long long), hipMemcpyDeviceToHost));
		FILE *sf = fopen(sto, "ab");
		if(sf) {
			fwrite(hs.data(), sizeof(unsigned long long), stn, sf);
			fclose(sf);
		}
	}
#endif
	return CCG_OK;
}

// The 128 x 128 tile kernels, in snp_launch_mfma2's shape: k_snp_mfma /
// k_snp_mfma_pair (mfma) or the VALU tiles k_snp_tile / k_snp_tile_pair, two
// blocks per CU in the plan.  k_snp_mfma is planned in k_snp_tile's KC-word
// chunks (it stages KCM-word ones) with its slices clamped to the f32-exact
// length; pair mode is not clamped, and k_snp_mfma_pair gives way to the VALU
// pair tiles when a slice is longer than that.
template <int ET>
static int snp_launch_tile128(ccg_ctx *ctx, const ccg_snp_args *a, const void *planes, int Wp, double nFactor, void *D,
                              void *N, long long rb, long long re, int rank, int world, bool mfma) {
	typedef typename Elem<ET>::T T;
	const long long n = a->n;
	hipDeviceProp_t prop;
	CCG_CHECK(hipGetDeviceProperties(&prop, ctx->device));
	TileRange tr;
	const int trc = tile_range(ctx, n, rb, re, rank, world, TILE, &tr);
	if(trc != CCG_OK || (world > 0 && tr.npanels == 0)) return trc;
	const long long f0 = tr.f0, f1 = tr.f1;
	const bool pair = a->pair != 0;
	const SplitPlan plan = plan_split(ctx, tr.t_end - tr.t_begin, 2LL * prop.multiProcessorCount, Wp, pair ? KCP : KC,
	                                  mfma && !pair ? MFMA_KMAX : 0);
	const int S = plan.S, Wk = plan.Wk;
	if(pair && Wk >= MFMA_KMAX) mfma = false;
	const long long batch = world > 0 ? 1 << 16 : 1 << 14;
	T *Nn = world > 0 ? NULL : (T *) N;
	DevMem counts;   // (with tr.d_pfx: freed once `idle` has waited for the launches)
	StreamSync idle(ctx->stream);
	if(S > 1) CCG_TRY(alloc_counts(ctx, (size_t) (f1 - f0) * (pair ? 2 : 1), counts));
	unsigned *const cnt = counts.as<unsigned>();
	const long long *const d_pfx = tr.d_pfx.as<long long>();
	for(long long t = tr.t_begin * S; t < tr.t_end * S; t += batch) {
		const long long items = tr.t_end * S - t < batch ? tr.t_end * S - t : batch;
		with_split_band(S > 1, world > 0, [&](auto SP, auto BD) {
			constexpr bool sp = decltype(SP)::value, bd = decltype(BD)::value;
			const uint2 *pl = (const uint2 *) planes;
			const uint4 *pp = (const uint4 *) planes;
			unsigned *cn = cnt ? cnt + (f1 - f0) : NULL;
			if(pair && mfma)
				k_snp_mfma_pair<ET, sp, bd><<<(unsigned) items, 256, 0, ctx->stream>>>(
				    pp, Wp, (int) n, t, items, S, Wk, a->norm, a->minLength, a->byteScale, (T *) D, Nn, rb, re, cnt, cn, f0,
				    d_pfx, tr.npanels, rank, world);
			else if(pair)
				k_snp_tile_pair<ET, sp, bd><<<(unsigned) items, 256, 0, ctx->stream>>>(
				    pp, Wp, (int) n, t, items, S, Wk, a->norm, a->minLength, a->byteScale, (T *) D, Nn, rb, re, cnt, cn, f0,
				    d_pfx, tr.npanels, rank, world);
			else if(mfma)
				k_snp_mfma<ET, sp, bd><<<(unsigned) items, 256, 0, ctx->stream>>>(
				    pl, Wp, (int) n, t, items, S, Wk, nFactor, a->byteScale, (T *) D, rb, re, cnt, f0, d_pfx, tr.npanels,
				    rank, world);
			else
				k_snp_tile<ET, sp, bd><<<(unsigned) items, 256, 0, ctx->stream>>>(
				    pl, Wp, (int) n, t, items, S, Wk, nFactor, a->byteScale, (T *) D, rb, re, cnt, f0, d_pfx, tr.npanels,
				    rank, world);
		});
		CCG_CHECK(hipGetLastError());
	}
	if(S > 1) CCG_CHECK(launch_finish<ET>(ctx, a, cnt, f0, f1, nFactor, (T *) D, Nn));
	CCG_CHECK(hipStreamSynchronize(ctx->stream));
	return CCG_OK;
}

// One matrix: the LT rows [rb, re) (world == 0) or one rank's rows of the band
// layout (world > 0; rb = 0, re = n).  CCG_DIST_MFMA picks the kernels: 2 (the
// default) the 256 x 256 MFMA tiles, 1 the 128 x 128 MFMA tiles, 0 the VALU
// tiles.  Pair mode with -P runs k_snp_pair_proxi whatever it says.
template <int ET>
static int snp_launch(ccg_ctx *ctx, const ccg_snp_args *a, const void *planes, int Wp, double nFactor, void *D, void *N,
                      long long rb, long long re, int rank, int world) {
	typedef typename Elem<ET>::T T;
	if(a->pair && a->proxi) {
		const int W32 = (a->len + 31) / 32;
		// maskProxi pairs of the LT elements [f0, f1)
		const auto run = [&](long long f0, long long f1, T *Dg, T *Ng) {
			const long long g = cdivll(f1 - f0, 4);
			if(f1 <= f0) return hipSuccess;
			k_snp_pair_proxi<ET><<<(unsigned) (g < 16384 ? g : 16384), 256, 0, ctx->stream>>>(
			    (const uint4 *) planes, Wp, W32, a->len, (int) a->proxi, f0, f1, a->norm, a->minLength, a->byteScale, Dg,
			    Ng);
			return hipGetLastError();
		};
		if(world == 0) {
			CCG_CHECK(run(tri(rb), tri(re), (T *) D, (T *) N));
			return CCG_OK;
		}
		// an owned band's rows are contiguous in both the full LT and the rank's
		// buffer with the same relative offsets, so each run of consecutive owned
		// bands is k_snp_pair_proxi over its LT range with D shifted by
		// off(first row) - tri(first row)
		const long long n = a->n, nb = cdivll(n, SB);
		const Shard sh{rank, world};
		for(long long g = rank; g < nb;) {
			long long g2 = g;
			while(world == 1 && g2 + 1 < nb) ++g2;   // world 1 owns every band
			const long long r0 = g * SB, r1 = (g2 + 1) * SB < n ? (g2 + 1) * SB : n;
			CCG_CHECK(run(tri(r0), tri(r1), (T *) D + (sh.off(r0) - tri(r0)), (T *) NULL));
			g = g2 + world;
		}
		CCG_CHECK(hipStreamSynchronize(ctx->stream));
		return CCG_OK;
	}
	const char *mf = getenv("CCG_DIST_MFMA");
	const int mode = mf ? atoi(mf) : 2;
	if(mode != 2) return snp_launch_tile128<ET>(ctx, a, planes, Wp, nFactor, D, N, rb, re, rank, world, mode != 0);
	if(a->pair) return snp_launch_mfma2<ET, true>(ctx, a, planes, Wp, nFactor, D, N, rb, re, rank, world);
	return snp_launch_mfma2<ET, false>(ctx, a, planes, Wp, nFactor, D, N, rb, re, rank, world);
}

static int snp_run(ccg_ctx *ctx, const ccg_snp_args *a, void *D, void *N, int *inc_out, int rank, int world,
                   bool host_in);

int ccg_snp_dev_impl(ccg_ctx *ctx, const ccg_snp_args *a, void *D, void *N, int *inc_out, bool host_in) {
	return snp_run(ctx, a, D, N, inc_out, 0, 0, host_in);
}

int ccg_snp_shard_dev_impl(ccg_ctx *ctx, const ccg_snp_args *a, int rank, int world, void *Dloc, int *inc_out,
                           bool host_in) {
	if(!a || world < 1 || rank < 0 || rank >= world) return CCG_EINVAL;
	if(a->row_begin || a->row_end) return CCG_EINVAL;
	return snp_run(ctx, a, Dloc, NULL, inc_out, rank, world, host_in);
}

// the bit planes of every taxon.  host_in: a->seqs / a->incs are host memory,
// streamed through a bounded staging buffer (ccg_stage_rows), so HBM holds the
// planes and the LT only (configs[4]: 25 GB of planes beside a 250 GB shard,
// where a device copy of the packed MSA would add another 25 GB).  mask: the
// device copy of the non-pair include mask (k_popsum reads it), allocated here.
static int snp_planes(ccg_ctx *ctx, const ccg_snp_args *a, int W32, int Wp, void *planes, bool host_in, DevMem &mask,
                      const int *widx) {
	const auto launch = [&](const uint64_t *seqs, const uint32_t *incs, long long t0, long long rows) {
		const long long pg = cdivll(rows * Wp, 256);
		k_planes<<<(unsigned) (pg < 262144 ? pg : 262144), 256, 0, ctx->stream>>>(
		    seqs, incs, (int) rows, a->stride, W32, Wp, a->pair, (uint2 *) planes + t0 * Wp, (uint4 *) planes + t0 * Wp,
		    widx);
		CCG_CHECK(hipGetLastError());
		return CCG_OK;
	};
	if(!host_in) return launch(a->seqs, a->incs, 0, a->n);
	if(!a->pair) {
		CCG_TRY(mask.alloc((size_t) a->stride * 4));
		CCG_CHECK(hipMemcpyAsync(mask.p, a->incs, (size_t) a->stride * 4, hipMemcpyHostToDevice, ctx->stream));
	}
	return ccg_stage_rows(ctx->stream, a->seqs, a->incs, a->n, a->stride, a->pair != 0,
	                      [&](const uint64_t *sseq, const uint32_t *sinc, long long t0, long long rows) {
		                      return launch(sseq, a->pair ? sinc : mask.as<uint32_t>(), t0, rows);
	                      });
}

static int snp_run(ccg_ctx *ctx, const ccg_snp_args *a, void *D, void *N, int *inc_out, int rank, int world,
                   bool host_in) {
	if(!a || a->n < 0 || a->len <= 0 || a->stride < (a->len + 31) / 32) return CCG_EINVAL;
	if(!ccg_etype_ok(a->etype)) return CCG_EINVAL;
	ctx->dist_slices = ctx->dist_slice_words = 0;   // until a launcher plans (n < 2 and -P's k_snp_pair_proxi: none)
	if(a->n < 2) {
		if(inc_out && !a->pair && host_in) {
			int s = 0;
			for(int w = 0; w < (a->len + 31) / 32; ++w) s += __builtin_popcount(a->incs[w]);
			*inc_out = s;
		} else if(inc_out && !a->pair) {
			DevMem d_inc;
			CCG_TRY(d_inc.alloc(sizeof(int)));
			StreamSync idle(ctx->stream);
			k_popsum<<<1, 256, 0, ctx->stream>>>(a->incs, (a->len + 31) / 32, d_inc.as<int>());
			CCG_CHECK(hipMemcpyAsync(inc_out, d_inc.p, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
			CCG_CHECK(hipStreamSynchronize(ctx->stream));
		}
		return CCG_OK;
	}
	const int W32 = (a->len + 31) / 32;
	const int kc = a->pair ? KCP : KC;
	// Non-pair mode: a word the global mask excludes entirely contributes to
	// no pair (fsacmp.c:552 counts included positions only), so the planes
	// keep only the other words (partial words stay masked); the pair kernels
	// then stream and multiply ~10% fewer words on the headline's alignment.
	// Pair mode's masks are per taxon and stay whole.
	std::vector<int> keep;
	int Wc = W32;
	if(!a->pair) {
		std::vector<uint32_t> hm((size_t) W32);
		if(host_in) std::memcpy(hm.data(), a->incs, (size_t) W32 * 4);
		else {
			CCG_CHECK(hipMemcpyAsync(hm.data(), a->incs, (size_t) W32 * 4, hipMemcpyDeviceToHost, ctx->stream));
			CCG_CHECK(hipStreamSynchronize(ctx->stream));
		}
		for(int w = 0; w < W32; ++w)
			if(hm[w]) keep.push_back(w);
		Wc = (int) keep.size();
		if(Wc == W32 || getenv("CCG_DIST_NOCOMPACT")) {
			keep.clear();
			Wc = W32;
		}
		if(Wc == 0) Wc = 1;   // nothing included: one all-zero word (every count 0)
	}
	const int Wp = (int) (cdivll(Wc, kc) * kc);
	const long long npad = cdivll(a->n, TILE2) * TILE2;   // whole panels of either tile size
	const size_t esz = a->pair ? sizeof(uint4) : sizeof(uint2);
	const size_t planes_b = ((size_t) npad * Wp * esz + 255) & ~(size_t) 255;
	// The planes, the included count, the compacted word list and (host_in) the
	// non-pair mask.  A CCG_CTX_NOSYNC context (a pipeline's dist) borrows the
	// first three from its workspace slot, the small ones behind the planes:
	// no hipMalloc / hipFree per matrix (hipFree waits for every stream of the
	// device, the other context's too).  Any other context owns them.
	DevMem planes, d_inc, d_widx, mask;
	if(ctx->flags & CCG_CTX_NOSYNC) {
		void *ws = NULL;
		CCG_TRY(ccg_ctx_workspace(ctx, CCG_WS_DIST, planes_b + 256 + keep.size() * sizeof(int), &ws));
		planes.borrow(ws);
		d_inc.borrow((char *) ws + planes_b);
		if(!keep.empty()) d_widx.borrow((char *) ws + planes_b + 256);
	} else {
		CCG_TRY(planes.alloc(planes_b));
		CCG_TRY(d_inc.alloc(sizeof(int)));
		if(!keep.empty()) CCG_TRY(d_widx.alloc(keep.size() * sizeof(int)));
	}
	StreamSync idle(ctx->stream);   // (after the holders: no launch still reads them when they free)
	// k_planes writes every word of rows < n: only the padding rows need zeros
	CCG_CHECK(hipMemsetAsync(planes.p + (size_t) a->n * Wp * esz, 0, (size_t) (npad - a->n) * Wp * esz, ctx->stream));
	if(d_widx.p)
		CCG_CHECK(hipMemcpyAsync(d_widx.p, keep.data(), keep.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
	// the compacted word list, or every word (a mask with no included word: one zero word)
	const int Wsrc = d_widx.p ? Wc : (a->pair || Wc == W32 ? W32 : 0);
	CCG_TRY(snp_planes(ctx, a, Wsrc, Wp, planes.p, host_in, mask, d_widx.as<int>()));
	int inc = 0;
	if(!a->pair) {
		k_popsum<<<1, 1024, 0, ctx->stream>>>(mask.p ? mask.as<uint32_t>() : a->incs, W32, d_inc.as<int>());
		CCG_CHECK(hipMemcpyAsync(&inc, d_inc.p, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
		CCG_CHECK(hipStreamSynchronize(ctx->stream));
	}
	// the stream is idle in non-pair mode (the read-back above); in pair mode
	// neither exists
	mask.release();
	d_widx.release();
	double nFactor = 1.0;
	if(!a->pair && a->norm) {
		nFactor = a->norm;
		nFactor /= inc;   // fsacmpthrd.c:171-176
	}
	long long rb = a->row_begin, re = a->row_end;
	if(rb == 0 && re == 0) re = a->n;
	if(rb < 0 || re > a->n || rb > re) return CCG_EINVAL;
	int rc = CCG_OK;
	ctx->dist_ms = 0;
	CCG_CHECK(hipEventRecord(ctx->ev0, ctx->stream));
	if(re > rb) {   // a shard takes every row: rb = 0, re = n
		rc = with_etype(a->etype, [&](auto et) {
			return snp_launch<decltype(et)::value>(ctx, a, planes.p, Wp, nFactor, D, N, rb, re, rank, world);
		});
	}
	CCG_CHECK(hipEventRecord(ctx->ev1, ctx->stream));
	CCG_CHECK(hipStreamSynchronize(ctx->stream));
	if(rc == CCG_OK) CCG_CHECK(hipEventElapsedTime(&ctx->dist_ms, ctx->ev0, ctx->ev1));
	if(inc_out) *inc_out = inc;
	return rc;
}

extern "C" int ccg_last_dist_ms(ccg_ctx *ctx, double *ms) {
	if(!ctx || !ms) return CCG_EINVAL;
	*ms = ctx->dist_ms;
	return CCG_OK;
}

extern "C" int ccg_last_dist_plan(ccg_ctx *ctx, int *slices, int *slice_words) {
	if(!ctx || !slices || !slice_words) return CCG_EINVAL;
	*slices = ctx->dist_slices;
	*slice_words = ctx->dist_slice_words;
	return CCG_OK;
}

// ------------------------------------------------------------------ Phylip round trip
// `ccphylo dist -W ... | ccphylo tree` passes each cell through text: printphy
// (phy.c:59-123) writes an integral d as "%d" and any other as "%.*f" with -x
// digits, and loadPhy (phy.c:469) reads it back with strtod (then the cast to
// the matrix type).  The fused `dist --tree` stores the same values in place:
// K = round-half-even(d * 10^p) exactly (d * 10^p = hi + lo without error),
// then K / 10^p is one correctly rounded division of exact operands, which is
// strtod's result for the printed decimal.  Cells whose product reaches 2^53
// (more digits than a double carries) set *bad; the caller refuses them.
template <typename T>
__global__ void k_round_decimal(T *__restrict__ D, long long elems, double P, int *__restrict__ bad) {
	for(long long e = (long long) blockIdx.x * blockDim.x + threadIdx.x; e < elems;
	    e += (long long) gridDim.x * blockDim.x) {
		const double x = (double) D[e];
		if(x == trunc(x)) continue;   // "%d" or the integer's exact digits
		const double hi = x * P, lo = fma(x, P, -hi);
		const double ah = fabs(hi);
		if(!(ah < 9007199254740992.0)) {   // K itself may not be a double past 2^53
			atomicOr(bad, 1);
			continue;
		}
		double K;
		if(ah < 4503599627370496.0) {
			K = rint(hi);   // half-even on hi; the exact tie needs lo == 0
			const double d = hi - K;
			if(d == 0.5 && lo > 0) K += 1.0;
			else if(d == -0.5 && lo < 0) K -= 1.0;
		} else {
			// 2^52 <= |hi| < 2^53: hi is an integer and |lo| <= 1/2 (half an
			// ulp), so x P rounds to hi unless lo is an exact tie, which goes
			// to the even neighbour (|K| <= 2^53 stays exact)
			K = hi;
			if(lo == 0.5 || lo == -0.5) {
				const double other = hi + (lo > 0 ? 1.0 : -1.0);
				K = fmod(hi, 2.0) == 0.0 ? hi : other;
			}
		}
		D[e] = (T) (K / P);
	}
}

extern "C" int ccg_round_decimal_dev(ccg_ctx *ctx, void *D, int64_t elems, int etype, int precision) {
	if(!ctx || (!D && elems) || elems < 0 || precision < 0 || precision > 22) return CCG_EINVAL;
	if(etype != 8 && etype != 4) return CCG_EUNSUP;
	CCG_CHECK(hipSetDevice(ctx->device));
	CCG_DEVICE_SYNC(ctx);
	if(!elems) return CCG_OK;
	double P = 1.0;
	for(int k = 0; k < precision; ++k) P *= 10.0;   // exact up to 10^22
	DevMem flag;
	CCG_TRY(flag.alloc(sizeof(int)));
	StreamSync idle(ctx->stream);
	int *d_bad = flag.as<int>(), bad = 0;
	CCG_CHECK(hipMemsetAsync(d_bad, 0, sizeof(int), ctx->stream));
	const long long g = cdivll(elems, 256);
	const unsigned grid = (unsigned) (g < 65536 ? g : 65536);
	if(etype == 8) k_round_decimal<double><<<grid, 256, 0, ctx->stream>>>((double *) D, elems, P, d_bad);
	else k_round_decimal<float><<<grid, 256, 0, ctx->stream>>>((float *) D, elems, P, d_bad);
	CCG_CHECK(hipGetLastError());
	CCG_CHECK(hipMemcpyAsync(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
	CCG_CHECK(hipStreamSynchronize(ctx->stream));
	if(bad) {
		ccg_set_last_msg("ccg_round_decimal_dev: a cell needs more than 15 significant digits at this precision");
		return CCG_EUNSUP;
	}
	return CCG_OK;
}
