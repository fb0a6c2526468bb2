// ltdcmp.hip -- `ccphylo phycmp` (phycmp.c:111-138): every sum the seven
// metrics of distcmp.c close from, in one streaming pass over two packed LTs.
//
// Per cell, with a from A and b from B (B's cell at rows perm[i], perm[j] when
// a perm is given), the reference's expressions with their C types: float rows
// multiply, add, subtract and take the minimum in float before widening
// (coscmp_f, bccmp_f, l1cmp_f ...), double rows do all of it in double.
//   ab += a b   aa += a a   bb += b b   a += a   b += b        (cos, p)
//   apb += a + b   mn += a < b ? a : b                          (bc)
//   l1 += |a - b|   l2 += (a - b)^2   linf = max |a - b|
//   chi2 += (a - b)^2 / (a + b)  where a != b
// The reference's serial chain over all cells cannot be kept, so every sum is
// a fixed-order reduction: thread t of a grid of CMP_GRID x CMP_BLOCK threads
// takes CMP_VEC consecutive cells a pass and keeps a compensated (Kahan) double
// per sum; a wave folds by a xor butterfly, a block adds its waves in order,
// and one closing block adds the CMP_GRID block partials, CMP_GRID / CMP_BLOCK
// in a row per thread and then by an LDS tree.  No floating-point atomic, no
// dependence on the device: two runs give the same bits.  Error: a thread's
// compensated sum is within 2 ulp-units of its terms' magnitude whatever its
// length, and 6 + 3 + 3 + 8 further additions follow, so each sum lies within
// about 22 * 2^-53 sum|term| of the exact one -- far inside 1e-13 sum|term|.
#include <string.h>
#include <stdlib.h>
#include "ccg_internal.h"

// tests/test_gpu_fit.py names these sizes
#define CMP_BLOCK 256
#define CMP_VEC 4         // cells per thread and pass (32 or 16 bytes of each LT)
#define CMP_GRID 1024     // blocks, whatever the size: one pass covers CMP_GRID * CMP_BLOCK * CMP_VEC cells
#define CMP_NSUM 11       // ccg_cmp_sums as an array; [10] is linf, a maximum

struct Kahan {
	double s, c;
	__device__ __forceinline__ void add(double x) {
		const double y = x - c, t = s + y;
		c = (t - s) - y;
		s = t;
	}
};

template <int ET>
__device__ __forceinline__ void cmp_cell(typename Elem<ET>::T a, typename Elem<ET>::T b, Kahan (&K)[10], double &linf) {
	typedef typename Elem<ET>::T T;
	const T ab = a * b, aa = a * a, bb = b * b, apb = a + b, mn = a < b ? a : b, df = a - b;
	const double d = (double) df, ad = d < 0 ? -d : d;
	K[0].add((double) ab);
	K[1].add((double) aa);
	K[2].add((double) bb);
	K[3].add((double) a);
	K[4].add((double) b);
	K[5].add((double) apb);
	K[6].add((double) mn);
	K[7].add(ad);
	K[8].add(d * d);
	if(d != 0) K[9].add(d * d / (double) apb);
	linf = linf < ad ? ad : linf;
}

template <int ET>
__global__ __launch_bounds__(CMP_BLOCK) void k_ltd_cmp(const typename Elem<ET>::T *__restrict__ A,
                                                      const typename Elem<ET>::T *__restrict__ B, int64_t cells,
                                                      const int *__restrict__ perm, double *__restrict__ part) {
	typedef typename Elem<ET>::T T;
	Kahan K[10] = {};
	double linf = 0;   // |a - b| >= 0
	const int64_t stride = (int64_t) CMP_GRID * CMP_BLOCK * CMP_VEC;
	for(int64_t base = ((int64_t) blockIdx.x * CMP_BLOCK + threadIdx.x) * CMP_VEC; base < cells; base += stride) {
		T a[CMP_VEC], b[CMP_VEC];
		const int cnt = cells - base < CMP_VEC ? (int) (cells - base) : CMP_VEC;
		if(cnt == CMP_VEC) {   // base is a multiple of CMP_VEC: aligned to the whole vector
			memcpy(a, __builtin_assume_aligned(A + base, CMP_VEC * ET), sizeof(a));
		} else {
			for(int u = 0; u < cnt; ++u) a[u] = A[base + u];
		}
		if(!perm) {
			if(cnt == CMP_VEC) {
				memcpy(b, __builtin_assume_aligned(B + base, CMP_VEC * ET), sizeof(b));
			} else {
				for(int u = 0; u < cnt; ++u) b[u] = B[base + u];
			}
		} else {
			int64_t i = ltd_row(base), j = base - tri(i);
			int pi = perm[i];
			for(int u = 0; u < cnt; ++u) {
				const int pj = perm[j];
				const int64_t hi = pi > pj ? pi : pj, lo = pi > pj ? pj : pi;
				b[u] = B[tri(hi) + lo];
				if(++j == i) {
					++i;
					j = 0;
					if(u + 1 < cnt) pi = perm[i];   // i < n while a cell follows
				}
			}
		}
#pragma unroll
		for(int u = 0; u < CMP_VEC; ++u) {
			if(u < cnt) cmp_cell<ET>(a[u], b[u], K, linf);
		}
	}
	double v[CMP_NSUM];
#pragma unroll
	for(int s = 0; s < 10; ++s) v[s] = K[s].s;
	v[10] = linf;
	// wave: xor butterfly (every lane ends with the same bits: x + y == y + x)
#pragma unroll
	for(int off = 1; off < 64; off <<= 1) {
#pragma unroll
		for(int s = 0; s < CMP_NSUM; ++s) {
			const double o = __shfl_xor(v[s], off, 64);
			v[s] = s == 10 ? (v[s] < o ? o : v[s]) : v[s] + o;
		}
	}
	__shared__ double sw[CMP_BLOCK / 64][CMP_NSUM];
	const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
	if(lane == 0) {
#pragma unroll
		for(int s = 0; s < CMP_NSUM; ++s) sw[wid][s] = v[s];
	}
	__syncthreads();
	if(threadIdx.x < CMP_NSUM) {
		const int s = threadIdx.x;
		double r = sw[0][s];
		for(int w = 1; w < CMP_BLOCK / 64; ++w) r = s == 10 ? (r < sw[w][s] ? sw[w][s] : r) : r + sw[w][s];
		part[(size_t) s * CMP_GRID + blockIdx.x] = r;
	}
}

// one block: out[s] from part[s][0 .. CMP_GRID)
__global__ __launch_bounds__(CMP_BLOCK) void k_ltd_cmp_close(const double *__restrict__ part, double *__restrict__ out) {
	__shared__ double sh[CMP_BLOCK];
	constexpr int PER = CMP_GRID / CMP_BLOCK;
	for(int s = 0; s < CMP_NSUM; ++s) {
		const double *p = part + (size_t) s * CMP_GRID + threadIdx.x * PER;
		double r = p[0];
		for(int u = 1; u < PER; ++u) r = s == 10 ? (r < p[u] ? p[u] : r) : r + p[u];
		sh[threadIdx.x] = r;
		__syncthreads();
		for(int h = CMP_BLOCK / 2; h > 0; h >>= 1) {
			if(threadIdx.x < h) {
				const double x = sh[threadIdx.x], y = sh[threadIdx.x + h];
				sh[threadIdx.x] = s == 10 ? (x < y ? y : x) : x + y;
			}
			__syncthreads();
		}
		if(threadIdx.x == 0) out[s] = sh[0];
		__syncthreads();
	}
}

static int cmp_check(int n, int etype, const int32_t *perm) {
	if(etype == 2 || etype == 1) {
		ccg_set_last_msg("ccg_ltd_cmp: short / byte elements are not implemented");
		return CCG_EUNSUP;
	}
	if(n < 2 || (etype != 8 && etype != 4)) return CCG_EINVAL;
	if(perm) {   // a permutation of 0 .. n-1: every index the kernel forms stays inside B
		unsigned char *seen = (unsigned char *) calloc((size_t) n, 1);
		if(!seen) return CCG_ENOMEM;
		int ok = 1;
		for(int i = 0; i < n && ok; ++i) {
			if(perm[i] < 0 || perm[i] >= n || seen[perm[i]]) ok = 0;
			else seen[perm[i]] = 1;
		}
		free(seen);
		if(!ok) {
			ccg_set_last_msg("ccg_ltd_cmp: perm is not a permutation of the rows");
			return CCG_EINVAL;
		}
	}
	return CCG_OK;
}

extern "C" int ccg_ltd_cmp_dev(ccg_ctx *c, const void *A, const void *B, int n, int etype, const int32_t *perm,
                               ccg_cmp_sums *out) {
	if(!c || !A || !B || !out) return CCG_EINVAL;
	CCG_TRY(cmp_check(n, etype, perm));
	if((((uintptr_t) A) | ((uintptr_t) B)) & (uintptr_t) (CMP_VEC * etype - 1)) {
		ccg_set_last_msg("ccg_ltd_cmp_dev: the LT buffers must be aligned to 32 bytes");   // the kernel loads whole vectors
		return CCG_EINVAL;
	}
	CCG_CHECK(hipSetDevice(c->device));
	CCG_DEVICE_SYNC(c);
	// workspace: block partials, the sums, then the perm
	const size_t npart = (size_t) CMP_NSUM * CMP_GRID, nd = npart + 16;
	void *ws = NULL;
	CCG_TRY(ccg_ctx_workspace(c, CCG_WS_FIT, nd * sizeof(double) + (perm ? (size_t) n * sizeof(int32_t) : 0), &ws));
	double *dpart = (double *) ws, *dout = dpart + npart;
	int *dperm = perm ? (int *) (dpart + nd) : NULL;
	if(perm) CCG_CHECK(hipMemcpyAsync(dperm, perm, (size_t) n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
	const int64_t cells = tri(n);
	CCG_CHECK(hipEventRecord(c->ev0, c->stream));
	with_etype(etype, [&](auto et) {
		constexpr int ET = decltype(et)::value;
		typedef typename Elem<ET>::T T;
		if constexpr(ET == 8 || ET == 4) {
			k_ltd_cmp<ET><<<CMP_GRID, CMP_BLOCK, 0, c->stream>>>((const T *) A, (const T *) B, cells, dperm, dpart);
		}
	});
	CCG_CHECK(hipGetLastError());
	k_ltd_cmp_close<<<1, CMP_BLOCK, 0, c->stream>>>(dpart, dout);
	CCG_CHECK(hipGetLastError());
	CCG_CHECK(hipEventRecord(c->ev1, c->stream));
	double h[CMP_NSUM];
	CCG_CHECK(hipMemcpyAsync(h, dout, sizeof(h), hipMemcpyDeviceToHost, c->stream));
	CCG_CHECK(hipStreamSynchronize(c->stream));
	CCG_CHECK(hipEventElapsedTime(&c->cmp_ms, c->ev0, c->ev1));
	memcpy(out, h, sizeof(h));
	return CCG_OK;
}

extern "C" int ccg_ltd_cmp(ccg_ctx *c, const void *A, const void *B, int n, int etype, const int32_t *perm,
                           ccg_cmp_sums *out) {
	if(!c || !A || !B || !out) return CCG_EINVAL;
	CCG_TRY(cmp_check(n, etype, perm));
	CCG_CHECK(hipSetDevice(c->device));
	const size_t bytes = (size_t) tri(n) * (size_t) etype;
	DevMem a, b;
	CCG_TRY(a.alloc(bytes));
	CCG_TRY(b.alloc(bytes));
	StreamSync idle(c->stream);
	CCG_CHECK(hipMemcpyAsync(a.p, A, bytes, hipMemcpyHostToDevice, c->stream));
	CCG_CHECK(hipMemcpyAsync(b.p, B, bytes, hipMemcpyHostToDevice, c->stream));
	return ccg_ltd_cmp_dev(c, a.p, b.p, n, etype, perm, out);
}

extern "C" int ccg_last_cmp_ms(ccg_ctx *c, double *ms) {
	if(!c || !ms) return CCG_EINVAL;
	*ms = c->cmp_ms;
	return CCG_OK;
}
