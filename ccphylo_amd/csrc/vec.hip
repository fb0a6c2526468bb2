// vec.hip -- `ccphylo tsv2phy` (tsv2phy.c:86): all-pairs distances between the
// rows of a dense m x n table, into the packed LT.
//
// The reference computes every cell as one serial chain over the columns
// (distcmp.c's *_d / *_f functions), rounding each product and each sum on its
// own.  The cells are independent, so the parallelism is over the pairs only:
// a block owns a T x T tile of pairs, a thread an RT x RT register tile, and
// every pair walks the columns 0 .. n-1 in order with the reference's exact
// expression (-ffp-contract=off: no FMA).  No split over the columns, no tree
// reduction, no matrix instruction -- all of them reorder or fuse the sums.
//
// The two row panels of a tile are staged K columns at a time through LDS as a
// transposed image s[k][row] (row stride T + 2: rows stay 16-byte aligned and
// the transposing stores of a wave meet at most two to a bank).  A thread owns
// pairs of neighbouring rows (2 t, 2 t + 1, and the same 32 further on) of both
// panels, so one column costs it a 16-byte read per pair (8 bytes for float
// rows) -- the widths that reach the LDS array's full rate -- and a wave's
// reads are 16 consecutive pairs of the second panel and a broadcast of the
// first: conflict-free.
// What depends on one row only (cos: sum x^2; p: sum x and the variance term)
// comes from a one-thread-per-row pre-pass in the same order and rounding.
#include <math.h>
#include <stdlib.h>
#include "ccg_internal.h"

#define VEC_K 32        // columns per LDS chunk
#define VEC_BLOCK 256   // 16 x 16 threads
#define VEC_T_BIG 64    // pairs per tile side: 4 x 4 per thread
#define VEC_T_SMALL 32  // 2 x 2 per thread: small tables still give every CU a tile
#define VEC_SMALL_M 3072 // rows up to which the small form is the faster one (measured: profiles/vec_tiles.txt)

template <int VT> struct VecElem;
template <> struct VecElem<8> { typedef double T; };
template <> struct VecElem<4> { typedef float T; };

// ---------------------------------------------------------------- pre-pass
// r0[i] = sum x^2 (cos), or the variance term sum x^2 - e * e / n (p);
// r1[i] = e = sum x (p).  Column order, starting from column 0's term.
template <int M, int VT>
__global__ void k_vec_rows(const void *__restrict__ Xv, int m, int n, int64_t stride, double *__restrict__ r0,
                           double *__restrict__ r1) {
	typedef typename VecElem<VT>::T V;
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if(i >= m) return;
	const V *x = (const V *) Xv + (int64_t) i * stride;
	V t = x[0];
	double e = (double) t, v = (double) (t * t);
	for(int k = 1; k < n; ++k) {
		t = x[k];
		e += (double) t;
		v += (double) (t * t);
	}
	if(M == CCG_VEC_PEARSON) {
		v -= e * e / (double) n;
		r1[i] = e;
	}
	r0[i] = v;
}

// ---------------------------------------------------------------- the cell
// one column of one pair: x from the row i (the reference's v1), y from row j
template <int M, bool FIRST, typename V>
__device__ __forceinline__ void vec_step(V x, V y, double &d, double &s, double ex) {
	if(M == CCG_VEC_COS || M == CCG_VEC_PEARSON) {
		const double t = (double) (x * y);
		d = FIRST ? t : d + t;
	} else if(M == CCG_VEC_BC) {
		const double t = (double) (x < y ? x : y), u = (double) (x + y);
		d = FIRST ? t : d + t;
		s = FIRST ? u : s + u;
	} else if(M == CCG_VEC_CHI2) {
		const double T = (double) (x - y);
		if(FIRST) {
			d = T ? T * T / (double) (x + y) : 0;
		} else if(T) {
			d += T * T / (double) (x + y);
		}
	} else if(M == CCG_VEC_LINF) {
		const double t = (double) (x - y);
		if(FIRST) {
			d = t < 0 ? -t : t;
		} else if(d < t) {
			d = t;
		} else if(t < 0 && d < -t) {
			d = -t;
		}
	} else {
		const double t = (double) (x - y);
		double u = t < 0 ? -t : t;
		if(M == CCG_VEC_L2) u = t * t;
		if(M == CCG_VEC_LN) u = pow(u, ex);
		d = FIRST ? u : d + u;
	}
}

// the closing expression; ri / rj the pre-pass values of the two rows
template <int M>
__device__ __forceinline__ double vec_close(double d, double s, double ri0, double rj0, double ri1, double rj1, int n,
                                            double ex) {
	if(M == CCG_VEC_COS) {
		if(!ri0 || !rj0) return -1;
		d = 1 - d / sqrt(ri0 * rj0);
		return d < 0 ? 0 : d;
	} else if(M == CCG_VEC_PEARSON) {
		d -= ri1 * rj1 / (double) n;
		if(!ri0 || !rj0) return 0;
		return d / sqrt(ri0 * rj0);
	} else if(M == CCG_VEC_BC) {
		d = 1 - 2 * d / s;
		return d < 0 ? 0 : d;
	} else if(M == CCG_VEC_L2 || M == CCG_VEC_CHI2) {
		return sqrt(d);
	} else if(M == CCG_VEC_LN) {
		d = pow(d, 1.0 / ex);
		return d < 0 ? 0 : d;
	}
	return d;
}

// the a-th row a thread owns in a panel: t = ty (first panel) or tx (second)
__device__ __forceinline__ int vec_row(int t, int a) { return (a >> 1) * 32 + t * 2 + (a & 1); }

__device__ __forceinline__ void vec_tile_of(long long t, int &ti, int &tj) {
	long long a = (long long) ((sqrt(8.0 * (double) t + 1.0) - 1.0) * 0.5);
	while(a * (a + 1) / 2 > t) --a;
	while((a + 1) * (a + 2) / 2 <= t) ++a;
	ti = (int) a;
	tj = (int) (t - a * (a + 1) / 2);
}

// ------------------------------------------------------------- pair kernel
// grid: one block per tile (ti, tj), tj <= ti, of the lower triangle
template <int M, int VT, int RT>
__global__ void __launch_bounds__(VEC_BLOCK)
k_vec_pairs(const void *__restrict__ Xv, int m, int n, int64_t stride, const double *__restrict__ r0,
            const double *__restrict__ r1, double ex, void *__restrict__ Dv, int etype) {
	typedef typename VecElem<VT>::T V;
	constexpr int T = 16 * RT;
	constexpr int LD = T * VEC_K / VEC_BLOCK;   // elements a thread stages per panel and chunk
	__shared__ __attribute__((aligned(16))) V sA[VEC_K][T + 2], sB[VEC_K][T + 2];
	const V *X = (const V *) Xv;
	int ti, tj;
	vec_tile_of(blockIdx.x, ti, tj);
	const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
	const int lc = tid & (VEC_K - 1), lr = tid / VEC_K;   // staging: column of the chunk, first row
	const int rowA = ti * T, rowB = tj * T;

	V na[LD], nb[LD];
	auto fetch = [&](int c0) {
		const int c = c0 + lc;
#pragma unroll
		for(int p = 0; p < LD; ++p) {
			const int r = lr + p * (VEC_BLOCK / VEC_K);
			const int ia = rowA + r, ib = rowB + r;
			na[p] = (c < n && ia < m) ? X[(int64_t) ia * stride + c] : (V) 0;
			nb[p] = (c < n && ib < m) ? X[(int64_t) ib * stride + c] : (V) 0;
		}
	};

	double d[RT][RT], s[RT][RT];
#pragma unroll
	for(int a = 0; a < RT; ++a) {
#pragma unroll
		for(int b = 0; b < RT; ++b) {
			d[a][b] = 0;
			s[a][b] = 0;
		}
	}

	fetch(0);
	for(int c0 = 0; c0 < n; c0 += VEC_K) {
#pragma unroll
		for(int p = 0; p < LD; ++p) {
			const int r = lr + p * (VEC_BLOCK / VEC_K);
			sA[lc][r] = na[p];
			sB[lc][r] = nb[p];
		}
		__syncthreads();
		if(c0 + VEC_K < n) fetch(c0 + VEC_K);   // the next chunk's loads fly during this chunk's columns
		const int kn = n - c0 < VEC_K ? n - c0 : VEC_K;
		int k = 0;
		if(c0 == 0) {   // every accumulator starts from column 0's term, not from 0
			V x[RT], y[RT];
#pragma unroll
			for(int a = 0; a < RT; ++a) {
				x[a] = sA[0][vec_row(ty, a)];
				y[a] = sB[0][vec_row(tx, a)];
			}
#pragma unroll
			for(int a = 0; a < RT; ++a) {
#pragma unroll
				for(int b = 0; b < RT; ++b) vec_step<M, true, V>(x[a], y[b], d[a][b], s[a][b], ex);
			}
			k = 1;
		}
#pragma unroll 2
		for(; k < kn; ++k) {
			V x[RT], y[RT];
#pragma unroll
			for(int a = 0; a < RT; ++a) {
				x[a] = sA[k][vec_row(ty, a)];
				y[a] = sB[k][vec_row(tx, a)];
			}
#pragma unroll
			for(int a = 0; a < RT; ++a) {
#pragma unroll
				for(int b = 0; b < RT; ++b) vec_step<M, false, V>(x[a], y[b], d[a][b], s[a][b], ex);
			}
		}
		__syncthreads();
	}

	constexpr bool ROWS = M == CCG_VEC_COS || M == CCG_VEC_PEARSON;
#pragma unroll
	for(int a = 0; a < RT; ++a) {
		const int i = rowA + vec_row(ty, a);
		if(i >= m) continue;
		const double ri0 = ROWS ? r0[i] : 0, ri1 = M == CCG_VEC_PEARSON ? r1[i] : 0;
		const int64_t base = tri(i);
#pragma unroll
		for(int b = 0; b < RT; ++b) {
			const int j = rowB + vec_row(tx, b);
			if(j >= i) continue;   // the diagonal tiles' upper part, and j >= m with it
			const double rj0 = ROWS ? r0[j] : 0, rj1 = M == CCG_VEC_PEARSON ? r1[j] : 0;
			const double v = vec_close<M>(d[a][b], s[a][b], ri0, rj0, ri1, rj1, n, ex);
			if(etype == 8) ((double *) Dv)[base + j] = v;
			else ((float *) Dv)[base + j] = (float) v;
		}
	}
}

// ---------------------------------------------------------------- launches
template <int M, int VT>
static void vec_launch(ccg_ctx *c, const ccg_vec_args *a, const double *r0, const double *r1, void *D, int tile) {
	const int m = a->m;
	if(M == CCG_VEC_COS || M == CCG_VEC_PEARSON)
		k_vec_rows<M, VT><<<(m + 255) / 256, 256, 0, c->stream>>>(a->X, m, a->n, a->stride, (double *) r0, (double *) r1);
	const long long nb = (m + tile - 1) / tile, tiles = nb * (nb + 1) / 2;
	if(tile == VEC_T_BIG)
		k_vec_pairs<M, VT, VEC_T_BIG / 16><<<(unsigned) tiles, VEC_BLOCK, 0, c->stream>>>(a->X, m, a->n, a->stride, r0, r1,
		                                                                               a->exponent, D, a->etype);
	else
		k_vec_pairs<M, VT, VEC_T_SMALL / 16><<<(unsigned) tiles, VEC_BLOCK, 0, c->stream>>>(a->X, m, a->n, a->stride, r0,
		                                                                                 r1, a->exponent, D, a->etype);
}

template <int VT>
static void vec_launch_metric(ccg_ctx *c, const ccg_vec_args *a, const double *r0, const double *r1, void *D, int tile) {
	switch(a->metric) {
		case CCG_VEC_COS: vec_launch<CCG_VEC_COS, VT>(c, a, r0, r1, D, tile); break;
		case CCG_VEC_CHI2: vec_launch<CCG_VEC_CHI2, VT>(c, a, r0, r1, D, tile); break;
		case CCG_VEC_BC: vec_launch<CCG_VEC_BC, VT>(c, a, r0, r1, D, tile); break;
		case CCG_VEC_L1: vec_launch<CCG_VEC_L1, VT>(c, a, r0, r1, D, tile); break;
		case CCG_VEC_L2: vec_launch<CCG_VEC_L2, VT>(c, a, r0, r1, D, tile); break;
		case CCG_VEC_LINF: vec_launch<CCG_VEC_LINF, VT>(c, a, r0, r1, D, tile); break;
		case CCG_VEC_LN: vec_launch<CCG_VEC_LN, VT>(c, a, r0, r1, D, tile); break;
		default: vec_launch<CCG_VEC_PEARSON, VT>(c, a, r0, r1, D, tile); break;
	}
}

static int vec_check(const ccg_vec_args *a) {
	if(!a) return CCG_EINVAL;
	if(a->etype == 2 || a->etype == 1) return CCG_EUNSUP;
	const char *bad = NULL;
	if(a->etype != 8 && a->etype != 4) bad = "ccg_vec_ltd: etype must be 8 or 4";
	else if(a->n < 1) bad = "ccg_vec_ltd: the table needs at least one column";
	else if(a->vtype != 8 && a->vtype != 4) bad = "ccg_vec_ltd: vtype must be 8 (double) or 4 (float)";
	else if(a->metric < CCG_VEC_COS || a->metric > CCG_VEC_PEARSON) bad = "ccg_vec_ltd: unknown metric";
	else if(a->metric == CCG_VEC_LN && !(a->exponent > 0 && a->exponent <= DBL_MAX))
		bad = "ccg_vec_ltd: the exponent of l<n> must be finite and > 0";
	else if(a->m >= 2 && a->stride < a->n) bad = "ccg_vec_ltd: the row stride is shorter than a row";
	if(bad) {
		ccg_set_last_msg(bad);
		return CCG_EINVAL;
	}
	return CCG_OK;
}

// the tile edge for m rows: the small form while the large one would leave
// CUs without a tile (CCG_VEC_TILE=32 / 64 forces one; tests drive both)
static int vec_tile(int m) {
	if(const char *e = getenv("CCG_VEC_TILE")) {
		const int v = atoi(e);
		if(v == VEC_T_BIG || v == VEC_T_SMALL) return v;
	}
	return m <= VEC_SMALL_M ? VEC_T_SMALL : VEC_T_BIG;
}

// device pointers throughout
static int vec_run(ccg_ctx *c, const ccg_vec_args *a, void *D) {
	c->vec_ms = 0;
	c->vec_pending = 0;
	c->vec_tile = 0;
	if(a->m < 2) return CCG_OK;
	void *ws = NULL;
	int rc = ccg_ctx_workspace(c, CCG_WS_VEC, 2 * (size_t) a->m * sizeof(double), &ws);
	if(rc) return rc;
	const double *r0 = (const double *) ws, *r1 = r0 + a->m;
	const int tile = vec_tile(a->m);
	CCG_CHECK(hipEventRecord(c->ev0, c->stream));
	if(a->vtype == 8) vec_launch_metric<8>(c, a, r0, r1, D, tile);
	else vec_launch_metric<4>(c, a, r0, r1, D, tile);
	CCG_CHECK(hipGetLastError());
	CCG_CHECK(hipEventRecord(c->ev1, c->stream));
	c->vec_tile = tile;
	c->vec_pending = 1;
	if(!(c->flags & CCG_CTX_NOSYNC)) {
		CCG_CHECK(hipStreamSynchronize(c->stream));
		CCG_CHECK(hipEventElapsedTime(&c->vec_ms, c->ev0, c->ev1));
		c->vec_pending = 0;
	}
	return CCG_OK;
}

extern "C" {

int ccg_vec_ltd_dev(ccg_ctx *c, const ccg_vec_args *a, void *D) {
	int rc = vec_check(a);
	if(rc) return rc;
	if(!c || (a->m > 1 && (!D || !a->X))) return CCG_EINVAL;
	CCG_CHECK(hipSetDevice(c->device));
	CCG_DEVICE_SYNC(c);   // inputs may come from other streams (e.g. torch's)
	return vec_run(c, a, D);
}

int ccg_vec_ltd(ccg_ctx *c, const ccg_vec_args *a, void *D) {
	int rc = vec_check(a);
	if(rc) return rc;
	if(!c || (a->m > 1 && (!D || !a->X))) return CCG_EINVAL;
	if(a->m < 2) return vec_run(c, a, NULL);
	CCG_CHECK(hipSetDevice(c->device));
	const size_t m = (size_t) a->m, rowb = (size_t) a->n * (size_t) a->vtype;
	const size_t xb = (m * rowb + 255) & ~(size_t) 255, lt = m * (m - 1) / 2 * (size_t) a->etype;
	DevMem mem;
	CCG_TRY(mem.alloc(xb + lt));
	hipStream_t st = c->stream;
	StreamSync idle(st);
	ccg_vec_args d = *a;
	d.X = mem.p;
	d.stride = a->n;   // packed on the way up
	CCG_CHECK(hipMemcpy2DAsync(mem.p, rowb, a->X, (size_t) a->stride * (size_t) a->vtype, rowb, m, hipMemcpyHostToDevice, st));
	CCG_TRY(vec_run(c, &d, mem.p + xb));
	CCG_CHECK(hipMemcpyAsync(D, mem.p + xb, lt, hipMemcpyDeviceToHost, st));
	CCG_CHECK(hipStreamSynchronize(st));
	return CCG_OK;
}

int ccg_last_vec_ms(ccg_ctx *c, double *ms) {
	if(!c || !ms) return CCG_EINVAL;
	if(c->vec_pending) {   // a CCG_CTX_NOSYNC call returned before its kernels ended
		CCG_CHECK(hipEventSynchronize(c->ev1));
		CCG_CHECK(hipEventElapsedTime(&c->vec_ms, c->ev0, c->ev1));
		c->vec_pending = 0;
	}
	*ms = c->vec_ms;
	return CCG_OK;
}

int ccg_last_vec_plan(ccg_ctx *c, int *tile, int *chunk) {
	if(!c || !tile || !chunk) return CCG_EINVAL;
	*tile = c->vec_tile;
	*chunk = c->vec_tile ? VEC_K : 0;
	return CCG_OK;
}

}   // extern "C"
