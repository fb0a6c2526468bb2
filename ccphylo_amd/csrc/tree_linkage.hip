// tree_linkage.hip -- the linkage tree methods of `ccphylo tree` on an
// HBM-resident packed lower-triangular matrix, for gfx950:
//   -m upgma  dnj.c:985 dnj with initDmin / UPGMApair / updateUPGMA / UPGMA_popArrange / minPos
//   -m ff     the same loop with updateFF
//   -m cf     hclust.c:1671 hclust with initDmin / minQ / updateCF / UPGMA_popArrange
// (-m mn is the NJ loop with an argmax, tree.hip.)
//
// Reference semantics (ccphylo 0.8.5): initDmin hclust.c:205, minQ hclust.c:353,
// updateUPGMA hclust.c:665, updateFF hclust.c:884, updateCF hclust.c:1102,
// UPGMA_popArrange hclust.c:1559, UPGMApair dnj.c:217, minPos dnj.c:977,
// limbLength nj.c:42 / :81.
//
// The criterion is D itself: Q[r] is the minimum of row r (its columns < r)
// and P[r] that column, or P[r] = -1 and Q[r] a lower bound (a "bounded row",
// hclust.c:870).  Per join, without in-kernel grid synchronisation (every
// kernel leaves per-chunk partials that the next single-block kernel folds):
//   k_lk_head    one block: folds the last join's partials (the new row j: its
//                serial row sum, count, minimum; the moved row; minPos's hint).
//                cf: minQ and the join.  upgma / ff: lists the bounded rows
//                that UPGMApair may rescan -- a superset: bound below the
//                running minimum taken over the hint and the exact rows above;
//   k_lk_rescan  upgma / ff: one wave per listed row, its fresh minimum;
//   k_lk_pick    upgma / ff, one block: UPGMApair's serial walk as a suffix
//                minimum over the rows in descending order.  Only rows the walk
//                touches (bound below its running minimum) take their fresh
//                (Q, P); the others stay bounded, as in the reference.  Then
//                limbLength and the join record;
//   k_lk_update  one thread per row k: the new D(k, j), sD / N of k, column
//                j's Q / P rule, row j's candidates and the contributions of
//                the new row sum of j;
//   k_lk_pop     UPGMA_popArrange: row n-1 into row i and column i.
#include <string.h>
#include <stdio.h>
#include <stdlib.h>
#include "ccg_tree_run.h"

#define LK_UPGMA 0
#define LK_FF 1
#define LK_CF 2
#define LK_NT XS_NT   // threads of the single-block kernels

struct LkCtl {
	int done, final_n, njoins;
	int i, j;            // the current join (j < i)
	int neg;             // limbLengthNeg
	int has_missing;
	int hint;            // UPGMApair's start row (minPos, dnj.c:1026-1032)
	int nlist;           // bounded rows listed for the rescan
	int serial_sums, chain_sums;
	long long rows, cells;   // bounded rows the walk rescanned, and their cells
	long long listed;        // rows the rescan kernel took (the superset)
};

struct LkBufs {
	double *sD, *Q, *contrib, *rq;
	int *N, *P, *list, *rj, *lf;
	double *rowq, *upq, *popq, *ppq;   // per-chunk partials (chunk = TB rows)
	int *rowk, *upk, *popk, *ppk, *cnt;
	ccg_join *joins;
	LkCtl *ctl;
};

// (q, k) candidates.  LAST: smaller q, then the later k (the `<=` scans);
// !LAST: smaller q, then the earlier k (updateFF's `dist < Q`, hclust.c:984).
// k < 0: no candidate.
template <bool LAST>
__device__ __forceinline__ void lk_take(double &bq, int &bk, double q, int k) {
	if(k < 0) return;
	if(bk < 0 || q < bq || (q == bq && (LAST ? k > bk : k < bk))) {
		bq = q;
		bk = k;
	}
}
// larger q, then the later k (`min <= dist`, hclust.c:856)
__device__ __forceinline__ void lk_take_max(double &bq, int &bk, double q, int k) {
	if(k < 0) return;
	if(bk < 0 || q > bq || (q == bq && k > bk)) {
		bq = q;
		bk = k;
	}
}

// KIND 0: lk_take<true>, 1: lk_take<false>, 2: lk_take_max
template <int KIND>
__device__ __forceinline__ void lk_takek(double &bq, int &bk, double q, int k) {
	if(KIND == 0) lk_take<true>(bq, bk, q, k);
	else if(KIND == 1) lk_take<false>(bq, bk, q, k);
	else lk_take_max(bq, bk, q, k);
}

template <int KIND>
__device__ __forceinline__ void lk_wave_reduce(double &q, int &k) {
	for(int o = 32; o > 0; o >>= 1) {
		const double oq = __shfl_xor(q, o, 64);
		const int ok = __shfl_xor(k, o, 64);
		lk_takek<KIND>(q, k, oq, ok);
	}
}

// block reduce; the result in thread 0 (sq / sk: blockDim / 64 entries)
template <int KIND>
__device__ __forceinline__ void lk_block_reduce(double &q, int &k, double *sq, int *sk) {
	lk_wave_reduce<KIND>(q, k);
	const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
	__syncthreads();
	if(lane == 0) {
		sq[wid] = q;
		sk[wid] = k;
	}
	__syncthreads();
	if(threadIdx.x == 0)
		for(int w = 1; w < nw; ++w) lk_takek<KIND>(q, k, sq[w], sk[w]);
}

// one wave: fold of G per-chunk partials; the result in every lane
template <int KIND>
__device__ __forceinline__ void lk_fold_wave(const double *pq, const int *pk, int G, double &bq, int &bk) {
	const int lane = threadIdx.x & 63;
	bq = 0;
	bk = -1;
	for(int g = lane; g < G; g += 64) lk_takek<KIND>(bq, bk, pq[g], pk[g]);
	lk_wave_reduce<KIND>(bq, bk);
}

// ------------------------------------------------------------------ init
// hclust.c:205 initDmin.  sD and N in nj.c:111 initSummaD's order: per row the
// row part (m < k) then the column part (m > k), each in increasing m, summed
// serially.  One wave per row: 64 contiguous cells at a time, lane 0 adds them
// in order; the row minimum with `dist <= min` (the later column).
template <int ET>
__global__ __launch_bounds__(TB) void k_lk_init_rows(const typename Elem<ET>::T *__restrict__ D, int n, double bs, LkBufs b) {
	__shared__ double buf[TB / 64][64];
	const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
	const int k = blockIdx.x * (TB / 64) + wid;
	if(k >= n) return;
	double s = 0, bq = 0;
	int c = 1, miss = 0, bk = -1;
	const typename Elem<ET>::T *row = D + tri(k);
	for(int m0 = 0; m0 < k; m0 += 64) {
		const int m = m0 + lane;
		const double d = m < k ? Elem<ET>::get(row[m], bs) : 0.0;
		const bool ok = m < k && 0 <= d;
		miss |= m < k && !ok;
		c += __popcll(__ballot(ok));
		lk_take<true>(bq, bk, d, ok ? m : -1);
		buf[wid][lane] = ok ? d : 0.0;
		__builtin_amdgcn_wave_barrier();
		if(lane == 0) {
			const int lim = k - m0 < 64 ? k - m0 : 64;
			for(int u = 0; u < lim; ++u) s += buf[wid][u];
		}
		__builtin_amdgcn_wave_barrier();
	}
	miss = __any(miss);
	lk_wave_reduce<0>(bq, bk);
	if(lane == 0) {
		b.sD[k] = s;
		b.N[k] = c;
		b.Q[k] = bk < 0 ? DBL_MAX : bq;
		b.P[k] = bk < 0 ? 0 : bk;
		if(miss) atomicOr(&b.ctl->has_missing, 1);
	}
}

template <int ET>
__global__ __launch_bounds__(TB) void k_lk_init_cols(const typename Elem<ET>::T *__restrict__ D, int n, double bs, LkBufs b) {
	const int k = blockIdx.x * TB + threadIdx.x;
	if(k >= n) return;
	double s = b.sD[k];
	int c = b.N[k];
	for(int m = k + 1; m < n; ++m) {
		const double d = Elem<ET>::get(D[tri(m) + k], bs);
		if(0 <= d) {
			s += d;
			++c;
		}
	}
	b.sD[k] = s;
	b.N[k] = c;
}

// ------------------------------------------------------------------ the walk over the rows
// Rows n-1 .. 1 in descending order, LK_NT at a time: calls f(r, m) with m =
// min(m0, v(r') for the rows r' > r), the running minimum UPGMApair holds when
// it reaches row r.  v and f are called by every thread of the block for its
// row (r >= 1) of each pass.
template <typename V, typename F>
__device__ __forceinline__ void lk_desc_walk(int n, double m0, V v, F f) {
	__shared__ double s_w[LK_NT / 64];
	const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
	double carry = m0;
	for(int c0 = 0; c0 < n - 1; c0 += LK_NT) {
		const int r = n - 1 - (c0 + tid);
		const double x = r >= 1 ? v(r) : DBL_MAX;
		const double inc = wave_incl_min(x);
		const double ex = dpp_d<DPP_WAVE_SHR1, 0xF>(DBL_MAX, inc);
		if(lane == 63) s_w[wid] = inc;
		__syncthreads();
		double pre = carry, all = carry;
		for(int w = 0; w < LK_NT / 64; ++w) {
			const double t = s_w[w];
			if(w < wid) pre = t < pre ? t : pre;
			all = t < all ? t : all;
		}
		const double m = ex < pre ? ex : pre;
		if(r >= 1) f(r, m);
		carry = all;
		__syncthreads();
	}
}

// limbLength, the join record (thread 0)
template <int ET>
__device__ __forceinline__ void lk_join(const typename Elem<ET>::T *__restrict__ D, double bs, const LkBufs &b, int i, int j) {
	LkCtl *ctl = b.ctl;
	const double Dij = Elem<ET>::get(D[tri(i) + j], bs);
	double Li, Lj;
	limb_length(&Li, &Lj, b.sD[i], b.sD[j], b.N[i], b.N[j], Dij, ctl->neg);
	ccg_join J;
	J.i = i;
	J.j = j;
	J.Li = Li;
	J.Lj = Lj;
	b.joins[ctl->njoins] = J;
	ctl->njoins += 1;
	ctl->i = i;
	ctl->j = j;
}

// ------------------------------------------------------------------ head
// n: the matrix size of this join; first: the run's first join (nothing to fold)
template <int ET, int MODE>
__global__ __launch_bounds__(LK_NT) void k_lk_head(const typename Elem<ET>::T *__restrict__ D, double bs, LkBufs b, int n, int first) {
	__shared__ double s_q[LK_NT / 64], s_hq;
	__shared__ int s_k[LK_NT / 64], s_hint, s_base, s_sc[LK_NT / 64];
	LkCtl *ctl = b.ctl;
	const int tid = threadIdx.x;
	if(ctl->done) return;
	if(!first) {
		// ---- the last join (i, j) at size np: its partials
		const int np = n + 1, i = ctl->i, j = ctl->j;
		const int G = (int) cdiv(np, TB);
		// the new row sum of j: the contributions in increasing k, summed serially
		// (hclust.c:735 / :819 `sd += dist`)
		double sd;
		bool chain = false;
		if(!exact_sum_w<LK_NT, XS_RB>(b.contrib, np, &sd)) {
			sd = serial_sum_t<LK_NT>(b.contrib, np);
			chain = true;
		}
		if(tid < 64) {
			int c = 0;
			for(int g = tid; g < G; g += 64) c += b.cnt[g];
			c = wave_sum_int(c);
			// row j's minimum (hclust.c:766 / :984 / :1203)
			double rq, uq, pq, ppq;
			int rk, uk, pk, ppk;
			if(MODE == LK_FF) lk_fold_wave<1>(b.rowq, b.rowk, (int) cdiv(j, TB), rq, rk);
			else lk_fold_wave<0>(b.rowq, b.rowk, (int) cdiv(j, TB), rq, rk);
			lk_fold_wave<2>(b.upq, b.upk, G, uq, uk);
			const bool move = i != n;   // UPGMA_popArrange moved row n into row i
			lk_fold_wave<0>(b.popq, b.popk, move ? (int) cdiv(i, TB) : 0, pq, pk);
			lk_fold_wave<0>(b.ppq, b.ppk, move ? (int) cdiv(n, TB) : 0, ppq, ppk);
			if(tid == 0) {
				const double Qj = rk < 0 ? DBL_MAX : rq;
				b.Q[j] = Qj;
				if(rk >= 0) b.P[j] = rk;
				else if(MODE != LK_FF) b.P[j] = 0;   // updateFF leaves P[j] (hclust.c:897-899)
				b.sD[j] = sd;
				b.N[j] = 1 + c;
				// the update's return value: the last k whose running `min <= dist` held (hclust.c:856)
				const int mi = uk >= 0 && Qj <= uq ? uk : j;
				int mj = 0;
				if(move) {
					const double Qi = pk < 0 ? DBL_MAX : pq;
					b.Q[i] = Qi;
					b.P[i] = pk < 0 ? 0 : pk;
					mj = ppk >= 0 && ppq <= Qi ? ppk : i;   // hclust.c:1651 `q <= min`
				}
				// dnj.c:1026-1032 (D->n is already n)
				int h;
				if(mj == n) h = mi;
				else if(mi == n) h = mj;
				else {
					const double qa = mi == j ? Qj : b.Q[mi], qb = b.Q[mj];
					h = (qb < qa || (mi < mj && qb == qa)) ? mj : mi;   // minPos dnj.c:977
				}
				s_hint = h;
				ctl->serial_sums += 1;
				ctl->chain_sums += chain;
			}
		}
		__syncthreads();
	}
	if(first || MODE == LK_CF) {
		// minQ hclust.c:353: the last row with the minimum
		double q = 0;
		int k = -1;
		for(int r = 1 + tid; r < n; r += LK_NT) lk_take<true>(q, k, b.Q[r], r);
		lk_block_reduce<0>(q, k, s_q, s_k);
		if(tid == 0) s_hint = k < 0 ? 0 : k;
		__syncthreads();
	}
	const int hint = s_hint;
	if(MODE == LK_CF) {
		if(tid == 0) {
			const int i = hint, j = b.P[hint];
			if((i == 0 && j == 0) || j < 0 || j >= i) {
				ctl->done = 1;
				ctl->final_n = n;
			} else {
				lk_join<ET>(D, bs, b, i, j);
			}
		}
		return;
	}
	// ---- upgma / ff: the bounded rows UPGMApair may rescan
	if(tid == 0) {
		ctl->hint = hint;
		s_hq = hint ? b.Q[hint] : DBL_MAX;
		s_base = 0;
	}
	__syncthreads();
	const double hq = s_hq;
	// lk_desc_walk's passes over the exact rows only, with a block-wide
	// compaction of the listed rows in each pass (descending row order)
	__shared__ double s_w2[LK_NT / 64];
	const int lane = tid & 63, wid = tid >> 6;
	double carry = hq;
	for(int c0 = 0; c0 < n - 1; c0 += LK_NT) {
		const int r = n - 1 - (c0 + tid);
		double Qr = DBL_MAX;
		int Pr = 0;
		if(r >= 1) {
			Qr = b.Q[r];
			Pr = b.P[r];
		}
		const double x = r >= 1 && Pr >= 0 ? Qr : DBL_MAX;   // exact rows only
		const double inc = wave_incl_min(x);
		const double ex = dpp_d<DPP_WAVE_SHR1, 0xF>(DBL_MAX, inc);
		if(lane == 63) s_w2[wid] = inc;
		__syncthreads();
		double pre = carry, all = carry;
		for(int w = 0; w < LK_NT / 64; ++w) {
			const double t = s_w2[w];
			if(w < wid) pre = t < pre ? t : pre;
			all = t < all ? t : all;
		}
		const double m = ex < pre ? ex : pre;
		const bool listed = r >= 1 && Pr < 0 && Qr < m;
		carry = all;
		int tot;
		const int off = block_excl_scan(listed ? 1 : 0, s_sc, &tot);
		const int base = s_base;
		if(r >= 1) b.lf[r] = listed;
		if(listed) b.list[base + off] = r;
		__syncthreads();
		if(tid == 0) s_base = base + tot;
		__syncthreads();
	}
	if(tid == 0) {
		ctl->nlist = s_base;
		ctl->listed += s_base;
	}
}

// ------------------------------------------------------------------ rescan
// one wave per listed row: its minimum with `q <= updateQ` (dnj.c:266: the later column)
template <int ET>
__global__ __launch_bounds__(TB) void k_lk_rescan(const typename Elem<ET>::T *__restrict__ D, double bs, LkBufs b, int n) {
	const LkCtl *ctl = b.ctl;
	if(ctl->done) return;
	const int nl = ctl->nlist;
	const int lane = threadIdx.x & 63;
	const int w0 = (int) blockIdx.x * (TB / 64) + (threadIdx.x >> 6), nw = (int) gridDim.x * (TB / 64);
	for(int e = w0; e < nl; e += nw) {
		const int r = b.list[e];
		if(r < 1 || r >= n) continue;
		const typename Elem<ET>::T *row = D + tri(r);
		double bq = 0;
		int bk = -1;
		for(int m = lane; m < r; m += 64) {
			const double d = Elem<ET>::get(row[m], bs);
			lk_take<true>(bq, bk, d, 0 <= d ? m : -1);
		}
		lk_wave_reduce<0>(bq, bk);
		if(lane == 0) {
			b.rq[r] = bk < 0 ? DBL_MAX : bq;
			b.rj[r] = bk < 0 ? 0 : bk;
		}
	}
}

// ------------------------------------------------------------------ pick
// dnj.c:217 UPGMApair.  e(r) = the fresh minimum of a listed row, else Q[r]
// (exact, or a bound no smaller than the walk's minimum there): the walk's
// running minimum at row r is min(hint's Q, e of the rows above r); it rescans
// row r iff r is bounded with Q[r] below that, and ends at the highest row with
// the smallest e, the hint's pair winning a tie.
template <int ET>
__global__ __launch_bounds__(LK_NT) void k_lk_pick(const typename Elem<ET>::T *__restrict__ D, double bs, LkBufs b, int n) {
	__shared__ double s_q[LK_NT / 64];
	__shared__ int s_k[LK_NT / 64];
	__shared__ long long s_rows, s_cells;
	LkCtl *ctl = b.ctl;
	if(ctl->done) return;
	const int tid = threadIdx.x;
	const int hint = ctl->hint;
	const double hq = hint ? b.Q[hint] : DBL_MAX;
	const int hp = hint ? b.P[hint] : 0;   // read before any row is rewritten
	if(tid == 0) {
		s_rows = 0;
		s_cells = 0;
	}
	__syncthreads();
	double bq = 0;
	int bk = -1;
	long long rows = 0, cells = 0;
	lk_desc_walk(n, hq,
	             [&](int r) { return b.lf[r] ? b.rq[r] : b.Q[r]; },
	             [&](int r, double m) {
		             const int Pr = b.P[r];
		             const double Qr = b.Q[r];
		             double e = Qr;
		             if(Pr < 0 && Qr < m) {   // the walk rescans row r: its fresh (Q, P) stay
			             e = b.rq[r];
			             b.Q[r] = e;
			             b.P[r] = b.rj[r];
			             rows += 1;
			             cells += r;
		             } else if(Pr < 0) {
			             return;              // stays bounded; never the walk's pair
		             }
		             lk_take<true>(bq, bk, e, r);
	             });
	lk_block_reduce<0>(bq, bk, s_q, s_k);
	if(rows) {
		atomicAdd((unsigned long long *) &s_rows, (unsigned long long) rows);
		atomicAdd((unsigned long long *) &s_cells, (unsigned long long) cells);
	}
	__syncthreads();
	if(tid == 0) {
		ctl->rows += s_rows;
		ctl->cells += s_cells;
		int i = 0, j = 0;
		if(bk >= 1 && bq < hq) {
			i = bk;
			j = b.P[bk];
		} else if(hint && hq != DBL_MAX) {
			i = hint;
			j = hp;
		}
		if((i == 0 && j == 0) || j < 0 || j >= i) {
			ctl->done = 1;
			ctl->final_n = n;
		} else {
			lk_join<ET>(D, bs, b, i, j);
		}
	}
}

// ------------------------------------------------------------------ update
// updateUPGMA / updateFF / updateCF, one thread per row k; chunk g = rows
// [g TB, g TB + TB).  GEN (missing cells): one block walks the chunks in
// order, carrying the reference's sD / N cursor lag: its cursor does not step
// where both D(i, k) and D(k, j) are missing (hclust.c:761-763, :844-846), so
// the updates of sD and N after such a k land one row low.
template <int ET, int MODE, bool GEN>
__global__ __launch_bounds__(TB) void k_lk_update(typename Elem<ET>::T *__restrict__ D, double bs, LkBufs b, int n) {
	__shared__ double sq[TB / 64], sq2[TB / 64];
	__shared__ int sk[TB / 64], sk2[TB / 64], s_sc[TB / 64], s_cn[TB / 64];
	const LkCtl *ctl = b.ctl;
	if(ctl->done) return;
	const int i = ctl->i, j = ctl->j;
	const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
	const long long ri = tri(i), rj = tri(j);
	int lag = 0;   // GEN: rows without a branch so far
	const int G = (int) cdiv(n, TB);
	for(int g = GEN ? 0 : (int) blockIdx.x; g < G; g += GEN ? 1 : (int) gridDim.x) {
		const int k = g * TB + tid;
		const bool act = k < n && k != i && k != j;
		int br = 0;   // 0 none, 1 both, 2 D_ik only, 3 D_kj only
		double Dik = -1, Dkj = -1, dist = -1;
		long long fkj = 0;
		if(act) {
			fkj = k < j ? rj + k : tri(k) + j;
			Dik = Elem<ET>::get(D[k < i ? ri + k : tri(k) + i], bs);
			Dkj = Elem<ET>::get(D[fkj], bs);
			if(0 <= Dik && 0 <= Dkj) {
				br = 1;
				dist = MODE == LK_UPGMA ? (Dik + Dkj) / 2 : MODE == LK_FF ? (Dik < Dkj ? Dkj : Dik) : (Dik < Dkj ? Dik : Dkj);
			} else if(0 <= Dik) {
				br = 2;
				dist = Dik;
			} else if(0 <= Dkj) {
				br = 3;
				dist = Dkj;
			}
		}
		int idx = k;
		if(GEN) {
			int tot;
			const int pre = block_excl_scan(act && br == 0 ? 1 : 0, s_sc, &tot);
			idx = k - lag - pre;
			lag += tot;
		}
		if(br == 1 || br == 2) D[fkj] = Elem<ET>::put(dist, 0, bs);
		if(br == 1) b.sD[idx] -= (Dik + Dkj - dist);
		if(br == 1 || br == 3) b.N[idx] -= 1;
		if(k < n) b.contrib[k] = br ? dist : 0.0;
		// row j's candidates (k < j)
		double rq = dist;
		int rk = act && k < j && (MODE == LK_FF || 0 <= dist) ? k : -1;
		// column j (k > j): the Q / P rule
		double uq = dist;
		int uk = -1;
		if(act && k > j && 0 <= dist) {
			const double Qk = b.Q[k];
			const int Pk = b.P[k];
			if(MODE == LK_CF) {
				if(dist <= Qk && (dist < Qk || Pk == i || Pk == k || Pk < j)) {   // hclust.c:1288-1289
					b.Q[k] = dist;
					b.P[k] = j;
					uk = k;
				}
			} else if(dist < Qk) {                                               // hclust.c:852 / :1070
				b.Q[k] = dist;
				b.P[k] = j;
				uk = k;
			} else if(Pk == i || Pk == j) {
				if(dist == Qk) {
					b.P[k] = j;
					uk = k;
				} else {
					b.P[k] = -1;   // a bounded row
				}
			}
		}
		const int cn = wave_sum_int(br ? 1 : 0);
		if(lane == 0) s_cn[wid] = cn;
		if(MODE == LK_FF) lk_block_reduce<1>(rq, rk, sq, sk);
		else lk_block_reduce<0>(rq, rk, sq, sk);
		lk_block_reduce<2>(uq, uk, sq2, sk2);
		if(tid == 0) {
			b.rowq[g] = rq;
			b.rowk[g] = rk;
			b.upq[g] = uq;
			b.upk[g] = uk;
			int c = 0;
			for(int w = 0; w < TB / 64; ++w) c += s_cn[w];
			b.cnt[g] = c;
		}
		__syncthreads();
	}
}

// ------------------------------------------------------------------ pop
// hclust.c:1559 UPGMA_popArrange at matrix size n (row nn = n - 1 into row /
// column i), one thread per row k
template <int ET>
__global__ __launch_bounds__(TB) void k_lk_pop(typename Elem<ET>::T *__restrict__ D, double bs, LkBufs b, int n) {
	__shared__ double sq[TB / 64], sq2[TB / 64];
	__shared__ int sk[TB / 64], sk2[TB / 64];
	const LkCtl *ctl = b.ctl;
	if(ctl->done) return;
	const int i = ctl->i, nn = n - 1;
	if(i == nn) return;
	const int tid = threadIdx.x, g = (int) blockIdx.x;
	const int k = g * TB + tid;
	double pq = 0, cq = 0;
	int pk = -1, ck = -1;
	if(k < nn && k != i) {
		const typename Elem<ET>::T v = D[tri(nn) + k];
		const double q = Elem<ET>::get(v, bs);
		if(k < i) {
			D[tri(i) + k] = v;
			if(0 <= q) {   // hclust.c:1622 `0 <= q && q <= Q`
				pq = q;
				pk = k;
			}
		} else {
			D[tri(k) + i] = v;
			if(0 <= q) {
				const double Qk = b.Q[k];
				if(q <= Qk && (b.P[k] < i || q < Qk)) {   // hclust.c:1647-1648
					b.Q[k] = q;
					b.P[k] = i;
					cq = q;
					ck = k;
				}
			}
		}
	}
	if(g == 0 && tid == 0) {
		b.sD[i] = b.sD[nn];
		b.N[i] = b.N[nn];
	}
	lk_block_reduce<0>(pq, pk, sq, sk);
	lk_block_reduce<0>(cq, ck, sq2, sk2);
	if(tid == 0) {
		b.popq[g] = pq;
		b.popk[g] = pk;
		b.ppq[g] = cq;
		b.ppk[g] = ck;
	}
}

// ------------------------------------------------------------------ host
static size_t lk_layout(LkBufs *bp, int n, char *m) {
	const size_t nb = (size_t) cdiv(n, TB) + 1;
	size_t sz = 0;
	auto take = [&](size_t bytes) {
		size_t off = sz;
		sz += (bytes + 255) & ~(size_t) 255;
		return off;
	};
	const size_t v8 = ((size_t) n + 1) * 8, v4 = ((size_t) n + 1) * 4;
	size_t o_sD = take(v8), o_Q = take(v8), o_c = take(v8), o_rq = take(v8);
	size_t o_N = take(v4), o_P = take(v4), o_l = take(v4), o_rj = take(v4), o_lf = take(v4);
	size_t o_q0 = take(nb * 8), o_q1 = take(nb * 8), o_q2 = take(nb * 8), o_q3 = take(nb * 8);
	size_t o_k0 = take(nb * 4), o_k1 = take(nb * 4), o_k2 = take(nb * 4), o_k3 = take(nb * 4), o_cn = take(nb * 4);
	size_t o_j = take((size_t) n * sizeof(ccg_join)), o_ctl = take(sizeof(LkCtl));
	if(!m) return sz;
	LkBufs &b = *bp;
	b.sD = (double *) (m + o_sD);
	b.Q = (double *) (m + o_Q);
	b.contrib = (double *) (m + o_c);
	b.rq = (double *) (m + o_rq);
	b.N = (int *) (m + o_N);
	b.P = (int *) (m + o_P);
	b.list = (int *) (m + o_l);
	b.rj = (int *) (m + o_rj);
	b.lf = (int *) (m + o_lf);
	b.rowq = (double *) (m + o_q0);
	b.upq = (double *) (m + o_q1);
	b.popq = (double *) (m + o_q2);
	b.ppq = (double *) (m + o_q3);
	b.rowk = (int *) (m + o_k0);
	b.upk = (int *) (m + o_k1);
	b.popk = (int *) (m + o_k2);
	b.ppk = (int *) (m + o_k3);
	b.cnt = (int *) (m + o_cn);
	b.joins = (ccg_join *) (m + o_j);
	b.ctl = (LkCtl *) (m + o_ctl);
	return sz;
}

template <int ET, int MODE>
static int lk_enqueue(hipStream_t st, typename Elem<ET>::T *D, double bs, const LkBufs &b, int n, int first, bool general,
                      unsigned rescan_blocks) {
	const unsigned gn = cdiv(n, TB);
	int launches = 0;
	k_lk_head<ET, MODE><<<1, LK_NT, 0, st>>>(D, bs, b, n, first);
	++launches;
	if(MODE != LK_CF) {
		const unsigned gr = rescan_blocks < gn ? rescan_blocks : gn;
		k_lk_rescan<ET><<<gr, TB, 0, st>>>(D, bs, b, n);
		k_lk_pick<ET><<<1, LK_NT, 0, st>>>(D, bs, b, n);
		launches += 2;
	}
	if(general) k_lk_update<ET, MODE, true><<<1, TB, 0, st>>>(D, bs, b, n);
	else k_lk_update<ET, MODE, false><<<gn, TB, 0, st>>>(D, bs, b, n);
	k_lk_pop<ET><<<cdiv(n - 1, TB), TB, 0, st>>>(D, bs, b, n);
	return launches + 2;
}

template <int ET>
static int lk_run_t(ccg_ctx *ctx, const ccg_tree_args *a, void *Dd, ccg_join *joins, int *njoins, int *final_n,
                    double *final_d, int64_t *stats) {
	typedef typename Elem<ET>::T T;
	T *D = (T *) Dd;
	const int n0 = a->n;
	const double bs = a->byteScale;
	const int mode = a->method == CCG_TREE_UPGMA ? LK_UPGMA : a->method == CCG_TREE_FF ? LK_FF : LK_CF;
	hipStream_t st = ctx->stream;
	void *mem;
	const size_t sz = lk_layout(NULL, n0, NULL);
	int rc = ccg_ctx_workspace(ctx, CCG_WS_TREE, sz, &mem);
	if(rc) return rc;
	CCG_CHECK(hipMemsetAsync(mem, 0, sz, st));
	LkBufs b;
	lk_layout(&b, n0, (char *) mem);
	LkCtl init;
	memset(&init, 0, sizeof(init));
	init.neg = (a->flags & 2) != 0;
	// the rescan grid (CCG_LK_RESCAN_BLOCKS: tests drive the one-block and the many-block form)
	unsigned rescan_blocks = 256;
	if(const char *e = getenv("CCG_LK_RESCAN_BLOCKS")) {
		const int v = atoi(e);
		if(v >= 1 && v <= 4096) rescan_blocks = (unsigned) v;
	}
	TreeRun<LkCtl> run(ctx, b.ctl);
	CCG_TRY(run.begin(init, false));   // (no per-kernel classes: a profiled run reports zeros)
	k_lk_init_rows<ET><<<cdiv(n0, TB / 64), TB, 0, st>>>(D, n0, bs, b);
	k_lk_init_cols<ET><<<cdiv(n0, TB), TB, 0, st>>>(D, n0, bs, b);
	run.launches += 2;
	CCG_CHECK(hipGetLastError());
	LkCtl h;
	CCG_TRY(run.read_ctl(h));
	const bool general = h.has_missing != 0;
	if(general && mode == LK_CF) {
		ccg_set_last_msg("tree method cf: a matrix with missing (negative) cells is not supported "
		                 "(updateCF miscounts N there, hclust.c:1188)");
		return CCG_EUNSUP;
	}
	int n = n0;
	const int stop_n = a->max_joins > 0 && a->max_joins < n0 - 2 ? n0 - a->max_joins : 2;
	while(n > stop_n) {
		const int first = n == n0;
		if(mode == LK_UPGMA) run.launches += lk_enqueue<ET, LK_UPGMA>(st, D, bs, b, n, first, general, rescan_blocks);
		else if(mode == LK_FF) run.launches += lk_enqueue<ET, LK_FF>(st, D, bs, b, n, first, general, rescan_blocks);
		else run.launches += lk_enqueue<ET, LK_CF>(st, D, bs, b, n, first, general, rescan_blocks);
		CCG_CHECK(hipGetLastError());
		--n;
		bool read;
		CCG_TRY(run.check(h, &read));
		if(read && h.done) break;
	}
	CCG_TRY(run.finish(h, n, b.joins, joins, njoins, final_n, final_d));
	if(*final_n == 2) CCG_TRY(run.final_distance<ET>(D, bs, final_d));
	TreeStats s = run.stats();
	s.rows = s.ref_rows = h.rows;
	s.cells = s.ref_cells = h.cells;
	s.serial_sums = h.serial_sums;
	s.chain_sums = h.chain_sums;
	s.write(stats, a->profile != 0, run.kt);
	return run.end();
}

// CCG_TREE_UPGMA / CCG_TREE_CF / CCG_TREE_FF on a device LT (consumed)
int ccg_tree_linkage_impl(ccg_ctx *ctx, const ccg_tree_args *a, void *Dd, ccg_join *joins, int *njoins, int *final_n,
                          double *final_d, int64_t *stats) {
	if(!ccg_etype_ok(a->etype)) return CCG_EINVAL;
	return with_etype(a->etype, [&](auto et) {
		return lk_run_t<decltype(et)::value>(ctx, a, Dd, joins, njoins, final_n, final_d, stats);
	});
}
