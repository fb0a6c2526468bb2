// merge.hip -- `ccphylo merge` (merge.c:122 merge, :309 jl_merge, :47
// normalize_ltdMatrix): K source LTs, each with its own rows of the union,
// accumulated into the union's packed LTs D and N in HBM.
//
// Per union cell the reference's chain is kept: the sources in file order,
//   weighted:    D = D + d * w   N = N + w
//   unweighted:  D = D + d       N = N + 1
// every step rounded in the element type (float rows multiply and add in
// float; the file is built with -ffp-contract=off and the product is a
// statement of its own, so no FMA forms).  With `first`, source 0 stores its
// product and weight instead of adding: a first-matrix cell is x, a later
// cell +0 + x, and the sign of zero differs as in the reference.  A source's
// union indices are distinct, so a union cell is touched at most once per
// source: no atomics.
//
// Two forms, the same bits:
//   gather   ordered by destination.  A thread owns MRG_VEC consecutive union
//            cells, loads D and N once, walks the batch's sources in order
//            through per-source inverse tables (union row -> source row, -1
//            where the source lacks it), fetches d and w at (max, min) of the
//            two source rows, keeps the chain in registers and stores D and N
//            once, coalesced.  A block first ors, over the union rows its
//            cells span, which sources hold one of them, and walks only those;
//            a block no source reaches stores nothing.
//            Bytes: 4 E per union cell of rows [0, n) that a reached block
//            holds, 4 bytes of table per cell and source, 2 E per source cell.
//   scatter  ordered by source.  A thread owns MRG_VEC consecutive cells of
//            one source, reads d and w coalesced and read-modify-writes the
//            union cells at (max, min) of the two union rows; one launch per
//            source, in order on the stream.
//            Bytes: 2 E read and 2 x 2 E of scattered read-modify-write per
//            source cell, whatever the union's size.
// The scatter form wins while the sources are small beside the union (its
// cost does not depend on the union's size), the gather form from about an
// eighth of the union's cells on: see MRG_CROSSOVER.
#include <stdlib.h>
#include <string.h>
#include "ccg_internal.h"

// tests/test_gpu_merge.py names these sizes
#define MRG_BLOCK 256
#define MRG_VEC 4         // cells per thread (32 or 16 bytes of D and of N)
#define MRG_MAX_SRC 16    // sources a call takes (CCG_MERGE_MAX_SRC)
// plan 0: gather where the batch's source cells are at least this share of the
// union's cells.  Measured on one MI355X (profiles/merge_bench.json): 16 double
// sources of random rows over a 20 000-row union, the share swept from 0.002
// to 0.8; scatter leads up to 0.10 (1.57 against 1.76 ms), gather from 0.20
// (2.36 against 2.85 ms), and the two cross at 0.13 (DESIGN.md 4 "merge").
#define MRG_CROSSOVER 0.13
static_assert(MRG_MAX_SRC == CCG_MERGE_MAX_SRC, "the header's batch size");
static_assert(MRG_MAX_SRC <= 32, "the block's source mask is one word");

struct MrgBatch {
	const void *d[MRG_MAX_SRC];
	const void *w[MRG_MAX_SRC];
	const int *inv;   // nsrc tables of n entries
	int nsrc, n, first;
};

// one step of the chain on the registers of a cell
template <class T, bool W>
__device__ __forceinline__ void mrg_step(T &D, T &N, T x, T w, bool init) {
	const T p = W ? x * w : x;
	const T one = W ? w : (T) 1;
	if(init) {
		D = p;
		N = one;
	} else {
		D = D + p;
		N = N + one;
	}
}

template <class T>
__device__ __forceinline__ void mrg_load(T (&v)[MRG_VEC], const T *p, int cnt) {
	if(cnt == MRG_VEC) {   // the offset is a multiple of MRG_VEC and the buffer aligned: one whole vector
		memcpy(v, __builtin_assume_aligned(p, MRG_VEC * sizeof(T)), sizeof(v));
	} else {
		for(int u = 0; u < MRG_VEC; ++u) v[u] = u < cnt ? p[u] : (T) 0;
	}
}
template <class T>
__device__ __forceinline__ void mrg_store(T *p, const T (&v)[MRG_VEC], int cnt) {
	if(cnt == MRG_VEC) {
		memcpy(__builtin_assume_aligned(p, MRG_VEC * sizeof(T)), v, sizeof(v));
	} else {
		for(int u = 0; u < cnt; ++u) p[u] = v[u];
	}
}

template <int ET, bool W>
__global__ __launch_bounds__(MRG_BLOCK) void k_merge_gather(typename Elem<ET>::T *__restrict__ D,
                                                           typename Elem<ET>::T *__restrict__ N, int64_t cells,
                                                           MrgBatch b) {
	typedef typename Elem<ET>::T T;
	__shared__ unsigned s_mask;
	const int64_t bbase = (int64_t) blockIdx.x * (MRG_BLOCK * MRG_VEC);   // < cells: the grid is cdiv(cells, ...)
	const int64_t bend = bbase + MRG_BLOCK * MRG_VEC < cells ? bbase + MRG_BLOCK * MRG_VEC : cells;
	const int64_t rlo = ltd_row(bbase), rhi = ltd_row(bend - 1);   // 1 <= rlo <= rhi < n
	if(threadIdx.x == 0) s_mask = 0;
	__syncthreads();
	for(int64_t r = rlo + threadIdx.x; r <= rhi; r += MRG_BLOCK) {
		unsigned mk = 0;
		for(int s = 0; s < b.nsrc; ++s) mk |= (unsigned) (b.inv[(size_t) s * b.n + r] >= 0) << s;
		if(mk) atomicOr(&s_mask, mk);
	}
	__syncthreads();
	unsigned mask = s_mask;
	const int64_t base = bbase + (int64_t) threadIdx.x * MRG_VEC;
	if(!mask || base >= cells) return;
	const int cnt = cells - base < MRG_VEC ? (int) (cells - base) : MRG_VEC;
	T Dv[MRG_VEC], Nv[MRG_VEC];
	mrg_load(Dv, D + base, cnt);
	mrg_load(Nv, N + base, cnt);
	int ri[MRG_VEC], cj[MRG_VEC];   // the union row and column of each cell
	{
		int64_t i = ltd_row(base), j = base - tri(i);
#pragma unroll
		for(int u = 0; u < MRG_VEC; ++u) {
			ri[u] = (int) i;
			cj[u] = (int) j;
			if(++j == i) {
				++i;
				j = 0;
			}
		}
	}
	while(mask) {
		const int s = __ffs(mask) - 1;
		mask &= mask - 1;
		const int *__restrict__ inv = b.inv + (size_t) s * b.n;
		const T *__restrict__ d = (const T *) b.d[s];
		const T *__restrict__ w = (const T *) b.w[s];
		const bool init = b.first && s == 0;
#pragma unroll
		for(int u = 0; u < MRG_VEC; ++u) {
			if(u < cnt) {   // rows of cells past the end may reach n: not looked up
				const int a = inv[ri[u]], c = inv[cj[u]];
				if(a >= 0 && c >= 0) {
					const int64_t f = a > c ? tri(a) + c : tri(c) + a;
					mrg_step<T, W>(Dv[u], Nv[u], d[f], W ? w[f] : (T) 1, init);
				}
			}
		}
	}
	mrg_store(D + base, Dv, cnt);
	mrg_store(N + base, Nv, cnt);
}

template <int ET, bool W>
__global__ __launch_bounds__(MRG_BLOCK) void k_merge_scatter(typename Elem<ET>::T *__restrict__ D,
                                                            typename Elem<ET>::T *__restrict__ N,
                                                            const typename Elem<ET>::T *__restrict__ d,
                                                            const typename Elem<ET>::T *__restrict__ w,
                                                            const int *__restrict__ idx, int64_t scells, int init) {
	typedef typename Elem<ET>::T T;
	const int64_t base = ((int64_t) blockIdx.x * MRG_BLOCK + threadIdx.x) * MRG_VEC;
	if(base >= scells) return;
	const int cnt = scells - base < MRG_VEC ? (int) (scells - base) : MRG_VEC;
	T dv[MRG_VEC], wv[MRG_VEC];
	mrg_load(dv, d + base, cnt);
	if(W) mrg_load(wv, w + base, cnt);
	int64_t i = ltd_row(base), j = base - tri(i);
	int ui = idx[i];
#pragma unroll
	for(int u = 0; u < MRG_VEC; ++u) {
		if(u < cnt) {
			const int uj = idx[j];
			const int64_t f = ui > uj ? tri(ui) + uj : tri(uj) + ui;
			T Dc = D[f], Nc = N[f];
			mrg_step<T, W>(Dc, Nc, dv[u], W ? wv[u] : (T) 1, init != 0);
			D[f] = Dc;
			N[f] = Nc;
			if(++j == i) {
				++i;
				j = 0;
				if(u + 1 < cnt) ui = idx[i];   // i < m while a cell follows
			}
		}
	}
}

template <int ET>
__global__ __launch_bounds__(MRG_BLOCK) void k_merge_close(typename Elem<ET>::T *__restrict__ D,
                                                          const typename Elem<ET>::T *__restrict__ N, int64_t cells) {
	typedef typename Elem<ET>::T T;
	const int64_t base = ((int64_t) blockIdx.x * MRG_BLOCK + threadIdx.x) * MRG_VEC;
	if(base >= cells) return;
	const int cnt = cells - base < MRG_VEC ? (int) (cells - base) : MRG_VEC;
	T Dv[MRG_VEC], Nv[MRG_VEC];
	mrg_load(Dv, D + base, cnt);
	mrg_load(Nv, N + base, cnt);
#pragma unroll
	for(int u = 0; u < MRG_VEC; ++u) Dv[u] = Nv[u] != 0 ? Dv[u] / Nv[u] : (T) -1;   // IEEE division in T
	mrg_store(D + base, Dv, cnt);
}

static inline unsigned mrg_grid(int64_t cells) {
	return (unsigned) ((cells + (int64_t) MRG_BLOCK * MRG_VEC - 1) / ((int64_t) MRG_BLOCK * MRG_VEC));
}

static int mrg_etype(int etype, const char *who) {
	if(etype == 2 || etype == 1) {
		char msg[160];
		snprintf(msg, sizeof(msg), "%s: short / byte elements are not implemented", who);
		ccg_set_last_msg(msg);
		return CCG_EUNSUP;
	}
	return etype == 8 || etype == 4 ? CCG_OK : CCG_EINVAL;
}

static int mrg_fail(const char *fmt, int a, int b, int c) {
	char msg[200];
	snprintf(msg, sizeof(msg), fmt, a, b, c);
	ccg_set_last_msg(msg);
	return CCG_EINVAL;
}

// everything the kernels index with: after this, every table entry is a row of
// its source or -1, and every union row a kernel forms lies in [0, n)
static int mrg_check(const ccg_merge_args *a, int n) {
	CCG_TRY(mrg_etype(a->etype, "ccg_ltd_merge"));
	if(a->nsrc < 1 || a->nsrc > MRG_MAX_SRC) return mrg_fail("ccg_ltd_merge: nsrc %d outside 1 .. %d", a->nsrc, MRG_MAX_SRC, 0);
	if(n < 0 || a->n_prev < 0 || a->n_prev > n) return mrg_fail("ccg_ltd_merge: n_prev %d outside 0 .. n = %d", a->n_prev, n, 0);
	if(a->plan != 0 && a->plan != CCG_MERGE_SCATTER && a->plan != CCG_MERGE_GATHER)
		return mrg_fail("ccg_ltd_merge: unknown plan %d", a->plan, 0, 0);
	int *seen = (int *) malloc(((size_t) n + 1) * sizeof(int));
	if(!seen) return CCG_ENOMEM;
	memset(seen, 0xFF, ((size_t) n + 1) * sizeof(int));
	int rc = CCG_OK;
	for(int s = 0; s < a->nsrc && rc == CCG_OK; ++s) {
		const ccg_merge_src *S = &a->src[s];
		if(S->m < 1 || !S->idx) rc = mrg_fail("ccg_ltd_merge: source %d has %d rows or no indices", s, S->m, 0);
		else if(S->m > 1 && (!S->d || (a->weighted && !S->w))) rc = mrg_fail("ccg_ltd_merge: source %d lacks a matrix", s, 0, 0);
		for(int i = 0; i < S->m && rc == CCG_OK; ++i) {
			const int u = S->idx[i];
			if(u < 0 || u >= n) rc = mrg_fail("ccg_ltd_merge: source %d row %d: index %d outside the union", s, i, u);
			else if(seen[u] == s) rc = mrg_fail("ccg_ltd_merge: source %d row %d: index %d repeated", s, i, u);
			else seen[u] = s;
		}
	}
	free(seen);
	return rc;
}

static inline bool mrg_misaligned(const void *p) { return ((uintptr_t) p & (uintptr_t) 31) != 0; }

extern "C" int ccg_ltd_merge_dev(ccg_ctx *c, const ccg_merge_args *a, void *D, void *N, int n) {
	if(!c || !a || !D || !N) return CCG_EINVAL;
	CCG_TRY(mrg_check(a, n));
	bool bad = mrg_misaligned(D) || mrg_misaligned(N);
	int64_t scells = 0, stab = 0;
	for(int s = 0; s < a->nsrc; ++s) {
		if(a->src[s].m < 2) continue;
		bad = bad || mrg_misaligned(a->src[s].d) || (a->weighted && mrg_misaligned(a->src[s].w));
		scells += tri(a->src[s].m);
		stab += a->src[s].m;
	}
	if(bad) {
		ccg_set_last_msg("ccg_ltd_merge_dev: the LT buffers must be aligned to 32 bytes");   // the kernels move whole vectors
		return CCG_EINVAL;
	}
	const int et = a->etype;
	const int64_t cells = tri(n), cells_prev = tri(a->n_prev);
	int plan = a->plan;
	if(!plan) plan = (double) scells >= MRG_CROSSOVER * (double) cells ? CCG_MERGE_GATHER : CCG_MERGE_SCATTER;
	if(!scells) plan = 0;
	CCG_CHECK(hipSetDevice(c->device));
	CCG_DEVICE_SYNC(c);
	// the tables: inverse per source (gather) or the sources' index vectors back to back (scatter)
	const size_t tab = plan == CCG_MERGE_GATHER ? (size_t) a->nsrc * (size_t) n : (size_t) stab;
	int *htab = NULL, *dtab = NULL;
	if(plan) {
		void *ws = NULL;
		CCG_TRY(ccg_ctx_workspace(c, CCG_WS_MERGE, (tab ? tab : 1) * sizeof(int), &ws));
		dtab = (int *) ws;
		htab = (int *) malloc((tab ? tab : 1) * sizeof(int));
		if(!htab) return CCG_ENOMEM;
		if(plan == CCG_MERGE_GATHER) {
			memset(htab, 0xFF, tab * sizeof(int));
			for(int s = 0; s < a->nsrc; ++s) {
				if(a->src[s].m < 2) continue;   // no cell: the table stays empty and every block passes it by
				for(int i = 0; i < a->src[s].m; ++i) htab[(size_t) s * n + a->src[s].idx[i]] = i;
			}
		} else {
			size_t o = 0;
			for(int s = 0; s < a->nsrc; ++s) {
				if(a->src[s].m < 2) continue;
				memcpy(htab + o, a->src[s].idx, (size_t) a->src[s].m * sizeof(int));
				o += a->src[s].m;
			}
		}
	}
	struct HostFree {
		void *p;
		~HostFree() { free(p); }
	} hf = {htab};
	StreamSync idle(c->stream);   // htab is read by the copy until the stream has passed it
	if(plan) CCG_CHECK(hipMemcpyAsync(dtab, htab, tab * sizeof(int), hipMemcpyHostToDevice, c->stream));
	CCG_CHECK(hipEventRecord(c->ev0, c->stream));
	if(cells > cells_prev) {
		CCG_CHECK(hipMemsetAsync((char *) D + (size_t) cells_prev * et, 0, (size_t) (cells - cells_prev) * et, c->stream));
		CCG_CHECK(hipMemsetAsync((char *) N + (size_t) cells_prev * et, 0, (size_t) (cells - cells_prev) * et, c->stream));
	}
	if(plan == CCG_MERGE_GATHER) {
		MrgBatch b;
		memset(&b, 0, sizeof(b));
		for(int s = 0; s < a->nsrc; ++s) {
			b.d[s] = a->src[s].d;
			b.w[s] = a->src[s].w;
		}
		b.inv = dtab;
		b.nsrc = a->nsrc;
		b.n = n;
		b.first = a->first;
		with_etype(et, [&](auto e) {
			constexpr int ET = decltype(e)::value;
			typedef typename Elem<ET>::T T;
			if constexpr(ET == 8 || ET == 4) {
				if(a->weighted) k_merge_gather<ET, true><<<mrg_grid(cells), MRG_BLOCK, 0, c->stream>>>((T *) D, (T *) N, cells, b);
				else k_merge_gather<ET, false><<<mrg_grid(cells), MRG_BLOCK, 0, c->stream>>>((T *) D, (T *) N, cells, b);
			}
		});
		CCG_CHECK(hipGetLastError());
	} else if(plan == CCG_MERGE_SCATTER) {
		size_t o = 0;
		for(int s = 0; s < a->nsrc; ++s) {
			const ccg_merge_src *S = &a->src[s];
			if(S->m < 2) continue;
			const int64_t sc = tri(S->m);
			const int init = a->first && s == 0;
			with_etype(et, [&](auto e) {
				constexpr int ET = decltype(e)::value;
				typedef typename Elem<ET>::T T;
				if constexpr(ET == 8 || ET == 4) {
					if(a->weighted)
						k_merge_scatter<ET, true><<<mrg_grid(sc), MRG_BLOCK, 0, c->stream>>>((T *) D, (T *) N, (const T *) S->d, (const T *) S->w, dtab + o, sc, init);
					else
						k_merge_scatter<ET, false><<<mrg_grid(sc), MRG_BLOCK, 0, c->stream>>>((T *) D, (T *) N, (const T *) S->d, NULL, dtab + o, sc, init);
				}
			});
			CCG_CHECK(hipGetLastError());
			o += S->m;
		}
	}
	CCG_CHECK(hipEventRecord(c->ev1, c->stream));
	CCG_CHECK(hipStreamSynchronize(c->stream));
	CCG_CHECK(hipEventElapsedTime(&c->merge_ms, c->ev0, c->ev1));
	c->merge_plan = plan;
	return CCG_OK;
}

extern "C" int ccg_ltd_merge(ccg_ctx *c, const ccg_merge_args *a, void *D, void *N, int n) {
	if(!c || !a || !D || !N) return CCG_EINVAL;
	CCG_TRY(mrg_check(a, n));
	CCG_CHECK(hipSetDevice(c->device));
	const size_t et = (size_t) a->etype, bytes = (size_t) tri(n) * et, prev = (size_t) tri(a->n_prev) * et;
	DevMem dD, dN, ds[MRG_MAX_SRC], dw[MRG_MAX_SRC];
	CCG_TRY(dD.alloc(bytes));
	CCG_TRY(dN.alloc(bytes));
	ccg_merge_args b = *a;
	StreamSync idle(c->stream);
	CCG_CHECK(hipMemcpyAsync(dD.p, D, prev, hipMemcpyHostToDevice, c->stream));
	CCG_CHECK(hipMemcpyAsync(dN.p, N, prev, hipMemcpyHostToDevice, c->stream));
	for(int s = 0; s < a->nsrc; ++s) {
		const size_t sb = (size_t) tri(a->src[s].m) * et;
		if(!sb) continue;
		CCG_TRY(ds[s].alloc(sb));
		CCG_CHECK(hipMemcpyAsync(ds[s].p, a->src[s].d, sb, hipMemcpyHostToDevice, c->stream));
		b.src[s].d = ds[s].p;
		if(a->weighted) {
			CCG_TRY(dw[s].alloc(sb));
			CCG_CHECK(hipMemcpyAsync(dw[s].p, a->src[s].w, sb, hipMemcpyHostToDevice, c->stream));
			b.src[s].w = dw[s].p;
		}
	}
	CCG_TRY(ccg_ltd_merge_dev(c, &b, dD.p, dN.p, n));
	CCG_CHECK(hipMemcpyAsync(D, dD.p, bytes, hipMemcpyDeviceToHost, c->stream));
	CCG_CHECK(hipMemcpyAsync(N, dN.p, bytes, hipMemcpyDeviceToHost, c->stream));
	CCG_CHECK(hipStreamSynchronize(c->stream));
	return CCG_OK;
}

extern "C" int ccg_ltd_merge_close_dev(ccg_ctx *c, void *D, const void *N, int n, int etype) {
	if(!c || !D || !N || n < 0) return CCG_EINVAL;
	CCG_TRY(mrg_etype(etype, "ccg_ltd_merge_close"));
	if(mrg_misaligned(D) || mrg_misaligned(N)) {
		ccg_set_last_msg("ccg_ltd_merge_close_dev: the LT buffers must be aligned to 32 bytes");
		return CCG_EINVAL;
	}
	CCG_CHECK(hipSetDevice(c->device));
	CCG_DEVICE_SYNC(c);
	const int64_t cells = tri(n);
	CCG_CHECK(hipEventRecord(c->ev0, c->stream));
	if(cells) {
		if(etype == 8) k_merge_close<8><<<mrg_grid(cells), MRG_BLOCK, 0, c->stream>>>((double *) D, (const double *) N, cells);
		else k_merge_close<4><<<mrg_grid(cells), MRG_BLOCK, 0, c->stream>>>((float *) D, (const float *) N, cells);
		CCG_CHECK(hipGetLastError());
	}
	CCG_CHECK(hipEventRecord(c->ev1, c->stream));
	CCG_CHECK(hipStreamSynchronize(c->stream));
	CCG_CHECK(hipEventElapsedTime(&c->merge_ms, c->ev0, c->ev1));
	return CCG_OK;
}

extern "C" int ccg_ltd_merge_close(ccg_ctx *c, void *D, const void *N, int n, int etype) {
	if(!c || !D || !N || n < 0) return CCG_EINVAL;
	CCG_TRY(mrg_etype(etype, "ccg_ltd_merge_close"));
	CCG_CHECK(hipSetDevice(c->device));
	const size_t bytes = (size_t) tri(n) * (size_t) etype;
	DevMem dD, dN;
	CCG_TRY(dD.alloc(bytes));
	CCG_TRY(dN.alloc(bytes));
	StreamSync idle(c->stream);
	CCG_CHECK(hipMemcpyAsync(dD.p, D, bytes, hipMemcpyHostToDevice, c->stream));
	CCG_CHECK(hipMemcpyAsync(dN.p, N, bytes, hipMemcpyHostToDevice, c->stream));
	CCG_TRY(ccg_ltd_merge_close_dev(c, dD.p, dN.p, n, etype));
	CCG_CHECK(hipMemcpyAsync(D, dD.p, bytes, hipMemcpyDeviceToHost, c->stream));
	CCG_CHECK(hipStreamSynchronize(c->stream));
	return CCG_OK;
}

extern "C" int ccg_last_merge_ms(ccg_ctx *c, double *ms) {
	if(!c || !ms) return CCG_EINVAL;
	*ms = c->merge_ms;
	return CCG_OK;
}

extern "C" int ccg_last_merge_plan(ccg_ctx *c, int *plan) {
	if(!c || !plan) return CCG_EINVAL;
	*plan = c->merge_plan;
	return CCG_OK;
}
