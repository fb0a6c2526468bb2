// nwck.hip -- the path-length LT of a Newick tree (`ccphylo nwck2phy`,
// nwck2phy.c:96-225) by replaying its split list in HBM.
//
// Split s (ccq_newick_splits) finds m = s + 1 rows and creates row m from row
// org.  For every k < m, with c = cell(org, k) read before this split writes:
//   new row      cell(m, k) = Lj                        for Lj < 0,
//                cell(m, org) = Lj + Li,
//                cell(m, k) = c < 0 ? -1 : Lj + c       otherwise;
//   originating  cell(org, k) = Li                      for Li < 0,
//   row / column cell(org, k) = c + Li                  for 0 <= c     (k != org).
// A cell is read as its element type, added in double and rounded once at the
// store (nwck2phy.c:117 / :181).  The reference also writes one cell past the
// end of the new row (:108, :120); the m cells of the row are written here.
//
// The cell of a pair is a chain of additions in split order along both root
// paths, O(depth) long, so a kernel per pair would be O(N^3) on the caterpillar
// trees NJ makes of line-like data.  The replay keeps the reference's O(N^2)
// and its bits: a split is one parallel step, thread k reads cell(org, k) and
// writes it and cell(m, k) -- no two threads of a step touch the same cell --
// and steps are ordered by __syncthreads() inside one block while m <=
// NW_PREFIX, by kernel boundaries after that.  The originating column (k > org)
// is a strided walk of the packed LT: one memory line per cell.
#include <string.h>
#include "ccg_internal.h"

// tests/test_gpu_fit.py names these sizes
#define NW_BLOCK 256      // threads per block of a step kernel
#define NW_PREFIX 1024    // the splits with m <= NW_PREFIX run in one block of NW_PREFIX threads

template <int ET>
__device__ __forceinline__ void nw_cell(typename Elem<ET>::T *__restrict__ D, int m, int org, double Li, double Lj,
                                        int k) {
	typedef typename Elem<ET>::T T;
	T *nr = D + tri(m) + k;
	if(k == org) {
		*nr = Lj < 0 ? (T) Lj : (T) (Lj + Li);
		return;
	}
	T *pc = k < org ? D + tri(org) + k : D + tri(k) + org;
	const double c = (double) *pc;
	*nr = Lj < 0 ? (T) Lj : c < 0 ? (T) -1.0 : (T) (Lj + c);
	if(Li < 0) {
		*pc = (T) Li;
	} else if(0 <= c) {
		*pc = (T) (c + Li);
	}
}

// splits [0, ns) in one block: m = s + 1 <= blockDim.x
template <int ET>
__global__ __launch_bounds__(NW_PREFIX) void k_nwck_prefix(typename Elem<ET>::T *__restrict__ D,
                                                          const ccg_split *__restrict__ sp, int ns) {
	const int k = threadIdx.x;
	for(int s = 0; s < ns; ++s) {
		const int m = s + 1;
		const ccg_split q = sp[s];
		if(k < m) nw_cell<ET>(D, m, q.org, q.Li, q.Lj, k);
		__syncthreads();   // the next split reads what this one wrote
	}
}

template <int ET>
__global__ __launch_bounds__(NW_BLOCK) void k_nwck_step(typename Elem<ET>::T *__restrict__ D, int m, int org, double Li,
                                                       double Lj) {
	const int k = blockIdx.x * NW_BLOCK + threadIdx.x;
	if(k < m) nw_cell<ET>(D, m, org, Li, Lj, k);
}

static int nwck_check(const ccg_split *sp, int ns, int etype) {
	if(etype == 2 || etype == 1) {
		ccg_set_last_msg("ccg_nwck_ltd: short / byte elements are not the path length in the reference (nwck2phy.c:245)");
		return CCG_EUNSUP;
	}
	if(!sp || ns < 0 || (etype != 8 && etype != 4)) return CCG_EINVAL;
	for(int s = 0; s < ns; ++s) {
		if(sp[s].org < 0 || sp[s].org > s) {   // row org must exist: every index a kernel forms stays below tri(ns + 1)
			ccg_set_last_msg("ccg_nwck_ltd: a split's originating row does not exist yet");
			return CCG_EINVAL;
		}
	}
	return CCG_OK;
}

extern "C" int ccg_nwck_ltd_dev(ccg_ctx *c, const ccg_split *sp, int ns, int etype, void *D) {
	if(!c) return CCG_EINVAL;
	CCG_TRY(nwck_check(sp, ns, etype));
	c->nwck_ms = 0;
	c->nwck_launches = 0;
	if(ns == 0) return CCG_OK;   // one leaf: no cell
	if(!D) return CCG_EINVAL;
	CCG_CHECK(hipSetDevice(c->device));
	CCG_DEVICE_SYNC(c);
	const int npre = ns < NW_PREFIX ? ns : NW_PREFIX;
	void *ws = NULL;
	CCG_TRY(ccg_ctx_workspace(c, CCG_WS_FIT, (size_t) NW_PREFIX * sizeof(ccg_split), &ws));
	CCG_CHECK(hipMemcpyAsync(ws, sp, (size_t) npre * sizeof(ccg_split), hipMemcpyHostToDevice, c->stream));
	CCG_CHECK(hipEventRecord(c->ev0, c->stream));
	long long launches = 1;
	with_etype(etype, [&](auto et) {
		constexpr int ET = decltype(et)::value;
		typedef typename Elem<ET>::T T;
		k_nwck_prefix<ET><<<1, NW_PREFIX, 0, c->stream>>>((T *) D, (const ccg_split *) ws, npre);
		for(int s = npre; s < ns; ++s, ++launches) {
			const int m = s + 1;
			k_nwck_step<ET><<<(unsigned) ((m + NW_BLOCK - 1) / NW_BLOCK), NW_BLOCK, 0, c->stream>>>(
				(T *) D, m, sp[s].org, sp[s].Li, sp[s].Lj);
		}
	});
	CCG_CHECK(hipGetLastError());
	CCG_CHECK(hipEventRecord(c->ev1, c->stream));
	CCG_CHECK(hipStreamSynchronize(c->stream));
	CCG_CHECK(hipEventElapsedTime(&c->nwck_ms, c->ev0, c->ev1));
	c->nwck_launches = launches;
	return CCG_OK;
}

extern "C" int ccg_nwck_ltd(ccg_ctx *c, const ccg_split *sp, int ns, int etype, void *D) {
	if(!c) return CCG_EINVAL;
	CCG_TRY(nwck_check(sp, ns, etype));
	if(ns == 0) return ccg_nwck_ltd_dev(c, sp, ns, etype, NULL);
	if(!D) return CCG_EINVAL;
	CCG_CHECK(hipSetDevice(c->device));
	const size_t bytes = (size_t) tri((int64_t) ns + 1) * (size_t) etype;
	DevMem d;
	CCG_TRY(d.alloc(bytes));
	StreamSync idle(c->stream);
	CCG_TRY(ccg_nwck_ltd_dev(c, sp, ns, etype, d.p));   // every cell is written: no memset
	CCG_CHECK(hipMemcpyAsync(D, d.p, bytes, hipMemcpyDeviceToHost, c->stream));
	CCG_CHECK(hipStreamSynchronize(c->stream));
	return CCG_OK;
}

extern "C" int ccg_last_nwck(ccg_ctx *c, double *ms, int64_t *launches) {
	if(!c || !ms || !launches) return CCG_EINVAL;
	*ms = c->nwck_ms;
	*launches = c->nwck_launches;
	return CCG_OK;
}
