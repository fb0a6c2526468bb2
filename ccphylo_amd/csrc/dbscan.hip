// dbscan.hip -- `ccphylo dbscan` (dbscan.c:31-163) on an HBM-resident packed LT.
//
// The reference walks the rows in order and gives row i the cluster of an
// earlier row.  Its result has a closed form (DESIGN.md "dbscan"): with
// nb(i,j) = d(i,j) <= maxDist, N[i] the neighbours of i in its row and column
// part, core(i) = minN <= N[i],
//   f(i) = the smallest j < i with nb(i,j)             for a core row,
//          the smallest j < i with nb(i,j) && core(j)  for a border row
//                                                       (0 < N[i] < minN),
//          i                                            where there is none,
//   C[i] = the root of i -> f(i) -> f(f(i)) -> ...
// so three kernels replace the serial walk:
//   k_dbscan_count   one pass over the LT: N (row part by wave, column part by
//                    an LDS histogram per block) and fany[i] = the smallest
//                    j < i with nb(i,j), which is f(i) of a core row;
//   k_dbscan_border  the border rows only (none at the default -N 1): a wave
//                    per row, 64 columns a step, up to the first core neighbour;
//   k_dbscan_jump    pointer jumping over f, then k_dbscan_roots counts C[i] == i.
// Every atomic is an integer add or min: the results do not depend on the
// order in which blocks run.  The LT is only read.
#include <string.h>
#include "ccg_internal.h"

// tile of k_dbscan_count: a block takes DB_TR rows x DB_TC columns of the LT
// (tests/test_gpu_dbscan.py names these sizes)
#define DB_TR 128
#define DB_TC 1024
#define DB_BLOCK 256
#define DB_NONE 0x7f7f7f7f   // fany's "no neighbour" (hipMemset of 0x7f bytes); above every row index

template <int ET>
__device__ __forceinline__ bool db_nb(typename Elem<ET>::T v, double bs, double maxDist) {
	return Elem<ET>::get(v, bs) <= maxDist;   // in double, as dbscan.c:66 (a missing cell, -1, passes when maxDist >= -1)
}

// grid (column tiles, row tiles); block (x, y) takes rows [y DB_TR, +DB_TR) x
// columns [x DB_TC, +DB_TC).  Row r holds its r cells at tri(r): the part of a
// row inside the tile is contiguous, but starts at any element, so each part
// is split into a head up to the next 16-byte boundary, 16-byte vectors, and
// a tail.  Wave w of the block takes the tile's rows w, w + 4, ...
template <int ET>
__global__ __launch_bounds__(DB_BLOCK) void k_dbscan_count(const typename Elem<ET>::T *__restrict__ D, int n, double bs,
                                                          double maxDist, int *__restrict__ N,
                                                          int *__restrict__ fany) {
	typedef typename Elem<ET>::T T;
	constexpr int VPE = 16 / ET;   // cells per 16-byte vector
	const int r0 = blockIdx.y * DB_TR, c0 = blockIdx.x * DB_TC;
	const int rend = r0 + DB_TR < n ? r0 + DB_TR : n;
	if(c0 >= rend - 1) return;   // the tile lies above the diagonal (uniform over the block)
	__shared__ int hist[DB_TC];
	for(int c = threadIdx.x; c < DB_TC; c += DB_BLOCK) hist[c] = 0;
	__syncthreads();
	const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
	for(int r = r0 + wid; r < rend; r += DB_BLOCK / 64) {
		const int len = (c0 + DB_TC < r ? c0 + DB_TC : r) - c0;   // cells of row r in the tile
		if(len <= 0) continue;
		const T *p = D + tri(r) + c0;
		int head = (int) ((16 - ((uintptr_t) p & 15)) & 15) / ET;
		if(head > len) head = len;
		const int nvec = (len - head) / VPE, tail = len - head - nvec * VPE;
		int cnt = 0, mn = DB_NONE;
		// head and tail cells, one per lane (head + tail < 2 VPE <= 32)
		if(lane < head + tail) {
			const int e = lane < head ? lane : head + nvec * VPE + (lane - head);
			if(db_nb<ET>(p[e], bs, maxDist)) {
				cnt = 1;
				mn = c0 + e;
				atomicAdd(&hist[e], 1);
			}
		}
		const uint4 *pv = (const uint4 *) (p + head);
		for(int v0 = lane; v0 < nvec; v0 += 4 * 64) {   // four loads in flight per lane before the first use
			uint4 q[4] = {};
#pragma unroll
			for(int u = 0; u < 4; ++u) {
				if(v0 + 64 * u < nvec) q[u] = pv[v0 + 64 * u];
			}
#pragma unroll
			for(int u = 0; u < 4; ++u) {
				const int v = v0 + 64 * u;
				if(v >= nvec) break;
				T e[VPE];
				memcpy(e, &q[u], 16);
				const int jb = head + v * VPE;
#pragma unroll
				for(int k = 0; k < VPE; ++k) {
					if(db_nb<ET>(e[k], bs, maxDist)) {
						++cnt;
						mn = mn < c0 + jb + k ? mn : c0 + jb + k;
						atomicAdd(&hist[jb + k], 1);
					}
				}
			}
		}
		cnt = __builtin_amdgcn_readlane(wave_incl_sum(cnt), 63);
		if(cnt) {   // uniform over the wave
			mn = __builtin_amdgcn_readlane(wave_incl_min_i(mn), 63);
			if(lane == 0) {
				atomicAdd(&N[r], cnt);      // a row spans ceil(r / DB_TC) blocks
				atomicMin(&fany[r], mn);
			}
		}
	}
	__syncthreads();
	for(int c = threadIdx.x; c < DB_TC; c += DB_BLOCK) {
		const int h = hist[c];
		if(h) atomicAdd(&N[c0 + c], h);   // hist[c] != 0 only for columns below a row of the tile: c0 + c < n
	}
}

// f of the rows that need no second look, and the list of border rows
__global__ void k_dbscan_classify(const int *__restrict__ N, const int *__restrict__ fany, int n, int minN,
                                  int *__restrict__ f, int *__restrict__ list, int *__restrict__ nlist) {
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if(i >= n) return;
	const int Ni = N[i];
	int fi = i;
	if(minN <= Ni) {
		if(fany[i] < i) fi = fany[i];
	} else if(Ni > 0) {
		list[atomicAdd(nlist, 1)] = i;   // the list's order is free: every entry is resolved on its own
	}
	f[i] = fi;
}

// a wave per border row: the first j < i with nb(i, j) and core(j)
template <int ET>
__global__ __launch_bounds__(DB_BLOCK) void k_dbscan_border(const typename Elem<ET>::T *__restrict__ D, double bs,
                                                           double maxDist, int minN, const int *__restrict__ N,
                                                           const int *__restrict__ list, int nlist,
                                                           int *__restrict__ f, unsigned long long *__restrict__ cells) {
	const int w = blockIdx.x * (DB_BLOCK / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
	if(w >= nlist) return;
	const int i = list[w];
	const typename Elem<ET>::T *row = D + tri(i);
	int j0 = 0;
	for(; j0 < i; j0 += 64) {
		const int j = j0 + lane;
		const bool hit = j < i && db_nb<ET>(row[j], bs, maxDist) && minN <= N[j];
		const unsigned long long b = __ballot(hit);
		if(b) {
			if(lane == 0) f[i] = j0 + __builtin_ctzll(b);
			j0 += 64;
			break;
		}
	}
	if(lane == 0) atomicAdd(cells, (unsigned long long) (j0 < i ? j0 : i));
}

__global__ void k_dbscan_jump(const int *__restrict__ in, int *__restrict__ out, int n, int *__restrict__ changed) {
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if(i >= n) return;
	const int a = in[i], b = in[a];
	out[i] = b;
	if(a != b) *changed = 1;
}

__global__ void k_dbscan_roots(const int *__restrict__ C, int n, int *__restrict__ nroots) {
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	const unsigned long long b = __ballot(i < n && C[i] == i);
	if((threadIdx.x & 63) == 0 && b) atomicAdd(nroots, __builtin_popcountll(b));
}

template <int ET>
static void launch_count(ccg_ctx *c, const void *D, int n, double bs, double maxDist, int *N, int *fany) {
	const dim3 grid((unsigned) ((n - 1 + DB_TC - 1) / DB_TC), (unsigned) ((n + DB_TR - 1) / DB_TR));
	k_dbscan_count<ET><<<grid, DB_BLOCK, 0, c->stream>>>((const typename Elem<ET>::T *) D, n, bs, maxDist, N, fany);
}

template <int ET>
static void launch_border(ccg_ctx *c, const void *D, double bs, double maxDist, int minN, const int *N,
                          const int *list, int nlist, int *f, unsigned long long *cells) {
	const unsigned grid = (unsigned) ((nlist + DB_BLOCK / 64 - 1) / (DB_BLOCK / 64));
	k_dbscan_border<ET><<<grid, DB_BLOCK, 0, c->stream>>>((const typename Elem<ET>::T *) D, bs, maxDist, minN, N, list,
	                                                     nlist, f, cells);
}

static int dbscan_args_ok(const ccg_dbscan_args *a) {
	if(a->n < 1) return 0;
	return ccg_etype_ok(a->etype) && ccg_etype_scale_ok(a->etype, a->byteScale);
}

// the count pass on zeroed N / DB_NONE fany
static int dbscan_count(ccg_ctx *c, const ccg_dbscan_args *a, const void *D, int *N, int *fany) {
	CCG_CHECK(hipMemsetAsync(N, 0, (size_t) a->n * sizeof(int), c->stream));
	CCG_CHECK(hipMemsetAsync(fany, 0x7f, (size_t) a->n * sizeof(int), c->stream));
	with_etype(a->etype, [&](auto et) {
		launch_count<decltype(et)::value>(c, D, a->n, a->byteScale, a->maxDist, N, fany);
	});
	CCG_CHECK(hipGetLastError());
	return CCG_OK;
}

extern "C" int ccg_dbscan_count_dev(ccg_ctx *c, const ccg_dbscan_args *a, const void *D, int32_t *N_dev,
                                    int32_t *fany_dev) {
	if(!c || !a || !D || !N_dev || !fany_dev || !dbscan_args_ok(a) || a->n < 2) return CCG_EINVAL;
	CCG_CHECK(hipSetDevice(c->device));
	CCG_DEVICE_SYNC(c);
	return dbscan_count(c, a, D, N_dev, fany_dev);
}

extern "C" int ccg_dbscan_dev(ccg_ctx *c, const ccg_dbscan_args *a, const void *D, int32_t *N, int32_t *C, int *nclust,
                              int64_t *stats) {
	if(!c || !a || !N || !C || !nclust || !dbscan_args_ok(a) || (a->n > 1 && !D)) return CCG_EINVAL;
	const int n = a->n;
	if(stats) memset(stats, 0, 4 * sizeof(int64_t));
	if(n == 1) {   // no cell: nothing to launch
		N[0] = 0;
		C[0] = 0;
		*nclust = 1;
		return CCG_OK;
	}
	CCG_CHECK(hipSetDevice(c->device));
	CCG_DEVICE_SYNC(c);   // D may come from another stream (e.g. torch's)
	// workspace: N, fany, f, f', border list (n ints each), then the counters
	void *ws = NULL;
	const size_t nn = ((size_t) n + 3) & ~(size_t) 3;
	int rc = ccg_ctx_workspace(c, CCG_WS_DBSCAN, (5 * nn + 8) * sizeof(int), &ws);
	if(rc) return rc;
	int *dN = (int *) ws, *dfany = dN + nn, *df0 = dfany + nn, *df1 = df0 + nn, *dlist = df1 + nn;
	int *dcnt = dlist + nn;   // [0] border rows, [1] changed, [2] roots, [4..5] the border pass's cells (u64)
	unsigned long long *dcells = (unsigned long long *) (dcnt + 4);
	int64_t launches = 0;
	CCG_CHECK(hipEventRecord(c->ev0, c->stream));
	CCG_CHECK(hipMemsetAsync(dcnt, 0, 8 * sizeof(int), c->stream));
	if((rc = dbscan_count(c, a, D, dN, dfany))) return rc;
	const unsigned g1 = (unsigned) ((n + 255) / 256);
	k_dbscan_classify<<<g1, 256, 0, c->stream>>>(dN, dfany, n, a->minN, df0, dlist, dcnt);
	CCG_CHECK(hipGetLastError());
	launches += 2;
	int nborder = 0;
	CCG_CHECK(hipMemcpyAsync(&nborder, dcnt, sizeof(int), hipMemcpyDeviceToHost, c->stream));
	CCG_CHECK(hipMemcpyAsync(N, dN, (size_t) n * sizeof(int), hipMemcpyDeviceToHost, c->stream));
	CCG_CHECK(hipStreamSynchronize(c->stream));
	if(nborder > 0) {   // never at minN <= 1: the LT is then read exactly once
		with_etype(a->etype, [&](auto et) {
			launch_border<decltype(et)::value>(c, D, a->byteScale, a->maxDist, a->minN, dN, dlist, nborder, df0, dcells);
		});
		CCG_CHECK(hipGetLastError());
		++launches;
	}
	// pointer jumping: a round halves the depth of every chain (n - 1 at most),
	// and one more round sees no change: ceil(log2 n) + 1 rounds at most
	int *cur = df0, *nxt = df1;
	for(int round = 0; round < 34; ++round) {
		int changed = 0;
		CCG_CHECK(hipMemsetAsync(dcnt + 1, 0, sizeof(int), c->stream));
		k_dbscan_jump<<<g1, 256, 0, c->stream>>>(cur, nxt, n, dcnt + 1);
		CCG_CHECK(hipGetLastError());
		++launches;
		CCG_CHECK(hipMemcpyAsync(&changed, dcnt + 1, sizeof(int), hipMemcpyDeviceToHost, c->stream));
		CCG_CHECK(hipStreamSynchronize(c->stream));
		int *t = cur;
		cur = nxt;
		nxt = t;
		if(!changed) break;
	}
	k_dbscan_roots<<<g1, 256, 0, c->stream>>>(cur, n, dcnt + 2);
	CCG_CHECK(hipGetLastError());
	++launches;
	CCG_CHECK(hipEventRecord(c->ev1, c->stream));
	unsigned long long bcells = 0;
	CCG_CHECK(hipMemcpyAsync(nclust, dcnt + 2, sizeof(int), hipMemcpyDeviceToHost, c->stream));
	CCG_CHECK(hipMemcpyAsync(&bcells, dcells, sizeof(bcells), hipMemcpyDeviceToHost, c->stream));
	CCG_CHECK(hipMemcpyAsync(C, cur, (size_t) n * sizeof(int), hipMemcpyDeviceToHost, c->stream));
	CCG_CHECK(hipStreamSynchronize(c->stream));
	if(stats) {
		float ms = 0;
		CCG_CHECK(hipEventElapsedTime(&ms, c->ev0, c->ev1));
		stats[0] = nborder;
		stats[1] = (int64_t) n * (n - 1) / 2 + (int64_t) bcells;
		stats[2] = launches;
		stats[3] = (int64_t) (ms * 1000.0f);
	}
	return CCG_OK;
}

extern "C" int ccg_dbscan(ccg_ctx *c, const ccg_dbscan_args *a, const void *D, int32_t *N, int32_t *C, int *nclust,
                          int64_t *stats) {
	if(!c || !a || !N || !C || !nclust || !dbscan_args_ok(a) || (a->n > 1 && !D)) return CCG_EINVAL;
	if(a->n == 1) return ccg_dbscan_dev(c, a, NULL, N, C, nclust, stats);
	CCG_CHECK(hipSetDevice(c->device));
	const size_t bytes = (size_t) a->n * (size_t) (a->n - 1) / 2 * (size_t) a->etype;
	DevMem d;
	CCG_TRY(d.alloc(bytes));
	StreamSync idle(c->stream);
	CCG_CHECK(hipMemcpyAsync(d.p, D, bytes, hipMemcpyHostToDevice, c->stream));
	return ccg_dbscan_dev(c, a, d.p, N, C, nclust, stats);
}
