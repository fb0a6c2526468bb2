// meth.hip -- `dist -y`: methylation motif sites cleared from the include masks
// (maskMotifs meth.c:141, called cdist.c:254 / :272 / :302).
//
// A motif strand of length m <= 32 matches at start p (0 <= p <= len - m) when
// the packed 2-bit code at p + k lies in the 4-bit set allow[k] for every k; a
// match clears the include bits of the positions p + k that are methylation
// sites.  A lane owns one 32-position include word w of one taxon:
//   - it loads alignment words w - 1, w, w + 1 (0 outside the row's data words)
//     and forms the four one-hot base planes over those 96 positions;
//   - per strand, the AND over k of the allowed-set planes shifted by k is the
//     mask of the 64 starts 32w - 32 .. 32w + 31, cut to 0 <= p <= len - m, so
//     that neither the zero word in front of the row nor the zero padding behind
//     position len - 1 (both read as `A`) completes a match;
//   - the start mask shifted by each site offset k lands on the clear bits of w.
// Starts in 32w .. 32w + 31 are the ones word w counts as matches.
// Pair mode writes `incs[t][w] &= ~clear`; non-pair mode folds a slice of taxa
// in registers and issues one atomicAnd per word and slice into the one mask
// (bitwise, so the order of slices and launches does not matter).
#include <string.h>
#include "ccg_internal.h"

#define METH_BATCH 64   // strands per launch: the table travels as a kernel argument (2.5 KB)
#define METH_SLICE 64   // non-pair: taxa folded per atomicAnd

struct MethTable {
	int n;
	ccg_motif m[METH_BATCH];
};

// bits 0, 2, 4 .. 62 of x packed into 32 bits
__device__ __forceinline__ uint32_t meth_even(uint64_t x) {
	x &= 0x5555555555555555ull;
	x = (x | (x >> 1)) & 0x3333333333333333ull;
	x = (x | (x >> 2)) & 0x0F0F0F0F0F0F0F0Full;
	x = (x | (x >> 4)) & 0x00FF00FF00FF00FFull;
	x = (x | (x >> 8)) & 0x0000FFFF0000FFFFull;
	x = (x | (x >> 16)) & 0x00000000FFFFFFFFull;
	return (uint32_t) x;
}

// Wd = data words of a row ((len + 31) / 32 <= stride): nothing past them is read
template <int PAIR>
__global__ __launch_bounds__(256) void k_meth(const uint64_t *__restrict__ seqs, uint32_t *incs, int n, int len,
                                              int stride, int Wd, const MethTable tab, unsigned long long *matches) {
	const int TS = PAIR ? 1 : METH_SLICE;
	// grid-stride over (taxon slice, group of 256 words): n * Wd exceeds 2^32 at config sizes
	const long long groups = (Wd + 255) / 256, slices = ((long long) n + TS - 1) / TS, units = groups * slices;
	unsigned long long cnt = 0;
	for(long long u = blockIdx.x; u < units; u += gridDim.x) {
		const long long sl = u / groups;
		const int w = (int) (u % groups) * 256 + (int) threadIdx.x;
		if(w >= Wd) continue;
		const int t0 = (int) (sl * TS), t1 = (long long) t0 + TS < n ? t0 + TS : n;
		uint32_t clear = 0;
		for(int t = t0; t < t1; ++t) {
			const uint64_t *row = seqs + (size_t) t * stride;
			const uint64_t xp = w > 0 ? row[w - 1] : 0, xc = row[w], xn = w + 1 < Wd ? row[w + 1] : 0;
			// one-hot planes, position 32 (w - 1) + i at bit 63 - i of [0] (i < 64) and 32 (w + 1) + i at bit 31 - i of [1]
			const uint64_t hi = ((uint64_t) meth_even(xp >> 1) << 32) | meth_even(xc >> 1);
			const uint64_t lo = ((uint64_t) meth_even(xp) << 32) | meth_even(xc);
			const uint32_t hn = meth_even(xn >> 1), ln = meth_even(xn);
			const uint64_t B64[4] = {~hi & ~lo, ~hi & lo, hi & ~lo, hi & lo};
			const uint32_t B32[4] = {~hn & ~ln, ~hn & ln, hn & ~ln, hn & ln};
			for(int j = 0; j < tab.n; ++j) {
				const int m = tab.m[j].len;
				// start s stands for p = 32w - 32 + s; 0 <= p <= len - m
				const int smin = w == 0 ? 32 : 0;
				const long long smaxl = (long long) len - m - 32ll * w + 32;
				if(smaxl < smin) continue;
				const int smax = smaxl > 63 ? 63 : (int) smaxl;
				uint64_t S = (~0ull >> smin) & (~0ull << (63 - smax));
				for(int k = 0; k < m; ++k) {
					const unsigned a = tab.m[j].allow[k];
					if(a == 15) continue;
					uint64_t h = 0;
					uint32_t x = 0;
#pragma unroll
					for(int b = 0; b < 4; ++b) {
						if(a & (1u << b)) {
							h |= B64[b];
							x |= B32[b];
						}
					}
					S &= k ? (h << k) | (((uint64_t) x << 32) >> (64 - k)) : h;
				}
				cnt += __popc((uint32_t) S);
				for(uint32_t mm = tab.m[j].meth; mm;) {
					const int k = __clz(mm);
					mm &= ~(0x80000000u >> k);
					clear |= (uint32_t) (S >> k);
				}
			}
		}
		if(clear) {
			if(PAIR) incs[(size_t) t0 * stride + w] &= ~clear;
			else atomicAnd(incs + w, ~clear);
		}
	}
	if(matches) {
		for(int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
		if((threadIdx.x & 63) == 0 && cnt) atomicAdd(matches, cnt);
	}
}

// getNpos of `rows` masks of Wd words, one block per mask at a time
__global__ __launch_bounds__(256) void k_meth_npos(const uint32_t *__restrict__ incs, int rows, int stride, int Wd,
                                                   int32_t *out) {
	__shared__ int ws[4];
	for(int t = blockIdx.x; t < rows; t += gridDim.x) {
		const uint32_t *m = incs + (size_t) t * stride;
		int s = 0;
		for(int w = threadIdx.x; w < Wd; w += blockDim.x) s += __popc(m[w]);
		for(int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
		__syncthreads();
		if((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = s;
		__syncthreads();
		if(threadIdx.x == 0) out[t] = ws[0] + ws[1] + ws[2] + ws[3];
	}
}

static int meth_check(const ccg_meth_args *a) {
	if(!a || a->n < 0 || a->nmotifs < 0) return CCG_EINVAL;
	if(a->n == 0 || a->nmotifs == 0) return CCG_OK;
	if(a->len <= 0 || a->stride < (a->len + 31) / 32 || !a->seqs || !a->incs || !a->motifs) return CCG_EINVAL;
	for(int j = 0; j < a->nmotifs; ++j) {
		const ccg_motif *m = a->motifs + j;
		if(m->len < 2 || m->len > 32) return CCG_EINVAL;
		for(int k = 0; k < m->len; ++k)
			if(m->allow[k] == 0 || m->allow[k] > 15) return CCG_EINVAL;
		if(m->len < 32 && (m->meth & (0xFFFFFFFFu >> m->len))) return CCG_EINVAL;
	}
	return CCG_OK;
}

// every strand over rows [0, rows) of device buffers, METH_BATCH strands a launch
static int meth_launch(ccg_ctx *c, const ccg_meth_args *a, const uint64_t *seqs, uint32_t *incs, int rows,
                       unsigned long long *matches) {
	const int Wd = (a->len + 31) / 32, TS = a->pair ? 1 : METH_SLICE;
	const long long units = (long long) ((Wd + 255) / 256) * (((long long) rows + TS - 1) / TS);
	const unsigned grid = (unsigned) (units < 262144 ? units : 262144);
	for(int j0 = 0; j0 < a->nmotifs; j0 += METH_BATCH) {
		MethTable tab;
		memset(&tab, 0, sizeof(tab));
		tab.n = a->nmotifs - j0 < METH_BATCH ? a->nmotifs - j0 : METH_BATCH;
		memcpy(tab.m, a->motifs + j0, (size_t) tab.n * sizeof(ccg_motif));
		if(a->pair) k_meth<1><<<grid, 256, 0, c->stream>>>(seqs, incs, rows, a->len, a->stride, Wd, tab, matches);
		else k_meth<0><<<grid, 256, 0, c->stream>>>(seqs, incs, rows, a->len, a->stride, Wd, tab, matches);
		CCG_CHECK(hipGetLastError());
	}
	return CCG_OK;
}

// the context's CCG_WS_METH slot: n getNpos counts, then the match counter
static int meth_counters(ccg_ctx *c, int n, int32_t **cnt, unsigned long long **mt) {
	void *p = NULL;
	const size_t cb = ((size_t) n * 4 + 7) & ~(size_t) 7;
	const int rc = ccg_ctx_workspace(c, CCG_WS_METH, cb + 8, &p);
	if(rc) return rc;
	*cnt = (int32_t *) p;
	*mt = (unsigned long long *) ((char *) p + cb);
	CCG_CHECK(hipMemsetAsync(*mt, 0, 8, c->stream));
	return CCG_OK;
}

static int meth_results(ccg_ctx *c, const ccg_meth_args *a, const int32_t *cnt, const unsigned long long *mt,
                        int32_t *inc_count, int64_t *matches) {
	if(inc_count) {
		const int rows = a->pair ? a->n : 1;
		CCG_CHECK(hipMemcpyAsync(inc_count, cnt, (size_t) rows * 4, hipMemcpyDeviceToHost, c->stream));
	}
	unsigned long long m = 0;
	if(matches) CCG_CHECK(hipMemcpyAsync(&m, mt, 8, hipMemcpyDeviceToHost, c->stream));
	if(inc_count || matches) CCG_CHECK(hipStreamSynchronize(c->stream));
	if(matches) *matches = (int64_t) m;
	if(inc_count && !a->pair)   // the one global mask, in every slot
		for(int t = 1; t < a->n; ++t) inc_count[t] = inc_count[0];
	return CCG_OK;
}

extern "C" {

int ccg_meth_mask_dev(ccg_ctx *c, const ccg_meth_args *a, int32_t *inc_count, int64_t *matches) {
	if(!c) return CCG_EINVAL;
	int rc = meth_check(a);
	if(rc) return rc;
	if(matches) *matches = 0;
	if(a->n == 0 || a->nmotifs == 0) return CCG_OK;
	CCG_CHECK(hipSetDevice(c->device));
	CCG_DEVICE_SYNC(c);   // inputs may come from other streams
	int32_t *cnt = NULL;
	unsigned long long *mt = NULL;
	if((rc = meth_counters(c, a->n, &cnt, &mt))) return rc;
	if((rc = meth_launch(c, a, a->seqs, a->incs, a->n, matches ? mt : NULL))) return rc;
	if(inc_count) {
		const int rows = a->pair ? a->n : 1;
		k_meth_npos<<<rows < 65536 ? rows : 65536, 256, 0, c->stream>>>(a->incs, rows, a->stride, (a->len + 31) / 32, cnt);
		CCG_CHECK(hipGetLastError());
	}
	if((rc = meth_results(c, a, cnt, mt, inc_count, matches))) return rc;
	if(!inc_count && !matches && !(c->flags & CCG_CTX_NOSYNC)) CCG_CHECK(hipStreamSynchronize(c->stream));
	return CCG_OK;
}

int ccg_meth_mask(ccg_ctx *c, const ccg_meth_args *a, int32_t *inc_count, int64_t *matches) {
	if(!c) return CCG_EINVAL;
	int rc = meth_check(a);
	if(rc) return rc;
	if(matches) *matches = 0;
	if(a->n == 0 || a->nmotifs == 0) return CCG_OK;
	CCG_CHECK(hipSetDevice(c->device));
	const size_t ib = (size_t) a->stride * 4;
	const int Wd = (a->len + 31) / 32;
	int32_t *cnt = NULL;
	unsigned long long *mt = NULL;
	if((rc = meth_counters(c, a->n, &cnt, &mt))) return rc;
	DevMem maskm;   // non-pair: the one global mask, read back after the last chunk
	StreamSync idle(c->stream);
	if(!a->pair) {
		CCG_TRY(maskm.alloc(ib));
		CCG_CHECK(hipMemcpyAsync(maskm.p, a->incs, ib, hipMemcpyHostToDevice, c->stream));
	}
	uint32_t *mask = maskm.as<uint32_t>();
	// the rows stream through a bounded staging buffer, as ccg_snp_ltd's do
	// (the copy into the stage waits for the previous chunk's kernels and read-back)
	CCG_TRY(ccg_stage_rows(c->stream, a->seqs, a->incs, a->n, a->stride, a->pair != 0,
	                       [&](uint64_t *sseq, uint32_t *sinc, long long t0, long long rows) {
		CCG_TRY(meth_launch(c, a, sseq, a->pair ? sinc : mask, (int) rows, matches ? mt : NULL));
		if(!a->pair) return CCG_OK;
		if(inc_count)
			k_meth_npos<<<rows < 65536 ? (int) rows : 65536, 256, 0, c->stream>>>(sinc, (int) rows, a->stride, Wd, cnt + t0);
		CCG_CHECK(hipGetLastError());
		CCG_CHECK(hipMemcpyAsync(a->incs + (size_t) t0 * a->stride, sinc, (size_t) rows * ib, hipMemcpyDeviceToHost,
		                         c->stream));
		return CCG_OK;
	}));
	if(!a->pair) {
		if(inc_count) k_meth_npos<<<1, 256, 0, c->stream>>>(mask, 1, a->stride, Wd, cnt);
		CCG_CHECK(hipGetLastError());
		CCG_CHECK(hipMemcpyAsync(a->incs, mask, ib, hipMemcpyDeviceToHost, c->stream));
	}
	return meth_results(c, a, cnt, mt, inc_count, matches);
}

}   // extern "C"
