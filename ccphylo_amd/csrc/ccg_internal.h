// ccg_internal.h -- shared device helpers of the gfx950 engine.
//
// Element types follow the reference LT container (matrix.c:59-71) and its
// ByteScale conversions (bytescale.h:22-23): dtouc(v, r) = v*BS + r stored
// through x86's 32-bit truncating conversion, uctod(u) = u / BS.
// Everything is compiled with -ffp-contract=off so that expressions like
// ((Ni + Nj - 4) >> 1) * d - sDi - sDj round exactly as the reference's.
#pragma once
#pragma clang diagnostic ignored "-Wunused-result"
#pragma clang diagnostic ignored "-Wunused-value"
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <float.h>
#include <type_traits>
#include "ccphylo_amd.h"

#define CCG_CHECK(expr)                                                        \
	do {                                                                       \
		hipError_t e_ = (expr);                                                \
		if(e_ != hipSuccess) {                                                 \
			ccg_set_last_error(e_, #expr, __FILE__, __LINE__);                 \
			return e_ == hipErrorOutOfMemory ? CCG_ENOMEM : CCG_EHIP;          \
		}                                                                      \
	} while(0)

// the same for a call that returns a CCG_* code
#define CCG_TRY(x)                        \
	do {                                  \
		const int rc_ = (x);              \
		if(rc_ != CCG_OK) return rc_;     \
	} while(0)

void ccg_set_last_error(hipError_t e, const char *what, const char *file, int line);
// free-form text for ccg_strerror(CCG_EHIP) (collective transports)
void ccg_set_last_msg(const char *msg);

// The slots of a context's workspace cache.  Every context keeps the tree's,
// dbscan's, the vec pre-pass's and the motif masking's slots from first use to
// ccg_destroy; the dist's slot is used by a CCG_CTX_NOSYNC context only (any
// other context allocates the dist's buffers per call and frees them with it).
enum ccg_ws_slot {
	CCG_WS_TREE,      // the tree drivers' run state (tree_layout, lk_run_t's buffers)
	CCG_WS_TREE_LB,   // DNJ's block lower bounds (optional: a run goes without)
	CCG_WS_DIST,      // the dist's bit planes, included count and word list (CCG_CTX_NOSYNC only)
	CCG_WS_DBSCAN,    // dbscan's per-row vectors and counters
	CCG_WS_VEC,       // the vec pre-pass's per-row values
	CCG_WS_METH,      // the motif masking's counters
	CCG_WS_FIT,       // the split prefix of the Newick replay; the LT comparison's perm, block partials and sums
	CCG_WS_MERGE,     // the merge's per-source index tables
	CCG_WS_COUNT
};

struct ccg_ctx {
	int device;
	hipStream_t stream;
	hipEvent_t ev0, ev1;
	char name[256];
	float dist_ms;   // the last dist call's pair kernels (HIP events on the engine stream)
	int dist_slices, dist_slice_words;   // its split-K plan (plan_split; 0, 0: no tile kernel ran)
	float vec_ms;    // the last vec call's pre-pass and pair kernel (the same events)
	int vec_pending; // ... still to be read from the events (a CCG_CTX_NOSYNC call)
	int vec_tile;    // its tile edge (0: nothing launched)
	float nwck_ms;   // the last Newick replay's kernels (the same events)
	long long nwck_launches;   // ... and how many there were
	float cmp_ms;    // the last LT comparison's two kernels
	float merge_ms;  // the last merge batch's (or close's) kernels
	int merge_plan;  // ... and the form the batch took (CCG_MERGE_SCATTER / _GATHER; 0: nothing ran)
	int flags;       // CCG_CTX_* (ccg_ctx_configure)
	int masked;      // the stream was created with a CU mask (ccg_ctx_configure)
	int ncu, cus;    // the device's CUs; the CUs the stream may use (0: all)
	// device workspaces kept across runs (ccg_ws_slot: grown on demand, freed
	// by ccg_destroy).  A run that uses one makes no hipFree, which waits for
	// every stream of the device.
	void *ws[CCG_WS_COUNT];
	size_t ws_bytes[CCG_WS_COUNT];
};
// slot k of the context's workspace cache, at least `bytes` long
int ccg_ctx_workspace(ccg_ctx *c, ccg_ws_slot k, size_t bytes, void **p);
// every device-pointer entry point first waits for the whole device (inputs
// may come from other streams) unless the caller orders them itself
#define CCG_DEVICE_SYNC(c) \
	do { \
		if(!((c)->flags & CCG_CTX_NOSYNC)) CCG_CHECK(hipDeviceSynchronize()); \
	} while(0)

// ---------------------------------------------------------------- host: owned memory
// Device memory in host code lives in a DevMem or in a context workspace slot
// (DESIGN.md 4).  A DevMem frees what it allocated when its scope ends, so a
// CCG_CHECK may return from anywhere below it; what it borrows (a slot's
// memory) it leaves alone.  p stays NULL when alloc fails.
struct DevMem {
	char *p = NULL;
	bool owned = false;
	DevMem() {}
	DevMem(const DevMem &) = delete;
	~DevMem() { release(); }
	// CCG_OK or CCG_ENOMEM (quietly: the sticky HIP error is cleared); 0 bytes allocate a few
	int alloc(size_t bytes) {
		release();
		if(hipMalloc((void **) &p, bytes ? bytes : 8) == hipSuccess) {
			owned = true;
			return CCG_OK;
		}
		(void) hipGetLastError();
		p = NULL;
		return CCG_ENOMEM;
	}
	void borrow(void *q) {
		release();
		p = (char *) q;
	}
	void release() {
		if(p && owned) hipFree(p);
		p = NULL;
		owned = false;
	}
	template <class T>
	T *as() const {
		return (T *) p;
	}
};
struct PinnedMem {
	unsigned char *p = NULL;
	PinnedMem() {}
	PinnedMem(const PinnedMem &) = delete;
	~PinnedMem() {
		if(p) hipHostFree(p);
	}
	bool alloc(size_t bytes) { return hipHostMalloc((void **) &p, bytes) == hipSuccess; }
};
// Waits for a stream when the scope ends.  Declared after the holders a
// function's launches use, it runs before they free: no launch of a call that
// returns early still reads the memory (on the success paths the stream is
// idle by then).
struct StreamSync {
	hipStream_t st;
	explicit StreamSync(hipStream_t s) : st(s) {}
	StreamSync(const StreamSync &) = delete;
	~StreamSync() { hipStreamSynchronize(st); }
};

// Packed host rows through a bounded device stage (the dist's planes and the
// motif masking read an MSA that may not fit beside their outputs): at most
// CCG_STAGE_BYTES of rows a chunk, at least one row; a row is its `stride`
// sequence words and, in pair mode, its `stride` include words, which lie
// behind the chunk's sequences.  Per chunk: the sequences are copied, the
// includes in pair mode, then body(sseq, sinc, t0, rows) runs (sinc NULL
// without pair) and returns a CCG_* code.  All of it is stream-ordered, so a
// chunk's copy waits for the previous chunk's kernels; the stage is freed
// once the stream is idle.
static const size_t CCG_STAGE_BYTES = (size_t) 256 << 20;
template <class F>
static inline int ccg_stage_rows(hipStream_t st, const uint64_t *seqs, const uint32_t *incs, long long n, int stride,
                                 bool pair, F &&body) {
	const size_t sb = (size_t) stride * 8, ib = (size_t) stride * 4, row_b = sb + (pair ? ib : 0);
	long long R = (long long) (CCG_STAGE_BYTES / row_b);
	if(R < 1) R = 1;
	if(R > n) R = n;
	DevMem stage;
	CCG_TRY(stage.alloc((size_t) R * row_b));
	StreamSync idle(st);
	uint64_t *sseq = stage.as<uint64_t>();
	uint32_t *sinc = pair ? (uint32_t *) (stage.p + (size_t) R * sb) : NULL;
	for(long long t0 = 0; t0 < n; t0 += R) {
		const long long rows = n - t0 < R ? n - t0 : R;
		CCG_CHECK(hipMemcpyAsync(sseq, seqs + (size_t) t0 * stride, (size_t) rows * sb, hipMemcpyHostToDevice, st));
		if(pair) CCG_CHECK(hipMemcpyAsync(sinc, incs + (size_t) t0 * stride, (size_t) rows * ib, hipMemcpyHostToDevice, st));
		CCG_TRY(body(sseq, sinc, t0, rows));
	}
	return CCG_OK;
}

// ---------------------------------------------------------------- element types
static inline bool ccg_etype_ok(int et) { return et == 8 || et == 4 || et == 2 || et == 1; }
// the integer types divide by the byte scale
static inline bool ccg_etype_scale_ok(int et, double byteScale) { return !(et == 2 || et == 1) || byteScale != 0; }
// the <ET> template argument from a checked runtime value: f(std::integral_constant<int, ET>())
template <class F>
static inline auto with_etype(int et, F &&f) {
	switch(et) {
		case 8: return f(std::integral_constant<int, 8>());
		case 4: return f(std::integral_constant<int, 4>());
		case 2: return f(std::integral_constant<int, 2>());
		default: return f(std::integral_constant<int, 1>());
	}
}

// ---------------------------------------------------------------- numerics
__device__ __forceinline__ int32_t cvt_i32_x86(double x) {
	// cvttsd2si: INT_MIN on overflow / NaN (the GPU instruction saturates)
	if(!(x > -2147483649.0 && x < 2147483648.0)) {
		return INT32_MIN;
	}
	return (int32_t) x;
}

template <int ET> struct Elem;
template <> struct Elem<8> {
	typedef double T;
	static __device__ __forceinline__ double get(T v, double) { return v; }
	static __device__ __forceinline__ T put(double v, double, double) { return v; }
};
template <> struct Elem<4> {
	typedef float T;
	static __device__ __forceinline__ double get(T v, double) { return (double) v; }
	static __device__ __forceinline__ T put(double v, double, double) { return (float) v; }
};
template <> struct Elem<2> {
	typedef uint16_t T;
	static __device__ __forceinline__ double get(T v, double bs) { return v / bs; }
	static __device__ __forceinline__ T put(double v, double r, double bs) {
		return (uint16_t) cvt_i32_x86(v * bs + r);
	}
};
template <> struct Elem<1> {
	typedef uint8_t T;
	static __device__ __forceinline__ double get(T v, double bs) { return v / bs; }
	static __device__ __forceinline__ T put(double v, double r, double bs) {
		return (uint8_t) cvt_i32_x86(v * bs + r);
	}
};

__host__ __device__ __forceinline__ int64_t tri(int64_t i) { return i * (i - 1) / 2; }
// the row of flat cell index idx of a packed LT: tri(i) <= idx < tri(i + 1)
__device__ __forceinline__ int64_t ltd_row(int64_t idx) {
	int64_t i = (int64_t) ((1.0 + sqrt(1.0 + 8.0 * (double) idx)) * 0.5);
	while(tri(i) > idx) --i;
	while(tri(i + 1) <= idx) ++i;
	return i;
}

// Q criterion exactly as nj.c:227 / dnj.c:103 write it
__device__ __forceinline__ double qcrit(int Ni, int Nj, double d, double sDi, double sDj) {
	double q = (double) ((Ni + Nj - 4) >> 1) * d;
	q = q - sDi;
	return q - sDj;
}

// ------------------------------------------------------------ reductions
// ------------------------------------------------------------ DPP wave ops
// Wave64 scans/reductions with DPP row shifts and row broadcasts (GFX9
// family): a few cycles per step instead of an LDS-crossbar ds_bpermute per
// __shfl.  Steps: row_shr 1,2,4,8 (inclusive within each 16-lane row), then
// row_bcast:15 into rows 1,3 and row_bcast:31 into rows 2,3; lanes without a
// source keep `old` (the identity).  Lane 63 ends with the whole wave.
#define DPP_ROW_SHR1 0x111
#define DPP_ROW_SHR2 0x112
#define DPP_ROW_SHR4 0x114
#define DPP_ROW_SHR8 0x118
#define DPP_WAVE_SHR1 0x138
#define DPP_ROW_BCAST15 0x142
#define DPP_ROW_BCAST31 0x143

template <int CTRL, int RM>
__device__ __forceinline__ int dpp_i(int old, int src) {
	return __builtin_amdgcn_update_dpp(old, src, CTRL, RM, 0xF, false);
}
template <int CTRL, int RM>
__device__ __forceinline__ double dpp_d(double old, double src) {
	const long long o = __double_as_longlong(old), v = __double_as_longlong(src);
	const int lo = __builtin_amdgcn_update_dpp((int) o, (int) v, CTRL, RM, 0xF, false);
	const int hi = __builtin_amdgcn_update_dpp((int) (o >> 32), (int) (v >> 32), CTRL, RM, 0xF, false);
	return __longlong_as_double(((long long) hi << 32) | (unsigned) lo);
}
template <int CTRL, int RM>
__device__ __forceinline__ long long dpp_l(long long old, long long src) {
	const int lo = __builtin_amdgcn_update_dpp((int) old, (int) src, CTRL, RM, 0xF, false);
	const int hi = __builtin_amdgcn_update_dpp((int) (old >> 32), (int) (src >> 32), CTRL, RM, 0xF, false);
	return ((long long) hi << 32) | (unsigned) lo;
}
__device__ __forceinline__ double readlane_d(double v, int lane) {
	const long long x = __double_as_longlong(v);
	const int lo = __builtin_amdgcn_readlane((int) x, lane), hi = __builtin_amdgcn_readlane((int) (x >> 32), lane);
	return __longlong_as_double(((long long) hi << 32) | (unsigned) lo);
}
__device__ __forceinline__ long long readlane_l(long long x, int lane) {
	const int lo = __builtin_amdgcn_readlane((int) x, lane), hi = __builtin_amdgcn_readlane((int) (x >> 32), lane);
	return ((long long) hi << 32) | (unsigned) lo;
}

#define CCG_DPP_STEPS(STEP)         \
	STEP(DPP_ROW_SHR1, 0xF)         \
	STEP(DPP_ROW_SHR2, 0xF)         \
	STEP(DPP_ROW_SHR4, 0xF)         \
	STEP(DPP_ROW_SHR8, 0xF)         \
	STEP(DPP_ROW_BCAST15, 0xA)      \
	STEP(DPP_ROW_BCAST31, 0xC)

// inclusive prefix sum over the wave
__device__ __forceinline__ int wave_incl_sum(int x) {
#define S_(C, R) x += dpp_i<C, R>(0, x);
	CCG_DPP_STEPS(S_)
#undef S_
	return x;
}
__device__ __forceinline__ long long wave_incl_sum_l(long long x) {
#define S_(C, R) x += dpp_l<C, R>(0, x);
	CCG_DPP_STEPS(S_)
#undef S_
	return x;
}
// inclusive prefix min over the wave
__device__ __forceinline__ double wave_incl_min(double x) {
#define S_(C, R)                               \
	{                                          \
		const double t_ = dpp_d<C, R>(DBL_MAX, x); \
		x = t_ < x ? t_ : x;                   \
	}
	CCG_DPP_STEPS(S_)
#undef S_
	return x;
}
__device__ __forceinline__ int wave_incl_min_i(int x) {
#define S_(C, R)                                 \
	{                                            \
		const int t_ = dpp_i<C, R>(INT32_MAX, x);  \
		x = t_ < x ? t_ : x;                     \
	}
	CCG_DPP_STEPS(S_)
#undef S_
	return x;
}
// exclusive prefix min: lane l gets min(carry, x[0..l-1])
__device__ __forceinline__ double wave_excl_min(double x, double carry) {
	const double inc = wave_incl_min(x);
	const double ex = dpp_d<DPP_WAVE_SHR1, 0xF>(DBL_MAX, inc);
	return ex < carry ? ex : carry;
}

// (q, idx) candidates: smaller q wins, equal q -> larger idx wins.  This is
// the closed form of the reference's sequential `q <= min` last-wins scans;
// being a total order, any association of the fold gives the same winner.
struct QArg {
	double q;
	int idx;
};

__device__ __forceinline__ bool qarg_better(double q, int idx, double bq, int bidx) {
	return q < bq || (q == bq && idx > bidx);
}

// wave-wide (q, idx) reduce; the result in every lane
__device__ __forceinline__ void qarg_wave_reduce(double &q, int &idx) {
#define S_(C, R)                                          \
	{                                                     \
		const double oq_ = dpp_d<C, R>(DBL_MAX, q);       \
		const int oi_ = dpp_i<C, R>(INT32_MIN, idx);      \
		if(qarg_better(oq_, oi_, q, idx)) {               \
			q = oq_;                                      \
			idx = oi_;                                    \
		}                                                 \
	}
	CCG_DPP_STEPS(S_)
#undef S_
	q = readlane_d(q, 63);
	idx = __builtin_amdgcn_readlane(idx, 63);
}

// the same, carrying a payload (cq, cp) of the winning element
__device__ __forceinline__ void qarg_wave_reduce_carry(double &q, int &idx, double &cq, int &cp) {
#define S_(C, R)                                          \
	{                                                     \
		const double oq_ = dpp_d<C, R>(DBL_MAX, q);       \
		const int oi_ = dpp_i<C, R>(INT32_MIN, idx);      \
		const double ocq_ = dpp_d<C, R>(DBL_MAX, cq);     \
		const int ocp_ = dpp_i<C, R>(0, cp);              \
		if(qarg_better(oq_, oi_, q, idx)) {               \
			q = oq_;                                      \
			idx = oi_;                                    \
			cq = ocq_;                                    \
			cp = ocp_;                                    \
		}                                                 \
	}
	CCG_DPP_STEPS(S_)
#undef S_
	q = readlane_d(q, 63);
	idx = __builtin_amdgcn_readlane(idx, 63);
	cq = readlane_d(cq, 63);
	cp = __builtin_amdgcn_readlane(cp, 63);
}

// four independent wave-wide (q, idx) reduces in lockstep (four dependency
// chains interleaved step by step), the second carrying a payload (cq, cp)
__device__ __forceinline__ void qarg_wave_reduce4(double (&q)[4], int (&idx)[4], double &cq, int &cp) {
#define S_(C, R)                                              \
	{                                                         \
		double oq_[4];                                        \
		int oi_[4];                                           \
		_Pragma("unroll") for(int t = 0; t < 4; ++t) {        \
			oq_[t] = dpp_d<C, R>(DBL_MAX, q[t]);              \
			oi_[t] = dpp_i<C, R>(INT32_MIN, idx[t]);          \
		}                                                     \
		const double ocq_ = dpp_d<C, R>(DBL_MAX, cq);         \
		const int ocp_ = dpp_i<C, R>(0, cp);                  \
		_Pragma("unroll") for(int t = 0; t < 4; ++t) {        \
			const bool b_ = qarg_better(oq_[t], oi_[t], q[t], idx[t]); \
			q[t] = b_ ? oq_[t] : q[t];                        \
			idx[t] = b_ ? oi_[t] : idx[t];                    \
			if(t == 1) {                                      \
				cq = b_ ? ocq_ : cq;                          \
				cp = b_ ? ocp_ : cp;                          \
			}                                                 \
		}                                                     \
	}
	CCG_DPP_STEPS(S_)
#undef S_
#pragma unroll
	for(int t = 0; t < 4; ++t) {
		q[t] = readlane_d(q[t], 63);
		idx[t] = __builtin_amdgcn_readlane(idx[t], 63);
	}
	cq = readlane_d(cq, 63);
	cp = __builtin_amdgcn_readlane(cp, 63);
}

// block-wide (q, idx) reduce; result valid in every thread.  `sq`/`si` are
// LDS scratch of blockDim/64 entries.
__device__ __forceinline__ void qarg_block_reduce(double &q, int &idx, double *sq, int *si) {
	qarg_wave_reduce(q, idx);
	const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
	__syncthreads();
	if(lane == 0) {
		sq[wid] = q;
		si[wid] = idx;
	}
	__syncthreads();
	q = sq[0];
	idx = si[0];
	for(int w = 1; w < nw; ++w) {
		if(qarg_better(sq[w], si[w], q, idx)) {
			q = sq[w];
			idx = si[w];
		}
	}
	__syncthreads();
}

// ---------------------------------------------------- in-kernel hand-offs
// Guideline 16 form R1: every handed-off byte is stored write-through (sc1)
// and loaded with sc1 loads by the consumer; each storing wave drains its
// stores (vmcnt(0)) before the workgroup barrier, then ONE lane takes an
// agent-scope ticket.  No release/acquire fences (an L2 write-back per block).
template <typename T>
__device__ __forceinline__ void st_wt(T *p, T v) {
	__hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <typename T>
__device__ __forceinline__ T ld_wt(const T *p) {
	return __hip_atomic_load(const_cast<T *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// true in every thread of the last block to arrive
__device__ __forceinline__ bool last_block_arrive(unsigned *counter) {
	__shared__ int s_last;
	asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
	__syncthreads();
	if(threadIdx.x == 0) {
		unsigned t = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		s_last = (t == gridDim.x * gridDim.y - 1);
	}
	__syncthreads();
	return s_last;
}
