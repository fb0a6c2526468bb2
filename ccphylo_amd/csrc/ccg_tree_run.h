// ccg_tree_run.h -- the host frame of the four tree drivers (tree_run_t,
// lk_run_t, tree_shard_run_t, tree_shard_dnj_run_t): the per-kernel timer,
// the run from the seeded control block to the copied joins, the statistics
// vector and the block lower bounds' memory.  Host code only; each driver
// keeps its own per-join body (the host drivers' frame).
#pragma once
#include <vector>
#include "ccg_tree_common.h"

// Per-kernel HIP-event timing (profile mode): one event after every launch,
// harvested in batches.
struct KTimer {
	bool on = false;
	hipStream_t st;
	hipEvent_t ev[1025];
	int cls[1025];
	int used;
	long long cnt[CCG_NKSTAT], ns[CCG_NKSTAT];
	void init(hipStream_t s, bool enable) {
		abort();   // (a timer that was never finished still holds its events)
		on = enable;
		st = s;
		used = 0;
		memset(cnt, 0, sizeof(cnt));
		memset(ns, 0, sizeof(ns));
		if(on) {
			for(int k = 0; k < 1025; ++k) hipEventCreate(&ev[k]);
			hipEventRecord(ev[0], st);
			used = 1;
		}
	}
	void harvest() {
		hipEventSynchronize(ev[used - 1]);
		for(int k = 1; k < used; ++k) {
			float ms = 0;
			hipEventElapsedTime(&ms, ev[k - 1], ev[k]);
			cnt[cls[k]] += 1;
			ns[cls[k]] += (long long) (ms * 1.0e6);
		}
		hipEvent_t t = ev[0];
		ev[0] = ev[used - 1];
		ev[used - 1] = t;
		used = 1;
	}
	void mark(int c) {
		if(!on) return;
		cls[used] = c;
		hipEventRecord(ev[used++], st);
		if(used == 1025) harvest();
	}
	// releases the events; later marks (e.g. a final collective) are not timed
	void abort() {
		if(!on) return;
		for(int k = 0; k < 1025; ++k) hipEventDestroy(ev[k]);
		on = false;
	}
	void finish() {
		if(!on) return;
		harvest();
		abort();
	}
};

// the seed of a run's control block
static inline TreeCtl tree_ctl_seed(const ccg_tree_args *a) {
	TreeCtl c;
	memset(&c, 0, sizeof(c));
	c.neg = (a->flags & 2) != 0;
	c.exact = a->exact != 0;
	c.method = a->method;
	c.hj = c.hi = -1;
	return c;
}

// The statistics vector of ccg_tree / ccg_tree_shard (ccphylo_amd.h): the
// only code that knows its indices.  A driver fills the fields it has.
struct TreeStats {
	long long rows = 0, cells = 0, launches = 0, us = 0;
	// profile only, behind the CCG_NKSTAT (launches, ns) pairs of the timer:
	long long cells_top = 0, cells_rest = 0, serial_sums = 0, chain_sums = 0;
	long long slot8 = 0;          // one GPU: S cells rescanned by the plan's helpers; sharded: the init's collective bytes
	long long hard_columns = 0;   // sharded: columns summed through the serial gather
	long long ref_rows = 0, ref_cells = 0;   // the reference rule's rescans (the linkage methods: their own rows / cells)
	void write(int64_t *stats, bool profile, const KTimer &kt) const {
		if(!stats) return;
		stats[0] = rows;
		stats[1] = cells;
		stats[2] = launches;
		stats[3] = us;
		if(!profile) return;
		for(int c = 0; c < CCG_NKSTAT; ++c) {
			stats[4 + 2 * c] = kt.cnt[c];
			stats[5 + 2 * c] = kt.ns[c];
		}
		const long long tail[8] = {cells_top, cells_rest, serial_sums, chain_sums, slot8, hard_columns, ref_rows, ref_cells};
		for(int k = 0; k < 8; ++k) stats[4 + 2 * CCG_NKSTAT + k] = tail[k];
	}
};

// One run on the context's stream: begin, the per-join check, finish, the
// final distance, end.  Ctl is the control block (TreeCtl, LkCtl: done,
// final_n, njoins) at device address dctl.  The destructor releases the
// timer's events of a run that returned early and waits for the stream, so
// the memory a driver declared before the frame is idle when it is freed.
template <class Ctl>
struct TreeRun {
	ccg_ctx *ctx;
	hipStream_t st;
	const Ctl *dctl;
	KTimer kt;
	long long launches = 0;
	int since_check = 0;
	float ms = 0;
	TreeRun(ccg_ctx *c, const Ctl *device_ctl) : ctx(c), st(c->stream), dctl(device_ctl) {}
	TreeRun(const TreeRun &) = delete;
	~TreeRun() {
		kt.abort();
		hipStreamSynchronize(st);
	}
	int read_ctl(Ctl &h) {
		CCG_CHECK(hipMemcpyAsync(&h, dctl, sizeof(h), hipMemcpyDeviceToHost, st));
		CCG_CHECK(hipStreamSynchronize(st));
		return CCG_OK;
	}
	int begin(const Ctl &seed, bool profile) {
		CCG_CHECK(hipMemcpyAsync((void *) dctl, &seed, sizeof(seed), hipMemcpyHostToDevice, st));
		CCG_CHECK(hipEventRecord(ctx->ev0, st));
		kt.init(st, profile);
		return CCG_OK;
	}
	// after each join: every 1024th reads the control block back into h (*read)
	int check(Ctl &h, bool *read) {
		*read = ++since_check == 1024;
		if(!*read) return CCG_OK;
		since_check = 0;
		return read_ctl(h);
	}
	// after the loop, n the matrix size it reached: the block into h, the run's
	// time, the join count, the final size and the joins (an async copy: end())
	int finish(Ctl &h, int n, const ccg_join *dev_joins, ccg_join *joins, int *njoins, int *final_n, double *final_d) {
		CCG_CHECK(hipEventRecord(ctx->ev1, st));
		kt.finish();
		CCG_TRY(read_ctl(h));
		CCG_CHECK(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
		if(h.done && h.final_n < 0) {   // a bounded wait of k_dnj_plan gave up (never expected)
			ccg_set_last_msg("k_dnj_plan / k_dnj_join: a block's bounded wait on another block timed out");
			return CCG_EHIP;
		}
		*njoins = h.njoins;
		*final_n = h.done ? h.final_n : n;
		*final_d = -1.0;
		if(h.njoins) CCG_CHECK(hipMemcpyAsync(joins, dev_joins, (size_t) h.njoins * sizeof(ccg_join), hipMemcpyDeviceToHost, st));
		return CCG_OK;
	}
	// D(1, 0) of a finished tree (final_n == 2), from where it lies on this device
	template <int ET>
	int final_distance(const void *dev_src, double bs, double *final_d) {
		typename Elem<ET>::T v;
		CCG_CHECK(hipMemcpyAsync(&v, dev_src, sizeof(v), hipMemcpyDeviceToHost, st));
		CCG_CHECK(hipStreamSynchronize(st));
		*final_d = (ET == 8 || ET == 4) ? (double) v : v / bs;
		return CCG_OK;
	}
	TreeStats stats() const {
		TreeStats s;
		s.launches = launches;
		s.us = (long long) (ms * 1000.0);
		return s;
	}
	int end() {
		CCG_CHECK(hipStreamSynchronize(st));
		return CCG_OK;
	}
};

// The block lower bounds (TreeBufs::lbm): the line of every owned row, the sD
// maxima, the thresholds and the skipped-cell slots, in one piece of memory.
struct LbLayout {
	long long LS;
	size_t lbb, msb, ubb, skb;
	size_t bytes() const { return lbb + msb + ubb + skb; }
};
static inline LbLayout lb_layout(int n0, long long owned_rows) {
	LbLayout l;
	l.LS = (n0 + LBW - 1) / LBW;
	l.lbb = ((size_t) owned_rows * l.LS * 4 + 255) & ~(size_t) 255;
	l.msb = ((size_t) (l.LS + 1) * 8 + 255) & ~(size_t) 255;
	l.ubb = ((size_t) n0 * 8 + 255) & ~(size_t) 255;
	l.skb = (size_t) (LB_SCAN + LB_HELP) * LB_SLOT * 8;
	return l;
}
// lbw: TreeBufs::lbw (0: one GPU; the world size of a sharded run)
static inline int lb_bind(TreeBufs &b, void *mem, const LbLayout &l, int lbw, hipStream_t st) {
	char *m = (char *) mem;
	b.lbm = (unsigned *) m;
	b.msd = (double *) (m + l.lbb);
	b.ubq = (double *) (m + l.lbb + l.msb);
	b.lbs = l.LS;
	b.lbw = lbw;
	b.lbskip = (long long *) (m + l.lbb + l.msb + l.ubb);
	CCG_CHECK(hipMemsetAsync(b.lbskip, 0, l.skb, st));
	return CCG_OK;
}
// the bounded-out cells into h, from the first `slots` per-wave slots
static inline int lb_harvest(const TreeBufs &b, size_t slots, hipStream_t st, TreeCtl &h) {
	if(!b.lbskip) return CCG_OK;
	std::vector<long long> sl(slots * LB_SLOT);
	// on the run's stream (a null-stream copy would wait for every blocking stream of the device)
	CCG_CHECK(hipMemcpyAsync(sl.data(), b.lbskip, sl.size() * 8, hipMemcpyDeviceToHost, st));
	CCG_CHECK(hipStreamSynchronize(st));
	for(size_t x = 0; x < slots; ++x) {
		h.cells_lbskip += sl[x * LB_SLOT];
		h.cells_help -= sl[x * LB_SLOT + 1];
	}
	return CCG_OK;
}
