// ccg_dnj_form.h -- the DNJ engines' launch knobs (DnjGrid) and the one place
// that decides which rescan form a join runs (ScanForm, dnj_scan_form).
//
// Host-only and free of HIP types: a plain C++ compiler reads it, so the
// decision is testable without a GPU (tests/test_scan_form.py).  tree.hip and
// tree_shard_dnj.hip launch from the ScanForm; the kernels it names live in
// ccg_dnj_search.h.
#pragma once
#include <stdio.h>
#include <stdlib.h>

#ifdef __HIPCC__
#define CCG_FORM_HD __host__ __device__ __forceinline__
#else
#define CCG_FORM_HD inline
#endif

#define DNJ_B 128        // capacity of S, the candidate rows rescanned speculatively
#define DNJ_BANDS 64     // S: the top rows with Q < m0, then the min-Q row of each
                         // of this many bands below them (DnjGrid::top/bands)
#define DNJ_BANDS_MAX 128  // CCG_S_BANDS up to this (two bands per lane of k_dnj_plan's wave 0)
#define SEG 2048         // cells per rescan unit (TB threads x 8)
#define LB_SEG_DEFAULT (2 * SEG)   // cells per unit of a run with the block bounds (DnjGrid::seg_lb)
#define TBF 1024         // threads of k_dnj_plan (one block)
#define FIND_RPT 16      // rows per thread per step of k_dnj_plan's listing (one step up to n = 15361)
#define PLAN_MAXB 256    // blocks of k_dnj_plan (one listing step of LT * FR rows each)
#define UHIST 64         // bins of k_dnj_plan's per-block histogram of entries by unit count (umax < UHIST)

// Entry e of the scan owns the fixed unit range [e umax, (e + 1) umax): umax is
// the units of the longest row (k_dnj_scan, ccg_dnj_search.h)
CCG_FORM_HD int dnj_umax(int n, int seg) { return n > 2 ? (n - 2) / seg + 1 : 1; }

// Grid of k_dnj_scan: min(ceil(n / scan_div), scan_max).  CCG_SCAN_DIV and
// CCG_SCAN_MAX override it (tests shrink the grid so that several grid
// waves of units run at small n).
struct DnjGrid {
	// prefold_n: every n folds each entry's units once (k_dnj_fold + k_dnj_join_pf); round 4, measured: the
	// headline's tree 6.61 -> 6.36 s (profiled), configs[1] 24.7k -> 25.0k joins/s, 4k Euclidean unchanged
	int scan_div = 4, scan_max = 2048, seg_mul = 0, prefold_n = 0;
	// below 16384 taxa the wave scan replaces the block scan while the joins list many rows: tree_run_t
	// sets small_wave from the rows listed per join over its last 1024-join window (> adapt_rows;
	// CCG_SCAN_ADAPT, 0: never; headline tree 6.23 -> 6.16 s at 1000, 6.11 at 500).  Clade SNP data (the headline) lists thousands of rows per join there,
	// Euclidean matrices a few hundred (configs[1]: 246), where the block scan is 2-3 % faster
	int small_wave = 0, adapt_rows = 500;
	int sphase_b = 512;   // CCG_SPHASE_BLOCKS
	// scan_prune 2: k_dnj_plan's helper blocks rescan S while the plan lists (CCG_PLAN_HELP; 0: S in
	// k_dnj_sphase after the plan): headline tree 5.96 -> 5.71 (128) / 5.67 s (256), profiled
	int plan_help = 256;
	int scan_cmp = 1, cmp_blocks = 1024;   // the compacted wave scan (CCG_SCAN_CMP=0: off) and its grid
	// scan_prune 2 pays while the joins list many cells: tree_run_t keeps it on (prune_on) while the last
	// 1024-join window listed more than prune_cells cells per join (CCG_PRUNE_CELLS; 0: always)
	long long prune_cells = 20000000;
	int prune_on = 1;
	// plan_qdelay: the listing waves hold their Q loads back by qdelay x 32 x 64 cycles so that wave 0's fold
	// loads go first (round 6, profiles/r06_config1_sweep.txt: 0 -> 2 gives configs[1] 23.5k -> 23.9k joins/s,
	// the headline tree 12.79k -> 12.90k; 4 and above lose at 10k)
	int s_top = 0, s_bands = -1, s_split_n = 16384, plan_qdelay = 2, scan_wave = -1, plan_multi = 1;
	int plan_regsel = 0, plan_fr = FIND_RPT;   // measured at 10k: S from registers 13.2 -> 15.4 us (Q arrives late), FR 1-8 within noise
	// tests only (CCG_TEST_WITHHOLD): bit 0, k_dnj_plan's block 0 never publishes its entry count (the
	// listing blocks' look-back must time out into an error); bit 1, it never tags the S header (the
	// helper blocks' wait must); either shortens the bounded spins so that the error comes quickly
	int test_withhold = 0;
	int join_pf = 1;   // with k_dnj_fold: k_dnj_join_pf (0: k_dnj_join; 2: its block-0 replay path always)
	// measured at the headline (configs[2], 50k, profiled tree; round 4): scan + fold per join 68.3 us with
	// k_dnj_fold, 72.4 with FoldTail, 84.2 with FoldTail + pruning (cells 2.12x -> 1.27x the reference's:
	// the S phase and the wait for its table lengthen every wave's chain more than the pruned loads save)
	int scan_fold = 0; // the fold at the scan's last arrivals (FoldTail) instead of k_dnj_fold (CCG_SCAN_FOLD=1)
	// band mode: the S rows' exact fresh minima bound the other entries, and an entry whose stale Q is not
	// below the bound at its row is one minQpair skips (dnj.c:78): 2 (default) k_dnj_sphase rescans S,
	// builds the table and keeps only the surviving entries for the compacted wave scan; 1: the S phase
	// inside the scan (with FoldTail, CCG_SCAN_FOLD=1); 0: off.  Headline tree (profiled, round 4):
	// 6.29 s off, 5.86-5.89 s with 2 while the joins list > 15-30M cells, 6.05 s with 2 throughout
	int scan_prune = 2;
	// the block lower bounds (TreeBufs::lbm, lb_unit): kept by the join and the requeue from the first join
	// of a matrix larger than lb_min_n on (CCG_SCAN_LB=0: off; CCG_LB_MIN_N), used by the compacted wave scan
	int lb = 1, lb_min_n = 16384;
	// with the bounds, the row-group scan modes (20, 21: float / u16 / u8 rows) may rescan bounded row groups
	// (CCG_LB_GROUPS=1: k_dnj_scan_gc<LB>, lb_unit_g: one column-sum load per lane for the group's rows
	// needing a block) instead of one bounded row per wave.  Measured (round 6, configs[3] on round 4's
	// cdist matrix, first 40k joins, the same cells): scan 40.9 s against 17.2 s for one row per wave --
	// the bounded scan is latency-bound, and the group form has a quarter of the units at 131 VGPRs
	// (3 waves/SIMD) against 68 (7): off by default
	int lb_groups = 0;
	// the bounded units' length in cells (a multiple of 64, at most 8 SEG).  A bounded unit is a latency chain
	// (threshold and sum, up to 256 block bounds and column-sum maxima, the surviving cells) whatever its length,
	// but a long unit leaves a row's surviving blocks to fewer waves.  Measured on the headline tree beside the
	// dist (tree_s, profiles/step_legs.json): seg(n) of a run without bounds 6.022 s, 2048 throughout 6.385,
	// 4096 5.921, 8192 6.078, 16384 6.752: LB_SEG_DEFAULT is 4096 (a floor: seg_bounded()).  seg_lb: set by tree_run_t once the bounds
	// are bound (0: none, seg(n) as without them); seg_lb_knob: CCG_SEG_LB (tests and sweeps; 0: the default,
	// -1 from CCG_SEG_LB=0: the lengths of a run without bounds)
	int seg_lb = 0, seg_lb_knob = 0;
	int scan_vblk = 1;  // with pruning: also the bound from every row above (the requeue's per-block
	                    // minima of V_k = max(q at the partner cell, Q_k)) (CCG_SCAN_VBLK=0: off)
	void load() {
		if(const char *e = getenv("CCG_JOIN_PF")) join_pf = atoi(e);
		if(const char *e = getenv("CCG_SCAN_FOLD")) scan_fold = atoi(e);
		if(const char *e = getenv("CCG_SCAN_PRUNE")) scan_prune = atoi(e);
		if(const char *e = getenv("CCG_SCAN_VBLK")) scan_vblk = atoi(e);
		if(const char *e = getenv("CCG_S_TOP")) s_top = atoi(e) > 0 ? atoi(e) : 0;
		if(const char *e = getenv("CCG_S_BANDS")) s_bands = atoi(e) >= 0 ? atoi(e) : -1;
		if(const char *e = getenv("CCG_S_SPLIT_N")) s_split_n = atoi(e);
		if(const char *e = getenv("CCG_SCAN_DIV")) scan_div = atoi(e) > 0 ? atoi(e) : 4;
		if(const char *e = getenv("CCG_SCAN_MAX")) scan_max = atoi(e) > 0 ? atoi(e) : 2048;
		if(const char *e = getenv("CCG_SEG_MUL")) seg_mul = atoi(e) > 0 ? atoi(e) : 0;
		if(const char *e = getenv("CCG_PREFOLD_N")) prefold_n = atoi(e) >= 0 ? atoi(e) : 0;
		if(const char *e = getenv("CCG_SCAN_ADAPT")) adapt_rows = atoi(e) > 0 ? atoi(e) : 0;
		if(const char *e = getenv("CCG_SPHASE_BLOCKS")) sphase_b = atoi(e) > 0 ? atoi(e) : 512;
		if(const char *e = getenv("CCG_PLAN_HELP")) plan_help = atoi(e) >= 0 && atoi(e) < 512 ? atoi(e) : 256;
		if(const char *e = getenv("CCG_SCAN_CMP")) scan_cmp = atoi(e);
		if(const char *e = getenv("CCG_PRUNE_CELLS")) prune_cells = atoll(e) > 0 ? atoll(e) : 0;
		prune_on = 1;
		if(const char *e = getenv("CCG_SCAN_CMPB")) cmp_blocks = atoi(e) > 0 ? atoi(e) : 1024;
		if(const char *e = getenv("CCG_PLAN_QDELAY")) plan_qdelay = atoi(e) >= 0 ? atoi(e) : 2;
		if(const char *e = getenv("CCG_SCAN_WAVE")) scan_wave = atoi(e);
		if(const char *e = getenv("CCG_PLAN_MULTI")) plan_multi = atoi(e);
		if(const char *e = getenv("CCG_PLAN_REGSEL")) plan_regsel = atoi(e);
		if(const char *e = getenv("CCG_PLAN_FR")) plan_fr = atoi(e) < 1 ? 1 : atoi(e) > FIND_RPT ? FIND_RPT : atoi(e);
		if(const char *e = getenv("CCG_TEST_WITHHOLD")) test_withhold = atoi(e) & 3;
		if(const char *e = getenv("CCG_SCAN_LB")) lb = atoi(e);
		if(const char *e = getenv("CCG_LB_MIN_N")) lb_min_n = atoi(e);
		if(const char *e = getenv("CCG_LB_GROUPS")) lb_groups = atoi(e);
		if(const char *e = getenv("CCG_SEG_LB")) {
			char *end;
			const long v = strtol(e, &end, 10);
			if(end != e && !*end && v == 0) seg_lb_knob = -1;
			else if(end != e && !*end && v >= 64 && v <= 8 * SEG && v % 64 == 0) seg_lb_knob = (int) v;
			else fprintf(stderr, "ccphylo_amd: CCG_SEG_LB=%s ignored (0, or a multiple of 64 up to %d)\n", e, 8 * SEG);
		}
	}
	// k_dnj_plan's last argument: the Q-load delay (low 14 bits), bits 14-15 the
	// test knob test_withhold, bit 16 turns
	// the register S selection off (on with CCG_PLAN_REGSEL=1)
	// and bits 17-20 the rows per thread per listing step less one (CCG_PLAN_FR)
	int plan_flags(bool prune = false, int helpers = 0) const {
		return (plan_qdelay & 0x3fff) | (test_withhold & 3) << 14 | (plan_regsel ? 0 : 1 << 16) | ((plan_fr - 1) & 15) << 17 | (prune ? 1 << 21 : 0) |
		       (helpers & 511) << 22;
	}
	// k_dnj_plan's grid: one listing step of (TBF - 64) FIND_RPT rows per block
	// (CCG_PLAN_MULTI=0: one block walks every step, the round-2 form)
	unsigned plan_blocks(int n) const {
		if(!plan_multi) return 1;
		const int step = (TBF - 64) * plan_fr;
		const int g = (n - 1 + step - 1) / step;
		return (unsigned) (g < 1 ? 1 : g > PLAN_MAXB ? PLAN_MAXB : g);
	}
	// rescans one unit per wave past 16384 taxa, where the units are long:
	// 16-byte row loads (k_dnj_scan_v, mode 4; the GEN form k_dnj_scan_w,
	// mode 1); one unit per block below (k_dnj_scan, mode 0).  Measured per
	// join at 50k (headline data): 88.4 (block) -> 72.0 (wave) -> 66.7 us
	// (wave, 16-byte loads) -> 65.2 us (+ nontemporal row loads and 16-byte
	// sD loads where aligned, mode 9; 8433 -> 8920 joins/s); 10k: 9.4 (block)
	// against 9.8 us (wave).  Float rows take the row-group form (mode 20,
	// k_dnj_scan_g, 4 rows per wave sharing the sD loads; 21: 8 rows, half
	// the columns per step): configs[3]'s first 30k joins rescan in 34.0 s
	// against 47.0 s with mode 4 on the same box.
	// CCG_SCAN_WAVE=0/1/4/9/20/21 forces a form.
	// Retired, measured and lost (their kernels are gone; the values still
	// resolve, to the base form they varied):
	//   5-8, 10-19 -> 4: k_dnj_scan_v's lone nontemporal and lone 16-byte-sD
	//     forms, its software-pipelined forms (two register sets, the next
	//     loads issued before the compares) and its double-width forms.  On
	//     configs[3] (float rows, first 30k joins) mode 4 took 41.7-47.0 s over
	//     boxes, 9: 46.0, 11: 46.8, 13: 47.0, 15: 47.5 -- none beat 4 or 9
	//   22, 23 -> 20: the (G, UC) = (4, 4) and (2, 8) row groups.  Double rows
	//     gain nothing from any row group at 50k (joins/s: G4/UC8 8472, G4/UC4
	//     8453, G2/UC8 8656 against 8901 for mode 9; modes 20, 22, 23), and
	//     on float rows neither beat (4, 8)
	// In the sharded engine (no row groups) modes >= 4 run k_dnj_scan_v.
	// past 16384 taxa: double rows (the headline) stream with the 16-byte
	// nontemporal wave scan (9); narrower rows (float -p, u16 -s, u8 -b) in row
	// groups (20), where the 8-byte sD load per cell outweighs the row bytes
	// and one sD load serves 4 rows
	int scan_mode(int n, int et = 8) const {
		return scan_wave >= 0 ? scan_wave : n > 16384 || small_wave ? (et == 8 ? 9 : 20) : 0;
	}
	// cells per rescan unit: SEG up to 8 units per row, then growing with n
	// (at most 8 SEG) so that a unit's fixed cost stays small beside its bytes
	int seg(int n) const {
		int m = seg_mul ? seg_mul : n / (8 * SEG);
		m = m < 1 ? 1 : m > 8 ? 8 : m;
		return m * SEG;
	}
	// the unit length of a join that scans under the block bounds (ScanForm::seg; seg_lb set): CCG_SEG_LB's as
	// it is, the default as a floor under seg(n) (from 49152 taxa on that one is longer, so the unit arrays
	// tree_layout sizes and the plan's UHIST bins hold at every n)
	int seg_bounded(int n) const { return seg_lb_knob > 0 || seg_lb > seg(n) ? seg_lb : seg(n); }
	// rows with many units: fold each row's unit partials once (k_dnj_fold)
	// instead of in every block of k_dnj_join
	bool prefold(int n) const { return n > prefold_n; }
	// S: `top` rows from the top, then up to `bands` band-minimum rows.  Small
	// matrices are latency-bound: 128 top rows, no bands; beyond s_split_n the
	// bands cut the rescanned cells several-fold (tools/sim_stages.c)
	int top(int n) const {
		// (round 4: 8 top rows in band mode measured the same as 16 at the headline; band mode with pruning
		// below 16384 taxa -- CCG_S_TOP=8 CCG_S_BANDS=64 -- took its tree 5.64 -> 5.43-5.51 s profiled, engine
		// cells 1.31 -> 1.16x, but costs configs[1]'s Euclidean trees, and switching band mode per window
		// needs the requeue and the next plan to agree; not done)
		const int t = s_top ? s_top : n > s_split_n ? 16 : DNJ_B;
		return t < 1 ? 1 : t > DNJ_B ? DNJ_B : t;
	}
	int bands(int n) const {
		int b = s_bands >= 0 ? s_bands : n > s_split_n ? DNJ_BANDS : 0;
		b = b > DNJ_BANDS_MAX ? DNJ_BANDS_MAX : b;
		return top(n) + b > DNJ_B ? DNJ_B - top(n) : b;
	}
	// k_dnj_sphase's grid (one wave per S unit, grid-stride)
	unsigned sphase_blocks() const { return sphase_b; }
	unsigned scan(int n) const {
		const long long g = (n + scan_div - 1) / scan_div;
		return (unsigned) (g < scan_max ? g : scan_max);
	}
};

// ------------------------------------------------------------------ scan form
// Everything one join's scan leg needs, decided once per join from the grid
// knobs, the matrix size, the element width (et bytes), whether entries may
// be missing (gen) and whether the block lower bounds exist (have_lbm).
enum ScanKernel {
	SCAN_BLOCK,      // k_dnj_scan: one unit per block
	SCAN_WAVE,       // k_dnj_scan_w: one unit per wave (the only wave form with missing entries)
	SCAN_WAVE16,     // k_dnj_scan_v: one unit per wave, 16-byte row loads
	SCAN_GROUP,      // k_dnj_scan_g: G rows per wave over the (group, unit) grid
	SCAN_GROUP_CMP   // k_dnj_scan_gc: row groups over the dense enumeration
};
enum ScanSphase {
	SPHASE_NONE,
	SPHASE_SCAN,     // k_dnj_sphase rescans S, then compacts the survivors
	SPHASE_COMPACT   // k_dnj_plan's helper blocks rescanned S: k_dnj_sphase<SLOOP = false> compacts only
};
struct ScanForm {
	ScanKernel kernel;
	bool stream;       // SCAN_WAVE16: nontemporal row loads and 16-byte sD loads
	int G, UC;         // the row groups' rows per wave and columns per lane per step: (4, 8) or (8, 4)
	int prune;         // 0: off; 1: the S phase inside the scan; 2: k_dnj_sphase before it
	bool cmp;          // the dense enumeration from the plan's unit histogram
	bool lb;           // under the block lower bounds (lb_unit / lb_unit_g)
	bool tfold;        // FoldTail: the scan folds the entries at their last arrivals
	int helpers;       // k_dnj_plan's helper blocks (they rescan S while the plan lists)
	ScanSphase sphase;
	bool fold;         // k_dnj_fold follows the scan ...
	int sfold;         // ... with this argument (S's entries folded already)
	unsigned grid;     // the scan's grid
	int launches;      // launches of the scan leg: the scan, k_dnj_sphase, k_dnj_fold
	int seg;           // cells per unit of this join's plan, scan, fold and join: seg(n), or seg_bounded(n) under the bounds
};

// CCG_SCAN_WAVE's value as the form that runs: 0 block; 1-3 wave; 4 16-byte
// wave and 9 its streaming form; 20 and 21 the (4, 8) and (8, 4) row groups.
// The retired values resolve to the form they varied (DnjGrid::scan_mode):
// 5-8 and 10-19 as 4, 22 and 23 as 20.  Values past 23 always ran the plain
// mode-4 kernel, never pruned: sm stays as it is for them.
inline int dnj_scan_base(int sm) {
	return sm <= 0 ? 0 : sm < 4 ? 1 : sm == 9 || sm == 21 || sm > 23 ? sm : sm < 20 ? 4 : 20;
}

inline ScanForm dnj_scan_form(const DnjGrid &g, int n, int et, bool gen, bool have_lbm) {
	const int sm = dnj_scan_base(g.scan_mode(n, et));
	const bool grp = sm == 20 || sm == 21, prefold = g.prefold(n);
	ScanForm f = {};
	f.tfold = prefold && g.scan_fold && sm >= 1;
	// the bounded scan is the compacted wave scan (below: f.lb follows from have_lbm && f.cmp; prune 1 needs
	// FoldTail, so !tfold covers it): where it will run with a length of its own, that length decides `fits`
	const bool lbseg = have_lbm && g.seg_lb > 0 && !gen && sm >= 4 && g.scan_cmp && !f.tfold &&
	                   dnj_umax(n, g.seg_bounded(n)) < UHIST;
	f.seg = lbseg ? g.seg_bounded(n) : g.seg(n);
	const bool fits = dnj_umax(n, f.seg) < UHIST;   // the plan's unit histogram covers every row
	// pruning: band mode, no missing entries, a wave form.  1 wants FoldTail;
	// 2 wants k_dnj_fold, and with row groups the compacted scan (its
	// enumeration is how the groups skip what k_dnj_sphase pruned)
	if(!gen && g.bands(n) && prefold && sm >= 4 && sm <= 23) {
		if(g.scan_prune == 1 && g.scan_fold) f.prune = 1;
		else if(g.scan_prune == 2 && g.prune_on && !g.scan_fold && (!grp || (g.scan_cmp && fits))) f.prune = 2;
	}
	f.helpers = f.prune == 2 ? g.plan_help : 0;
	f.sphase = f.prune != 2 ? SPHASE_NONE : g.plan_help ? SPHASE_COMPACT : SPHASE_SCAN;
	f.cmp = !gen && sm >= 4 && g.scan_cmp && !f.tfold && f.prune != 1 && fits;
	if(gen || sm < 4) f.kernel = sm >= 1 ? SCAN_WAVE : SCAN_BLOCK;
	else if(have_lbm && f.cmp && grp && g.lb_groups && f.prune == 0) {
		// bounded row groups: 4 rows per wave share each column-sum load (the one (G, UC) built)
		f.kernel = SCAN_GROUP_CMP;
		f.lb = true;
		f.G = 4;
		f.UC = 8;
	} else if(have_lbm && f.cmp) {
		// the compacted wave scan under the block lower bounds (every element type, plain loads)
		f.kernel = SCAN_WAVE16;
		f.lb = true;
	} else if(grp) {
		f.kernel = f.cmp ? SCAN_GROUP_CMP : SCAN_GROUP;
		f.G = sm == 21 ? 8 : 4;
		f.UC = sm == 21 ? 4 : 8;
	} else {
		f.kernel = SCAN_WAVE16;
		f.stream = sm == 9;
	}
	f.grid = f.cmp && g.scan(n) > (unsigned) g.cmp_blocks ? (unsigned) g.cmp_blocks : g.scan(n);
	f.fold = prefold && !f.tfold;
	f.sfold = f.prune == 2;
	f.launches = 1 + (f.sphase != SPHASE_NONE) + f.fold;
	return f;
}

// The sharded engine has the block and the two wave kernels only (no missing
// entries, no row groups, no pruning; RecTail folds the units into records):
// every mode from 4 up runs k_dnj_scan_v, 9 streaming
inline ScanForm dnj_scan_form_shard(const DnjGrid &g, int n, int et, bool have_lbm) {
	const int sm = g.scan_mode(n, et);
	ScanForm f = {};
	f.kernel = sm >= 4 ? SCAN_WAVE16 : sm >= 1 ? SCAN_WAVE : SCAN_BLOCK;
	f.stream = sm == 9;
	f.lb = have_lbm && sm >= 4;
	f.grid = g.scan(n);
	f.launches = 1;
	f.seg = g.seg(n);
	return f;
}
