/* linkage_oracle.c -- serial CPU restatement of the reference's tree methods
 * upgma, cf, ff and mn (tree.c:332-392), written from its behaviour; the line
 * numbers cite the reference source each rule was read from.  Built on the
 * helpers of the project's oracle (oracle/ccoracle.c, included below: the
 * typed LT access ld / st, limb_length, update_d, pop_arrange, min_q_row,
 * min_pos).  Compiled by tests/linkage_oracle.py into a temporary directory
 * with -ffp-contract=off, so every expression rounds as the reference's
 * x86-64 build does.
 *
 * TEST INFRASTRUCTURE ONLY: the checker of tests/test_linkage_oracle.py (against
 * the goldens and the live reference binary) and tests/test_gpu_linkage.py. */
#include "../oracle/ccoracle.c"

static inline int64_t cell(int64_t a, int64_t b) { return a > b ? tri(a) + b : tri(b) + a; }

/* hclust.c:205-277 initDmin (sD and N as nj.c:111 initSummaD builds them) */
static void init_dmin(const Ltd *D, int n, double *sD, int32_t *N, double *Q, int32_t *P) {
	for(int k = 0; k < n; ++k) {
		sD[k] = 0;
		N[k] = 1;
	}
	for(int64_t i = 0; i < n; ++i) {
		double min = DBL_MAX;
		int pos = 0;
		for(int64_t j = 0; j < i; ++j) {
			double d = ld(D, tri(i) + j);
			if(0 <= d) {
				if(d <= min) {
					min = d;
					pos = (int) j;
				}
				sD[i] += d;
				sD[j] += d;
				++N[i];
				++N[j];
			}
		}
		Q[i] = min;
		P[i] = pos;
	}
}

/* hclust.c:665 updateUPGMA (m = 0), hclust.c:884 updateFF (m = 1), hclust.c:1102
 * updateCF (m = 2; only for matrices without missing cells: its "only D_ik"
 * branch at :1188 / :1271 advances the base pointer of N). */
static int update_linkage(Ltd *D, int n, double *sD, int32_t *N, double *Q, int32_t *P, int i, int j, int m) {
	int nn = 1, p = j;
	double sd = 0, min = DBL_MAX;
	/* the reference's sDvec / Nptr cursor: it advances once per k that takes a
	 * branch, once for j and once for i, but not where both cells are missing
	 * (hclust.c:761-763, :844-846), so after such a k the updates of sD and N
	 * land one row low; Q and P are indexed by k itself */
	int64_t c = 0;
	Q[j] = DBL_MAX;
	if(m != 1) P[j] = 0;   /* updateFF leaves P[j] (hclust.c:897-899) */
	for(int64_t k = 0; k < n; ++k) {
		if(k == j) {
			min = Q[j];   /* "save min" (hclust.c:773 / :991 / :1210) */
			p = j;
			++c;
			continue;
		}
		if(k == i) {
			++c;
			continue;
		}
		const int64_t fi = cell(i, k), fj = cell(k, j);
		const double Dik = ld(D, fi), Dkj = ld(D, fj);
		double dist;
		if(0 <= Dik && 0 <= Dkj) {
			dist = m == 0 ? (k < j ? (Dik + Dkj) / 2 : (Dkj + Dik) / 2) : m == 1 ? (Dik < Dkj ? Dkj : Dik) : (Dik < Dkj ? Dik : Dkj);
			st(D, fj, dist, 0);
			sD[c] -= (Dik + Dkj - dist);
			sd += dist;
			--N[c];
			++c;
			++nn;
		} else if(0 <= Dik) {
			dist = Dik;
			st(D, fj, dist, 0);
			++c;         /* "sD(k) is new": sD and N stay */
			sd += Dik;
			++nn;
		} else if(0 <= Dkj) {
			dist = Dkj;
			--N[c];
			++c;
			sd += Dkj;
			++nn;
		} else {
			dist = -1;
		}
		if(k < j) {
			/* row j (hclust.c:766 / :1203: `0 <= dist && dist <= Q`; FF :984: `dist < Q`) */
			if(m == 1 ? dist < Q[j] : (0 <= dist && dist <= Q[j])) {
				Q[j] = dist;
				P[j] = (int) k;
			}
		} else if(m == 2) {
			/* column j, updateCF (hclust.c:1288-1296) */
			if(0 <= dist && dist <= Q[k]) {
				if(dist < Q[k] || P[k] == i || P[k] == k || P[k] < j) {
					Q[k] = dist;
					P[k] = j;
					if(min <= dist) {
						min = dist;
						p = (int) k;
					}
				}
			}
		} else if(0 <= dist) {
			/* column j, updateUPGMA / updateFF (hclust.c:851-873 / :1069-1091) */
			if(dist < Q[k]) {
				Q[k] = dist;
				P[k] = j;
				if(min <= dist) {
					min = dist;
					p = (int) k;
				}
			} else if(P[k] == i || P[k] == j) {
				if(dist == Q[k]) {
					P[k] = j;
					if(min <= dist) {
						min = dist;
						p = (int) k;
					}
				} else {
					P[k] = -1;   /* a bounded row: Q[k] is a lower bound */
				}
			}
		}
	}
	N[j] = nn;
	sD[j] = sd;
	return p;
}

/* hclust.c:1559-1669 UPGMA_popArrange */
static int linkage_pop_arrange(Ltd *D, int *np, double *sD, int32_t *N, double *Q, int32_t *P, int pos) {
	const int n = --*np;
	int p;
	if(pos == n) return 0;
	sD[pos] = sD[n];
	N[pos] = N[n];
	Q[pos] = DBL_MAX;
	P[pos] = 0;
	for(int64_t k = 0; k < pos; ++k) {
		const double v = ld(D, tri(n) + k);
		memcpy((char *) D->base + (tri(pos) + k) * D->et, (char *) D->base + (tri(n) + k) * D->et, (size_t) D->et);
		if(0 <= v && v <= Q[pos]) {
			Q[pos] = v;
			P[pos] = (int) k;
		}
	}
	double min = Q[pos];
	p = pos;
	for(int64_t k = pos + 1; k < n; ++k) {
		const double v = ld(D, tri(n) + k);
		memcpy((char *) D->base + (tri(k) + pos) * D->et, (char *) D->base + (tri(n) + k) * D->et, (size_t) D->et);
		if(0 <= v && v <= Q[k]) {
			if(P[k] < pos || v < Q[k]) {
				Q[k] = v;
				P[k] = pos;
				if(v <= min) {
					min = v;
					p = (int) k;
				}
			}
		}
	}
	return p;
}

/* dnj.c:217-293 UPGMApair from hint row i; 0: no pair */
static uint64_t upgma_pair(const Ltd *D, int n, double *Q, int32_t *P, int i, int64_t *stats) {
	uint64_t pos = 0;
	double min = DBL_MAX;
	if(i && min != Q[i]) {
		min = Q[i];
		pos = ((uint64_t) (uint32_t) i << 32) | (uint32_t) P[i];
	}
	for(i = n - 1; i >= 1; --i) {
		if(Q[i] < min) {
			if(P[i] < 0) {
				double uq = DBL_MAX;
				int mj = 0;
				for(int64_t j = 0; j < i; ++j) {
					const double q = ld(D, tri(i) + j);
					if(0 <= q && q <= uq) {
						uq = q;
						mj = (int) j;
					}
				}
				if(stats) {
					stats[0] += 1;
					stats[1] += i;
				}
				P[i] = mj;
				Q[i] = uq;
				if(uq < min) {
					min = uq;
					pos = ((uint64_t) (uint32_t) i << 32) | (uint32_t) mj;
				}
			} else {
				min = Q[i];
				pos = ((uint64_t) (uint32_t) i << 32) | (uint32_t) P[i];
			}
		}
	}
	return pos;
}

/* nj.c:297-362 initQ_MN: the last maximal cell in row-major order */
static uint64_t init_q_mn(const Ltd *D, int n, const double *sD, const int32_t *N) {
	double max = -DBL_MAX;
	int mi = 0, mj = 0;
	for(int64_t i = 1; i < n; ++i) {
		const int64_t base = tri(i);
		for(int64_t j = 0; j < i; ++j) {
			double q = ld(D, base + j);
			if(0 <= q) {
				q = ((N[i] + N[j] - 4) >> 1) * q - sD[i] - sD[j];
				if(max <= q) {
					max = q;
					mi = (int) i;
					mj = (int) j;
				}
			}
		}
	}
	return ((uint64_t) mi << 32) | (uint32_t) mj;
}

/* method: 3 upgma, 4 cf, 5 ff, 6 mn (the engine's CCG_TREE_* ids).  D is
 * destroyed.  stats (may be NULL): [0] rows, [1] cells UPGMApair rescanned.
 * Returns the joins made; -1 for another method. */
int lk_tree(int n, int etype, double byteScale, void *Dbase, int method, int flags, orc_join *joins, int *final_n,
            double *final_d, int64_t *stats, int max_joins) {
	const int lim = max_joins > 0 ? max_joins : INT_MAX;
	const int neg = (flags & 2) != 0;
	Ltd D = {etype, byteScale, Dbase};
	int nj = 0;
	if(method < 3 || method > 6) return -1;
	double *sD = malloc((size_t) (n + 1) * sizeof(double)), *Q = malloc((size_t) (n + 1) * sizeof(double));
	int32_t *N = malloc((size_t) (n + 1) * sizeof(int32_t)), *P = malloc((size_t) (n + 1) * sizeof(int32_t));
	if(stats) stats[0] = stats[1] = 0;
	init_dmin(&D, n, sD, N, Q, P);   /* mn: nj.c:111 initSummaD, the same sD / N */
	if(method == 6) {
		/* nj.c:1560-1610 nj with minDist = initQ_MN */
		uint64_t pair;
		while(n != 2 && nj < lim && (pair = init_q_mn(&D, n, sD, N))) {
			const int j = (int) (pair & 0xFFFFFFFFu), i = (int) (pair >> 32);
			double Li, Lj;
			limb_length(&Li, &Lj, i, j, sD, N, ld(&D, tri(i) + j), neg);
			joins[nj].i = i; joins[nj].j = j; joins[nj].Li = Li; joins[nj].Lj = Lj; ++nj;
			update_d(&D, n, sD, N, i, j, Li, Lj);
			--n;
			pop_arrange(&D, n, i);
			sD[i] = sD[n];
			N[i] = N[n];
		}
	} else if(method == 4) {
		/* hclust.c:1671-1720 hclust with initDmin / minQ / updateCF / UPGMA_popArrange */
		while(n != 2 && nj < lim) {
			const int i = min_q_row(Q, n), j = P[i];
			if(i == 0 && j == 0) break;
			double Li, Lj;
			limb_length(&Li, &Lj, i, j, sD, N, ld(&D, tri(i) + j), neg);
			joins[nj].i = i; joins[nj].j = j; joins[nj].Li = Li; joins[nj].Lj = Lj; ++nj;
			update_linkage(&D, n, sD, N, Q, P, i, j, 2);
			linkage_pop_arrange(&D, &n, sD, N, Q, P, i);
		}
	} else {
		/* dnj.c:985-1052 dnj with initDmin / minQ / UPGMApair / updateUPGMA or
		 * updateFF / UPGMA_popArrange / minPos */
		int hint = min_q_row(Q, n);
		uint64_t pos;
		while(n != 2 && nj < lim && (pos = upgma_pair(&D, n, Q, P, hint, stats))) {
			const int j = (int) (pos & 0xFFFFFFFFu), i = (int) (pos >> 32);
			double Li, Lj;
			limb_length(&Li, &Lj, i, j, sD, N, ld(&D, tri(i) + j), neg);
			joins[nj].i = i; joins[nj].j = j; joins[nj].Li = Li; joins[nj].Lj = Lj; ++nj;
			const int mi = update_linkage(&D, n, sD, N, Q, P, i, j, method == 3 ? 0 : 1);
			const int mj = linkage_pop_arrange(&D, &n, sD, N, Q, P, i);
			/* dnj.c:1026-1032 (D->n is already the new size) */
			if(mj == n) hint = mi;
			else if(mi == n) hint = mj;
			else hint = min_pos(Q, mi, mj);
		}
	}
	*final_n = n;
	*final_d = n == 2 ? ld(&D, 0) : -1.0;
	free(sD);
	free(Q);
	free(N);
	free(P);
	return nj;
}
