/*
 * nwck_parse.c -- the split list of a Newick line, and the closing of the
 * phycmp metrics.
 *
 * ccq_newick_splits restates getNwck, getSizeNwck, splitNwck, stripNwck and
 * getLimbNwck (ref nwck.c:157-359) and the driver loop of nwck2phy.c:96-161:
 * names[org] is split until it no longer splits, each split peeling the last
 * sub-node off into a new row.  The decisions are the reference's, with its
 * length bookkeeping: a peeled node is stored one byte short (nwck.c:329)
 * until getLimbNwck finds a ':' and cuts the node there.
 *
 * The reference walks a node's text backwards on every split (O(N * text) for
 * a caterpillar).  Here one forward pass records, for every byte boundary e,
 *   ps[e]   the last ',' or '(' before e at e's nesting level (groups between
 *           are skipped), the byte at which the backward walk from e stops,
 *   lev[e]  the nesting level at e, which tells a walk that runs out of the
 *           node balanced (stop == 0) from one that runs out inside a group,
 *   pc[e]   the last ':' before e,
 * so every walk is a table look-up and the whole line costs O(text + N).
 * The walks only ever cover bytes of the node, and the bytes the reference
 * overwrites with NUL lie on node borders, so the tables of the original
 * text answer for the edited one; strtod reads the edited copy.
 */
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include <errno.h>
#include "hostint.h"

typedef struct {
	int64_t seq, len;
} node_t;

typedef struct {
	unsigned char *buf;       /* the node text, edited as the reference edits it */
	int64_t *ps, *pc;
	int32_t *lev;
	char *err;
	size_t errlen;
} parse_t;

static int refuse(parse_t *P, const char *what, int64_t seq) {
	snprintf(P->err, P->errlen, "Undefined in the reference (%s) at node:\t%s", what, (char *) P->buf + seq);
	return -1;
}

/* the backward walk of splitNwck (nwck.c:311) over [s, e): the byte it stops
 * at with stop == 1, or -1 with *stop <= 0 when it runs out of the node */
static int64_t walk(const parse_t *P, int64_t s, int64_t e, int *stop) {
	const int64_t q = P->ps[e];
	if(q >= s) {
		*stop = 1;
		return q;
	}
	*stop = P->lev[e] - P->lev[s];   /* '(' minus ')' over the node: <= 0 here */
	return -1;
}

/* getLimbNwck (nwck.c:249); 0, 1 (invalid limb, message in err) or -1 (refused) */
static int limb(parse_t *P, node_t *nd, double *L) {
	int64_t len = nd->len;
	*L = -1.0;
	if(len == 0) return 0;
	if(P->buf[nd->seq + len - 1] == ')') return 0;
	/* `while(--len && *--seq != ':')` looks at bytes len - 2 .. 1 of the node; a
	 * node of one byte steps before its first byte */
	if(len == 1) return refuse(P, "limb search leaves the node", nd->seq);
	const int64_t c = P->pc[nd->seq + len - 1];   /* last ':' before byte len - 1 */
	if(c < nd->seq + 1) return 0;
	P->buf[c] = 0;
	nd->len = c - nd->seq;
	char *end;
	*L = strtod((char *) P->buf + c + 1, &end);
	if(*end) {
		snprintf(P->err, P->errlen, "Invalid limb length at node:\t%s", (char *) P->buf + nd->seq);
		return 1;
	}
	return 0;
}

/* splitNwck (nwck.c:296): *did = 1 with nj, Li, Lj set; return as limb() */
static int split(parse_t *P, node_t *ni, node_t *nj, double *Li, double *Lj, int *did) {
	*did = 0;
	for(;;) {
		if(!ni->len) return 0;
		int stop;
		int64_t q = walk(P, ni->seq, ni->seq + ni->len, &stop);
		if(q < 0 && stop == 0) {
			/* stripNwck */
			if(P->buf[ni->seq] == '(' && P->buf[ni->seq + ni->len - 1] == ')') {
				ni->len -= 2;
				++ni->seq;
				P->buf[ni->seq + ni->len] = 0;
				if(ni->len) continue;
			}
			return 0;
		}
		if(q < 0) return refuse(P, "unbalanced parentheses", ni->seq);
		P->buf[q] = 0;
		nj->len = ni->len - (q - ni->seq) - 2;
		nj->seq = q + 1;
		ni->len = q - ni->seq;
		if(nj->len < 0) return refuse(P, "empty last sub-node", ni->seq);
		(void) walk(P, ni->seq, q, &stop);
		int rc;
		if(stop != 0) {
			*Li = 0;
			if((rc = limb(P, nj, Lj))) return rc;
		} else {
			if((rc = limb(P, ni, Li))) return rc;
			if((rc = limb(P, nj, Lj))) return rc;
			if(*Lj < 0 && 0 <= *Li) *Lj = 0;
		}
		*did = 1;
		return 0;
	}
}

static void str_set(ccq_str *s, const char *p, size_t len) {
	if(!s) return;
	if(s->size < len + 1) {
		uint32_t size = s->size ? s->size : 1;
		while(size < len + 1) size <<= 1;
		s->seq = ccq_xrealloc(s->seq, size);
		s->size = size;
	}
	memcpy(s->seq, p, len);
	s->seq[len] = 0;
	s->len = (uint32_t) len;
}

int ccq_newick_splits(const char *line, size_t len, ccq_str *header, char ***names_out, ccq_split **splits_out,
                      int *n_out, char *err, size_t errlen) {
	char dummy[1];
	parse_t P = {0};
	P.err = err ? err : dummy;
	P.errlen = err ? errlen : 0;
	if(P.errlen) P.err[0] = 0;
	*names_out = NULL;
	*splits_out = NULL;
	*n_out = 0;
	/* getNwck: the header runs up to the first '(', the node from there to the last ')' */
	const char *open = memchr(line, '(', len);
	if(!open) {
		snprintf(P.err, P.errlen, "Undefined in the reference (no '(' in line)");
		return -1;
	}
	str_set(header, line, (size_t) (open - line));
	const char *body = open + 1;
	const int64_t blen = (int64_t) (len - (size_t) (body - line));
	int64_t L = blen;
	while(--L > 0 && body[L] != ')');
	if(L < 1) {
		snprintf(P.err, P.errlen, "Undefined in the reference (no node between '(' and ')')");
		return -1;
	}
	P.buf = ccq_xmalloc((size_t) blen + 1);
	memcpy(P.buf, body, (size_t) blen);
	P.buf[blen] = 0;
	P.buf[L] = 0;
	for(int64_t i = 0; i < L; ++i) {
		if(!P.buf[i]) P.buf[i] = ' ';   /* a NUL byte inside the node would end the reference's strings early */
	}
	/* the tables, over the boundaries 0 .. L */
	P.ps = ccq_xmalloc(((size_t) L + 1) * sizeof(int64_t));
	P.pc = ccq_xmalloc(((size_t) L + 1) * sizeof(int64_t));
	P.lev = ccq_xmalloc(((size_t) L + 1) * sizeof(int32_t));
	int64_t *stack = ccq_xmalloc(((size_t) L + 1) * sizeof(int64_t));
	int64_t sp = 0, cur = -1, colon = -1;
	int32_t lv = 0;
	int n = 1;
	for(int64_t i = 0; i <= L; ++i) {
		P.ps[i] = cur;
		P.pc[i] = colon;
		P.lev[i] = lv;
		if(i == L) break;
		const unsigned char c = P.buf[i];
		if(c == ',') {
			cur = i;
			++n;
		} else if(c == '(') {
			stack[sp++] = cur;
			cur = i;
			++lv;
		} else if(c == ')') {
			cur = sp ? stack[--sp] : -1;   /* below the line's first level nothing was seen */
			--lv;
		} else if(c == ':') {
			colon = i;
		}
	}
	free(stack);
	node_t *nodes = ccq_xmalloc((size_t) n * sizeof(node_t));
	ccq_split *splits = ccq_xmalloc((size_t) n * sizeof(ccq_split));
	nodes[0].seq = 0;
	nodes[0].len = L;
	int m = 1, org = 0, rc = 0;
	while(m != n) {
		if(org >= m) {
			rc = refuse(&P, "more commas than nodes", nodes[m - 1].seq);
			break;
		}
		double Li = 0, Lj = 0;
		int did;
		if((rc = split(&P, &nodes[org], &nodes[m], &Li, &Lj, &did))) break;
		if(did) {
			splits[m - 1].org = org;
			splits[m - 1].Li = Li;
			splits[m - 1].Lj = Lj;
			++m;
		} else {
			++org;
		}
	}
	if(!rc) {
		char **names = ccq_xmalloc((size_t) n * sizeof(char *));
		for(int i = 0; i < n; ++i) {
			const char *p = (const char *) P.buf + nodes[i].seq;
			const size_t l = strlen(p);
			names[i] = ccq_xmalloc(l + 1);
			memcpy(names[i], p, l + 1);
		}
		*names_out = names;
		*splits_out = splits;
		*n_out = n;
	} else {
		free(splits);
	}
	free(nodes);
	free(P.buf);
	free(P.ps);
	free(P.pc);
	free(P.lev);
	return rc;
}

/* getNwck's framing (nwck.c:176, :205): everything up to the next '(' belongs
 * to the header, newlines included; the line ends at the first newline after it */
int ccq_read_nwck(ccq_reader *r, char **buf, size_t *cap, size_t *len) {
	int c, open = 0;
	size_t l = 0;
	while((c = ccq_getc(r)) != EOF) {
		if(open && c == '\n') {
			*len = l;
			return 1;
		}
		if(c == '(') open = 1;
		if(l + 1 > *cap) {
			*cap = *cap ? *cap << 1 : 1024;
			*buf = ccq_xrealloc(*buf, *cap);
		}
		(*buf)[l++] = (char) c;
	}
	*len = 0;
	return 0;
}

void ccq_newick_splits_free(char **names, ccq_split *splits, int n) {
	if(names) {
		for(int i = 0; i < n; ++i) free(names[i]);
	}
	free(names);
	free(splits);
}

/* phycmp.c:111-138 with distcmp.c's closing expressions */
double ccq_cmp_metric(const ccg_cmp_sums *s, int64_t cells, int which) {
	double d;
	switch(which) {
		case 0:   /* cos (distcmp.c:426) */
			if(!s->aa || !s->bb) return -1;
			d = 1 - s->ab / sqrt(s->aa * s->bb);
			return d < 0 ? 0 : d;
		case 1: return sqrt(s->chi2);
		case 2:   /* bc (:308) */
			d = 1 - 2 * s->mn / s->apb;
			return d < 0 ? 0 : d;
		case 3: return s->l1;
		case 4: return sqrt(s->l2);
		case 5: return s->linf;
		case 6: {   /* p (:539) */
			const long n = (long) cells;
			const double v11 = s->aa - s->a * s->a / n, v12 = s->ab - s->a * s->b / n, v22 = s->bb - s->b * s->b / n;
			if(!v11 || !v22) return 0;
			return v12 / sqrt(v11 * v22);
		}
	}
	return NAN;
}

static const char *const cmp_names[7] = {"cos", "chi2", "bc", "l1", "l2", "linf", "p"};

void ccq_print_phycmp(FILE *out, const ccg_cmp_sums *s, int64_t cells, int flag) {
	for(int k = 0; k < 7; ++k) {
		if(flag & (1 << k)) fprintf(out, "%s:\t%f\n", cmp_names[k], ccq_cmp_metric(s, cells, k));
	}
}
