/*
 * motif.c -- `dist -y`: the methylation motif file, a scalar restatement of the
 * motif search on one packed row, and the held-back inclusion lines of a
 * pair-mode load (the all-taxa search itself is ccg_meth_mask on the GPU).
 *
 * ref: methparse.c:27 getMethBitTable, :84 strrcMeth, :103 FileBuffgetFsaMethSeq,
 * :180 qseq2methMotif, :254 getMethMotifs; meth.c:76 matchMotif, :122 maskMotif,
 * :141 maskMotifs; cdist.c:254 / :272 / :302 (where the masks are cleared).
 */
#include <stdlib.h>
#include <string.h>
#include "ccphylo_host.h"
#include "hostint.h"

/* IUPAC letter -> 4-bit set (A 1, C 2, G 4, T/U 8), +16 for an uppercase
 * letter (a methylation site); 0 for every byte the parser drops */
static int motif_code(int c) {
	static const char low[] = "acgturyswkmbdhvxn";
	static const unsigned char set[] = {1, 2, 4, 8, 8, 5, 10, 6, 9, 12, 3, 14, 13, 11, 7, 15, 15};
	for(int k = 0; low[k]; ++k) {
		if(c == low[k]) return set[k];
		if(c == low[k] - 32) return set[k] | 16;
	}
	return 0;
}

/* the complement of a set (A <-> T, C <-> G), the site bit kept */
static unsigned char motif_comp(unsigned char c) {
	return (unsigned char) ((c & 16) | ((c & 1) << 3) | ((c & 2) << 1) | ((c & 4) >> 1) | ((c & 8) >> 3));
}

/* strrcMeth, literally: len / 2 pairs are swapped and complemented from the
 * two ends inward; an odd length then complements the last left element it
 * wrote once more -- not the middle one, which stays as written */
static void motif_strrc(unsigned char *q, int len) {
	for(int i = 0; i < len / 2; ++i) {
		const unsigned char carry = motif_comp(q[i]);
		q[i] = motif_comp(q[len - 1 - i]);
		q[len - 1 - i] = carry;
	}
	if(len & 1) q[len / 2 - 1] = motif_comp(q[len / 2 - 1]);   /* len >= 3 here */
}

static void motif_set(ccq_motif *m, const unsigned char *q, int len) {
	memset(m, 0, sizeof(*m));
	m->len = len;
	for(int k = 0; k < len; ++k) {
		m->allow[k] = q[k] & 15;
		if(q[k] & 16) m->meth |= 0x80000000u >> k;
	}
}

int ccq_load_motifs(const char *path, ccq_motif **motifs, int *n, char *err, size_t errlen) {
	*motifs = NULL;
	*n = 0;
	if(errlen) err[0] = 0;
	ccq_reader *r = ccq_open(path);
	if(!r) {
		snprintf(err, errlen, "cannot open the methylation motif file \"%s\"", path);
		return 1;
	}
	int cap = 8, rec = 0, c;
	ccq_motif *M = ccq_xmalloc(cap * sizeof(ccq_motif));
	while(ccq_peek(r) != EOF) {
		char name[96] = "";
		unsigned char q[32];
		int len = 0, widest = 0, h = 0;
		++rec;
		if(ccq_peek(r) == '>') {
			(void) ccq_getc(r);
			while((c = ccq_getc(r)) != EOF && c != '\n') {
				if(h + 1 < (int) sizeof(name) && c != '\r') name[h++] = (char) c;
			}
			name[h] = 0;
		}
		while((c = ccq_peek(r)) != EOF && c != '>') {
			++r->pos;
			const int code = motif_code(c);
			if(code) {
				if(len < 32) q[len] = (unsigned char) code;
				++len;
			}
		}
		const char *why = NULL;
		if(len == 0) why = "has no bases";
		else if(len == 1) why = "has one base; motifs of 2 to 32 bases are supported";
		else if(len > 32) why = "is longer than 32 bases; motifs of 2 to 32 bases are supported";
		for(int k = 0; !why && k < len; ++k) {
			const int wd = __builtin_popcount(q[k] & 15);
			if(wd > widest) widest = wd;
		}
		for(int k = 0; !why && k < len; ++k) {
			if((q[k] & 16) && __builtin_popcount(q[k] & 15) < widest)
				why = "marks a site (uppercase) on a base narrower than its widest degenerate base, "
				      "where the reference is undefined";
		}
		if(why) {
			snprintf(err, errlen, "methylation motif record %d (\"%s\") of \"%s\" %s", rec, name, path, why);
			free(M);
			ccq_close(r);
			return 1;
		}
		if(*n + 2 > cap) {
			cap <<= 1;
			M = ccq_xrealloc(M, cap * sizeof(ccq_motif));
		}
		motif_set(M + (*n)++, q, len);   /* as written, then strrcMeth of it (methparse.c:266-274) */
		motif_strrc(q, len);
		motif_set(M + (*n)++, q, len);
	}
	ccq_close(r);
	*motifs = M;
	return 0;
}

int64_t ccq_meth_clear_row(const uint64_t *seq, int len, const ccq_motif *motifs, int n, uint32_t *clear_words) {
	int64_t found = 0;
	memset(clear_words, 0, (size_t) (len / 32 + 1) * sizeof(uint32_t));
	for(int j = 0; j < n; ++j) {
		const ccq_motif *m = motifs + j;
		for(int p = 0; p + m->len <= len; ++p) {
			int k = 0;
			for(; k < m->len; ++k) {
				const int q = p + k;
				const unsigned code = (unsigned) (seq[q >> 5] >> (62 - 2 * (q & 31))) & 3u;
				if(!((m->allow[k] >> code) & 1)) break;
			}
			if(k < m->len) continue;
			++found;
			for(k = 0; k < m->len; ++k) {
				if(m->meth & (0x80000000u >> k)) clear_words[(p + k) >> 5] |= 0x80000000u >> ((p + k) & 31);
			}
		}
	}
	return found;
}

/* a pair-mode record of a motif load, in record order (ccq_msa.pend) */
void ccq_msa_pend_push(ccq_msa *M, char *name, int inc, int row) {
	if((M->npend & (M->npend + 1)) == 0) {   /* grows at 0, 1, 3, 7, ... entries */
		M->pend = ccq_xrealloc(M->pend, (size_t) (2 * M->npend + 2) * sizeof(ccq_pend));
	}
	ccq_pend *p = M->pend + M->npend++;
	p->name = name;
	p->inc = inc;
	p->row = row;
}

int ccq_meth_masked_npos(const uint64_t *seq, const uint32_t *inc, int len, const ccq_motif *motifs, int n) {
	const int W = len / 32 + 1;
	uint32_t *clr = ccq_xmalloc((size_t) W * sizeof(uint32_t));
	ccq_meth_clear_row(seq, len, motifs, n, clr);
	int c = 0;
	for(int w = 0; w < (len + 31) / 32; ++w) c += __builtin_popcount(inc[w] & ~clr[w]);
	free(clr);
	return c;
}

void ccq_msa_meth_finish(ccq_msa *M, const int32_t *inc_count, FILE *log) {
	if(!M->pair || !M->npend) return;
	unsigned char *keep = ccq_xmalloc((size_t) (M->n > 0 ? M->n : 1));
	memset(keep, 1, (size_t) (M->n > 0 ? M->n : 1));
	for(int e = 0; e < M->npend; ++e) {
		ccq_pend *p = M->pend + e;
		int inc = p->inc, in = 0;
		if(p->row >= 0) {
			inc = inc_count[p->row];
			in = keep[p->row] = (unsigned) inc >= M->minLength;
		}
		fprintf(log, in ? "# Included:\t%s\t( %d / %d )\n" : "# Excluded:\t%s\t( %d / %d )\n", p->name, inc, M->len);
		free(p->name);
	}
	int out = 0;
	const size_t W = (size_t) M->W;
	for(int t = 0; t < M->n; ++t) {
		if(!keep[t]) {
			free(M->headers[t]);
			continue;
		}
		if(out != t) {
			M->headers[out] = M->headers[t];
			memmove(M->seqs + out * W, M->seqs + t * W, W * sizeof(uint64_t));
			memmove(M->incs + out * W, M->incs + t * W, W * sizeof(uint32_t));
		}
		++out;
	}
	M->n = out;
	free(keep);
	free(M->pend);
	M->pend = NULL;
	M->npend = 0;
}
