/*
 * merge_names.c -- the name bookkeeping of `ccphylo merge` (ref merge.c:33
 * syncMatrices over hashmapstrindex.c): a name gets the next union index at
 * its first appearance, and the union lists the names in that order.
 *
 * The reference's table is only reliable up to 126 names (its insert computes
 * the bucket before the table grows and its grow leaves the new half
 * uncleared); this one is an open-addressing table over an insertion-ordered
 * name array and is correct at any size.
 */
#include <stdlib.h>
#include <string.h>
#include "hostint.h"

struct ccq_namemap {
	int n, cap;           /* names held; names allocated */
	char **names;         /* insertion order */
	uint64_t *hash;       /* of names[i] */
	int *seen_mat;        /* ccq_merge_index: the matrix that last used index i ... */
	int *seen_row;        /* ... and its row */
	int mats;             /* matrices indexed so far */
	size_t slots;         /* power of two, > 2 n */
	int *table;           /* index + 1, 0 = empty */
};

static uint64_t name_hash(const char *s) {   /* FNV-1a */
	uint64_t h = 1469598103934665603ull;
	for(; *s; ++s) {
		h = (h ^ (unsigned char) *s) * 1099511628211ull;
	}
	return h;
}

ccq_namemap *ccq_namemap_new(void) {
	ccq_namemap *M = ccq_xmalloc(sizeof(*M));
	memset(M, 0, sizeof(*M));
	M->cap = 64;
	M->names = ccq_xmalloc((size_t) M->cap * sizeof(char *));
	M->hash = ccq_xmalloc((size_t) M->cap * sizeof(uint64_t));
	M->seen_mat = ccq_xmalloc((size_t) M->cap * sizeof(int));
	M->seen_row = ccq_xmalloc((size_t) M->cap * sizeof(int));
	M->slots = 256;
	M->table = calloc(M->slots, sizeof(int));
	if(!M->table) {
		exit(12);
	}
	return M;
}

void ccq_namemap_free(ccq_namemap *M) {
	if(!M) {
		return;
	}
	for(int i = 0; i < M->n; ++i) {
		free(M->names[i]);
	}
	free(M->names);
	free(M->hash);
	free(M->seen_mat);
	free(M->seen_row);
	free(M->table);
	free(M);
}

static void table_put(ccq_namemap *M, int i) {
	size_t k = M->hash[i] & (M->slots - 1);
	while(M->table[k]) {
		k = (k + 1) & (M->slots - 1);
	}
	M->table[k] = i + 1;
}

int ccq_namemap_add(ccq_namemap *M, const char *name) {
	const uint64_t h = name_hash(name);
	for(size_t k = h & (M->slots - 1); M->table[k]; k = (k + 1) & (M->slots - 1)) {
		const int i = M->table[k] - 1;
		if(M->hash[i] == h && !strcmp(M->names[i], name)) {
			return i;
		}
	}
	if(M->n == M->cap) {
		M->cap *= 2;
		M->names = ccq_xrealloc(M->names, (size_t) M->cap * sizeof(char *));
		M->hash = ccq_xrealloc(M->hash, (size_t) M->cap * sizeof(uint64_t));
		M->seen_mat = ccq_xrealloc(M->seen_mat, (size_t) M->cap * sizeof(int));
		M->seen_row = ccq_xrealloc(M->seen_row, (size_t) M->cap * sizeof(int));
	}
	const int i = M->n++;
	const size_t len = strlen(name) + 1;
	M->names[i] = memcpy(ccq_xmalloc(len), name, len);
	M->hash[i] = h;
	M->seen_mat[i] = -1;
	M->seen_row[i] = 0;
	if((size_t) M->n * 2 >= M->slots) {   /* rebuilt whole: every slot of the new table is cleared */
		free(M->table);
		M->slots *= 2;
		M->table = calloc(M->slots, sizeof(int));
		if(!M->table) {
			exit(12);
		}
		for(int k = 0; k < i; ++k) {
			table_put(M, k);
		}
	}
	table_put(M, i);
	return i;
}

int ccq_namemap_n(const ccq_namemap *M) {
	return M->n;
}

const char *ccq_namemap_name(const ccq_namemap *M, int i) {
	return i >= 0 && i < M->n ? M->names[i] : NULL;
}

int ccq_merge_index(ccq_namemap *M, const ccq_names *T, int m, int32_t *idx, int *row_a, int *row_b) {
	const int mat = M->mats++;
	for(int r = 0; r < m; ++r) {
		const int i = ccq_namemap_add(M, (const char *) T->names[r]->seq);
		if(M->seen_mat[i] == mat) {
			*row_a = M->seen_row[i];
			*row_b = r;
			return -1;
		}
		M->seen_mat[i] = mat;
		M->seen_row[i] = r;
		idx[r] = i;
	}
	return 0;
}
