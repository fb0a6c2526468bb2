/*
 * tsv.c -- the dense table reader and the Phylip writer of `ccphylo tsv2phy`
 * (ref tsv.c:30 loadTsv, tsv2phy.c:64-108).
 *
 * loadTsv's rules: the first line is dropped as a header, and so is every
 * further line while the next one starts with '#'; the column count is 1 + the
 * separators of the last dropped line (a separator in its first byte is not
 * counted); every following line is one row of that many strtod numbers; an
 * entry of 32 or more bytes or with trailing bytes is malformatted; the input
 * must end with '\n'.  Not taken over: nan / inf entries are refused (a NaN's
 * sign differs between the reference's CPU and the GPU, so such a table has no
 * pinned result), and where the reference reads past a truncated row this
 * reader reports the end of file.
 */
#include <errno.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include "ccphylo_host.h"
#include "hostint.h"

int ccq_load_tsv(ccq_reader *r, char sep_, int vtype, void **X, int *m_out, int *n_out, char *msg, size_t msglen) {
	const int sep = (unsigned char) sep_;
	*X = NULL;
	*m_out = 0;
	*n_out = 0;
	if(msg && msglen) msg[0] = 0;
	if(vtype != 8 && vtype != 4) {
		if(msg) snprintf(msg, msglen, "ccq_load_tsv: vtype must be 8 or 4");
		return 1;
	}
	/* header, and the '#' lines after it */
	int N, c;
	do {
		N = 1;
		for(int first = 1;; first = 0) {
			if((c = ccq_getc(r)) == EOF) return 0;   /* zero rows */
			if(c == '\n') break;
			if(!first && c == sep) ++N;
		}
		if((c = ccq_peek(r)) == EOF) return 0;
	} while(c == '#');

	size_t cap = 1024, m = 0;
	char *mat = ccq_xmalloc(cap * (size_t) N * (size_t) vtype);
	char cell[33], *end;
	while(ccq_peek(r) != EOF) {
		if(m == cap) {
			cap <<= 1;
			mat = ccq_xrealloc(mat, cap * (size_t) N * (size_t) vtype);
		}
		for(int k = 0; k < N; ++k) {
			const int stop = k + 1 < N ? sep : '\n';
			int len = 0;
			while((c = ccq_getc(r)) != stop) {
				if(c == EOF) {
					if(msg) snprintf(msg, msglen, "Unexpected end of file");
					free(mat);
					return 1;
				}
				cell[len++] = (char) c;
				if(len == 32) {
					cell[32] = 0;
					if(msg) snprintf(msg, msglen, "Malformatted entry at pos:\t(%zu,%d) %s", m, k + 1, cell);
					free(mat);
					return 1;
				}
			}
			cell[len] = 0;
			double v = strtod(cell, &end);
			if(*end != 0) {
				if(msg) snprintf(msg, msglen, "Malformatted entry at pos:\t(%zu,%d) %s", m, k + 1, cell);
				free(mat);
				return 1;
			}
			if(vtype == 4) v = (double) (float) v;
			if(!isfinite(v)) {
				if(msg) snprintf(msg, msglen, "Non-finite entry at pos:\t(%zu,%d) %s: the GPU engine takes finite tables only",
				                 m, k + 1, cell);
				free(mat);
				return 1;
			}
			if(vtype == 8) ((double *) mat)[m * (size_t) N + (size_t) k] = v;
			else ((float *) mat)[m * (size_t) N + (size_t) k] = (float) v;
		}
		++m;
		if(m > 0x7fffffff) {
			if(msg) snprintf(msg, msglen, "ccq_load_tsv: too many rows");
			free(mat);
			return 1;
		}
	}
	*X = mat;
	*m_out = (int) m;
	*n_out = N;
	return 0;
}

/* tsv2phy.c:64-108: "%10d" of m, then per row its index ("\n%d" with format
 * bit 1, else "\n%-10d") and the cells "\t%.*g"; one '\n' closes the output */
void ccq_print_tsvphy(FILE *out, const void *D, int etype, int m, unsigned format, int precision) {
	fprintf(out, "%10d", m);
	int64_t f = 0;
	for(int i = 0; i < m; ++i) {
		fprintf(out, (format & 1) ? "\n%d" : "\n%-10d", i);
		for(int j = 0; j < i; ++j, ++f) {
			fprintf(out, "\t%.*g", precision, etype == 8 ? ((const double *) D)[f] : (double) ((const float *) D)[f]);
		}
	}
	fprintf(out, "%c", '\n');
}
