/*
 * ccphylo_host.h -- host-side stable API surface of ccphylo_amd (plain C).
 *
 * These are the reference's I/O boundaries re-implemented (not copied) so
 * that `ccphylo dist` / `ccphylo tree` stay byte-compatible:
 *   - Phylip reader / writer            (ref phy.c:251 loadPhy, phy.c:59 printphy)
 *   - dbscan table writer               (ref dbscan.c:165 print_dbscan)
 *   - Newick builder, replayed from the join list produced on the GPU
 *                                       (ref nwck.c:35 formNode, :79 formLastNode,
 *                                        :114 formLastBiNode, str.c:51 byteshift)
 *   - FASTA / MSA loading, 2-bit packing and include masks
 *                                       (ref seqparse.c:28, qseqs.c:60, fsacmp.c:32-503,
 *                                        cdist.c:196 ltdMsaMatrix_get)
 * All compute on the hot path goes through include/ccphylo_amd.h.
 */
#ifndef CCPHYLO_HOST_H
#define CCPHYLO_HOST_H
#include <stdint.h>
#include <stdio.h>
#include "ccphylo_amd.h"   /* ccg_cmp_sums */

#ifdef __cplusplus
extern "C" {
#endif

/* growable byte string with the reference's capacity semantics (qseqs.h) */
typedef struct {
	uint32_t size;   /* capacity in bytes; drives Newick child order (nwck.c:45) */
	uint32_t len;
	unsigned char *seq;
} ccq_str;

ccq_str *ccq_new(uint32_t size);
void ccq_free(ccq_str *s);

/* ---- buffered, gzip-transparent reader (ref filebuff.c:52) ---- */
typedef struct ccq_reader ccq_reader;
ccq_reader *ccq_open(const char *path);          /* "-" = stdin; NULL on failure */
void ccq_close(ccq_reader *r);
int ccq_peek(ccq_reader *r);                      /* EOF at end */

/* ---- Phylip ---- */
/* A loaded matrix: packed LT, element type et (8/4/2/1), ByteScale bs. */
typedef struct {
	int n;
	int size;              /* allocated rows (matrix.h `size`) */
	int et;
	double bs;
	void *mat;             /* n(n-1)/2 elements of et bytes */
} ccq_ltd;

ccq_ltd *ccq_ltd_new(int size, int et, double bs);
void ccq_ltd_free(ccq_ltd *D);
void ccq_ltd_reserve(ccq_ltd *D, int size);
double ccq_ltd_get(const ccq_ltd *D, int64_t flat);
void ccq_ltd_set(ccq_ltd *D, int64_t flat, double v, double round);

/* Name table reused across matrices, as in tree.c:61-66 + phy.c:360-379. */
typedef struct {
	int cap;               /* entries allocated */
	ccq_str **names;
	ccq_str *header;       /* '#' comment line of the current matrix */
} ccq_names;

ccq_names *ccq_names_new(int n, uint32_t init_size);
void ccq_names_free(ccq_names *T);

/* Names 0..n-1 as `ccphylo dist | ccphylo tree` would hold them: the field
 * ccq_print_phy writes for names[i] under `format` (phy.c:59), stored the
 * way ccq_load_phy reads a row "field<sep>" (phy.c:360-379: byte by byte
 * with capacity doubling, trailing white space trimmed), so a Newick
 * replayed over them has that pipeline's child order (nwck.c:45 compares
 * capacities).  Used by the fused `dist --tree` path. */
void ccq_names_set(ccq_names *T, char **names, int n, unsigned format, char sep);

/* Loads the next matrix (phy.c:251 semantics).  Returns n (0 at EOF / on a
 * malformed file, with *err set), grows D and T as needed. */
int ccq_load_phy(ccq_reader *r, ccq_ltd *D, ccq_names *T, char sep, char quotes, int *err);

/* phy.c:59 printphy.  names[i] are C strings (may be modified by the quote
 * strip, as in the reference).  include may be NULL.  format bit 1 =
 * relaxed names, bit 4 = comment line; CCQ_PHY_KEEP_DIRS prints a name with
 * its directories (nwck2phy.c:424 sets noStripDir), which are cut otherwise. */
#define CCQ_PHY_KEEP_DIRS 0x100u
void ccq_print_phy(FILE *out, const ccq_ltd *D, char **names, const unsigned char *include,
                   const char *comment, unsigned format, int precision);

/* ---- dbscan ---- */
/* dbscan.c:165 print_dbscan, preceded by the "#header" line of dbscan.c:220
 * when header is not NULL and not empty: "## n nclust maxDist minN", the
 * column names, then name, neighbours and cluster of every sample. */
void ccq_print_dbscan(FILE *out, const char *header, char **names, const int32_t *N, const int32_t *C, int n,
                      int nclust, double maxDist, int minN);

/* ---- dense tables (tsv2phy) ---- */
/* tsv.c:30 loadTsv: drops the header line and the '#' lines after it, takes
 * the column count from the last dropped line, then reads every line as one
 * row of strtod numbers separated by `sep`.  On success returns 0 with *X a
 * malloc'ed m x n row-major array of double (vtype 8) or float (vtype 4, each
 * number rounded from its double as `-p` stores it); *m = 0 and *X = NULL for
 * an input without rows.  Otherwise returns the exit status the CLI ends with
 * (1) and the reason in msg: the reference's "Malformatted entry at pos:" (an
 * entry of 32 or more bytes, trailing bytes) and "Unexpected end of file" (no
 * final newline), and -- unlike the reference -- a nan / inf entry. */
int ccq_load_tsv(ccq_reader *r, char sep, int vtype, void **X, int *m, int *n, char *msg, size_t msglen);
/* tsv2phy.c:64-108: the Phylip text of a packed LT (etype 8 / 4) whose names
 * are the row indices 0 .. m-1; format bit 1 = relaxed names. */
void ccq_print_tsvphy(FILE *out, const void *D, int etype, int m, unsigned format, int precision);

/* ---- Newick replay (GPU join list -> tree string) ---- */
typedef struct {
	int32_t i, j;          /* rows joined (j < i) at the time of the join */
	double Li, Lj;
} ccq_join;

/* Applies formNode(names[j], names[i], Lj, Li) and the row exchange for
 * every join, then the closing node(s) (dnj.c:1024-1049 / nj.c:1581-1607).
 * n0 = taxa at start, final_n / final_d as returned by the engine.
 * flags: tree -f (1 = bifurcating root).  Result in T->names[0]. */
void ccq_replay_newick(ccq_names *T, int n0, const ccq_join *joins, int njoins,
                       int final_n, double final_d, int flags, int precision);
/* The same bytes by editing the strings join by join as nwck.c does (O(N^2)
 * bytes for caterpillar trees); ccq_replay_newick replays only capacities and
 * lengths, then writes the string once.  Kept for tests and comparison. */
void ccq_replay_newick_strings(ccq_names *T, int n0, const ccq_join *joins, int njoins,
                               int final_n, double final_d, int flags, int precision);
/* tree.c:95-97: a two-taxon matrix */
void ccq_newick_pair(ccq_names *T, double d, int precision);

/* ---- Newick -> split list (`nwck2phy`) ---- */
/* Split s creates row s + 1 from row org: the last sub-node of names[org] is
 * peeled off with limb Lj, the rest keeps the row with limb Li (layout of
 * ccg_split, include/ccphylo_amd.h). */
typedef struct {
	int32_t org;
	double Li, Lj;
} ccq_split;

/* getNwck / getSizeNwck / splitNwck / stripNwck / getLimbNwck (nwck.c:157-359)
 * under the driver loop of nwck2phy.c:96-161, in O(text + N): `line` holds one
 * input line without its newline, anything before the first '(' goes to
 * `header` (may be NULL).  On success returns 0 with *n leaves, their names in
 * row order as the reference prints them and *n - 1 splits, both malloc'ed
 * (ccq_newick_splits_free).  Decisions are the reference's, its length
 * bookkeeping included (a peeled node is kept one byte short until a ':' is
 * found in it).  Returns 1 with the reference's "Invalid limb length at
 * node:\t<text>" in err where it exits with that, and -1 with a message naming
 * the node where the reference is undefined: its limb search would leave the
 * node's bytes (a one-byte node without ')', e.g. the B of "(A:1,BB)"), a
 * node's parentheses do not balance, or commas outnumber the nodes. */
int ccq_newick_splits(const char *line, size_t len, ccq_str *header, char ***names, ccq_split **splits, int *n,
                      char *err, size_t errlen);
void ccq_newick_splits_free(char **names, ccq_split *splits, int n);
/* The next line of a Newick file for ccq_newick_splits, framed as getNwck
 * (nwck.c:157) frames it: the bytes up to the first '(' (earlier newlines
 * included) and on to the newline, without it, in *buf (realloc'ed; *cap its
 * size).  Returns 0 at the end of the input; a last line without a newline is
 * dropped, as in the reference. */
int ccq_read_nwck(ccq_reader *r, char **buf, size_t *cap, size_t *len);

/* ---- phycmp ---- */
/* Closes metric `which` (0 cos, 1 chi2, 2 bc, 3 l1, 4 l2, 5 linf, 6 p: the
 * bits of `phycmp -f`) from the sums of ccg_ltd_cmp over `cells` cells as
 * distcmp.c does: cos = 1 - ab / sqrt(aa bb), -1 at a zero norm, < 0 -> 0;
 * bc = 1 - 2 mn / apb, < 0 -> 0; chi2 and l2 take sqrt; p = (ab - a b / n) /
 * sqrt((aa - a a / n)(bb - b b / n)), 0 at a zero variance. */
double ccq_cmp_metric(const ccg_cmp_sums *s, int64_t cells, int which);
/* phycmp.c:111-138: "cos:\t%f" ... "p:\t%f" for the bits of flag, in that order */
void ccq_print_phycmp(FILE *out, const ccg_cmp_sums *s, int64_t cells, int flag);

/* ---- merge ---- */
/* The name -> union index map of `merge` (merge.c:33 syncMatrices): a name
 * gets the next index at its first appearance, and the union lists its names
 * in that order.  Correct at any size, where the reference's table can
 * register a name twice from the 127th name on (hashmapstrindex.c:30-48). */
typedef struct ccq_namemap ccq_namemap;
ccq_namemap *ccq_namemap_new(void);
void ccq_namemap_free(ccq_namemap *M);
/* the index of `name` (copied), new or known */
int ccq_namemap_add(ccq_namemap *M, const char *name);
int ccq_namemap_n(const ccq_namemap *M);
/* name i as stored (owned by the map); NULL outside 0 .. n-1 */
const char *ccq_namemap_name(const ccq_namemap *M, int i);
/* The index vector of one loaded matrix: idx[r] = the union index of
 * T->names[r], r < m, new names appended to the map.  Returns 0, or -1 with
 * *row_a < *row_b the two rows that carry one name (the reference would then
 * update a cell outside the LT); names before row_b stay registered. */
int ccq_merge_index(ccq_namemap *M, const ccq_names *T, int m, int32_t *idx, int *row_a, int *row_b);

/* ---- FASTA / MSA ---- */
void ccq_code_table(unsigned flag, unsigned char table[256]);
/* seqparse.c:28 FileBuffgetFsa: header (with '>') and codes (< 8 kept) */
int ccq_read_fasta(ccq_reader *r, ccq_str *header, ccq_str *seq, const unsigned char *table);
int ccq_pack(const unsigned char *codes, int len, uint64_t *out);
void ccq_init_inc(uint32_t *inc, int len);
void ccq_inc_update(uint32_t *inc, unsigned char *seq, unsigned char *ref, int len, unsigned proxi, int variant);
int ccq_npos(const uint32_t *inc, int len);

/* One strand of a methylation motif (`dist -y`), the layout of ccg_motif
 * (include/ccphylo_amd.h): allow[k] the 4-bit base set (A 1, C 2, G 4, T 8)
 * of base k, meth bit 31 - k set where base k is a methylation site. */
typedef struct {
	int32_t len;
	uint32_t meth;
	uint8_t allow[32];
} ccq_motif;

/* A record after the reference of a pair-mode motif load, in record order.
 * row >= 0: kept provisionally in that row, its line waiting for the count
 * after motif masking; row = -1: excluded at once, inc its final count. */
typedef struct ccq_pend {
	char *name;
	int inc, row;
} ccq_pend;

/* An MSA loaded per ltdMsaMatrix_get (cdist.c:196-333): included taxa only,
 * packed seqs (stride W = len/32 + 1 words) and mask(s). */
typedef struct {
	int n, len, W, pair;
	char **headers;
	uint64_t *seqs;        /* n * W */
	uint32_t *incs;        /* W (non-pair) or n * W (pair) */
	unsigned minLength;    /* after the minCov adjustment (cdist.c:289) */
	int npend;             /* a pair-mode motif load: the records whose line is held back */
	struct ccq_pend *pend;
} ccq_msa;

/* Reads every record; logs "# Included/# Excluded" to `log` like the
 * reference.  variant: 0, 8 or 32 (dist.c:802-806). */
ccq_msa *ccq_load_msa(ccq_reader *r, unsigned flag, unsigned minLength, double minCov,
                      unsigned proxi, FILE *log);
void ccq_msa_free(ccq_msa *M);
/* The same result as ccq_load_msa, the per-sequence work (codes, packing,
 * include masks) on `threads` host threads over windows of the input
 * (fasta_par.c); the Included/Excluded lines and the length-mismatch exit
 * come in record order as the reference prints them. */
ccq_msa *ccq_load_msa_par(ccq_reader *r, unsigned flag, unsigned minLength, double minCov, unsigned proxi, int threads,
                          FILE *log);

/* ---- methylation motifs (`dist -y`) ---- */
/* getMethMotifs (methparse.c:254): a FASTA file (gzip accepted) whose records'
 * IUPAC letters give one base set each -- an uppercase letter also marks a
 * methylation site -- every other byte dropped.  Each record yields two
 * entries: the motif as written, then strrcMeth of it (methparse.c:84: for an
 * odd length not the true reverse complement, reproduced as it is).  Returns 0
 * with *motifs malloc'ed (2 per record), or 1 with the reason, naming the
 * record, in err: an unreadable file, or a motif where the reference is
 * undefined -- no base, one base, more than 32, or a site on a base whose set
 * is narrower than the motif's widest set. */
int ccq_load_motifs(const char *path, ccq_motif **motifs, int *n, char *err, size_t errlen);
/* maskMotifs (meth.c:141) on one packed row, position by position: strand j
 * matches at start p, 0 <= p <= len - m, when the 2-bit code at p + k is in
 * allow[k] for all k (a code stored as 00 is `A`; matches may overlap).
 * clear_words (len / 32 + 1 words, overwritten) gets bit 31 - (pos % 32) of
 * word pos / 32 for every site of every match; returns the matches. */
int64_t ccq_meth_clear_row(const uint64_t *seq, int len, const ccq_motif *motifs, int n, uint32_t *clear_words);
/* ccq_load_msa / ccq_load_msa_par for `dist -y` (nmotifs = 0: exactly those).
 * The record that becomes the reference is masked here before its inclusion
 * test (cdist.c:302-305).  Non-pair mode is otherwise unchanged: the caller
 * clears the sites of all taxa from M->incs with ccg_meth_mask.  Pair mode
 * counts a record after masking (cdist.c:254-259): a record that fails before
 * masking is excluded at once, the others are kept provisionally and every
 * line after the reference's is held back in M->pend for ccq_msa_meth_finish. */
ccq_msa *ccq_load_msa_meth(ccq_reader *r, unsigned flag, unsigned minLength, double minCov, unsigned proxi,
                           const ccq_motif *motifs, int nmotifs, FILE *log);
ccq_msa *ccq_load_msa_par_meth(ccq_reader *r, unsigned flag, unsigned minLength, double minCov, unsigned proxi,
                               int threads, const ccq_motif *motifs, int nmotifs, FILE *log);
/* After ccg_meth_mask on a pair-mode motif load: inc_count[row] decides the
 * provisional rows (kept when >= M->minLength), the held-back lines go to
 * `log` in record order with the reference's bytes, and the rows are
 * compacted (M->n shrinks).  Does nothing for any other load. */
void ccq_msa_meth_finish(ccq_msa *M, const int32_t *inc_count, FILE *log);

/* Multi-file FASTA with -r (cdist.c:36 ltdFsaMatrix_get): entry `tmpl` of
 * every file; n = nfiles (every file keeps its slot), include[nfiles] the
 * inclusion flags.  NULL where the reference exits(1). */
ccq_msa *ccq_load_fsa_files(char **files, int nfiles, const char *tmpl, unsigned flag, unsigned minLength,
                            double minCov, unsigned proxi, unsigned char *include, FILE *log);

/* KMA count matrices (*.mat[.gz]) of template `tmpl` for ccg_kma_ltd
 * (ltdmatrixthrd.c:376 ltdMatrixThrd's inclusion rules; every file read once,
 * `threads` at a time).  Exclusions are logged like the reference. */
typedef struct {
	int nfiles, n;             /* files given, samples included */
	int status;                /* 0, or -3 when a file cannot be read */
	unsigned char *include;    /* per file */
	int *file_of;              /* included sample -> file index */
	int64_t stride1, stride2;  /* rows per sample in rec1 / rec2 */
	uint16_t *rec1, *rec2;     /* n x stride x 8 (see ccg_kma_args) */
	int32_t *len1, *len2;
} ccq_kma;
ccq_kma *ccq_load_kma(char **files, int nfiles, const char *tmpl, unsigned minDepth, unsigned minLength,
                      double minCov, int threads, FILE *log);
void ccq_kma_free(ccq_kma *K);

#ifdef __cplusplus
}
#endif
#endif
