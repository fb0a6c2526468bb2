/*
 * main.c -- `ccphylo dist`, `tree`, `dbscan`, `tsv2phy`, `nwck2phy`, `phycmp` and `merge`, the stable
 * CLI surface, with the hot path on the GPU engine (include/ccphylo_amd.h).
 *
 * Mirrors ref main.c:99 (dispatch), dist.c:473 main_dist / :42 makeMatrix /
 * cdist.c:196 ltdMsaMatrix_get, and tree.c:146 main_tree / :37 formTree:
 * same options, same stdout bytes, same stderr progress lines.  Option forms
 * the GPU engine does not implement (-V, -y, -a, union inputs, the z / p /
 * np count-matrix metrics, the tree methods upgma and frank) are
 * refused with an error instead of being silently approximated.
 *
 * Every command is: a struct of its options with the defaults in its
 * initialiser, a table of option rows in help order, a cli_cmd descriptor, one
 * cli_parse (host/cliopt.c walks argv and prints `-h` from the same table),
 * the post-parse checks, the run.  What differs between commands' argument
 * handling -- message formats that mirror the reference's cmdline.c or the
 * command's own main_*, a bare `--`, one input or a list -- is descriptor data;
 * an oddity of one option (`merge -H` ends its short-option word) is a bit on
 * its row.
 *
 * Extra (not in the reference): `tree --fast_sums` uses a fixed-order
 * parallel row sum instead of the reference's serial one;
 * `--device N` selects the GPU; `tree --gpus G [--transport rccl|host]`
 * shards the matrix over G ranks (host/mgpu.c); `dist --tree FILE` runs
 * dist and the tree in HBM without the Phylip text (`-m`, `--gpus`,
 * `--transport`, `--fast_sums` as for tree); `dist --dbscan FILE
 * [--max_distance E] [--min_neighbors N]` clusters that LT in HBM the same way
 * (alone, or before --tree); `tsv2phy --tree FILE [--tree_method M]` hands
 * the table's LT to the tree in HBM, and writes the Phylip text only with -o;
 * `tree --phycmp FILE [--phycmp_flag F]` replays each tree's path lengths in
 * HBM and writes the `phycmp` lines of matrix against tree to FILE;
 * `phycmp --by_name` maps the second matrix's rows onto the first's by name;
 * `merge --tree FILE [--tree_method M]` hands the merged LT to the tree in HBM.
 */
#include <ctype.h>
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include "ccphylo_amd.h"
#include "ccphylo_host.h"
#include "mgpu.h"
#include "cliopt.h"

/* the descriptors' message formats: cmdline.c's, and tsv2phy.c's and merge.c's own */
#define UNKNOWN_CMDLINE "Unknown argument:\t\"%s\"\n"
#define UNKNOWN_OWN "Unknown argument or option: \"%s\"\n"
#define EXTRA_CMDLINE "Unexpected non-option argument(s).\n"
#define EXTRA_OWN "Too many non-option arguments handed.\n"

static void die_opt(const char *kind, const char *opt) {
	fprintf(stderr, "%s argument:\t\"%s\"\n", kind, opt);
	exit(1);
}

/* "-" is stdout */
static FILE *open_out(const char *name) {
	return (name[0] == '-' && name[1] == 0) ? stdout : fopen(name, "wb");
}

/* dist.c:74-84: the -n file; one stream where it names the -o file */
static FILE *open_nout(const char *noutname, const char *outname, FILE *out) {
	return strcmp(noutname, outname) ? open_out(noutname) : out;
}

/* the message of a failed open; the status is errno where the caller passes it on, else 1 */
static int errno_fail(int pass) {
	fprintf(stderr, "Error: %d (%s)\n", errno, strerror(errno));
	return (pass && errno) ? errno : 1;
}

/* the tree methods of this command line: `tree -m`, --tree_method of the fused pipelines, the -M listing */
static const struct {
	const char *name;
	int id;
	const char *text;
} tree_methods[] = {{"nj", CCG_TREE_NJ, "Neighbor-Joining"},     {"cf", CCG_TREE_CF, "K-means Closest First"},
                    {"ff", CCG_TREE_FF, "K-means Furthest First"}, {"mn", CCG_TREE_MN, "Minimum Neighbors"},
                    {"hnj", CCG_TREE_HNJ, "Heuristic Neighbor-Joining"}, {"dnj", CCG_TREE_DNJ, "Dynamic Neighbor-Joining"}};

static int tree_method_id(const char *name) {
	for(size_t k = 0; k < sizeof(tree_methods) / sizeof(tree_methods[0]); ++k) {
		if(!strcmp(name, tree_methods[k].name)) return tree_methods[k].id;
	}
	return -1;
}

static const cli_name transports[] = {{"rccl", CCQ_TRANSPORT_RCCL}, {"host", CCQ_TRANSPORT_HOST}, {NULL, 0}};

static ccg_ctx *open_gpu(int device) {
	ccg_ctx *ctx = NULL;
	int rc = ccg_init(device, &ctx);
	if(rc) {
		fprintf(stderr, "ccphylo_amd: cannot open GPU %d: %s\n", device, ccg_strerror(rc));
		exit(1);
	}
	return ctx;
}

/* ================================================================ tree */
typedef struct {
	const char *in, *outname, *method, *cmpname;
	int cmpflag, flag, precision, fast, device, stats, gpus, transport;
	cli_prec pr;   /* etype, byte scale */
	char sep, quotes;
} TreeOpts;

#define F(f) offsetof(TreeOpts, f)
static const cli_opt tree_opts[] = {
	{'i', "input", CLI_STR, F(in), 0, "Input file", "stdin"},
	{'o', "output", CLI_STR, F(outname), 0, "Output file", "stdout"},
	{'S', "separator", CLI_CHAR, F(sep), 0, "Separator", "\\t"},
	{'q', "quotes", CLI_CHAR, F(quotes), 0, "Quote taxa", "\\0"},
	{'x', "print_precision", CLI_INT, F(precision), 0, "Floating point print precision", "9"},
	{'m', "method", CLI_STR, F(method), 0, "Tree construction method.", "dnj"},
	{'M', "method_help", CLI_UNSET, F(method), 0, "Help on option \"-m\"", ""},
	{'f', "flag", CLI_INT, F(flag), 0, "Output flags", "0"},
	{'F', "flag_help", CLI_FLAG, F(flag), -1, "Help on option \"-f\"", ""},
	{'p', "float_precision", CLI_FLAG, F(pr.mark), 4, "Float precision on distance matrix", "False / double"},
	{'s', "short_precision", CLI_PREC, F(pr), 2, "Short precision on distance matrix", "False / double / 1e0"},
	{'b', "byte_precision", CLI_PREC, F(pr), 1, "Byte precision on distance matrix", "False / double / 1e0"},
	{'g', "free", CLI_IGNORE, 0, 0, "Gradually free up D", "False"},   /* host memory knobs: no effect on HBM */
	{'H', "mmap", CLI_IGNORE, 0, 0, "Allocate matrix on the disk", "False"},
	{'T', "tmp", CLI_DROP, 0, 0, "Set directory for temporary files", ""},
	{'t', "threads", CLI_DROP, 0, 1, "Number of threads", "1"},
	{'h', "help", CLI_HELP, 0, 0, "Shows this helpmessage", ""},
	{0, "gpus", CLI_INT, F(gpus), 0, "Shard the matrix over G GPUs (nj, dnj)", "off"},
	{0, "transport", CLI_ENUM, F(transport), 0, "rccl / host collectives for --gpus", "rccl", 0, transports},
	{0, "fast_sums", CLI_FLAG, F(fast), 1, "Parallel row sums (not the reference's)", "False"},
	{0, "phycmp", CLI_STR, F(cmpname), 0, "Compare each tree's path lengths with its matrix", "off"},
	{0, "phycmp_flag", CLI_INT, F(cmpflag), 0, "phycmp -f flags for --phycmp", "1"},
	{0, "device", CLI_INT, F(device), 0, "First GPU", "0"},
	{0, "stats", CLI_FLAG, F(stats), 1},
	{0}};
static const cli_cmd tree_cmd = {"#CCPhylo forms tree(s) in newick format given a set of phylip distance matrices.",
                                 tree_opts, UNKNOWN_CMDLINE, EXTRA_CMDLINE, 1, 0, F(in)};
#undef F

static int perm_by_name(char **names1, char **names2, int n, int32_t *perm, char *msg, size_t msglen);

/* tree --phycmp: how well the tree just written represents its matrix.  The
 * very string `nwck` is parsed as `nwck2phy` parses it, its splits are
 * replayed into W_dev (n(n-1)/2 cells, free by now), the rows are mapped onto
 * the matrix's by name, and A_dev -- the matrix as loaded -- is compared with
 * it as `phycmp --by_name matrix tree-matrix` does.  0, or 1 with a message. */
static int tree_phycmp(ccg_ctx *ctx, const TreeOpts *o, FILE *cmp, const char *nwck, char **taxa, int n,
                       const void *A_dev, void *W_dev) {
	const int et = o->pr.mark;
	char **leaves = NULL;
	ccq_split *splits = NULL;
	int nl = 0, rc;
	if(n < 2) {
		fprintf(stderr, "ccphylo_amd: tree --phycmp: a matrix of one entry has no distance to compare.\n");
		return 1;
	}
	const size_t errlen = strlen(nwck) + 128;   /* a message quotes the node, which may be most of the string */
	char *err = malloc(errlen);
	if((rc = ccq_newick_splits(nwck, strlen(nwck), NULL, &leaves, &splits, &nl, err, errlen))) {
		fprintf(stderr, rc > 0 ? "%s\n" : "ccphylo_amd: tree --phycmp: %s\n", err);
		free(err);
		return 1;
	}
	int32_t *perm = malloc((size_t) n * sizeof(int32_t));
	int bad = 0;
	if(nl != n) {
		fprintf(stderr, "ccphylo_amd: tree --phycmp: the tree has %d leaves for %d entries of the matrix.\n", nl, n);
		bad = 1;
	} else if(perm_by_name(taxa, leaves, n, perm, err, errlen)) {
		fprintf(stderr, "ccphylo_amd: tree --phycmp: the tree's leaves do not map one to one onto the matrix's entries: %s.\n", err);
		bad = 1;
	}
	if(!bad) {
		ccg_cmp_sums sums;
		if((rc = ccg_nwck_ltd_dev(ctx, (const ccg_split *) splits, n - 1, et, W_dev)) ||
		   (rc = ccg_ltd_cmp_dev(ctx, A_dev, W_dev, n, et, perm, &sums))) {
			fprintf(stderr, "ccphylo_amd: tree --phycmp failed: %s\n", ccg_strerror(rc));
			bad = 1;
		} else {
			ccq_print_phycmp(cmp, &sums, (int64_t) n * (n - 1) / 2, o->cmpflag);
			fflush(cmp);
		}
	}
	free(perm);
	free(err);
	ccq_newick_splits_free(leaves, splits, nl);
	return bad;
}

static int main_tree(int argc, char **argv) {
	TreeOpts o = {.in = "-", .outname = "-", .method = "dnj", .cmpflag = 1, .precision = 9,
	              .transport = CCQ_TRANSPORT_RCCL, .pr = {8, 1.0}, .sep = '\t'};
	int rc = cli_parse(&tree_cmd, argc, argv, &o);
	if(rc != CLI_GO) return rc;
	if(o.flag == -1) {
		fprintf(stdout, "# Format flags output, add them to combine them.\n");
		fprintf(stdout, "#\n");
		fprintf(stdout, "#   1:\tStrictly bifurcate the root\n");
		fprintf(stdout, "#   2:\tAllow negative branchlengths\n");
		fprintf(stdout, "#\n");
		return 0;
	}
	if(!o.method || !strcmp(o.method, "mh")) {
		fprintf(stdout, "# Tree construction methods:\n#\n");
		for(size_t k = 0; k < sizeof(tree_methods) / sizeof(tree_methods[0]); ++k) {
			fprintf(stdout, "# %-8s\t%s\n", tree_methods[k].name, tree_methods[k].text);
		}
		fprintf(stdout, "#\n");
		return 0;
	}
	const int m = tree_method_id(o.method);
	if(m < 0 && (!strcmp(o.method, "upgma") || !strcmp(o.method, "frank"))) {
		/* upgma: the engine has it (CCG_TREE_UPGMA, C ABI and Python); this command line does not offer it yet */
		fprintf(stderr, "ccphylo_amd: tree method \"%s\" is not implemented by this command line (nj, cf, ff, mn, hnj, dnj are).\n", o.method);
		return 1;
	}
	if(m < 0) die_opt("Invalid", "\"-m\"");
	const int et = o.pr.mark, gpus = o.gpus;
	const double bs = o.pr.scale;
	if((et == 2 || et == 1) && bs == 0) die_opt("Invalid", et == 2 ? "\"--short_precision\"" : "\"--byte_precision\"");
	if(gpus < 0) die_opt("Invalid", "\"--gpus\"");
	if(gpus && (m == CCG_TREE_CF || m == CCG_TREE_FF || m == CCG_TREE_MN)) {
		fprintf(stderr, "ccphylo_amd: --gpus with tree method \"%s\" is not supported: the sharded engine runs nj, dnj and hnj.\n", o.method);
		return 1;
	}
	if(o.cmpname && (gpus || et == 2 || et == 1)) {
		fprintf(stderr, "ccphylo_amd: tree --phycmp with %s is not implemented.\n", gpus ? "--gpus" : "short / byte precision (-s / -b)");
		return 1;
	}

	FILE *out = open_out(o.outname);
	if(!out) return errno_fail(1);
	ccq_reader *r = ccq_open(o.in);
	if(!r) return errno_fail(1);
	FILE *cmp = NULL;
	if(o.cmpname && !(cmp = fopen(o.cmpname, "wb"))) return errno_fail(1);
	ccg_ctx *ctx = NULL;
	ccq_ltd *D = ccq_ltd_new(32, et, bs);        /* tree.c:52 */
	ccq_names *T = ccq_names_new(32, 4);         /* tree.c:61-66 */
	int err = 0, n;
	/* --phycmp: the entries' names and a device copy of the matrix, taken before the tree consumes either */
	char **taxa = NULL;
	void *A_dev = NULL, *W_dev = NULL;
	ccg_join *joins = NULL;
	size_t jcap = 0;
	clock_t t0 = clock(), t1;
	while((n = ccq_load_phy(r, D, T, o.sep, o.quotes, &err)) > 0) {
		t1 = clock();
		fprintf(stderr, "# Total time used loading matrix: %.2f s.\n", (double) (t1 - t0) / 1000000);
		t0 = t1;
		if(cmp) {
			taxa = malloc((size_t) n * sizeof(char *));
			for(int i = 0; i < n; ++i) taxa[i] = strdup((char *) T->names[i]->seq);
			if(n >= 2) {
				if(!ctx) ctx = open_gpu(o.device);
				const size_t bytes = (size_t) n * (size_t) (n - 1) / 2 * (size_t) et;
				int mrc;
				if((mrc = ccg_malloc(ctx, &A_dev, bytes)) || (mrc = ccg_malloc(ctx, &W_dev, bytes)) ||
				   (mrc = ccg_memcpy_h2d(ctx, A_dev, D->mat, bytes)) || (mrc = ccg_memcpy_h2d(ctx, W_dev, D->mat, bytes))) {
					fprintf(stderr, "ccphylo_amd: tree --phycmp: no device copy of the matrix: %s\n", ccg_strerror(mrc));
					return 1;
				}
			}
		}
		if(n > 2) {
			if(jcap < (size_t) n) {
				jcap = n;
				joins = realloc(joins, jcap * sizeof(ccg_join));
			}
			ccg_tree_args ta = {n, et, bs, m, o.flag, !o.fast, 0, 0};
			int nj = 0, fn = 0;
			double fd = 0;
			int64_t st[12 + 2 * CCG_NKSTAT];
			memset(st, 0, sizeof(st));
			if(gpus) {
				/* one matrix over G ranks, one thread per rank (host/mgpu.c) */
				ccq_mgpu mc = {gpus, o.device, o.transport, -1};
				char emsg[320] = "";
				rc = ccq_mgpu_tree(&mc, D->mat, &ta, joins, &nj, &fn, &fd, emsg, sizeof(emsg));
				if(rc) {
					fprintf(stderr, "ccphylo_amd: sharded tree construction failed: %s\n", emsg);
					return 1;
				}
			} else {
				if(!ctx) ctx = open_gpu(o.device);
				rc = cmp ? ccg_tree_dev(ctx, &ta, W_dev, joins, &nj, &fn, &fd, st)
				         : ccg_tree(ctx, &ta, D->mat, joins, &nj, &fn, &fd, st);
			}
			if(rc) {
				fprintf(stderr, "ccphylo_amd: tree construction failed: %s\n", ccg_strerror(rc));
				return 1;
			}
			if(o.stats && !gpus) {
				fprintf(stderr, "# gpu: %d joins, %lld rows / %lld cells rescanned, %lld launches, %.3f ms\n", nj,
				        (long long) st[0], (long long) st[1], (long long) st[2], st[3] / 1000.0);
			}
			ccq_replay_newick(T, n, (const ccq_join *) joins, nj, fn, fd, o.flag, o.precision);
		} else if(n == 2) {
			ccq_newick_pair(T, ccq_ltd_get(D, 0), o.precision);
		}
		if(T->header->len) {
			fprintf(out, ">%s%s;\n", (char *) T->header->seq, (char *) T->names[0]->seq);
		} else {
			fprintf(out, "%s;\n", (char *) T->names[0]->seq);
		}
		t1 = clock();
		fprintf(stderr, "# Total time used Constructing tree: %.2f s.\n", (double) (t1 - t0) / 1000000);
		t0 = t1;
		if(cmp) {
			fflush(out);   /* the tree is written whatever the comparison says */
			const int bad = tree_phycmp(ctx, &o, cmp, (char *) T->names[0]->seq, taxa, n, A_dev, W_dev);
			for(int i = 0; i < n; ++i) free(taxa[i]);
			free(taxa);
			if(A_dev) ccg_free(ctx, A_dev);
			if(W_dev) ccg_free(ctx, W_dev);
			A_dev = W_dev = NULL;
			if(bad) {
				err = 1;
				break;
			}
		}
	}
	if(out != stdout) fclose(out);
	else fflush(stdout);
	if(cmp) fclose(cmp);
	ccq_close(r);
	ccq_ltd_free(D);
	ccq_names_free(T);
	free(joins);
	if(ctx) ccg_destroy(ctx);
	return err ? 1 : 0;
}

/* ============================================================== dbscan */
typedef struct {
	const char *in, *outname;
	int device, minN;
	cli_prec pr;   /* etype, byte scale */
	char sep, quotes;
	double maxDist;
} DbscanOpts;

#define F(f) offsetof(DbscanOpts, f)
static const cli_opt dbscan_opts[] = {
	{'i', "input", CLI_STR, F(in), 0, "Input file", "stdin"},
	{'o', "output", CLI_STR, F(outname), 0, "Output file", "stdout"},
	{'S', "separator", CLI_CHAR, F(sep), 0, "Separator", "\\t"},
	{'q', "quotes", CLI_CHAR, F(quotes), 0, "Quote taxa", "\\0"},
	{'N', "min_neighbors", CLI_INT, F(minN), 0, "Minimum neighbors", "1"},
	{'e', "max_distance", CLI_DBL, F(maxDist), 0, "Maximum distance", "10.0"},
	{'p', "float_precision", CLI_FLAG, F(pr.mark), 4, "Float precision on distance matrix", "double"},
	{'s', "short_precision", CLI_PREC, F(pr), 2, "Short precision on distance matrix", "double / 1e0"},
	{'b', "byte_precision", CLI_PREC, F(pr), 1, "Byte precision on distance matrix", "double / 1e0"},
	{'H', "mmap", CLI_IGNORE, 0, 0, "Allocate matrix on the disk", "False"},   /* host memory knob: no effect on HBM */
	{'T', "tmp", CLI_DROP, 0, 0, "Set directory for temporary files", ""},
	{'h', "help", CLI_HELP, 0, 0, "Shows this helpmessage", ""},
	{0, "device", CLI_INT, F(device), 0, "GPU", "0"},
	{0}};
static const cli_cmd dbscan_cmd = {"#CCPhylo make a DBSCAN given a set of phylip distance matrices.", dbscan_opts,
                                   UNKNOWN_CMDLINE, EXTRA_CMDLINE, 1, 0, F(in)};
#undef F

/* dbscan.c:267 main_dbscan / :181 make_dbscan: every matrix of the input
 * through ccg_dbscan, printed by ccq_print_dbscan */
static int main_dbscan(int argc, char **argv) {
	DbscanOpts o = {.in = "-", .outname = "-", .minN = 1, .pr = {8, 1.0}, .sep = '\t', .maxDist = 10.0};
	int rc = cli_parse(&dbscan_cmd, argc, argv, &o);
	if(rc != CLI_GO) return rc;
	const int et = o.pr.mark;
	const double bs = o.pr.scale;
	if((et == 2 || et == 1) && bs == 0) die_opt("Invalid", et == 2 ? "\"--short_precision\"" : "\"--byte_precision\"");
	FILE *out = open_out(o.outname);
	if(!out) return errno_fail(1);
	ccq_reader *r = ccq_open(o.in);
	if(!r) return errno_fail(1);
	ccg_ctx *ctx = NULL;
	ccq_ltd *D = ccq_ltd_new(32, et, bs);
	ccq_names *T = ccq_names_new(32, 4);
	int32_t *N = NULL;
	char **names = NULL;
	int err = 0, n, cap = 0;
	while((n = ccq_load_phy(r, D, T, o.sep, o.quotes, &err)) > 0) {
		if(cap < n) {
			cap = n;
			N = realloc(N, 2 * (size_t) cap * sizeof(int32_t));
			names = realloc(names, (size_t) cap * sizeof(char *));
		}
		if(!ctx) ctx = open_gpu(o.device);
		ccg_dbscan_args da = {n, et, bs, o.maxDist, o.minN};
		int nclust = 0;
		rc = ccg_dbscan(ctx, &da, D->mat, N, N + cap, &nclust, NULL);
		if(rc) {
			fprintf(stderr, "ccphylo_amd: dbscan failed: %s\n", ccg_strerror(rc));
			return 1;
		}
		for(int i = 0; i < n; ++i) names[i] = (char *) T->names[i]->seq;
		ccq_print_dbscan(out, T->header->len ? (char *) T->header->seq : NULL, names, N, N + cap, n, nclust,
		                 o.maxDist, o.minN);
	}
	if(out != stdout) fclose(out);
	else fflush(stdout);
	ccq_close(r);
	ccq_ltd_free(D);
	ccq_names_free(T);
	free(N);
	free(names);
	if(ctx) ccg_destroy(ctx);
	return err ? 1 : 0;
}

/* ================================================================ dist */
/* --tree_method of the fused pipelines (dist --tree, tsv2phy --tree) -> CCG_TREE_*; -1 with a message */
static int fused_tree_method(const char *tmethod) {
	const int m = tree_method_id(tmethod);
	if(m < 0) fprintf(stderr, "ccphylo_amd: --tree_method %s: the fused pipeline runs nj, cf, ff, mn, hnj and dnj.\n", tmethod);
	return m;
}

/* the tail of a fused run: the engine's joins replayed over the names T holds
 * (ccq_names_set), the Newick line written and the file closed */
typedef struct {
	const ccg_join *joins;
	int nj, fn;
	double fd;
} Joins;

static void fused_write_newick(FILE *tout, ccq_names *T, int n, const Joins *J, int tflag, int precision) {
	ccq_replay_newick(T, n, (const ccq_join *) J->joins, J->nj, J->fn, J->fd, tflag, precision);
	fprintf(tout, "%s;\n", (char *) T->names[0]->seq);
	if(tout != stdout) fclose(tout);
}

typedef struct {
	cli_list files;
	const char *outname, *noutname, *treename, *tmethod, *dbname, *unsup, *tmpl, *method, *methname;
	double maxDist, minCov;
	int minN, precision, device, gpus, transport, fast, tflag;
	unsigned flag, norm, minLength, proxi, minDepth, threads;
	cli_prec pr;   /* etype, byte scale */
} DistOpts;

#define F(f) offsetof(DistOpts, f)
static const cli_opt dist_opts[] = {
	{'i', "input", CLI_LIST, F(files), 0, "Input file(s)", "stdin"},
	{'o', "output", CLI_STR, F(outname), 0, "Output file", "stdout"},
	{'n', "nucleotide_numbers", CLI_STR, F(noutname), 0, "Output number of nucleotides included", "False/None"},
	{'x', "print_precision", CLI_INT, F(precision), 0, "Floating point print precision", "9"},
	{'y', "methylation_motifs", CLI_STR, F(methname), 0, "Mask methylation motifs from <file>", "False/None"},
	{'L', "min_len", CLI_INT, F(minLength), 0, "Minimum overlapping length", "1"},
	{'C', "min_cov", CLI_PCT, F(minCov), 0, "Minimum coverage", "50.0%"},
	{'W', "normalization_weight", CLI_INT, F(norm), 0, "Normalization weight", "0 / None"},
	{'P', "proximity", CLI_INT, F(proxi), 0, "Minimum proximity between SNPs", "0"},
	{'f', "flag", CLI_INT, F(flag), 0, "Output flags", "1"},
	{'F', "flag_help", CLI_FLAG, F(flag), -1, "Help on option \"-f\"", ""},
	{'p', "float_precision", CLI_FLAG, F(pr.mark), 4, "Float precision on distance matrix", "double"},
	{'s', "short_precision", CLI_PREC, F(pr), 2, "Short precision on distance matrix", "double / 1e0"},
	{'b', "byte_precision", CLI_PREC, F(pr), 1, "Byte precision on distance matrix", "double / 1e0"},
	{'t', "threads", CLI_INT, F(threads), 0, "Number of threads", "1"},
	{'h', "help", CLI_HELP, 0, 0, "Shows this helpmessage", ""},
	{0, "tree", CLI_STR, F(treename), 0, "Also build the tree in HBM, Newick to FILE", "off"},
	{0, "dbscan", CLI_STR, F(dbname), 0, "Also cluster in HBM, table to FILE", "off"},
	{0, "max_distance", CLI_DBL, F(maxDist), 0, "dbscan -e for --dbscan", "10.0"},
	{0, "min_neighbors", CLI_INT, F(minN), 0, "dbscan -N for --dbscan", "1"},
	{0, "tree_method", CLI_STR, F(tmethod), 0, "nj / cf / ff / mn / hnj / dnj for --tree", "dnj"},
	{0, "tree_flag", CLI_INT, F(tflag), 0, "tree -f flags for --tree", "0"},
	{0, "gpus", CLI_INT, F(gpus), 0, "Shard --tree over G GPUs", "1"},
	{0, "transport", CLI_ENUM, F(transport), 0, "rccl / host collectives for --gpus", "rccl", 0, transports},
	/* the reference's options that its help does not list either, and this engine's own */
	{'d', "distance", CLI_STR, F(method)},
	{'D', "distance_help", CLI_UNSET, F(method)},
	{'r', "reference", CLI_STR, F(tmpl)},
	{'E', "min_depth", CLI_UDBL, F(minDepth)},
	{'l', "significance_lvl", CLI_DROP},
	{'S', "separator", CLI_DROP},
	{'T', "tmp", CLI_DROP},
	{'H', "mmap", CLI_IGNORE},
	{'a', "add", CLI_UNSUP, F(unsup)},
	{'V', "nucleotide_variations", CLI_UNSUP, F(unsup)},
	{0, "device", CLI_INT, F(device)},
	{0, "fast_sums", CLI_FLAG, F(fast), 1},
	{0}};
/* a bare `--` is an unknown option here, and the trailing words are the input list (dist.c:565) */
static const cli_cmd dist_cmd = {"#CCPhylo dist calculates distances between samples based on overlaps between nucleotide count matrices created by e.g. KMA.",
                                 dist_opts, UNKNOWN_CMDLINE, NULL, 0, 1, F(files)};
#undef F

/* dist.c:736-790: -d name -> metric; z, p, np -> -1 (not on the GPU engine) */
static int kma_metric_id(const char *m, int *id, unsigned *lnorm) {
	static const struct {
		const char *name;
		int id;
	} tab[] = {{"cos", CCG_KMA_COS}, {"z", -1}, {"chi2", CCG_KMA_CHI2}, {"nchi2", CCG_KMA_NCHI2},
	           {"nc", CCG_KMA_NC}, {"c", CCG_KMA_C}, {"np", -1}, {"p", -1}, {"nbc", CCG_KMA_NBC},
	           {"bc", CCG_KMA_BC}, {"nl1", CCG_KMA_NL1}, {"nl2", CCG_KMA_NL2}, {"nlinf", CCG_KMA_NLINF},
	           {"l1", CCG_KMA_L1}, {"l2", CCG_KMA_L2}, {"linf", CCG_KMA_LINF}};
	for(size_t k = 0; k < sizeof(tab) / sizeof(tab[0]); ++k) {
		if(!strcmp(m, tab[k].name)) {
			*id = tab[k].id;
			return 0;
		}
	}
	char *e;
	if(m[0] == 'l') {
		*lnorm = (unsigned) strtoul(m + 1, &e, 10);
		*id = CCG_KMA_LN;
		return *e != 0;
	}
	if(!strncmp(m, "nl", 2)) {
		*lnorm = (unsigned) strtoul(m + 2, &e, 10);
		*id = CCG_KMA_NLN;
		return *e != 0;
	}
	return 1;
}

/* filebuff.c:26 fileExist: the format is the file's first raw byte */
static int first_byte(const char *path) {
	FILE *f = fopen(path, "rb");
	if(!f) return EOF;
	int c = fgetc(f);
	fclose(f);
	return c;
}

/* dist.c:138-180 with count matrices: ltdMatrixThrd's samples, cmpMats per
 * pair on the GPU (ccg_kma_ltd), printphy of D (and N) */
static int dist_kma(const DistOpts *o, int metric, unsigned lnorm) {
	const int et = o->pr.mark;
	const double bs = o->pr.scale;
	if(metric < 0) {
		fprintf(stderr, "ccphylo_amd: distance method is not implemented by the GPU engine (z, p, np).\n");
		return 1;
	}
	FILE *out = open_out(o->outname);
	if(!out) return errno_fail(0);
	FILE *nout = NULL;
	if(o->noutname && !(nout = open_nout(o->noutname, o->outname, out))) return errno_fail(0);
	ccq_kma *K = ccq_load_kma(o->files.v, o->files.n, o->tmpl, o->minDepth, o->minLength, o->minCov,
	                          o->threads > 16 ? (int) o->threads : 16, stderr);
	if(K->status) return 1;
	const int n = K->n;
	ccq_ltd *D = ccq_ltd_new(n > 1 ? n : 2, et, bs), *N = ccq_ltd_new(n > 1 ? n : 2, et, bs);
	D->n = N->n = 0;
	if(n > 1) {
		ccg_ctx *ctx = open_gpu(o->device);
		ccg_kma_args a;
		memset(&a, 0, sizeof(a));
		a.n = n;
		a.metric = metric;
		a.lnorm = lnorm;
		a.norm = o->norm;
		a.minDepth = o->minDepth;
		a.minLength = o->minLength;
		a.minCov = o->minCov;
		a.etype = et;
		a.byteScale = bs;
		a.stride1 = K->stride1;
		a.rec1 = K->rec1;
		a.len1 = K->len1;
		a.stride2 = K->stride2;
		a.rec2 = K->rec2;
		a.len2 = K->len2;
		int64_t fatal = -1;
		int rc = ccg_kma_ltd(ctx, &a, D->mat, N->mat, &fatal);
		ccg_destroy(ctx);
		if(rc) {
			fprintf(stderr, "ccphylo_amd: distance computation failed: %s\n", ccg_strerror(rc));
			return 1;
		}
		if(fatal >= 0) {
			int64_t i = 1;
			while((i + 1) * i / 2 <= fatal) ++i;
			const int64_t j = fatal - i * (i - 1) / 2;
			fprintf(stderr, "Template (\"%s\") did not exceed threshold for inclusion:\t%s\n", o->tmpl,
			        o->files.v[K->file_of[j]]);
			return 1;
		}
		if(et >= 4) {   /* cmpMatThrd's warning (it names files[row]) */
			for(int64_t i = 1, f = 0; i < n; ++i) {
				for(int64_t j = 0; j < i; ++j, ++f) {
					if(ccq_ltd_get(D, f) == -1.0) {
						fprintf(stderr, "No sufficient overlap between samples:\t%s\t%s\n", o->files.v[i],
						        o->files.v[K->file_of[j]]);
					}
				}
			}
		}
		D->n = N->n = n;
	}
	if(1 < D->n) {
		ccq_print_phy(out, D, o->files.v, K->include, o->tmpl, o->flag, o->precision);
		if(nout && 1 < N->n) ccq_print_phy(nout, N, o->files.v, K->include, o->tmpl, o->flag, o->precision);
	}
	if(out != stdout) fclose(out);
	else fflush(stdout);
	if(nout && nout != out && nout != stdout) fclose(nout);
	ccq_ltd_free(D);
	ccq_ltd_free(N);
	ccq_kma_free(K);
	return 0;
}

/* cmpFsaThrd's pair order over file indices (fsacmpthrd.c:192-218): the
 * skip condition is `&&`, so a pair with one excluded file is not skipped;
 * cells (pi, pj) get these pairs in turn */
static void fsa_cell_pairs(const unsigned char *include, int n, int64_t cells, int *pi_, int *pj_) {
	int first = 0;
	while(first < n && !include[first]) ++first;
	int si = first + 1, sj = 0;
	for(int64_t c = 0; c < cells; ++c) {
		int i = si, j = sj;
		while(!include[i] && !include[j]) {
			while(i < n && !include[i]) ++i;
			while(j < i && !include[j]) ++j;
			if(i == j) {
				++i;
				j = 0;
			}
		}
		pi_[c] = i;
		pj_[c] = j;
		si = i;
		sj = j + 1;
		if(si == sj) {
			++si;
			sj = 0;
		}
	}
}

/* dist.c:138-180 with FASTA files and -r: ltdFsaMatrix_get (cdist.c:36) */
static int dist_fsa_files(const DistOpts *o) {
	const int et = o->pr.mark;
	const double bs = o->pr.scale;
	FILE *out = open_out(o->outname);
	if(!out) return errno_fail(0);
	FILE *nout = o->noutname ? open_nout(o->noutname, o->outname, out) : NULL;
	unsigned char *include = calloc((size_t) o->files.n, 1);
	ccq_msa *M = ccq_load_fsa_files(o->files.v, o->files.n, o->tmpl, o->flag, o->minLength, o->minCov, o->proxi, include,
	                                stderr);
	if(!M) return 1;
	int Dn = 0;
	for(int f = 0; f < o->files.n; ++f) Dn += include[f] != 0;
	ccq_ltd *D = ccq_ltd_new(Dn > 1 ? Dn : 2, et, bs), *N = ccq_ltd_new(Dn > 1 ? Dn : 2, et, bs);
	D->n = N->n = 0;
	const int W = M->W;
	if(!Dn) {
		fprintf(stderr, "All sequences were trimmed away.\n");
	} else {
		ccg_ctx *ctx = open_gpu(o->device);
		ccg_snp_args sa;
		memset(&sa, 0, sizeof(sa));
		sa.len = M->len;
		sa.stride = W;
		sa.pair = M->pair;
		sa.norm = o->norm;
		sa.minLength = M->minLength;
		sa.proxi = M->pair ? o->proxi : 0;
		sa.etype = et;
		sa.byteScale = bs;
		int rc = CCG_OK;
		if(!M->pair) {
			fprintf(stderr, "# %d / %d bases included in distance matrix.\n", ccq_npos(M->incs, M->len), M->len);
		}
		if(M->pair || Dn == o->files.n) {
			/* pairs of included files in order (cmpairFsaThrd skips with `||`) */
			uint64_t *sq = malloc((size_t) Dn * W * 8);
			uint32_t *ic = malloc((size_t) (M->pair ? Dn : 1) * W * 4);
			for(int f = 0, r = 0; f < o->files.n; ++f) {
				if(!include[f]) continue;
				memcpy(sq + (size_t) r * W, M->seqs + (size_t) f * W, (size_t) W * 8);
				if(M->pair) memcpy(ic + (size_t) r * W, M->incs + (size_t) f * W, (size_t) W * 4);
				++r;
			}
			if(!M->pair) memcpy(ic, M->incs, (size_t) W * 4);
			sa.n = Dn;
			sa.seqs = sq;
			sa.incs = ic;
			if(Dn > 1) rc = ccg_snp_ltd(ctx, &sa, D->mat, (M->pair && nout) ? N->mat : NULL, NULL);
			free(sq);
			free(ic);
		} else if(Dn > 1) {
			/* all files, then the cells in cmpFsaThrd's quirky pair order */
			ccq_ltd *F = ccq_ltd_new(o->files.n, et, bs);
			sa.n = o->files.n;
			sa.seqs = M->seqs;
			sa.incs = M->incs;
			rc = ccg_snp_ltd(ctx, &sa, F->mat, NULL, NULL);
			const int64_t cells = (int64_t) Dn * (Dn - 1) / 2;
			int *pi_ = malloc((size_t) cells * sizeof(int)), *pj_ = malloc((size_t) cells * sizeof(int));
			fsa_cell_pairs(include, o->files.n, cells, pi_, pj_);
			for(int64_t c = 0; c < cells; ++c) {
				const int64_t src = (int64_t) pi_[c] * (pi_[c] - 1) / 2 + pj_[c];
				memcpy((char *) D->mat + c * et, (char *) F->mat + src * et, (size_t) et);
			}
			free(pi_);
			free(pj_);
			ccq_ltd_free(F);
		}
		ccg_destroy(ctx);
		if(rc) {
			fprintf(stderr, "ccphylo_amd: distance computation failed: %s\n", ccg_strerror(rc));
			return 1;
		}
		D->n = Dn;
		if(M->pair) N->n = Dn;
	}
	if(1 < D->n) {
		ccq_print_phy(out, D, o->files.v, include, o->tmpl, o->flag, o->precision);
		if(nout && 1 < N->n) ccq_print_phy(nout, N, o->files.v, include, o->tmpl, o->flag, o->precision);
	}
	if(out != stdout) fclose(out);
	else fflush(stdout);
	if(nout && nout != out && nout != stdout) fclose(nout);
	ccq_ltd_free(D);
	ccq_ltd_free(N);
	ccq_msa_free(M);
	free(include);
	return 0;
}

/* `dist -y FILE` (dist.c:127-132): the motif file, or exit(1) with the reason */
static int load_motifs_or_die(const char *path, ccq_motif **mo) {
	int n = 0;
	char err[512];
	if(ccq_load_motifs(path, mo, &n, err, sizeof(err))) {
		fprintf(stderr, "ccphylo_amd: -y: %s.\n", err);
		exit(1);
	}
	return n;
}

/* After a motif load: every included taxon's sites leave the include mask(s)
 * on the GPU (maskMotifs at cdist.c:254 / :272, ccg_meth_mask), then a
 * pair-mode load drops the records that fall below minLength and prints the
 * held-back lines.  The packed rows go up once more for the distances. */
static int apply_motifs(ccq_msa *M, const ccq_motif *mo, int nmo, int device) {
	if(!nmo) return 0;
	int32_t *cnt = NULL;
	if(M->n > 0) {
		ccg_ctx *ctx = open_gpu(device);
		ccg_meth_args ma;
		memset(&ma, 0, sizeof(ma));
		ma.n = M->n;
		ma.len = M->len;
		ma.stride = M->W;
		ma.seqs = M->seqs;
		ma.incs = M->incs;
		ma.pair = M->pair;
		ma.motifs = (const ccg_motif *) mo;
		ma.nmotifs = nmo;
		cnt = malloc((size_t) M->n * sizeof(int32_t));
		const int rc = ccg_meth_mask(ctx, &ma, cnt, NULL);
		ccg_destroy(ctx);
		if(rc) {
			fprintf(stderr, "ccphylo_amd: methylation motif masking failed: %s\n", ccg_strerror(rc));
			return 1;
		}
	}
	ccq_msa_meth_finish(M, cnt, stderr);
	free(cnt);
	return 0;
}

/* `dist --tree FILE`: the MSA's distances and the tree in HBM, without the
 * Phylip text (configs[4]: a 1e6-taxon matrix has no text form).  With
 * --gpus G > 1 the LT is written straight into the ranks' row bands
 * (ccg_snp_ltd_shard) and the sharded tree consumes it there; with one GPU
 * the single-GPU engine runs on the full LT.  The Newick equals `ccphylo
 * dist | ccphylo tree` for the same MSA: integer SNP counts print exactly,
 * -W normalised distances are rounded to -x digits as the text would round
 * them (ccg_round_decimal_dev), taxon names as that pipeline's reader holds
 * them (ccq_names_set). */
static int dist_tree(const DistOpts *o) {
	const int et = o->pr.mark;
	const double bs = o->pr.scale;
	const int m = fused_tree_method(o->tmethod);
	if(m < 0) return 1;
	if(o->gpus > 1 && (m == CCG_TREE_CF || m == CCG_TREE_FF || m == CCG_TREE_MN)) {
		fprintf(stderr, "ccphylo_amd: --gpus with --tree_method %s is not supported: the sharded engine runs nj, dnj and hnj.\n", o->tmethod);
		return 1;
	}
	if(o->treename && o->norm && (et == 2 || et == 1)) {
		/* the pipeline's text round trip of -W cells through dtouc is not restated */
		fprintf(stderr, "ccphylo_amd: -W with -s / -b and --tree: use `ccphylo dist ... | ccphylo tree`.\n");
		return 1;
	}
	if(o->dbname && o->gpus > 1) {
		fprintf(stderr, "ccphylo_amd: --gpus with --dbscan is not supported: the clustering runs on one GPU.\n");
		return 1;
	}
	if(o->dbname && (et == 2 || et == 1) && (o->norm || bs != 1.0)) {
		/* scaled or -W cells: the pipeline's text round trip through dtouc is not restated */
		fprintf(stderr, "ccphylo_amd: -s / -b with a scale or -W and --dbscan is not supported: use `ccphylo dist ... | ccphylo dbscan`.\n");
		return 1;
	}
	FILE *tout = NULL, *dout = NULL;
	if(o->treename) tout = open_out(o->treename);
	if(o->dbname) dout = open_out(o->dbname);
	if((o->treename && !tout) || (o->dbname && !dout)) return errno_fail(0);
	ccq_reader *r = ccq_open(o->files.n ? o->files.v[0] : "-");
	if(!r) return errno_fail(0);
	if(ccq_peek(r) != '>') {
		fprintf(stderr, "ccphylo_amd: --tree / --dbscan need an MSA (FASTA) input.\n");
		return 1;
	}
	ccq_motif *mo = NULL;
	const int nmo = o->methname ? load_motifs_or_die(o->methname, &mo) : 0;
	ccq_msa *M = ccq_load_msa_par_meth(r, o->flag, o->minLength, o->minCov, o->proxi,
	                                   o->threads > 16 ? (int) o->threads : 16, mo, nmo, stderr);
	ccq_close(r);
	if(apply_motifs(M, mo, nmo, o->device)) return 1;
	free(mo);
	const int n = M->n;
	if(o->treename && n < 3) {
		fprintf(stderr, "ccphylo_amd: --tree needs at least 3 included sequences (%d).\n", n);
		return 1;
	}
	if(n < 2) {   /* `dist` prints no matrix, `dbscan` no table */
		if(dout != stdout) fclose(dout);
		ccq_msa_free(M);
		return 0;
	}
	if(!M->pair) fprintf(stderr, "# %d / %d bases included in distance matrix.\n", ccq_npos(M->incs, M->len), M->len);
	ccg_snp_args sa;
	memset(&sa, 0, sizeof(sa));
	sa.n = n;
	sa.len = M->len;
	sa.stride = M->W;
	sa.seqs = M->seqs;
	sa.incs = M->incs;
	sa.pair = M->pair;   /* -f 2: per-taxon masks, fsacmpair per cell (and -P maskProxi) */
	sa.proxi = M->pair ? o->proxi : 0;
	sa.norm = o->norm;
	sa.minLength = M->minLength;
	sa.etype = et;
	sa.byteScale = bs;
	ccg_tree_args ta = {n, et, bs, m, o->tflag, !o->fast, 0, 0};
	ccg_join *joins = malloc((size_t) n * sizeof(ccg_join));
	ccg_dbscan_args da = {n, et, bs, o->maxDist, o->minN};
	int32_t *dbN = o->dbname ? malloc(2 * (size_t) n * sizeof(int32_t)) : NULL;
	int nclust = 0;
	int nj = 0, fn = 0, inc = 0;
	double fd = 0;
	/* -W distances are not integral: the Phylip text of `dist | tree` rounds
	 * them to -x digits, and so does this path (ccg_round_decimal_dev) */
	const int rp = o->norm ? o->precision : -1;
	char emsg[320] = "";
	clock_t t0 = clock();
	int rc;
	if(o->gpus <= 1) {
		/* one GPU: the full LT (the world-1 band layout) and the single-GPU
		 * engine, which also runs the missing-entry rules of updateD
		 * (nj.c:1021-1030) and -m hnj, exactly as `dist | tree` would */
		ccg_ctx *ctx = open_gpu(o->device);
		void *dD = NULL;
		const size_t lt = (size_t) n * (size_t) (n - 1) / 2 * (size_t) et;
		if((rc = ccg_malloc(ctx, &dD, lt))) snprintf(emsg, sizeof(emsg), "LT buffer: %s", ccg_strerror(rc));
		else if((rc = ccg_snp_ltd_shard(ctx, &sa, 0, 1, dD, &inc)))
			snprintf(emsg, sizeof(emsg), "ccg_snp_ltd_shard: %s", ccg_strerror(rc));
		else if(rp >= 0 && (rc = ccg_round_decimal_dev(ctx, dD, (int64_t) n * (n - 1) / 2, et, rp)))
			snprintf(emsg, sizeof(emsg), "ccg_round_decimal_dev: %s", ccg_strerror(rc));
		/* round, then cluster, then the tree: it consumes the buffer, ccg_dbscan_dev only reads it */
		else if(o->dbname && (rc = ccg_dbscan_dev(ctx, &da, dD, dbN, dbN + n, &nclust, NULL)))
			snprintf(emsg, sizeof(emsg), "ccg_dbscan_dev: %s", ccg_strerror(rc));
		else if(o->treename && (rc = ccg_tree_dev(ctx, &ta, dD, joins, &nj, &fn, &fd, NULL)))
			snprintf(emsg, sizeof(emsg), "ccg_tree_dev: %s", ccg_strerror(rc));
		if(dD) ccg_free(ctx, dD);
		ccg_destroy(ctx);
	} else {
		ccq_mgpu mc = {o->gpus, o->device, o->transport, rp};
		rc = ccq_mgpu_dist_tree(&mc, &sa, &ta, joins, &nj, &fn, &fd, &inc, emsg, sizeof(emsg));
		if(rc == CCG_EUNSUP)
			fprintf(stderr, "ccphylo_amd: the matrix has missing entries (pairs below the minimum length); "
			                "their updateD rules run on one GPU: use --gpus 1.\n");
	}
	if(rc) {
		fprintf(stderr, "ccphylo_amd: dist --%s failed: %s\n", o->treename ? "tree" : "dbscan", emsg);
		return 1;
	}
	fprintf(stderr, "# Total time used computing distances and %s: %.2f s.\n", o->treename ? "tree" : "clusters",
	        (double) (clock() - t0) / 1000000);
	ccq_names *T = ccq_names_new(32, 4);   /* as tree.c:61-66 */
	ccq_names_set(T, M->headers, n, o->flag, '\t');
	if(o->dbname) {   /* before the replay, which edits the names */
		char **names = malloc((size_t) n * sizeof(char *));
		for(int i = 0; i < n; ++i) names[i] = (char *) T->names[i]->seq;
		ccq_print_dbscan(dout, NULL, names, dbN, dbN + n, n, nclust, o->maxDist, o->minN);
		free(names);
		if(dout != stdout) fclose(dout);
		free(dbN);
	}
	if(o->treename) fused_write_newick(tout, T, n, &(Joins){joins, nj, fn, fd}, o->tflag, o->precision);
	fflush(stdout);
	ccq_names_free(T);
	free(joins);
	ccq_msa_free(M);
	return 0;
}

/* one MSA: cdist.c:196 ltdMsaMatrix_get on the GPU (ccg_snp_ltd), printphy of D (and N) */
static int dist_msa(const DistOpts *o) {
	const int et = o->pr.mark;
	const double bs = o->pr.scale;
	FILE *out = open_out(o->outname);
	if(!out) return errno_fail(0);
	/* dist.c:74-84 opens (truncates) it; cdist.c:367 then prints N to outfile */
	FILE *nout = o->noutname ? open_nout(o->noutname, o->outname, out) : NULL;
	ccq_reader *r = ccq_open(o->files.n ? o->files.v[0] : "-");
	if(!r) return errno_fail(0);
	if(!(o->flag & 16) && ccq_peek(r) != '>') {
		fprintf(stderr, "ccphylo_amd: count-matrix (.mat) / union input is not implemented by the GPU engine.\n");
		return 1;
	}
	/* the per-sequence work on host threads (fasta_par.c; the same result as
	 * the serial ccq_load_msa) */
	ccq_motif *mo = NULL;
	const int nmo = o->methname ? load_motifs_or_die(o->methname, &mo) : 0;
	ccq_msa *M = ccq_load_msa_par_meth(r, o->flag, o->minLength, o->minCov, o->proxi,
	                                   o->threads > 16 ? (int) o->threads : 16, mo, nmo, stderr);
	ccq_close(r);
	if(apply_motifs(M, mo, nmo, o->device)) return 1;
	free(mo);
	int n = M->n;
	if(n * (n - 1) / 2 < 1) {
		fprintf(stderr, "Adjustning number of nodes to %d, to conform with the matrix size.\n", n * (n - 1) / 2);
	}
	ccq_ltd *D = ccq_ltd_new(n > 1 ? n : 2, et, bs), *N = NULL;
	if(!n) {
		fprintf(stderr, "All sequences were trimmed away.\n");
		D->n = 0;
	} else {
		if(o->noutname) N = ccq_ltd_new(n > 1 ? n : 2, et, bs);
		ccg_ctx *ctx = open_gpu(o->device);
		ccg_snp_args sa;
		memset(&sa, 0, sizeof(sa));
		sa.n = n;
		sa.len = M->len;
		sa.stride = M->W;
		sa.seqs = M->seqs;
		sa.incs = M->incs;
		sa.pair = M->pair;
		sa.norm = o->norm;
		sa.minLength = M->minLength;
		sa.proxi = M->pair ? o->proxi : 0;
		sa.etype = et;
		sa.byteScale = bs;
		int inc = 0;
		if(!M->pair) {
			inc = ccq_npos(M->incs, M->len);
			fprintf(stderr, "# %d / %d bases included in distance matrix.\n", inc, M->len);
		}
		int rc = ccg_snp_ltd(ctx, &sa, D->mat, N ? N->mat : NULL, NULL);
		if(rc) {
			fprintf(stderr, "ccphylo_amd: distance computation failed: %s\n", ccg_strerror(rc));
			return 1;
		}
		ccg_destroy(ctx);
		D->n = n;
		if(N) N->n = M->pair ? n : 0;
	}
	if(1 < D->n) {
		ccq_print_phy(out, D, M->headers, NULL, NULL, o->flag, o->precision);
		if(N && 1 < N->n) ccq_print_phy(out, N, M->headers, NULL, NULL, o->flag, o->precision);
	}
	if(out != stdout) fclose(out);
	else fflush(stdout);
	if(nout && nout != out && nout != stdout) fclose(nout);
	ccq_ltd_free(D);
	ccq_ltd_free(N);
	ccq_msa_free(M);
	return 0;
}

static int main_dist(int argc, char **argv) {
	DistOpts o = {.outname = "-", .tmethod = "dnj", .method = "cos", .maxDist = 10.0, .minCov = 0.5, .minN = 1,
	              .precision = 9, .transport = CCQ_TRANSPORT_RCCL, .flag = 1, .minLength = 1, .minDepth = 15,
	              .threads = 1, .pr = {8, 1.0}};
	const int rc = cli_parse(&dist_cmd, argc, argv, &o);
	if(rc != CLI_GO) return rc;
	if(o.minCov < 0 || 1 < o.minCov) die_opt("Invalid", "\"--min_cov\"");
	if(o.pr.scale == 0) die_opt("Invalid", o.pr.mark == 2 ? "\"--short_precision\"" : "\"--byte_precision\"");
	if(o.flag == (unsigned) -1) {
		fprintf(stdout, "# Format flags output, add them to combine them.\n");
		fprintf(stdout, "#\n");
		fprintf(stdout, "#   1:\tRelaxed Phylip\n");
		fprintf(stdout, "#   2:\tDistances are pairwise, always true on *.mat files\n");
		fprintf(stdout, "#   4:\tInclude template name in phylip file\n");
		fprintf(stdout, "#   8:\tInclude insignificant bases in distance calculation, only affects fasta input\n");
		fprintf(stdout, "#  16:\tDistances based on fasta input\n");
		fprintf(stdout, "#  32:\tDo not include insignificant bases in pruning\n");
		fprintf(stdout, "#\n");
		return 0;
	}
	if(!o.method) {
		fprintf(stdout, "# Distance calculation methods:\n");
		fprintf(stdout, "#\n");
		fprintf(stdout, "# cos:\tCalculate distance between positions as the angle between the count vectors.\n");
		fprintf(stdout, "# z:\tMake consensus comparison if vectors passes a McNemar test\n");
		fprintf(stdout, "# chi2:\tCalculate the chi square distance\n");
		fprintf(stdout, "# nchi2:\tCalculate the normalized chi square distance\n");
		fprintf(stdout, "# c:\tCalculate the Clausen distance between the count vectors. d(A,B) = (||A-B||_1 / sum(max{Ai, Bi}))\n");
		fprintf(stdout, "# nc:\tCalculate the normalized Clausen distance between the count vectors.\n");
		fprintf(stdout, "# bc:\tCalculate the Bray-Curtis dissimilarity between the count vectors.\n");
		fprintf(stdout, "# nbc:\tCalculate the normalized Bray-Curtis dissimilarity between the count vectors.\n");
		fprintf(stdout, "# ln:\tCalculate distance between positions as the n-norm distance between the count vectors. Replace \"n\" with the waned norm\n");
		fprintf(stdout, "# linf:\tCalculate distance between positions as the l_infinity distance between the count vectors.\n");
		fprintf(stdout, "# nln:\tCalculate distance between positions as the normalized n-norm distance between the count vectors. Replace last \"n\" with the waned norm\n");
		fprintf(stdout, "# nlinf:\tCalculate distance between positions as the normalized l_infinity distance between the count vectors.\n");
		fprintf(stdout, "#\n");
		return 0;
	}
	int metric;
	unsigned lnorm = 0;
	if(kma_metric_id(o.method, &metric, &lnorm)) die_opt("Invalid", "\"-d\"");
	if(o.unsup) {
		fprintf(stderr, "ccphylo_amd: dist option \"%s\" is not implemented by the GPU engine.\n", o.unsup);
		return 1;
	}
	if(o.methname && o.files.n > 1 && !(o.tmpl && !(o.flag & 16) && first_byte(o.files.v[0]) != '>')) {
		fprintf(stderr, "ccphylo_amd: -y with several FASTA files (-r) is not implemented by the GPU engine: use one MSA.\n");
		return 1;
	}
	if(o.tmpl && o.files.n > 1 && !(o.flag & 16) && first_byte(o.files.v[0]) != '>') {   /* dist.c:99-108: .mat input ignores -y */
		return dist_kma(&o, metric, lnorm);
	}
	if(o.tmpl && o.files.n > 1) return dist_fsa_files(&o);
	if(o.files.n > 1) {
		fprintf(stderr, "ccphylo_amd: multi-file dist input is not implemented by the GPU engine (use one MSA).\n");
		return 1;
	}
	return (o.treename || o.dbname) ? dist_tree(&o) : dist_msa(&o);
}

/* ============================================================= tsv2phy */
typedef struct {
	const char *in, *outname, *method, *treename, *tmethod;
	int flag, precision, vtype, device;
	cli_prec scaled;   /* -s / -b were given; their value is not used */
	char sep;
} TsvOpts;

#define F(f) offsetof(TsvOpts, f)
static const cli_opt tsv2phy_opts[] = {
	{'i', "input", CLI_STR, F(in), 0, "Input file", "stdin"},
	{'o', "output", CLI_STR, F(outname), 0, "Output file", "stdout"},
	{'S', "separator", CLI_CHAR, F(sep), 0, "Separator", "\\t"},
	{'x', "print_precision", CLI_INT, F(precision), 0, "Floating point print precision", "9"},
	{'d', "distance", CLI_STR, F(method), 0, "Distance method", "cos"},
	{'D', "distance_help", CLI_UNSET, F(method), 0, "Help on option \"-d\"", ""},
	{'f', "flag", CLI_INT, F(flag), 0, "Output flags", "1"},
	{'F', "flag_help", CLI_FLAG, F(flag), -1, "Help on option \"-f\"", ""},
	{'p', "float_precision", CLI_FLAG, F(vtype), 4, "Float precision on distance matrix", "False / double"},
	{'s', "short_precision", CLI_PREC, F(scaled), 1, "Short precision on distance matrix", "False / double / 1e0"},
	{'b', "byte_precision", CLI_PREC, F(scaled), 1, "Byte precision on distance matrix", "False / double / 1e0"},
	{'H', "mmap", CLI_IGNORE, 0, 0, "Allocate matrix on the disk", "False"},   /* host memory knob: no effect on HBM */
	{'T', "tmp", CLI_DROP, 0, 0, "Set directory for temporary files", ""},
	{'h', "help", CLI_HELP, 0, 0, "Shows this helpmessage", ""},
	{0, "tree", CLI_STR, F(treename)},
	{0, "tree_method", CLI_STR, F(tmethod)},
	{0, "device", CLI_INT, F(device)},
	{0}};
static const cli_cmd tsv2phy_cmd = {"#CCPhylo tsv2phy converts tsv files to phylip distance files.", tsv2phy_opts,
                                    UNKNOWN_OWN, EXTRA_OWN, 1, 0, F(in)};
#undef F

/* -d of tsv2phy (tsv2phy.c:316-357) -> CCG_VEC_* and the exponent of l<n>;
 * exits like the reference's invaArg where it refuses too */
static int tsv_metric_id(const char *method, double *exponent) {
	*exponent = 0;
	if(!strcmp(method, "cos")) return CCG_VEC_COS;
	if(!strcmp(method, "chi2")) return CCG_VEC_CHI2;
	if(!strcmp(method, "bc")) return CCG_VEC_BC;
	if(!strcmp(method, "l1")) return CCG_VEC_L1;
	if(!strcmp(method, "l2")) return CCG_VEC_L2;
	if(!strcmp(method, "linf")) return CCG_VEC_LINF;
	if(*method == 'l') {
		char *e;
		*exponent = strtod(method + 1, &e);
		if(*e != 0) {
			fprintf(stderr, "Invalid value parsed at %s.\n", "\"--distance ln\"");
			exit(1);
		}
		/* the reference takes "l", "l0" and "l-1" and prints pow(d, 1 / n) of them */
		if(!(*exponent > 0) || *exponent * 0 != 0) {
			fprintf(stderr, "ccphylo_amd: -d %s: the norm of l<n> must be finite and > 0.\n", method);
			exit(1);
		}
		return CCG_VEC_LN;
	}
	if(!strcmp(method, "p")) return CCG_VEC_PEARSON;
	fprintf(stderr, "Invalid value parsed at %s.\n", "\"--distance\"");
	exit(1);
}

/* tsv2phy.c:154 main_tsv2phy / :35 tsv2phy: the table goes up once, the cells
 * come from ccg_vec_ltd_dev and the LT stays in HBM: it is read back for the
 * Phylip text, and with --tree FILE handed to ccg_tree_dev in place */
static int main_tsv2phy(int argc, char **argv) {
	TsvOpts o = {.in = "-", .method = "cos", .tmethod = "dnj", .flag = 1, .precision = 9, .vtype = 8, .sep = '\t'};
	int rc = cli_parse(&tsv2phy_cmd, argc, argv, &o);
	if(rc != CLI_GO) return rc;
	if(o.flag == -1) {
		fprintf(stdout, "Format flags output format, add them to combine them.\n");
		fprintf(stdout, "#\n");
		fprintf(stdout, "# 1:\tRelaxed Phylip\n");
		fprintf(stdout, "#\n");
		return 0;
	}
	if(!o.method) {
		fprintf(stdout, "# Distance calculation methods:\n");
		fprintf(stdout, "#\n");
		fprintf(stdout, "# cos:\tCalculate cosine distance between vectors.\n");
		fprintf(stdout, "# chi2:\tCalculate the chi square distance\n");
		fprintf(stdout, "# bc:\tCalculate the Bray-Curtis dissimilarity between vectors.\n");
		fprintf(stdout, "# ln:\tCalculate distance between vectors as the n-norm distance between the count vectors. Replace \"n\" with the waned norm\n");
		fprintf(stdout, "# linf:\tCalculate distance between vectors as the l_infinity distance between the count vectors.\n");
		fprintf(stdout, "# p:\tCalculate Pearsons correlation between vectors.\n");
		fprintf(stdout, "#\n");
		return 0;
	}
	double exponent;
	const int metric = tsv_metric_id(o.method, &exponent);
	if(o.scaled.mark) {
		/* the reference's own short and byte rows are defective: tsv2phy.c:316-357
		 * never sets distcmp_s, so -s computes cos whatever -d says; bc -b prints
		 * all zeros and linf -b prints wrapped bytes (all three seen on a 7 x 5
		 * table).  There is nothing to be compatible with */
		fprintf(stderr, "ccphylo_amd: tsv2phy -s / -b is not supported: the reference's short and byte rows do not compute the chosen distance; use double or -p.\n");
		return 1;
	}
	const int tm = o.treename ? fused_tree_method(o.tmethod) : 0;
	if(tm < 0) return 1;
	ccq_reader *r = ccq_open(o.in);
	if(!r) return errno_fail(1);
	/* with --tree the Phylip text is written only where -o asks for it */
	if(!o.outname && !o.treename) o.outname = "-";
	FILE *out = NULL, *tout = NULL;
	if(o.outname) out = open_out(o.outname);
	if(o.treename) tout = open_out(o.treename);
	if((o.outname && !out) || (o.treename && !tout)) return errno_fail(1);
	void *X = NULL;
	int m = 0, n = 0;
	char msg[256];
	rc = ccq_load_tsv(r, o.sep, o.vtype, &X, &m, &n, msg, sizeof(msg));
	ccq_close(r);
	if(rc) {
		fprintf(stderr, "%s\n", msg);
		return rc;
	}
	if(!m) {
		fprintf(stderr, "Input matrix contained zero rows.\n");
		return 0;
	}
	if(o.treename && m < 3) {
		fprintf(stderr, "ccphylo_amd: --tree needs at least 3 rows (%d).\n", m);
		return 1;
	}
	const size_t cells = (size_t) m * (size_t) (m - 1) / 2;
	double *D = out ? malloc((cells ? cells : 1) * sizeof(double)) : NULL;
	ccg_join *joins = o.treename ? malloc((size_t) m * sizeof(ccg_join)) : NULL;
	if((out && !D) || (o.treename && !joins)) {
		fprintf(stderr, "Error: out of host memory\n");
		return 12;
	}
	int nj = 0, fn = 0;
	double fd = 0;
	if(m > 1) {   /* a one-row table has no cell: nothing to launch */
		ccg_ctx *ctx = open_gpu(o.device);
		void *dX = NULL, *dD = NULL;
		char emsg[320] = "";
		const size_t xb = (size_t) m * (size_t) n * (size_t) o.vtype;
		ccg_vec_args va = {m, n, n, o.vtype, NULL, metric, exponent, 8};
		ccg_tree_args ta = {m, 8, 1.0, tm, 0, 1, 0, 0};
		if((rc = ccg_malloc(ctx, &dX, xb)) || (rc = ccg_malloc(ctx, &dD, cells * sizeof(double))))
			snprintf(emsg, sizeof(emsg), "device buffers: %s", ccg_strerror(rc));
		else if((rc = ccg_memcpy_h2d(ctx, dX, X, xb))) snprintf(emsg, sizeof(emsg), "upload: %s", ccg_strerror(rc));
		else {
			va.X = dX;
			if((rc = ccg_vec_ltd_dev(ctx, &va, dD))) snprintf(emsg, sizeof(emsg), "ccg_vec_ltd_dev: %s", ccg_strerror(rc));
			else if(out && (rc = ccg_memcpy_d2h(ctx, D, dD, cells * sizeof(double))))
				snprintf(emsg, sizeof(emsg), "read back: %s", ccg_strerror(rc));
			/* the text first: the tree consumes the buffer */
			else if(o.treename && (rc = ccg_tree_dev(ctx, &ta, dD, joins, &nj, &fn, &fd, NULL)))
				snprintf(emsg, sizeof(emsg), "ccg_tree_dev: %s", ccg_strerror(rc));
		}
		if(dX) ccg_free(ctx, dX);
		if(dD) ccg_free(ctx, dD);
		ccg_destroy(ctx);
		if(rc) {
			fprintf(stderr, "ccphylo_amd: tsv2phy failed: %s\n", emsg);
			return 1;
		}
	}
	free(X);
	if(out) {
		ccq_print_tsvphy(out, D, 8, m, (unsigned) o.flag, o.precision);
		if(out != stdout) fclose(out);
		else fflush(stdout);
	}
	if(o.treename) {
		/* the names `tsv2phy | tree` would hold: the row indices as printed under -f */
		char **names = malloc((size_t) m * sizeof(char *));
		char *digits = malloc((size_t) m * 12);
		for(int i = 0; i < m; ++i) {
			names[i] = digits + (size_t) i * 12;
			snprintf(names[i], 12, "%d", i);
		}
		ccq_names *T = ccq_names_new(32, 4);   /* as tree.c:61-66 */
		ccq_names_set(T, names, m, (unsigned) o.flag, '\t');
		fused_write_newick(tout, T, m, &(Joins){joins, nj, fn, fd}, 0, o.precision);
		fflush(stdout);
		ccq_names_free(T);
		free(names);
		free(digits);
	}
	free(D);
	free(joins);
	return 0;
}

/* ============================================================ nwck2phy */
typedef struct {
	const char *in, *outname;
	int flag, precision, device;
	cli_prec pr;   /* etype; the scale is not used */
} NwckOpts;

#define F(f) offsetof(NwckOpts, f)
static const cli_opt nwck2phy_opts[] = {
	{'i', "input", CLI_STR, F(in), 0, "Input file", "stdin"},
	{'o', "output", CLI_STR, F(outname), 0, "Output file", "stdout"},
	{'x', "print_precision", CLI_INT, F(precision), 0, "Floating point print precision", "9"},
	{'f', "flag", CLI_INT, F(flag), 0, "Output flags", "1"},
	{'F', "flag_help", CLI_FLAG, F(flag), -1, "Help on option \"-f\"", ""},
	{'p', "float_precision", CLI_FLAG, F(pr.mark), 4, "Float precision on distance matrix", "False / double"},
	{'s', "short_precision", CLI_PREC, F(pr), 2, "Short precision on distance matrix", "False / double / 1e0"},
	{'b', "byte_precision", CLI_PREC, F(pr), 1, "Byte precision on distance matrix", "False / double / 1e0"},
	{'H', "mmap", CLI_IGNORE, 0, 0, "Allocate matrix on the disk", "False"},   /* host memory knob: no effect on HBM */
	{'T', "tmp", CLI_DROP, 0, 0, "Set directory for temporary files", ""},
	{'h', "help", CLI_HELP, 0, 0, "Shows this helpmessage", ""},
	{0, "device", CLI_INT, F(device), 0, "GPU", "0"},
	{0}};
static const cli_cmd nwck2phy_cmd = {"#CCPhylo nwck2phy converts newick files to phylip distance files.", nwck2phy_opts,
                                     UNKNOWN_CMDLINE, EXTRA_CMDLINE, 1, 0, F(in)};
#undef F

/* nwck2phy.c:33 newick2phy: every line's split list through ccg_nwck_ltd, printed by ccq_print_phy */
static int main_nwck2phy(int argc, char **argv) {
	NwckOpts o = {.in = "-", .outname = "-", .flag = 1, .precision = 9, .pr = {8, 1.0}};
	const int prc = cli_parse(&nwck2phy_cmd, argc, argv, &o);
	if(prc != CLI_GO) return prc;
	const int et = o.pr.mark;
	if(o.flag == -1) {
		fprintf(stdout, "Format flags output format, add them to combine them.\n");
		fprintf(stdout, "#\n");
		fprintf(stdout, "# 1:\tRelaxed Phylip\n");
		fprintf(stdout, "#\n");
		return 0;
	}
	if(et == 2 || et == 1) {
		/* the reference adds separately scaled and rounded encodings there (nwck2phy.c:245): not the path length */
		fprintf(stderr, "ccphylo_amd: nwck2phy with short / byte precision (-s / -b) is not implemented.\n");
		return 1;
	}
	FILE *out = open_out(o.outname);
	if(!out) return errno_fail(1);
	ccq_reader *r = ccq_open(o.in);
	if(!r) return errno_fail(1);
	ccg_ctx *ctx = NULL;
	ccq_ltd *D = ccq_ltd_new(128, et, 1.0);
	ccq_str *header = ccq_new(64);
	char *line = NULL, *err = NULL;
	size_t cap = 0, len;
	int status = 0;
	while(ccq_read_nwck(r, &line, &cap, &len)) {
		char **names = NULL;
		ccq_split *splits = NULL;
		int n = 0;
		err = realloc(err, len + 128);   /* a message quotes the node, which may be most of the line */
		const int rc = ccq_newick_splits(line, len, header, &names, &splits, &n, err, len + 128);
		if(rc) {
			/* rc 1: the reference's own exit and message; -1: where it is undefined */
			fprintf(stderr, rc > 0 ? "%s\n" : "ccphylo_amd: nwck2phy: %s\n", err);
			status = 1;
			break;
		}
		ccq_ltd_reserve(D, n);
		D->n = n;
		if(n > 1) {
			if(!ctx) ctx = open_gpu(o.device);
			const int grc = ccg_nwck_ltd(ctx, (const ccg_split *) splits, n - 1, et, D->mat);
			if(grc) {
				fprintf(stderr, "ccphylo_amd: nwck2phy failed: %s\n", ccg_strerror(grc));
				return 1;
			}
		}
		ccq_print_phy(out, D, names, NULL, (char *) header->seq, (unsigned) o.flag | CCQ_PHY_KEEP_DIRS, o.precision);
		fflush(out);
		ccq_newick_splits_free(names, splits, n);
	}
	if(out != stdout) fclose(out);
	else fflush(stdout);
	ccq_close(r);
	ccq_ltd_free(D);
	ccq_free(header);
	free(line);
	free(err);
	if(ctx) ccg_destroy(ctx);
	return status;
}

/* ============================================================== phycmp */
typedef struct {
	cli_list files;   /* none: stdin holds both matrices */
	const char *outname;
	int flag, device, by_name;
	cli_prec pr;      /* etype; the scale is not used */
	char sep;
} PhycmpOpts;

#define F(f) offsetof(PhycmpOpts, f)
static const cli_opt phycmp_opts[] = {
	{'i', "input", CLI_LIST, F(files), 0, "Input file(s)", "stdin", CLI_NEEDS_ONE},   /* cmdline.c:185, :216 */
	{'o', "output", CLI_STR, F(outname), 0, "Output file", "stdout"},
	{'S', "separator", CLI_CHAR, F(sep), 0, "Separator", "\\t"},
	{'f', "flag", CLI_INT, F(flag), 0, "Output flags", "1"},
	{'F', "flag_help", CLI_FLAG, F(flag), -1, "Help on option \"-f\"", ""},
	{'p', "float_precision", CLI_FLAG, F(pr.mark), 4, "Float precision on distance matrix", "False / double"},
	{'s', "short_precision", CLI_PREC, F(pr), 2, "Short precision on distance matrix", "False / double / 1e0"},
	{'b', "byte_precision", CLI_PREC, F(pr), 1, "Byte precision on distance matrix", "False / double / 1e0"},
	{'H', "mmap", CLI_IGNORE, 0, 0, "Allocate matrix on the disk", "False"},   /* host memory knob: no effect on HBM */
	{'T', "tmp", CLI_DROP, 0, 0, "Set directory for temporary files", ""},
	{'h', "help", CLI_HELP, 0, 0, "Shows this helpmessage", ""},
	{0, "by_name", CLI_FLAG, F(by_name), 1, "Match the second matrix's rows by name", "False"},
	{0, "device", CLI_INT, F(device), 0, "GPU", "0"},
	{0}};
/* non-options: the input files (phycmp.c:295) */
static const cli_cmd phycmp_cmd = {"# CCPhylo phycmp compares two distance matrices in phylip format.", phycmp_opts,
                                   UNKNOWN_CMDLINE, NULL, 1, 1, F(files)};
#undef F

typedef struct {
	const char *name;
	int row;
} name_row;

static int name_row_cmp(const void *a, const void *b) {
	return strcmp(((const name_row *) a)->name, ((const name_row *) b)->name);
}

/* perm[i] = the row of names2 called names1[i]; 0, or 1 with a message when
 * the two name sets differ or a name repeats */
static int perm_by_name(char **names1, char **names2, int n, int32_t *perm, char *msg, size_t msglen) {
	name_row *t = malloc((size_t) n * sizeof(name_row));
	int rc = 0;
	for(int i = 0; i < n; ++i) {
		t[i].name = names2[i];
		t[i].row = i;
	}
	qsort(t, (size_t) n, sizeof(name_row), name_row_cmp);
	for(int i = 1; i < n && !rc; ++i) {
		if(!strcmp(t[i - 1].name, t[i].name)) {
			snprintf(msg, msglen, "entry \"%s\" repeats", t[i].name);
			rc = 1;
		}
	}
	unsigned char *used = calloc((size_t) n, 1);
	for(int i = 0; i < n && !rc; ++i) {
		name_row key = {names1[i], 0};
		const name_row *hit = bsearch(&key, t, (size_t) n, sizeof(name_row), name_row_cmp);
		if(!hit) {
			snprintf(msg, msglen, "entry \"%s\" is in one matrix only", names1[i]);
			rc = 1;
		} else if(used[hit->row]) {
			snprintf(msg, msglen, "entry \"%s\" repeats", names1[i]);
			rc = 1;
		} else {
			used[hit->row] = 1;
			perm[i] = hit->row;
		}
	}
	free(used);
	free(t);
	return rc;
}

/* phycmp.c:176 main_phycmp / :56 phyfilecmp: two matrices, one pass of ccg_ltd_cmp */
static int main_phycmp(int argc, char **argv) {
	PhycmpOpts o = {.outname = "-", .flag = 1, .pr = {8, 1.0}, .sep = '\t'};
	const int prc = cli_parse(&phycmp_cmd, argc, argv, &o);
	if(prc != CLI_GO) return prc;
	const int et = o.pr.mark;
	if(o.flag == -1) {
		fprintf(stdout, "# Distance calculation methods:\n");
		fprintf(stdout, "#\n");
		fprintf(stdout, "# 1\tcos: Calculate cosine distance between vectors.\n");
		fprintf(stdout, "# 2\tchi2: Calculate the chi square distance\n");
		fprintf(stdout, "# 4\tbc: Calculate the Bray-Curtis dissimilarity between vectors.\n");
		fprintf(stdout, "# 8\tl1: Calculate distance between vectors as the 1-norm distance between the count vectors.\n");
		fprintf(stdout, "# 16\tl2: Calculate distance between vectors as the 2-norm distance between the count vectors.\n");
		fprintf(stdout, "# 32\tlinf: Calculate distance between vectors as the l_infinity distance between the count vectors.\n");
		fprintf(stdout, "# 64\tp: Calculate Pearsons correlation between vectors.\n");
		fprintf(stdout, "#\n");
		return 0;
	}
	if(et == 2 || et == 1) {
		fprintf(stderr, "ccphylo_amd: phycmp with short / byte precision (-s / -b) is not implemented.\n");
		return 1;
	}
	if(o.files.n > 2) {
		fprintf(stderr, "ccphylo_amd: phycmp takes two matrices: two files, or one file that holds both.\n");
		return 1;
	}
	FILE *out = open_out(o.outname);
	if(!out) return errno_fail(1);
	ccq_reader *r = ccq_open(o.files.n ? o.files.v[0] : "-");
	if(!r) return errno_fail(1);
	ccq_ltd *D1 = ccq_ltd_new(32, et, 1.0), *D2 = ccq_ltd_new(32, et, 1.0);
	ccq_names *T1 = ccq_names_new(32, 4), *T2 = ccq_names_new(32, 4);
	int err = 0;
	const int n1 = ccq_load_phy(r, D1, T1, o.sep, 0, &err);
	if(o.files.n == 2) {   /* else one file, or stdin, holds both */
		ccq_close(r);
		if(!(r = ccq_open(o.files.v[1]))) return errno_fail(1);
	}
	const int n2 = ccq_load_phy(r, D2, T2, o.sep, 0, &err);
	ccq_close(r);
	/* phycmp.c:96-105 */
	if(n1 <= 0 || n2 <= 0) {
		fprintf(stderr, "Missing matrix\n");
		return 1;
	} else if(n1 != n2) {
		fprintf(stderr, "Matrices differ in size.\n");
		return 1;
	}
	const int n = n1;
	char **nm1 = malloc((size_t) n * sizeof(char *)), **nm2 = malloc((size_t) n * sizeof(char *));
	for(int i = 0; i < n; ++i) {
		nm1[i] = (char *) T1->names[i]->seq;
		nm2[i] = (char *) T2->names[i]->seq;
	}
	int32_t *perm = NULL;
	if(o.by_name) {
		char msg[512];
		perm = malloc((size_t) n * sizeof(int32_t));
		if(perm_by_name(nm1, nm2, n, perm, msg, sizeof(msg))) {
			fprintf(stderr, "ccphylo_amd: phycmp --by_name: %s.\n", msg);
			return 1;
		}
	} else {
		for(int i = 0; i < n; ++i) {
			if(strcmp(nm1[i], nm2[i])) {
				fprintf(stderr, "Matrices has different entries.\n");
				return 1;
			}
		}
	}
	if(n < 2) {
		/* the reference reads the first cell of an empty buffer there */
		fprintf(stderr, "ccphylo_amd: phycmp: a matrix of one entry has no distance to compare.\n");
		return 1;
	}
	ccg_ctx *ctx = open_gpu(o.device);
	ccg_cmp_sums sums;
	const int rc = ccg_ltd_cmp(ctx, D1->mat, D2->mat, n, et, perm, &sums);
	if(rc) {
		fprintf(stderr, "ccphylo_amd: phycmp failed: %s\n", ccg_strerror(rc));
		return 1;
	}
	ccq_print_phycmp(out, &sums, (int64_t) n * (n - 1) / 2, o.flag);
	if(out != stdout) fclose(out);
	else fflush(stdout);
	free(nm1);
	free(nm2);
	free(perm);
	ccq_ltd_free(D1);
	ccq_ltd_free(D2);
	ccq_names_free(T1);
	ccq_names_free(T2);
	ccg_destroy(ctx);
	return 0;
}

/* =============================================================== merge */
typedef struct {
	const char *in, *outname, *wname, *nname, *treename, *tmethod;
	int flag, precision, et, device;
	cli_prec scaled;   /* -s / -b were given; their value is not used */
	char sep;
} MergeOpts;

#define F(f) offsetof(MergeOpts, f)
static const cli_opt merge_opts[] = {
	{'i', "input", CLI_STR, F(in), 0, "Input multi phylip distance file", "stdin"},
	{'o', "output", CLI_STR, F(outname), 0, "Output file", "stdout"},
	{'w', "nucleotides_weights", CLI_STR, F(wname), 0, "Weigh distance with this Phylip file", ""},
	{'n', "nucleotide_numbers", CLI_STR, F(nname), 0, "Output number of nucleotides included", "False/None"},
	{'S', "separator", CLI_CHAR, F(sep), 0, "Separator", "\\t"},
	{'x', "print_precision", CLI_INT, F(precision), 0, "Floating point print precision", "9"},
	{'f', "flag", CLI_INT, F(flag), 0, "Output flags", "1"},
	{'F', "flag_help", CLI_FLAG, F(flag), -1, "Help on option \"-f\"", ""},
	{'p', "float_precision", CLI_FLAG, F(et), 4, "Float precision on distance matrix", "double"},
	{'s', "short_precision", CLI_PREC, F(scaled), 1, "Short precision on distance matrix", "double / 1e0"},
	{'b', "byte_precision", CLI_PREC, F(scaled), 1, "Byte precision on distance matrix", "double / 1e0"},
	/* host memory knob: no effect on HBM.  -H ends its short-option word (-Hp does not reach p) */
	{'H', "mmap", CLI_IGNORE, 0, 0, "Allocate matrix on the disk", "False", CLI_ENDS_WORD},
	{'T', "tmp", CLI_DROP, 0, 0, "Set directory for temporary files", ""},
	{'h', "help", CLI_HELP, 0, 0, "Shows this helpmessage", ""},
	{0, "tree", CLI_STR, F(treename)},
	{0, "tree_method", CLI_STR, F(tmethod)},
	{0, "device", CLI_INT, F(device)},
	{0}};
static const cli_cmd merge_cmd = {"#CCPhylo merges matrices from a multi Phylip file into one matrix", merge_opts,
                                  UNKNOWN_OWN, EXTRA_OWN, 1, 0, F(in)};
#undef F

/* The union's accumulators in HBM and the batch being staged (merge.c:122 /
 * :309 on the engine): every parsed matrix goes to the device at once and
 * waits there until CCG_MERGE_MAX_SRC are staged or the input ends. */
typedef struct {
	ccg_ctx *ctx;
	int et;
	void *dD, *dN;       /* packed LTs of `cap` rows */
	int cap;
	ccg_merge_args a;    /* a.nsrc sources staged; a.n_prev the union's rows after the last batch */
	int32_t *idx[CCG_MERGE_MAX_SRC];
	double dev_ms;       /* device time of the batches and the close */
} MergeRun;

static int merge_fail(const char *what, int rc) {
	fprintf(stderr, "ccphylo_amd: merge failed: %s: %s\n", what, ccg_strerror(rc));
	return 1;
}

/* applies the staged batch to a union of n rows */
static int merge_flush(MergeRun *R, int n) {
	int rc;
	if(n > R->cap) {   /* capacity doubling; the packed prefix keeps its place (flat index i(i-1)/2 + j) */
		const int cap = n > 2 * R->cap ? n : 2 * R->cap;
		const size_t bytes = (size_t) cap * (size_t) (cap - 1) / 2 * (size_t) R->et;
		const size_t keep = (size_t) R->a.n_prev * (size_t) (R->a.n_prev ? R->a.n_prev - 1 : 0) / 2 * (size_t) R->et;
		void *nD = NULL, *nN = NULL;
		if((rc = ccg_malloc(R->ctx, &nD, bytes)) || (rc = ccg_malloc(R->ctx, &nN, bytes))) return merge_fail("union buffers", rc);
		if(keep && ((rc = ccg_memcpy_d2d(R->ctx, nD, R->dD, keep)) || (rc = ccg_memcpy_d2d(R->ctx, nN, R->dN, keep))))
			return merge_fail("union growth", rc);
		if(R->dD) ccg_free(R->ctx, R->dD);
		if(R->dN) ccg_free(R->ctx, R->dN);
		R->dD = nD;
		R->dN = nN;
		R->cap = cap;
	}
	if((rc = ccg_ltd_merge_dev(R->ctx, &R->a, R->dD, R->dN, n))) return merge_fail("ccg_ltd_merge_dev", rc);
	double ms = 0;
	ccg_last_merge_ms(R->ctx, &ms);
	R->dev_ms += ms;
	for(int s = 0; s < R->a.nsrc; ++s) {
		if(R->a.src[s].d) ccg_free(R->ctx, (void *) R->a.src[s].d);
		if(R->a.src[s].w) ccg_free(R->ctx, (void *) R->a.src[s].w);
		free(R->idx[s]);
	}
	R->a.nsrc = 0;
	R->a.first = 0;
	R->a.n_prev = n;
	return 0;
}

/* stages one parsed matrix (W NULL: unweighted); idx is taken over */
static int merge_stage(MergeRun *R, const ccq_ltd *D, const ccq_ltd *W, int32_t *idx, int first, int n_union) {
	const int s = R->a.nsrc++;
	ccg_merge_src *S = &R->a.src[s];
	const size_t bytes = (size_t) D->n * (size_t) (D->n - 1) / 2 * (size_t) R->et;
	int rc;
	memset(S, 0, sizeof(*S));
	S->m = D->n;
	S->idx = R->idx[s] = idx;
	if(first) R->a.first = 1;
	if(bytes) {
		void *p = NULL;
		if((rc = ccg_malloc(R->ctx, &p, bytes))) return merge_fail("source buffer", rc);
		S->d = p;
		if((rc = ccg_memcpy_h2d(R->ctx, p, D->mat, bytes))) return merge_fail("upload", rc);
		if(W) {
			if((rc = ccg_malloc(R->ctx, &p, bytes))) return merge_fail("source buffer", rc);
			S->w = p;
			if((rc = ccg_memcpy_h2d(R->ctx, p, W->mat, bytes))) return merge_fail("upload", rc);
		}
	}
	return R->a.nsrc == CCG_MERGE_MAX_SRC ? merge_flush(R, n_union) : 0;
}

static int main_merge(int argc, char **argv) {
	MergeOpts o = {.in = "-", .tmethod = "dnj", .flag = 1, .precision = 9, .et = 8, .sep = '\t'};
	const int prc = cli_parse(&merge_cmd, argc, argv, &o);
	if(prc != CLI_GO) return prc;
	const int et = o.et;
	if(o.flag == -1) {
		fprintf(stdout, "# Format flags output, add them to combine them.\n");
		fprintf(stdout, "#\n");
		fprintf(stdout, "#   1:\tRelaxed Phylip\n");
		fprintf(stdout, "#   2:\tDistances are pairwise, always true on *.mat files\n");
		fprintf(stdout, "#   4:\tInclude template name in phylip file\n");
		fprintf(stdout, "#   8:\tInclude insignificant bases in distance calculation, only affects fasta input\n");
		fprintf(stdout, "#  16:\tInclude reference, only affects fasta input\n");
		fprintf(stdout, "#  32:\tDistances based on fasta input\n");
		fprintf(stdout, "#\n");
		return 0;
	}
	if(o.scaled.mark) {
		/* merge.c:163-174 multiplies the scaled integers of d and w without unscaling them, and its
		 * sums wrap: there is nothing to be compatible with */
		fprintf(stderr, "ccphylo_amd: merge -s / -b is not supported: the reference multiplies the scaled integers of distance and weight without unscaling them; use double or -p.\n");
		return 1;
	}
	const int tm = o.treename ? fused_tree_method(o.tmethod) : 0;
	if(tm < 0) return 1;
	ccq_reader *r = ccq_open(o.in), *rw = o.wname ? ccq_open(o.wname) : NULL;
	if(!r || (o.wname && !rw)) return errno_fail(1);
	MergeRun R;
	memset(&R, 0, sizeof(R));
	R.ctx = open_gpu(o.device);
	R.et = R.a.etype = et;
	R.a.weighted = o.wname != NULL;
	ccq_ltd *Dh = ccq_ltd_new(64, et, 1.0), *Wh = o.wname ? ccq_ltd_new(64, et, 1.0) : NULL;
	ccq_names *T = ccq_names_new(64, 32);
	ccq_namemap *M = ccq_namemap_new();
	int err = 0;
	for(int mat = 0;; ++mat) {
		const int m = ccq_load_phy(r, Dh, T, o.sep, 0, &err);
		if(mat && !m) break;   /* a size of 0 or the end of the file ends the input (merge.c:183) */
		/* the weights' names overwrite the distances' (merge.c:144 / :184) */
		if(Wh && ccq_load_phy(rw, Wh, T, o.sep, 0, &err) != m) {
			fprintf(stderr, "Distance and included nucleotides does not concur!\n");
			return 1;
		}
		if(!m) continue;   /* an empty first matrix: the reference reads on */
		int32_t *idx = malloc((size_t) m * sizeof(int32_t));
		int ra = 0, rb = 0;
		if(!idx) {
			fprintf(stderr, "Error: out of host memory\n");
			return 12;
		}
		if(ccq_merge_index(M, T, m, idx, &ra, &rb)) {
			/* the reference then updates cell (k, k) of the union, which lies outside row k */
			fprintf(stderr, "ccphylo_amd: merge: matrix %d holds the name \"%s\" twice, on rows %d and %d.\n", mat + 1,
			        (char *) T->names[rb]->seq, ra + 1, rb + 1);
			return 1;
		}
		Dh->n = m;
		if(merge_stage(&R, Dh, Wh, idx, mat == 0, ccq_namemap_n(M))) return 1;
	}
	ccq_close(r);
	if(rw) ccq_close(rw);
	const int n = ccq_namemap_n(M);
	if(o.treename && n < 3) {
		fprintf(stderr, "ccphylo_amd: --tree needs at least 3 entries (%d).\n", n);
		return 1;
	}
	if(R.a.nsrc && merge_flush(&R, n)) return 1;
	/* with --tree the Phylip texts are written only where -o / -n ask for them */
	if(!o.outname && !o.treename) o.outname = "-";
	if(o.wname && !o.nname && !o.treename) o.nname = "-";
	if(!o.wname) o.nname = NULL;
	const size_t cells = (size_t) n * (size_t) (n ? n - 1 : 0) / 2;
	ccq_ltd *Do = ccq_ltd_new(n > 1 ? n : 2, et, 1.0), *No = o.nname ? ccq_ltd_new(n > 1 ? n : 2, et, 1.0) : NULL;
	ccg_join *joins = o.treename ? malloc((size_t) n * sizeof(ccg_join)) : NULL;
	int nj = 0, fn = 0, rc = 0;
	double fd = 0;
	Do->n = n;
	if(No) No->n = n;
	if(cells) {
		double ms = 0;
		ccg_tree_args ta = {n, et, 1.0, tm, 0, 1, 0, 0};
		if((rc = ccg_ltd_merge_close_dev(R.ctx, R.dD, R.dN, n, et))) return merge_fail("ccg_ltd_merge_close_dev", rc);
		ccg_last_merge_ms(R.ctx, &ms);
		R.dev_ms += ms;
		if(o.outname && (rc = ccg_memcpy_d2h(R.ctx, Do->mat, R.dD, cells * (size_t) et))) return merge_fail("read back", rc);
		if(No && (rc = ccg_memcpy_d2h(R.ctx, No->mat, R.dN, cells * (size_t) et))) return merge_fail("read back", rc);
		/* the tree of `merge | tree`: cells as the Phylip text would round them, then the engine, which consumes D */
		if(o.treename && (rc = ccg_round_decimal_dev(R.ctx, R.dD, (int64_t) cells, et, o.precision)))
			return merge_fail("ccg_round_decimal_dev", rc);
		if(o.treename && (rc = ccg_tree_dev(R.ctx, &ta, R.dD, joins, &nj, &fn, &fd, NULL))) return merge_fail("ccg_tree_dev", rc);
	}
	if(R.dD) ccg_free(R.ctx, R.dD);
	if(R.dN) ccg_free(R.ctx, R.dN);
	ccg_destroy(R.ctx);
	if(getenv("CCPHYLO_MERGE_TIMES")) fprintf(stderr, "# merge: %.3f ms on the device\n", R.dev_ms);
	char **names = malloc(((size_t) n + 1) * sizeof(char *));
	for(int i = 0; i < n; ++i) names[i] = strdup(ccq_namemap_name(M, i));
	FILE *out = NULL, *nout = NULL, *tout = NULL;
	if(o.outname) out = open_out(o.outname);
	if(o.nname) nout = open_out(o.nname);
	if(o.treename) tout = open_out(o.treename);
	if((o.outname && !out) || (o.nname && !nout) || (o.treename && !tout)) return errno_fail(1);
	if(o.treename) {   /* the names `merge | tree` would hold, taken before the writer strips quotes */
		ccq_names *Tt = ccq_names_new(32, 4);   /* as tree.c:61-66 */
		ccq_names_set(Tt, names, n, (unsigned) o.flag, '\t');
		fused_write_newick(tout, Tt, n, &(Joins){joins, nj, fn, fd}, 0, o.precision);
		fflush(stdout);
		ccq_names_free(Tt);
	}
	if(out) ccq_print_phy(out, Do, names, NULL, "Merged", (unsigned) o.flag, o.precision);
	if(nout) {
		ccq_print_phy(nout, No, names, NULL, "Merged", (unsigned) o.flag, o.precision);
		if(nout != stdout) fclose(nout);
	}
	if(out && out != stdout) fclose(out);
	fflush(stdout);
	for(int i = 0; i < n; ++i) free(names[i]);
	free(names);
	free(joins);
	ccq_ltd_free(Do);
	if(No) ccq_ltd_free(No);
	ccq_ltd_free(Dh);
	if(Wh) ccq_ltd_free(Wh);
	ccq_names_free(T);
	ccq_namemap_free(M);
	return 0;
}

static int main_help(FILE *out) {
	fprintf(out, "# CCPhylo (ccphylo_amd: MI355X engine for dist, tree and their matrices)\n");
	fprintf(out, "# Usage: ccphylo <command> [options]\n");
	fprintf(out, "#    %-16s\t%s\n", "dist", "all-pairs SNP distances of an MSA (GPU)");
	fprintf(out, "#    %-16s\t%s\n", "tree", "NJ / DNJ trees from Phylip matrices (GPU)");
	fprintf(out, "#    %-16s\t%s\n", "dbscan", "DBSCAN clusters from Phylip matrices (GPU)");
	fprintf(out, "#    %-16s\t%s\n", "tsv2phy", "all-pairs distances of a table's rows (GPU)");
	fprintf(out, "#    %-16s\t%s\n", "nwck2phy", "path-length matrices of Newick trees (GPU)");
	fprintf(out, "#    %-16s\t%s\n", "phycmp", "cos, chi2, bc, l1, l2, linf and Pearson of two Phylip matrices (GPU)");
	fprintf(out, "#    %-16s\t%s\n", "merge", "the matrices of a multi Phylip file into one (GPU)");
	return out == stderr;
}

int main(int argc, char **argv) {
	if(argc < 2) {
		fprintf(stderr, "Too few arguments handed.\n");
		return main_help(stderr);
	}
	if(!strcmp(argv[1], "dist")) return main_dist(argc - 1, argv + 1);
	if(!strcmp(argv[1], "tree")) return main_tree(argc - 1, argv + 1);
	if(!strcmp(argv[1], "dbscan")) return main_dbscan(argc - 1, argv + 1);
	if(!strcmp(argv[1], "tsv2phy")) return main_tsv2phy(argc - 1, argv + 1);
	if(!strcmp(argv[1], "nwck2phy")) return main_nwck2phy(argc - 1, argv + 1);
	if(!strcmp(argv[1], "phycmp")) return main_phycmp(argc - 1, argv + 1);
	if(!strcmp(argv[1], "merge")) return main_merge(argc - 1, argv + 1);
	if(!strcmp(argv[1], "-h") || !strcmp(argv[1], "--help")) return main_help(stdout);
	fprintf(stderr, "ccphylo_amd: command \"%s\" is outside the GPU engine's scope (dist, tree, dbscan, tsv2phy, nwck2phy, phycmp, merge).\n", argv[1]);
	return 1;
}
