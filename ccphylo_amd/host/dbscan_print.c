/* dbscan_print.c -- the output table of `ccphylo dbscan` (ref dbscan.c:165
 * print_dbscan and the header line of dbscan.c:220). */
#include "ccphylo_host.h"

void ccq_print_dbscan(FILE *out, const char *header, char **names, const int32_t *N, const int32_t *C, int n,
                      int nclust, double maxDist, int minN) {
	if(header && *header) fprintf(out, "#%s\n", header);
	fprintf(out, "## %d\t%d\t%lf\t%d\n", n, nclust, maxDist, minN);
	fprintf(out, "#%s\t%s\t%s\n", "Sample", "Neighbors", "Cluster");
	for(int i = 0; i < n; ++i) fprintf(out, "%s\t%d\t%d\n", names[i], N[i], C[i]);
}
