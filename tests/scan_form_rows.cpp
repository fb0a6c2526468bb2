// The DNJ scan-form resolver (ccphylo_amd/csrc/ccg_dnj_form.h) as a filter:
// one setting per input line, the resolved ScanForm per output line.
//
//   shard n et gen have_lbm prune_on small_wave [CCG_NAME=value ...]
//
// The CCG_* settings go through the environment and DnjGrid::load(), as in
// the engine; prune_on and small_wave are the two fields tree_run_t adapts
// per window.  shard = 1 asks the sharded engine's resolver.  prune_prev is
// the prune of the form at n - 1, which picks the requeue's kernel.
//
// TEST INFRASTRUCTURE ONLY (tests/test_scan_form.py compiles it with the host
// compiler on first use).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "ccg_dnj_form.h"

int main() {
	static const char *KERNEL[] = {"block", "wave", "wave16", "group", "group_cmp"};
	static const char *SPHASE[] = {"none", "scan", "compact"};
	char line[2048];
	while(fgets(line, sizeof(line), stdin)) {
		std::vector<std::string> tok;
		for(char *t = strtok(line, " \t\n"); t; t = strtok(NULL, " \t\n")) tok.push_back(t);
		if(tok.size() < 7) continue;
		int v[7];
		for(int k = 0; k < 7; ++k) v[k] = atoi(tok[k].c_str());
		std::vector<std::string> names;
		for(size_t k = 7; k < tok.size(); ++k) {
			const size_t eq = tok[k].find('=');
			names.push_back(tok[k].substr(0, eq));
			setenv(names.back().c_str(), tok[k].c_str() + eq + 1, 1);
		}
		DnjGrid g;
		g.load();
		for(const std::string &s : names) unsetenv(s.c_str());
		const int n = v[1], et = v[2];
		const bool gen = v[3] != 0, lbm = v[4] != 0;
		g.prune_on = v[5];
		g.small_wave = v[6];
		const ScanForm f = v[0] ? dnj_scan_form_shard(g, n, et, lbm) : dnj_scan_form(g, n, et, gen, lbm);
		const int prev = v[0] ? 0 : dnj_scan_form(g, n - 1, et, gen, lbm).prune;
		printf("kernel=%s stream=%d G=%d UC=%d prune=%d cmp=%d lb=%d tfold=%d helpers=%d sphase=%s fold=%d sfold=%d "
		       "grid=%u launches=%d prune_prev=%d\n",
		       KERNEL[f.kernel], (int) f.stream, f.G, f.UC, f.prune, (int) f.cmp, (int) f.lb, (int) f.tfold, f.helpers,
		       SPHASE[f.sphase], (int) f.fold, f.sfold, f.grid, f.launches, prev);
	}
	return 0;
}
