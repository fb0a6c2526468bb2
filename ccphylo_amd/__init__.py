"""ccphylo_amd -- MI355X (gfx950) engine for ccphylo's `dist`, `tree`, `dbscan`, `tsv2phy`, `nwck2phy`,
`phycmp` and `merge` hot path.

Native pieces (built in-tree by ``__graft_entry__.build()`` / ``make -C ccphylo_amd``):
  lib/libccphylo_amd.so   HIP kernels + C-ABI (include/ccphylo_amd.h)
  lib/libccphylo_host.so  Phylip / Newick / FASTA host layer (include/ccphylo_host.h)
  bin/ccphylo             the `ccphylo dist` / `tree` / `dbscan` / `tsv2phy` / `nwck2phy` / `phycmp` / `merge` CLI

Python here is only a thin ctypes layer for tests and the benchmark.
"""
from .native import (CCG_TREE_CF, CCG_TREE_DNJ, CCG_TREE_FF, CCG_TREE_HNJ, CCG_TREE_MN, CCG_TREE_NJ, CCG_TREE_UPGMA, CLI_PATH, CcgError, Device, ETYPES, JOIN_DTYPE,  # noqa: F401
                     engine_lib, host_lib, load_msa, load_phylip, newick_from_phylip, write_dbscan)
from .native import (CCG_VEC_BC, CCG_VEC_CHI2, CCG_VEC_COS, CCG_VEC_L1, CCG_VEC_L2, CCG_VEC_LINF, CCG_VEC_LN,  # noqa: F401
                     CCG_VEC_PEARSON, load_tsv, vec_metric, write_tsvphy)
from .native import MOTIF_DTYPE, load_motifs, meth_clear_row  # noqa: F401
from .native import CMP_METRICS, CMP_SUMS, SPLIT_DTYPE, cmp_close, newick_splits  # noqa: F401
from .native import MERGE_GATHER, MERGE_MAX_SRC, MERGE_SCATTER, MergeArgs  # noqa: F401

__version__ = "0.1.0"
