"""popgenomicstools_amd — MI355X (gfx950) window-scan engine for PopGenomicsTools'
fstWindow / hetWindow / dxyWindow hot path.

Layout
  csrc/            HIP kernels (pgt_kernels.hip, pgt_af_kernels.hip, pgt_dxy_pops_kernels.hip, pgt_fst_pops_kernels.hip, pgt_dstat_pops_kernels.hip, pgt_fd_pops_kernels.hip, pgt_f3_pops_kernels.hip, pgt_f4_pops_kernels.hip, pgt_f4ratio_pops_kernels.hip, pgt_dstat_jack_kernels.hip, pgt_align_kernels.hip) + the C-ABI (pgt_api.cpp, pgt_windows.cpp)
  host/            the retained C++ hosts: reference argv + TSV, reduction in libpgtwin
  _lib.py          ctypes binding of include/pgtwin.h
  window_scan.py   host-side mirror of the three tools over numpy / torch buffers
  build.py         in-tree hipcc build
"""
from .window_scan import (  # noqa: F401
    Context,
    all_quartet_order,
    all_trio_order,
    align_segments,
    align_segments_runs,
    align_sites,
    build_windows_bp,
    build_windows_extreme,
    build_windows_sites,
    dxy_window,
    dxy_window_pops,
    dstat_window_pops,
    f3_window_pops,
    f4_window_pops,
    f4ratio_alphas,
    f4ratio_window_pops,
    pbs_item_order,
    pbs_window_pops,
    pbsn1_of,
    fd_window_pops,
    fst_window,
    fst_window_pops,
    pi_window_pops,
    het_window,
    ihs_window,
    middle_triple_order,
    pair_order,
    pairing_order,
    plan_shards,
    ratio_order,
    run_lengths,
    target_order,
    topology_order,
    trio_order,
    xpehh_window,
)

__all__ = ["Context", "build_windows_sites", "build_windows_bp", "fst_window", "het_window",
           "dxy_window", "dxy_window_pops", "fst_window_pops", "pi_window_pops", "dstat_window_pops", "fd_window_pops", "f3_window_pops", "f4_window_pops", "f4ratio_window_pops", "f4ratio_alphas", "middle_triple_order", "ratio_order", "pbs_window_pops", "pbsn1_of", "pbs_item_order", "pair_order", "trio_order", "all_trio_order", "all_quartet_order", "pairing_order", "topology_order", "target_order", "align_segments", "align_segments_runs", "align_sites", "ihs_window", "xpehh_window", "build_windows_extreme", "plan_shards", "run_lengths"]
