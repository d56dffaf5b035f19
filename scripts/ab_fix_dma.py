#!/usr/bin/env python
"""A/B of the fixed walk's two-buffer stage (treeinfer_kernels.h, TI_FIX_DMA:
the peeled stages filled by LDS-DMA into two LDS buffers, one barrier a
stage), in one process: the sides alternate inside every round, so one box
and one clock state serve both.

  A  fd_parent  -DTI_FIX_DMA=0   the kernel as it was (scripts/build_variant.py;
                                 its twelve bheap_fix_kernel instantiations hash
                                 to the parent commit's code)
  B  the in-tree library (the defaults)

Workloads, figures and the counting rule are those of scripts/ab_fix_rotate.py
(its helpers are imported; that script stays the record of its own change):
c2, c2_nan, c2_64k and c2_hist at bench.py's shape, the one-stream kernel ms
and the two-stream ms per batch, the second stream taken only after
ab_bin_search.second_stream's overlap check.  One JSON line per (round,
workload, side) goes to --out.

  python scripts/ab_fix_dma.py --rounds 7 --out profiles/fix_dma_ab.jsonl
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import ab_fix_rotate  # noqa: E402

if __name__ == "__main__":
    ab_fix_rotate.VARIANTS = {"A": "fd_parent"}
    ab_fix_rotate.LAUNCH_ENV = {}
    if not any(a == "--sides" or a.startswith("--sides=") for a in sys.argv[1:]):
        sys.argv += ["--sides", "AB"]
    if not any(a == "--out" or a.startswith("--out=") for a in sys.argv[1:]):
        sys.argv += ["--out", os.path.join(ROOT, "profiles", "fix_dma_ab.jsonl")]
    ab_fix_rotate.main()
