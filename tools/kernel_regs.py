#!/usr/bin/env python3
"""register / scratch / LDS use of every kernel in build/icp_k_*.s, build/gicp_k.s, build/feat_k.s, build/color_k.s, build/keypoint_k.s, build/normals_k.s, build/sym_k.s and build/segment_k.s
(optionally filtered by a substring of the kernel's name, or by a family: the listing's name without `_k.s`).
build/feat_k.s holds the descriptor, matching and scoring kernels and those of Fast Global Registration: `kernel_regs.py fgr` lists
batch_fgr_terms<F, false / true> and batch_fgr_finalize; `kernel_regs.py segment` lists the plane segmentation's batch_plane_score<F>,
batch_plane_refit<F> and batch_plane_decide<F> (build/segment_k.s)"""
import os
import re
import subprocess
import sys

import glob
paths = sorted(glob.glob("fast-point-cloud-registration-with-gpus_amd/csrc/build/icp_k_*.s") + glob.glob("fast-point-cloud-registration-with-gpus_amd/csrc/build/gicp_k.s") + glob.glob("fast-point-cloud-registration-with-gpus_amd/csrc/build/feat_k.s") + glob.glob("fast-point-cloud-registration-with-gpus_amd/csrc/build/color_k.s")
               + glob.glob("fast-point-cloud-registration-with-gpus_amd/csrc/build/keypoint_k.s") + glob.glob("fast-point-cloud-registration-with-gpus_amd/csrc/build/normals_k.s")
               + glob.glob("fast-point-cloud-registration-with-gpus_amd/csrc/build/sym_k.s") + glob.glob("fast-point-cloud-registration-with-gpus_amd/csrc/build/segment_k.s"))
flt = sys.argv[1] if len(sys.argv) > 1 else ""
rows = []
for p in paths:
    family = os.path.basename(p)[:-len("_k.s")] if p.endswith("_k.s") else ""
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", open(p).read(), re.S):
        name, body = m.group(1), m.group(2)
        g = lambda k: re.search(r"\.amdhsa_%s (\d+)" % k, body).group(1)
        rows.append((name, g("next_free_vgpr"), g("next_free_sgpr"), g("private_segment_fixed_size"), g("group_segment_fixed_size"), family))
names = subprocess.run(["c++filt"], input="\n".join(r[0] for r in rows), capture_output=True, text=True).stdout.split("\n")
for (name, v, sg, sc, lds, family), dn in zip(rows, names):
    dn = re.sub(r"\(.*", "", dn)
    if flt in dn or (flt and flt == family):
        print(f"{dn[:70]:70s} vgpr {v:>4s} sgpr {sg:>4s} scratch {sc:>5s} lds {lds:>6s}")
