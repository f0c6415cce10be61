"""Sub-timers of rdoq_wave, the one-block-per-wave quantiser of tu_trial and of the inter RQT (diagnostic build -DFCU_PROFILE
-DFCU_PROFILE_RDOQ=3 as libfcu_prof_rdoq_tail.so): a measurement script, not a test.  Same workload and arguments as
tests/prof_run.py (`frames` 4K frames x 4 QPs, the first `ctus` CTUs of each).  Five timers -- set-up + uncoded tail, main walk
(with its record stores where it has them), last-position search, sign pass, sign hiding + last level -- each split by block
size (4x4, 8x8, 16x16 and larger); timer t of size class s sits in slot 3 t + s, moved up by one from slot 10 on, which stays
the CTU total (FCU_WTOC, csrc/fcu_engine.h).  The library, from fast-cu-decision-hevc_amd/csrc:
  hipcc --offload-arch=gfx950 -std=c++17 -O3 -ffp-contract=off -fPIC -shared -DFCU_WAVES_PER_EU=4 -Wno-unused-value \
        -mllvm -amdgpu-remove-redundant-endcf=false -DFCU_PROFILE -DFCU_PROFILE_RDOQ=3 -o ../libfcu_prof_rdoq_tail.so fcu_kernels.hip
(tests/prof_run_rmd.py's library: the same line with -DFCU_PROFILE_RMD and -o ../libfcu_prof_rmd.so)."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g

pkg = g.load_package()
pkg.engine._lib = None
pkg.engine.lib_path = lambda: os.path.join(os.path.dirname(pkg.engine.__file__), os.environ.get("FCU_LIB", "libfcu_prof_rdoq_tail.so"))
import torch
from bench import gen_textured_gpu

W, H = 3840, 2160
frames = int(sys.argv[1]) if len(sys.argv) > 1 else 16
nct = int(sys.argv[2]) if len(sys.argv) > 2 else 4
dev = torch.device("cuda", 0)
eng = pkg.CuEngine(W, H, max_chains=frames * 4)
ci = 0
for f in range(frames):
    fr = gen_textured_gpu(torch, dev, W, H, seed=7 + f)
    for qp in (22, 27, 32, 37):
        out = torch.zeros(pkg.engine.CTU_OUT_BYTES * nct, dtype=torch.uint8, device=dev)
        eng.init_chain(ci, fr, qp=qp, out=out)
        ci += 1
t = time.time()
eng.compress_chains(0, frames * 4, nct)
eng.sync()
dt = time.time() - t
print("chains", frames * 4, "ctus", nct, "time", dt, "CTU/s", frames * 4 * nct / dt)
timers = ["setup_tail", "main_walk", "last_pos", "sign_pass", "sign_hiding"]
sizes = ["4x4", "8x8", ">=16x16"]
acc = np.zeros(17)
sampled = range(0, frames * 4, max(1, frames * 4 // 64))
for c in sampled:
    acc += np.array(eng.debug_counters(c), dtype=float)
n = len(sampled) * nct
total = acc[10]
print("%-16s %6.2f%%  %8.2f Mticks/CTU" % ("ctu_total", 100.0, total / n / 1e6))
by_size = np.zeros(3)
tail = np.zeros(3)
for ti, tn in enumerate(timers):
    for si, sn in enumerate(sizes):
        s = ti * 3 + si
        v = acc[s + (s >= 10)]
        by_size[si] += v
        if ti >= 2:
            tail[si] += v
        print("%-12s %-8s %6.2f%%  %8.2f Mticks/CTU" % (tn, sn, 100 * v / total, v / n / 1e6))
for si, sn in enumerate(sizes):
    print("rdoq_wave %-8s all five %6.2f%% %8.2f Mticks/CTU; last_pos + sign_pass + sign_hiding %6.2f%% %8.2f Mticks/CTU"
          % (sn, 100 * by_size[si] / total, by_size[si] / n / 1e6, 100 * tail[si] / total, tail[si] / n / 1e6))
print("rdoq_wave all sizes: %6.2f%% %8.2f Mticks/CTU; tail passes %6.2f%% %8.2f Mticks/CTU"
      % (100 * by_size.sum() / total, by_size.sum() / n / 1e6, 100 * tail.sum() / total, tail.sum() / n / 1e6))
