"""Section profile of an intra CTU with the sub-timers of the lane-private RDOQ, rdoq<0>, taken on lane 0 (diagnostic build
-DFCU_PROFILE -DFCU_PROFILE_RDOQ=2 as libfcu_prof_walk.so): a measurement script, not a test.  Same workload and arguments as
tests/prof_run.py (`frames` 4K frames x 4 QPs, the first `ctus` CTUs of each); slots 11..15 = set-up + uncoded tail, main loop,
last-position search, signs, sign hiding of the rdoq<0> calls lane 0 took part in (first pass, chroma search)."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g

pkg = g.load_package()
pkg.engine._lib = None
pkg.engine.lib_path = lambda: os.path.join(os.path.dirname(pkg.engine.__file__), os.environ.get("FCU_LIB", "libfcu_prof_walk.so"))
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
names = ["rmd", "pass1_total", "pass1_rdoq", "pass1_bits", "pass2_rqt", "chroma_batched", "chroma_total", "cu_syntax", "seq_rdoq", "replay",
         "ctu_total", "rdoq0_setup_tail", "rdoq0_main_loop", "rdoq0_last_pos", "rdoq0_signs", "rdoq0_sign_hiding"]
acc = np.zeros(17)
sampled = range(0, frames * 4, max(1, frames * 4 // 64))
for c in sampled:
    acc += np.array(eng.debug_counters(c), dtype=float)
n = len(sampled) * nct
for i, nm in enumerate(names):
    print("%-16s %6.2f%%  %8.2f Mticks/CTU" % (nm, 100 * acc[i] / acc[10], acc[i] / n / 1e6))
print("rdoq<0> on lane 0, all five: %8.2f Mticks/CTU" % (acc[11:16].sum() / n / 1e6))
