"""Section profile of an intra CTU with section 7 (`cu_syntax`, the bits of a finished intra candidate CU) split into its parts
(diagnostic build -DFCU_PROFILE -DFCU_PROFILE_CUSYN as libfcu_prof_cusyn.so): a measurement script, not a test.  Same workload
and arguments as tests/prof_run_rmd.py (`frames` 4K frames x 4 QPs, the first `ctus` CTUs of each).  Slots 11 / 12 carry section
7 of the 2Nx2N / NxN candidates, 13 / 14 the time inside code_coeff_nxn for luma / chroma levels within the 2Nx2N calls, 15 the
number of candidate CUs that took each path to their bits (21 bits each): merged with the chroma search's coder, merged with a
chroma-only walk, walked in full."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g

pkg = g.load_package()
pkg.engine._lib = None
pkg.engine.lib_path = lambda: os.path.join(os.path.dirname(pkg.engine.__file__), os.environ.get("FCU_LIB", "libfcu_prof_cusyn.so"))
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
         "ctu_total", "cu_syntax_2Nx2N", "cu_syntax_NxN", "2Nx2N_luma_coeff", "2Nx2N_chroma_coeff"]
acc = np.zeros(17)
paths = np.zeros(3)
sampled = range(0, frames * 4, max(1, frames * 4 // 64))
for c in sampled:
    v = eng.debug_counters(c)
    acc += np.array(v, dtype=float)
    paths += [(int(v[15]) >> (21 * k)) & ((1 << 21) - 1) for k in range(3)]
n = len(sampled) * nct
for i, nm in enumerate(names):
    print("%-18s %6.2f%%  %8.2f Mticks/CTU" % (nm, 100 * acc[i] / acc[10], acc[i] / n / 1e6))
print("%-18s %6.2f%%  %8.2f Mticks/CTU" % ("2Nx2N_rest", 100 * (acc[11] - acc[13] - acc[14]) / acc[10], (acc[11] - acc[13] - acc[14]) / n / 1e6))
print("2Nx2N luma levels as a share of cu_syntax: %.1f%%" % (100 * acc[13] / max(acc[7], 1)))
tot = max(paths.sum(), 1)
print("intra candidate CUs per CTU by path: merged with the search's chroma coder %.1f (%.1f%%), merged with a chroma-only walk %.1f (%.1f%%), walked %.1f (%.1f%%)"
      % (paths[0] / n, 100 * paths[0] / tot, paths[1] / n, 100 * paths[1] / tot, paths[2] / n, 100 * paths[2] / tot))
