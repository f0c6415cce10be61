"""Section profile of an intra CTU with the pixel stages of the small-TU trials split out (diagnostic build -DFCU_PROFILE
-DFCU_PROFILE_PIX as libfcu_prof_pix.so): a measurement script, not a test.  Same workload and arguments as tests/prof_run.py
(`frames` 4K frames x 4 QPs, the first `ctus` CTUs of each).  Slots 1, 2, 8 and 10 keep their sections; the other twelve carry
the pixel stages of pu_first_pass_batched and tu_trial before / after the quantiser, by block size (4x4, 8x8, 16x16 and up).
"before" = prediction + residual, forward transform, level_double; "after" = levels to raster order + dequantisation, inverse
transform, reconstruction + SSE (tu_trial: with the cbf / coefficient store)."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g

pkg = g.load_package()
pkg.engine._lib = None
pkg.engine.lib_path = lambda: os.path.join(os.path.dirname(pkg.engine.__file__), os.environ.get("FCU_LIB", "libfcu_prof_pix.so"))
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
# slot -> name (FCU_PIX_SLOT in fcu_engine.h)
names = {1: "pass1_total", 2: "pass1_rdoq", 8: "seq_rdoq", 10: "ctu_total",
         3: "pass1_pre_4x4", 4: "pass1_pre_8x8", 5: "pass1_pre_16up", 6: "pass1_post_4x4", 7: "pass1_post_8x8", 9: "pass1_post_16up",
         11: "tu_pre_4x4", 12: "tu_pre_8x8", 13: "tu_pre_16up", 14: "tu_post_4x4", 15: "tu_post_8x8", 0: "tu_post_16up"}
order = [10, 1, 2, 8, 3, 4, 5, 6, 7, 9, 11, 12, 13, 14, 15, 0]
acc = np.zeros(17)
sampled = range(0, frames * 4, max(1, frames * 4 // 64))
for c in sampled:
    acc += np.array(eng.debug_counters(c), dtype=float)
n = len(sampled) * nct
for i in order:
    print("%-16s %6.2f%%  %8.2f Mticks/CTU" % (names[i], 100 * acc[i] / acc[10], acc[i] / n / 1e6))
small = acc[3] + acc[4] + acc[6] + acc[7] + acc[11] + acc[12] + acc[14] + acc[15]
big = acc[5] + acc[9] + acc[13] + acc[0]
print("pixel stages of 4x4 and 8x8 blocks, all eight: %6.2f%%  %8.2f Mticks/CTU" % (100 * small / acc[10], small / n / 1e6))
print("pixel stages of 16x16 and larger, all four:    %6.2f%%  %8.2f Mticks/CTU" % (100 * big / acc[10], big / n / 1e6))
