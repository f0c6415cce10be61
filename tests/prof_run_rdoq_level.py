"""The coefficient loop of the lane-private RDOQ, rdoq<0>, on lane 0 by kind of iteration (diagnostic build -DFCU_PROFILE
-DFCU_PROFILE_RDOQ=4 as libfcu_prof_level.so; with -DFCU_RDOQ_LEVELS_REF as well, the engine on coded_level() + ic_rate(), whose
two parts are timed apart): a measurement script, not a test.  Same workload and arguments as tests/prof_run_walk.py (`frames`
4K frames x 4 QPs, the first `ctus` CTUs of each).  Per CTU, in ticks and iterations: iterations in which no lane of the batch
has a candidate level, iterations in which at least one lane takes the level choice, the head and tail of the coefficient
groups; inside the level choice, where lane 0 takes it itself: the level choice, the rates of rateIncUp / rateIncDown (0 in
the build on level_choice(), which forms them in the same pass), the record store with the c1 / c2 / Rice update."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g

pkg = g.load_package()
pkg.engine._lib = None
pkg.engine.lib_path = lambda: os.path.join(os.path.dirname(pkg.engine.__file__), os.environ.get("FCU_LIB", "libfcu_prof_level.so"))
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
MASK = (1 << 40) - 1
ticks, count = np.zeros(16), np.zeros(16)
sampled = range(0, frames * 4, max(1, frames * 4 // 64))
for c in sampled:
    for i, v in enumerate(eng.debug_counters(c)[:16]):
        packed = i in (0, 1, 11, 12, 13)                         # ticks + (count << 40)
        ticks[i] += (v & MASK) if packed else v
        count[i] += (v >> 40) if packed else 0
n = len(sampled) * nct
for i, nm in ((2, "pass1_rdoq"), (3, "chroma_rdoq"), (8, "seq_rdoq"), (10, "ctu_total")):
    print("%-44s %6.2f%%  %8.2f Mticks/CTU" % (nm, 100 * ticks[i] / ticks[10], ticks[i] / n / 1e6))
print("rdoq<0> on lane 0, per CTU:")
rows = ((1, "calls, up to the end of the walk", "calls"), (0, "group heads and tails", "intervals"),
        (11, "iterations, no lane with a candidate level", "iterations"), (12, "iterations, a lane in the level choice", "iterations"),
        (13, "  lane 0 in it: level choice", "coefficients"), (14, "  lane 0 in it: rateIncUp / rateIncDown", None),
        (15, "  lane 0 in it: record store + state update", None))
for i, nm, unit in rows:
    line = "%-44s %8.2f Mticks/CTU" % (nm, ticks[i] / n / 1e6)
    if unit:
        line += "  %9.0f %s/CTU" % (count[i] / n, unit)
        if count[i]:
            line += "  %7.0f ticks each" % (ticks[i] / count[i])
    print(line)
