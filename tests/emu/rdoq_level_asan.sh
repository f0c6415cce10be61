#!/bin/bash
# Host-side check of level_choice() (the level choice of RDOQ's first loop and the rates of its record in one pass): the
# emulator's engine translation unit with -DFCU_EMU_CHECK_RDOQ_LEVELS plus rdoq_level_asan_driver.cpp under the address and
# undefined-behaviour sanitizers, run directly (its own main, no GPU).  Python only writes the frames of
# tests/rdoq_level_cases.py as raw 4:2:0 files for the program to read.
# -fno-sanitize=shift: the dequantiser shifts negative products left as the reference does (two's complement).
set -e
cd "$(dirname "$0")"
tmp=$(mktemp -d)
trap 'rm -rf "$tmp"' EXIT
python3 - "$tmp" <<'EOF'
import os, sys
out = sys.argv[1]
here = os.getcwd()
root = os.path.dirname(os.path.dirname(here))
sys.path[:0] = [root, os.path.join(root, "tests"), os.path.join(root, "oracle")]
import __graft_entry__ as g
import hmo_py
from rdoq_level_cases import INTRA_CASES, LDP_CLIP, frame, ldp_pictures
pkg = g.load_package()
def write(name, planes):
    with open(os.path.join(out, name), "wb") as f:
        for p in planes:
            f.write(p.tobytes())
manifest = []
for k, (src, w, h, qp) in enumerate(INTRA_CASES):
    write("intra%d.yuv" % k, frame(pkg, src, w, h))
    manifest.append("intra intra%d.yuv %d %d %d" % (k, w, h, qp))
_, w, h, base_qp, _, n_pic, sr = LDP_CLIP
assert n_pic == 2
pics = ldp_pictures(pkg)
write("ldp0.yuv", pics[0])
write("ldp1.yuv", pics[1])
_, qp, lam = hmo_py.ldp_slice(0, base_qp)
o = hmo_py.Encoder(*pics[0], qp, lambda_override=lam)
o.compress_frame()
o.deblock()
write("ldp0_dbk.yuv", o.rec)
manifest.append("ldp ldp0.yuv ldp1.yuv ldp0_dbk.yuv %d %d %d %d" % (w, h, base_qp, sr))
with open(os.path.join(out, "manifest.txt"), "w") as f:
    f.write("\n".join(manifest) + "\n")
EOF
g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize=shift -fno-sanitize-recover=undefined -o rdoq_level_asan_driver rdoq_level_asan_driver.cpp
./rdoq_level_asan_driver "$tmp"
