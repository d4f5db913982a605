"""Host replay of the T1 decoder's column step (tests/cpp/t1_walk_fused_sim.cpp):
the crop, transform and block order of scripts/t1_walk_sim.py, the nested walk
replayed with one loop iteration per MQ decision and with one per sample (the
sign decision in the iteration of the decision that leads to it), and both
priced in wave-VALU with the per-step instruction counts of the two builds
(scripts/t1_isa_count.py --all).
  python scripts/t1_walk_fused_sim.py [H W [Q]] [--symbol SPP,CUP] [--sample SPP,CUP] [--column N] [--mrp N]"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "scripts")]

import pyoracle  # noqa: E402
import synth  # noqa: E402
from t1_walk_sim import blocks  # noqa: E402


def opt(name, default):
    if name in sys.argv:
        return [int(v) for v in sys.argv[sys.argv.index(name) + 1].split(",")]
    return default


def main():
    pos = []
    for a in sys.argv[1:]:
        if a.startswith("--"):
            break
        pos.append(int(a))
    H, W = pos[:2] if len(pos) > 1 else (2048, 4096)
    q = pos[2] if len(pos) > 2 else 0  # drop q bit-planes (a lossy encode's quantisation)
    # VALU per wave step: SPP and cleanup symbol step, SPP and cleanup sample
    # step (sign region entered), column set-up, refinement decision
    symbol, sample = opt("--symbol", [64, 78]), opt("--sample", [86, 103])
    column, mrp = opt("--column", [95])[0], opt("--mrp", [37])[0]
    pyoracle.build()
    img = synth.synth_plane(H, W, 12, 3, 0, "smooth").astype(np.int32) - 2048
    coef = np.ascontiguousarray(img)
    pyoracle.dwt_fwd(coef, 0, 0, 6, False)
    if q:
        coef = (np.sign(coef) * (np.abs(coef) >> q)).astype(np.int32)
    exe = os.path.join(tempfile.gettempdir(), "t1_walk_fused_sim")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wno-unknown-pragmas", "-o", exe,
                    os.path.join(ROOT, "tests/cpp/t1_walk_fused_sim.cpp"), "-L" + os.path.join(ROOT, "oracle", "build"),
                    "-lgrk_oracle", "-Wl,-rpath," + os.path.join(ROOT, "oracle", "build")], check=True)
    bl = blocks(coef, 6)
    parts = [np.array([len(bl)], dtype="<u4").tobytes()]
    for x, y, w, h, o in bl:
        parts.append(np.array([w, h, o, 1, 0], dtype="<i4").tobytes())
        parts.append(np.ascontiguousarray(coef[y:y + h, x:x + w], dtype="<i4").tobytes())
    r = subprocess.run([exe], input=b"".join(parts), capture_output=True, check=True)
    res = json.loads(r.stdout)
    print("crop %d x %d, 5/3, %d planes dropped, %d blocks" % (H, W, q, res["blocks"]))
    print("%-10s %12s %12s %12s %12s %12s %12s" % ("pass", "decisions", "sign", "ideal", "symbol steps", "sample steps",
                                                   "column steps"))
    tot = [0.0, 0.0]
    for p, name in zip(res["passes"], ("SPP", "refinement", "cleanup")):
        print("%-10s %12d %12d %12d %12d %12d %12d" % (name, p["decisions"], p["sign_decisions"], p["ideal_steps"],
                                                       p["symbol_steps"], p["sample_steps"], p["column_steps"]))
        if name == "refinement":
            v = [p["symbol_steps"] * mrp + p["column_steps"] * column] * 2
        else:
            k = 0 if name == "SPP" else 1
            v = [p["symbol_steps"] * symbol[k] + p["column_steps"] * column,
                 p["sample_steps"] * sample[k] + p["column_steps"] * column]
        print("%-10s wave-VALU: one iteration per decision %.1f M, per sample %.1f M" % ("", v[0] / 1e6, v[1] / 1e6))
        tot[0] += v[0]
        tot[1] += v[1]
    print("decoder wave-VALU %.1f M -> %.1f M (%+.1f %%)" % (tot[0] / 1e6, tot[1] / 1e6, 100 * (tot[1] / tot[0] - 1)))


if __name__ == "__main__":
    main()
