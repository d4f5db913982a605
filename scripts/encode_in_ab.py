"""Encode input layout A/B: what reading pixel-interleaved samples costs or
saves against the planar planes.  One process, one Codec, device-resident
uint16 frames: the bench's 8K 12-bit RGB frame (tests/golden/synth.py, seed 3),
9/7 and 5/3, and a DCI 4K 12-bit frame (4096 x 2160, 9/7 and 5/3).  Per frame
and wavelet the legs alternate round by round, in `runs` separate runs of
`rounds` rounds each:
  A  planar uint16 (c,h,w) compress -- the path every encode took before
  B  interleaved uint16 (h,w,c) compress (layout="hwc")
  C  permute().contiguous() of the (h,w,c) frame on the device, then the
     planar compress: what a caller holding pixels did before (total_ms
     includes the permute, timed with device events around it)
Reports per leg the median over the runs' medians of dcshift_mct_ms, the
level-0 DWT launch (grkgpu_set_launch_timing: its kernel and ms; the 5/3
level 0 is the fused DC shift + RCT + DWT, so dcshift_mct_ms is ~0 there),
loader_ms = their sum, and total_ms; for leg A also the min and max of the
runs' medians (its own run-to-run spread).  The three legs' codestreams are
checked equal.  "plugin_upload": the DCI 4K frame from pageable host memory as
the plugin uploads it -- int32 planes (4 B/sample, before) against the PPM
raster as it stands in the file, big-endian uint16 pixels (2 B/sample) --
h2d_ms and total_ms medians.  One JSON line (--out FILE: also written there)."""
import argparse
import datetime
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "golden")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import grokimagecompression_amd as grk  # noqa: E402
import synth  # noqa: E402

KEYS = ("dcshift_mct_ms", "level0_ms", "loader_ms", "total_ms")


def one(codec, leg, planar, pixels, bits, p):
    """One compress of a leg: (codestream view, its times)."""
    permute_ms = 0.0
    if leg == "A":
        cs = codec.compress(planar, bits, p, view=True)
    elif leg == "B":
        cs = codec.compress(pixels, bits, p, view=True, layout="hwc")
    else:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t = pixels.permute(2, 0, 1).contiguous()
        e1.record()
        cs = codec.compress(t, bits, p, view=True)
        e1.synchronize()
        permute_ms = e0.elapsed_time(e1)
    st = codec.stats()
    l0 = [t for t in codec.launch_times() if t["level0"] == 0]
    level0 = l0[0]["ms"] if l0 else 0.0
    return cs, {"dcshift_mct_ms": st["dcshift_mct_ms"], "level0_ms": level0,
                "loader_ms": st["dcshift_mct_ms"] + level0, "permute_ms": permute_ms,
                "total_ms": st["total_ms"] + permute_ms}, (l0[0]["kernel"] if l0 else "")


def run(codec, frame, bits, runs, rounds, warmup):
    planar = torch.from_numpy(frame.astype(np.uint16)).cuda()
    pixels = planar.permute(1, 2, 0).contiguous()
    res = {}
    for tag, irr in (("97", True), ("53", False)):
        p = grk.CParams.make(irreversible=irr)
        ref = bytes(codec.compress(planar, bits, p, view=True))
        meds = {leg: {k: [] for k in KEYS + ("permute_ms",)} for leg in "ABC"}
        kern = {}
        for _ in range(runs):
            times = {leg: {k: [] for k in KEYS + ("permute_ms",)} for leg in "ABC"}
            for r in range(warmup + rounds):
                for leg in "ABC":
                    cs, t, kern[leg] = one(codec, leg, planar, pixels, bits, p)
                    if r == 0:
                        assert bytes(cs) == ref, "leg %s: another codestream" % leg
                    del cs
                    if r >= warmup:
                        for k, v in t.items():
                            times[leg][k].append(v)
            for leg in "ABC":
                for k, v in times[leg].items():
                    meds[leg][k].append(statistics.median(v))
        for leg in "ABC":
            out = {k: round(statistics.median(v), 4) for k, v in meds[leg].items()}
            out["level0_kernel"] = kern[leg]
            if leg == "A":
                out["spread"] = {k: [round(min(meds[leg][k]), 4), round(max(meds[leg][k]), 4)] for k in KEYS}
            res["%s_%s" % (tag, leg)] = out
    return res


def upload(codec, frame, bits, rounds, warmup):
    p = grk.CParams.make(irreversible=True)
    legs = {"int32_planar": (np.ascontiguousarray(frame.astype(np.int32)), "chw"),
            "u16be_interleaved": (np.ascontiguousarray(frame.transpose(1, 2, 0)).astype(">u2"), "hwc")}
    times = {k: {"h2d_ms": [], "total_ms": []} for k in legs}
    ref = None
    for r in range(warmup + rounds):
        for k, (a, layout) in legs.items():
            cs = bytes(codec.compress(a, bits, p, view=True, layout=layout))
            ref = cs if ref is None else ref
            assert cs == ref
            st = codec.stats()
            if r >= warmup:
                for key in times[k]:
                    times[k][key].append(st[key])
    return {k: dict({key: round(statistics.median(v), 4) for key, v in t.items()}, bytes=int(legs[k][0].nbytes))
            for k, t in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--small", action="store_true", help="small frames (a rehearsal of the script, not a measurement)")
    ap.add_argument("--out")
    args = ap.parse_args()
    codec = grk.Codec(0)
    codec.set_launch_timing(True)
    out = {"device": torch.cuda.get_device_name(0), "date": datetime.date.today().isoformat(),
           "runs": args.runs, "rounds": args.rounds,
           "legs": "A planar u16, B interleaved u16, C permute().contiguous() + planar; device-resident; "
                   "median of the runs' medians, ms; A.spread = [min, max] of its runs' medians"}
    sizes = {"8k_12bit": (4320, 7680), "dci4k_12bit": (2160, 4096)}
    if args.small:
        sizes = {"small_12bit": (270, 480)}
    for name, (h, w) in sizes.items():
        frame = synth.synth_image(h, w, 3, 12, 3)
        out[name] = run(codec, frame, 12, args.runs, args.rounds, args.warmup)
    out["plugin_upload"] = upload(codec, frame, 12, args.rounds, args.warmup)
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
