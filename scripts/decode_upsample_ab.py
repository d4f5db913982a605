"""Upsampled decode A/B: what a 4:2:0 stream decoded straight to full-size
pixels (Codec.decompress(upsample=True), GRKGPU_LAYOUT_UPSAMPLE) costs against
the 4:4:4 interleaved narrow decode it sits beside.  One process, one Codec;
the bench's 8K 12-bit frame (tests/golden/synth.py, seed 3) in uint16 and a 4K
8-bit frame in uint8, 9/7 and 5/3, each coded once 4:4:4 without MCT and once
4:2:0 from the same luma (chroma = every second sample of every second row).
Per frame and wavelet the legs alternate round by round, each into a device
tensor (h,w,c):
  A  4:4:4, interleaved narrow decode (the comparator: code that was there)
  B  4:2:0, upsample=True
and, after them, the same 4:2:0 stream the way it had to be decoded before:
  P  planar narrow host planes (a list), chroma replicated by np.repeat and
     the three planes stacked to (h,w,c) on the host; wall_ms includes that
Reports median, min and max of dcshift_mct_ms and total_ms (grkgpu_get_stats)
and of the wall-clock time of the call per leg as one JSON line (--out FILE:
also written there)."""
import argparse
import datetime
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "golden")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import grokimagecompression_amd as grk  # noqa: E402
import synth  # noqa: E402

KEYS = ("dcshift_mct_ms", "total_ms", "wall_ms")
SUBS = [(1, 1), (2, 2), (2, 2)]


def summary(times):
    return {k: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
            for k, v in times.items()}


def host_upsample(planes, h, w):
    """The parent's way: replicate the chroma planes on the host."""
    full = [planes[0]] + [np.repeat(np.repeat(p, 2, axis=0), 2, axis=1)[:h, :w] for p in planes[1:]]
    return np.stack(full, axis=2)


def run(codec, frame, bits, narrow, rounds, warmup):
    c, h, w = frame.shape
    planes420 = [frame[0]] + [np.ascontiguousarray(frame[k][::2, ::2]) for k in (1, 2)]
    res = {}
    for tag, irr in (("97", True), ("53", False)):
        p = grk.CParams.make(irreversible=irr, mct=0)
        cs444 = bytes(codec.compress(frame, bits, p, view=True))
        cs420 = codec.compress_subsampled(planes420, bits, (w, h), SUBS, p)
        tdt = getattr(torch, np.dtype(narrow).name)
        legs = [("A", cs444, {}, torch.empty((h, w, c), dtype=tdt, device="cuda:0")),
                ("B", cs420, {"upsample": True}, torch.empty((h, w, c), dtype=tdt, device="cuda:0"))]
        times = {leg: {k: [] for k in KEYS} for leg in ("A", "B", "P")}

        def record(leg, r, t0):
            st = codec.stats()
            st["wall_ms"] = (time.perf_counter() - t0) * 1e3
            if r >= warmup:
                for k in KEYS:
                    times[leg][k].append(st[k])

        for r in range(warmup + rounds):
            for leg, cs, kw, out in legs:
                t0 = time.perf_counter()
                codec.decompress(cs, out=out, layout="hwc", **kw)
                record(leg, r, t0)
        for r in range(warmup + rounds):
            t0 = time.perf_counter()
            got = codec.decompress(cs420, dtype=narrow)
            st = codec.stats()  # the decode's own figures, before the host's part
            ref = host_upsample(got, h, w)
            st["wall_ms"] = (time.perf_counter() - t0) * 1e3
            if r >= warmup:
                for k in KEYS:
                    times["P"][k].append(st[k])
        # B holds what P builds; A's luma is the same plane
        b = legs[1][3].cpu().numpy()
        assert np.array_equal(b, ref)
        assert np.array_equal(legs[0][3].cpu().numpy()[:, :, 0], b[:, :, 0])
        res[tag] = {leg: summary(times[leg]) for leg in times}
        res[tag]["bytes"] = {"cs444": len(cs444), "cs420": len(cs420)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.rounds < 5:
        ap.error("at least 5 rounds")
    codec = grk.Codec(0)
    out = {"device": torch.cuda.get_device_name(0), "date": datetime.date.today().isoformat(),
           "rounds": args.rounds, "legs": "A 4:4:4 hwc narrow, B 4:2:0 upsample=True hwc narrow (device tensors), "
           "P 4:2:0 planar host planes + np.repeat; ms"}
    out["8k_12bit_uint16"] = run(codec, synth.synth_image(4320, 7680, 3, 12, 3), 12, np.uint16, args.rounds,
                                 args.warmup)
    out["4k_8bit_uint8"] = run(codec, synth.synth_image(2160, 3840, 3, 8, 3), 8, np.uint8, args.rounds, args.warmup)
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
