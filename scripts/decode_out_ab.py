"""Decode output format A/B: what the narrow and interleaved outputs of
grkgpu_decompress_to cost or save against the int32 planes.  One process, one
Codec; the bench's 8K 12-bit RGB frame (tests/golden/synth.py, seed 3) in
uint16 and a 4K 8-bit RGB frame in uint8, 9/7 and 5/3.  Per frame and wavelet
the legs alternate round by round:
  A  int32 planar (grkgpu_decompress: the path every decode took before)
  B  narrow planar
  C  narrow interleaved (h,w,c)
each into a pinned host buffer and into a device tensor.  Reports the medians
of dcshift_mct_ms, d2h_ms and total_ms (grkgpu_get_stats) per leg as one JSON
line (--out FILE: also written there)."""
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

KEYS = ("dcshift_mct_ms", "d2h_ms", "total_ms")


def buffers(c, h, w, narrow, device):
    """The three legs' outputs: (leg, out, layout)."""
    legs = []
    for leg, dt, layout in (("A", np.int32, "chw"), ("B", narrow, "chw"), ("C", narrow, "hwc")):
        shape = (c, h, w) if layout == "chw" else (h, w, c)
        t = torch.empty(shape, dtype=getattr(torch, np.dtype(dt).name))
        out = t.cuda() if device else t.pin_memory().numpy()
        legs.append((leg, out, layout))
    return legs


def run(codec, frame, bits, narrow, rounds, warmup):
    c, h, w = frame.shape
    res = {}
    for tag, irr in (("97", True), ("53", False)):
        cs = bytes(codec.compress(frame, bits, grk.CParams.make(irreversible=irr), view=True))
        ref = None
        for device in (False, True):
            legs = buffers(c, h, w, narrow, device)
            times = {leg: {k: [] for k in KEYS} for leg, _, _ in legs}
            for r in range(warmup + rounds):
                for leg, out, layout in legs:
                    codec.decompress(cs, out=out, layout=layout)
                    st = codec.stats()
                    if r >= warmup:
                        for k in KEYS:
                            times[leg][k].append(st[k])
            # the three legs hold the same image
            img = [o.cpu().numpy() if device else o for _, o, _ in legs]
            ref = img[0] if ref is None else ref
            assert np.array_equal(img[0], ref) and np.array_equal(img[1], ref.astype(narrow))
            assert np.array_equal(img[2], ref.astype(narrow).transpose(1, 2, 0))
            for leg, _, _ in legs:
                res["%s_%s_%s" % (tag, "device" if device else "pinned", leg)] = {
                    k: round(statistics.median(v), 4) for k, v in times[leg].items()}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out")
    args = ap.parse_args()
    codec = grk.Codec(0)
    out = {"device": torch.cuda.get_device_name(0), "date": datetime.date.today().isoformat(),
           "rounds": args.rounds, "legs": "A int32 planar, B narrow planar, C narrow interleaved; medians, ms"}
    frame = torch.from_numpy(synth.synth_image(4320, 7680, 3, 12, 3)).cuda()
    out["8k_12bit_uint16"] = run(codec, frame, 12, np.uint16, args.rounds, args.warmup)
    frame = torch.from_numpy(synth.synth_image(2160, 3840, 3, 8, 3)).cuda()
    out["4k_8bit_uint8"] = run(codec, frame, 8, np.uint8, args.rounds, args.warmup)
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
