"""Converting decode A/B: what sYCC -> RGB and the output precision cost in the
store of the last decode kernel (Codec.decompress(colour="sycc", out_prec=,
prec_mode=), grkgpu_decompress_convert) against the plain store beside them.
One process, one Codec; the bench's 8K 12-bit frame (tests/golden/synth.py,
seed 3), 9/7 and 5/3, every leg into a device tensor (h,w,c):
  444       the frame 4:4:4 (default MCT)
              plain_u16       uint16                      (code that was there)
              sycc_u16        colour="sycc", uint16
              scale_u8        out_prec=8 "scale", uint8   (precision alone)
              sycc_scale_u8   colour="sycc", out_prec=8 "scale", uint8
  420_12    the frame 4:2:0 (chroma = every second sample of every second row, no MCT)
              plain_u16       upsample=True, uint16       (code that was there)
              scale_u8        upsample=True, out_prec=8 "scale", uint8
              sycc_scale_u8   colour="sycc", out_prec=8 "scale", uint8
  420_8     the same from the frame >> 4 (8 bits)
              plain_u8        upsample=True, uint8        (code that was there)
              sycc_u8         colour="sycc", uint8
The legs of a stream alternate round by round.  The figure is dcshift_mct_ms of
grkgpu_get_stats: the HIP-event interval around the final launches of the
decode, which for these single-tile streams is the one converting launch
(grkgpu_get_launch_times covers the DWT launches only).  Reports best, median
and max per leg, and the algorithmic bytes the launch moves, as one JSON line
(--out FILE: appended there).

--legs plain runs only the legs the parent commit has, so that the same script
measures an older build of the library (GRKGPU_LIB=path) in alternating
processes on the same box; --cache DIR keeps the codestreams between them."""
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

SUBS = [(1, 1), (2, 2), (2, 2)]
SCALE8 = dict(out_prec=8, prec_mode="scale")
SYCC8 = dict(colour="sycc", **SCALE8)
LEGS = {"444": [("plain_u16", np.uint16, {}), ("sycc_u16", np.uint16, dict(colour="sycc")),
                ("scale_u8", np.uint8, SCALE8), ("sycc_scale_u8", np.uint8, SYCC8)],
        "420_12": [("plain_u16", np.uint16, dict(upsample=True)), ("scale_u8", np.uint8, dict(upsample=True, **SCALE8)),
                   ("sycc_scale_u8", np.uint8, SYCC8)],
        "420_8": [("plain_u8", np.uint8, dict(upsample=True)), ("sycc_u8", np.uint8, dict(colour="sycc"))]}


def streams(codec, cache, h, w):
    """{(stream, wavelet): codestream}, coded once (and kept in `cache`)."""
    out, frame = {}, None
    for tag, irr in (("97", True), ("53", False)):
        for name in LEGS:
            path = os.path.join(cache, "convert_ab_%s_%s_%dx%d.j2k" % (name, tag, w, h)) if cache else None
            if path and os.path.exists(path):
                out[name, tag] = open(path, "rb").read()
                continue
            if frame is None:
                frame = synth.synth_image(h, w, 3, 12, 3)
            if name == "444":
                cs = bytes(codec.compress(frame, 12, grk.CParams.make(irreversible=irr), view=True))
            else:
                f, bits = (frame, 12) if name == "420_12" else (frame >> 4, 8)
                planes = [np.ascontiguousarray(f[0])] + [np.ascontiguousarray(f[k][::2, ::2]) for k in (1, 2)]
                cs = codec.compress_subsampled(planes, bits, (w, h), SUBS, grk.CParams.make(irreversible=irr, mct=0))
            if path:
                os.makedirs(cache, exist_ok=True)
                with open(path, "wb") as fh:
                    fh.write(cs)
            out[name, tag] = cs
    return out


def launch_bytes(name, dtype, h, w):
    """Algorithmic bytes of the final launch: int32 coefficients read, samples written."""
    read = 4 * h * w * 3 if name == "444" else 4 * (h * w + 2 * ((h + 1) // 2) * ((w + 1) // 2))
    return read + 3 * h * w * np.dtype(dtype).itemsize


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--size", default="7680x4320")
    ap.add_argument("--legs", choices=("all", "plain"), default="all")
    ap.add_argument("--cache")
    ap.add_argument("--label", default="")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.rounds < 5:
        ap.error("at least 5 rounds")
    w, h = (int(v) for v in args.size.split("x"))
    codec = grk.Codec(0)
    css = streams(codec, args.cache, h, w)
    res = {"device": torch.cuda.get_device_name(0), "date": datetime.date.today().isoformat(), "label": args.label,
           "lib": os.path.basename(os.path.dirname(grk.LIB_PATH)), "size": args.size, "rounds": args.rounds,
           "figure": "dcshift_mct_ms: best / median / max"}
    for (name, tag), cs in sorted(css.items()):
        legs = [leg for leg in LEGS[name] if args.legs == "all" or leg[0].startswith("plain")]
        outs = {leg: torch.empty((h, w, 3), dtype=getattr(torch, np.dtype(dt).name), device="cuda:0")
                for leg, dt, _ in legs}
        times = {leg: [] for leg, _, _ in legs}
        for r in range(args.warmup + args.rounds):
            for leg, dt, kw in legs:
                codec.decompress(cs, out=outs[leg], layout="hwc", **kw)
                if r >= args.warmup:
                    times[leg].append(codec.stats()["dcshift_mct_ms"])
        res["%s_%s" % (name, tag)] = {
            leg: {"best": round(min(times[leg]), 4), "median": round(statistics.median(times[leg]), 4),
                  "max": round(max(times[leg]), 4), "bytes": launch_bytes(name, dt, h, w)} for leg, dt, _ in legs}
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
