"""Palette store A/B: what the JP2 palette lookup costs in the store of the last
decode kernel (Codec.decompress_jp2, k_palette_pixels<uint8, 3>) against the
two plain stores it sits between.  One process, one Codec; an 8K
single-component 8-bit image (tests/golden/synth.py, seed 3, component 0 >> 4),
5/3, one tile, every leg into device memory:
  plain_gray_u8     Codec.decompress of the index codestream, uint8 (h,w): 4 B read + 1 B written per pixel
  plain_rgb_hwc_u8  Codec.decompress of the 3-component 8-bit frame (no MCT), uint8 (h,w,3): 12 B read + 3 B written
  palette_hwc_u8    Codec.decompress_jp2 of the index codestream inside a JP2 file with a 256 x 3 8-bit palette,
                    uint8 (h,w,3): 4 B read + 3 B written
and, for the writer, compress against compress_jp2 of the gray frame (gather_ms
and total_ms of grkgpu_get_stats): the boxes ride in the gather's header blob.
The legs alternate round by round.  The decode figure is dcshift_mct_ms: the
HIP-event interval around the final launches, for these single-tile streams
the one store launch (the palette table goes to the device before it, in the
H2D interval).  Reports best, median and max per leg and the
algorithmic bytes, as one JSON line (--out FILE: appended there).

--legs plain runs only the legs an older build has, so that the same script
measures the parent commit's library (GRKGPU_LIB=path) in alternating
processes on the same box; --cache DIR keeps the codestreams between them."""
import argparse
import datetime
import json
import os
import statistics
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "golden")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import grokimagecompression_amd as grk  # noqa: E402
import synth  # noqa: E402


def box(typ, payload):
    return struct.pack(">I", 8 + len(payload)) + typ + payload


def palette_file(cs, h, w):
    """the index codestream inside a JP2 file with a 256 x 3 palette of 8-bit columns"""
    r = np.random.RandomState(1)
    pal = r.randint(0, 256, size=(256, 3)).astype(np.uint8)
    hdr = (box(b"ihdr", struct.pack(">IIHBBBB", h, w, 1, 7, 7, 0, 0)) + box(b"colr", bytes([1, 0, 0]) + struct.pack(">I", 16)) +
           box(b"pclr", struct.pack(">HB", 256, 3) + bytes([7, 7, 7]) + pal.tobytes()) +
           box(b"cmap", b"".join(struct.pack(">HBB", 0, 1, i) for i in range(3))))
    return (box(b"jP  ", b"\x0d\x0a\x87\x0a") + box(b"ftyp", b"jp2 \0\0\0\0jp2 ") + box(b"jp2h", hdr) + box(b"jp2c", cs))


def streams(codec, cache, h, w):
    out = {}
    frame = None
    for name in ("gray", "rgb"):
        path = os.path.join(cache, "palette_ab_%s_%dx%d.j2k" % (name, w, h)) if cache else None
        if path and os.path.exists(path):
            out[name] = open(path, "rb").read()
            continue
        if frame is None:
            frame = synth.synth_image(h, w, 3, 12, 3) >> 4
        img = frame[:1] if name == "gray" else frame
        out[name] = bytes(codec.compress(np.ascontiguousarray(img), 8, grk.CParams.make(mct=0), view=True))
        if path:
            os.makedirs(cache, exist_ok=True)
            with open(path, "wb") as fh:
                fh.write(out[name])
    return out, frame


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
    css, frame = streams(codec, args.cache, h, w)
    px = h * w
    legs = [("plain_gray_u8", lambda: codec.decompress(css["gray"], dtype=np.uint8, device_out=True), 5 * px),
            ("plain_rgb_hwc_u8", lambda: codec.decompress(css["rgb"], dtype=np.uint8, layout="hwc", device_out=True),
             15 * px)]
    if args.legs == "all":
        jp2 = palette_file(css["gray"], h, w)
        legs.append(("palette_hwc_u8",
                     lambda: codec.decompress_jp2(jp2, dtype=np.uint8, layout="hwc", colour=None, device_out=True),
                     7 * px))
    res = {"device": torch.cuda.get_device_name(0), "date": datetime.date.today().isoformat(), "label": args.label,
           "lib": os.path.basename(os.path.dirname(grk.LIB_PATH)), "size": args.size, "rounds": args.rounds,
           "figure": "dcshift_mct_ms: best / median / max"}
    times = {leg: [] for leg, _, _ in legs}
    for r in range(args.warmup + args.rounds):
        for leg, fn, _ in legs:
            fn()
            if r >= args.warmup:
                times[leg].append(codec.stats()["dcshift_mct_ms"])
    res["decode"] = {leg: {"best": round(min(times[leg]), 4), "median": round(statistics.median(times[leg]), 4),
                           "max": round(max(times[leg]), 4), "bytes": nbytes,
                           "TB_per_s": round(nbytes / statistics.median(times[leg]) / 1e9, 3)} for leg, _, nbytes in legs}
    # the writer: the boxes in the gather blob
    if frame is None:
        frame = synth.synth_image(h, w, 3, 12, 3) >> 4
    gray = torch.from_numpy(np.ascontiguousarray(frame[:1]).astype(np.uint8)).cuda()
    enc = [("compress", lambda: codec.compress(gray, 8, grk.CParams.make(mct=0), view=True))]
    if args.legs == "all":
        enc.append(("compress_jp2", lambda: codec.compress_jp2(gray, 8, colour_space="gray", params=grk.CParams.make(mct=0))))
    et = {leg: {"gather_ms": [], "total_ms": []} for leg, _ in enc}
    for r in range(args.warmup + args.rounds):
        for leg, fn in enc:
            fn()
            if r >= args.warmup:
                st = codec.stats()
                for k in et[leg]:
                    et[leg][k].append(st[k])
    res["encode"] = {leg: {k: {"best": round(min(v), 4), "median": round(statistics.median(v), 4), "max": round(max(v), 4)}
                           for k, v in et[leg].items()} for leg, _ in enc}
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
