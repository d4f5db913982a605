"""Colour-converting decode A/B: what eYCC -> RGB and CMYK -> RGB cost in the
store of the last decode kernel (Codec.decompress(colour="eycc" | "cmyk"),
Codec.decompress_jp2(colour="auto_rgb")) against the only route there was
before them, and against the plain stores beside them.  One process, one
Codec; the bench's 8K frame (tests/golden/synth.py, seed 3), 5/3 lossless,
every leg into host memory, as a consumer without a GPU pipeline receives it:

  cmyk8   a 4-component 8-bit CMYK .jp2 (EnumCS 12) -> (h,w,3) uint8
            fused      decompress_jp2(colour="auto_rgb", dtype=uint8, layout="hwc")
            host       decompress_jp2(colour="auto") -> (4,h,w) int32 host planes, then
                       the numpy closed form (tests/colour_fixtures.py) on the CPU,
                       cast and interleaved
  eycc12  a 3-component 12-bit eYCC stream -> (h,w,3) uint16
            fused      decompress(colour="eycc", dtype=uint16, layout="hwc")
            host       decompress() -> (3,h,w) int32, then the numpy closed form
  store   the final launch alone (dcshift_mct_ms of grkgpu_get_stats, the HIP-event
          interval around it), into a device tensor (h,w,c):
            cmyk8:   plain_u8 (4 channels)   cmyk_u8 (3 channels)
            eycc12:  plain_u16   sycc_u16 (the int/f64 chroma terms)   eycc_u16 (the f64 map)

The legs alternate round by round.  wall_ms is a host clock around calls that
end in a stream synchronise (and, for "host", the CPU pass); pcie_bytes what
leaves the device.  One JSON line (--out FILE: appended there)."""
import argparse
import datetime
import json
import os
import statistics
import struct
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import colour_fixtures as cf  # noqa: E402
import grokimagecompression_amd as grk  # noqa: E402
import synth  # noqa: E402


def _box(typ, payload=b""):
    return struct.pack(">I", 8 + len(payload)) + typ + payload


def jp2_cmyk(cs, h, w):
    head = _box(b"ihdr", struct.pack(">IIHBBBB", h, w, 4, 7, 7, 0, 0)) + _box(b"colr", bytes([1, 0, 0]) + struct.pack(">I", 12))
    return (_box(b"jP  ", b"\x0d\x0a\x87\x0a") + _box(b"ftyp", b"jp2 " + b"\0\0\0\0" + b"jp2 ") + _box(b"jp2h", head) +
            _box(b"jp2c", cs))


def stat(v):
    return {"best": round(min(v), 3), "median": round(statistics.median(v), 3), "max": round(max(v), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--size", default="7680x4320")
    ap.add_argument("--label", default="")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.rounds < 5:
        ap.error("at least 5 rounds")
    w, h = (int(v) for v in args.size.split("x"))
    codec = grk.Codec(0)
    f12 = synth.synth_image(h, w, 3, 12, 3)
    f8 = np.concatenate([f12 >> 4, (f12[:1] >> 4) ^ 0x5A])  # four 8-bit inks
    p = grk.CParams.make(mct=0)
    cmyk = jp2_cmyk(codec.compress(f8, 8, p), h, w)
    eycc = codec.compress(f12, 12, p)
    del f12, f8

    def cmyk_host():
        planes, _ = codec.decompress_jp2(cmyk, colour="auto")
        rgb = cf.cmyk_to_rgb(list(planes), [8] * 4)
        return np.stack(rgb, axis=-1).astype(np.uint8)

    def eycc_host():
        planes = codec.decompress(eycc)
        return np.stack(cf.eycc_to_rgb(planes[0], planes[1], planes[2], 12), axis=-1).astype(np.uint16)

    routes = {
        "cmyk8": [("fused", lambda: codec.decompress_jp2(cmyk, colour="auto_rgb", dtype=np.uint8, layout="hwc")[0],
                   3 * h * w), ("host", cmyk_host, 16 * h * w)],
        "eycc12": [("fused", lambda: codec.decompress(eycc, colour="eycc", dtype=np.uint16, layout="hwc"), 6 * h * w),
                   ("host", eycc_host, 12 * h * w)],
    }
    res = {"device": torch.cuda.get_device_name(0), "date": datetime.date.today().isoformat(), "label": args.label,
           "size": args.size, "rounds": args.rounds}
    for name, legs in routes.items():
        wall = {leg: [] for leg, _, _ in legs}
        outs = {}
        for r in range(args.warmup + args.rounds):
            for leg, fn, _ in legs:
                t0 = time.perf_counter()
                outs[leg] = fn()
                if r >= args.warmup:
                    wall[leg].append((time.perf_counter() - t0) * 1e3)
        assert np.array_equal(outs["fused"], outs["host"]), name  # faster and different is not faster
        res[name] = {leg: dict(wall_ms=stat(wall[leg]), pcie_bytes=b) for leg, _, b in legs}
    # the final launch alone, into device tensors
    stores = {
        "cmyk8": (cmyk[cmyk.index(b"jp2c") + 4:], [("plain_u8", torch.uint8, 4, {}), ("cmyk_u8", torch.uint8, 3, dict(colour="cmyk"))]),
        "eycc12": (eycc, [("plain_u16", torch.uint16, 3, {}), ("sycc_u16", torch.uint16, 3, dict(colour="sycc")),
                          ("eycc_u16", torch.uint16, 3, dict(colour="eycc"))]),
    }
    for name, (cs, legs) in stores.items():
        bufs = {leg: torch.empty((h, w, c), dtype=dt, device="cuda:0") for leg, dt, c, _ in legs}
        times = {leg: [] for leg, _, _, _ in legs}
        for r in range(args.warmup + args.rounds):
            for leg, dt, c, kw in legs:
                codec.decompress(cs, out=bufs[leg], layout="hwc", **kw)
                if r >= args.warmup:
                    times[leg].append(codec.stats()["dcshift_mct_ms"])
        ncomp = 4 if name == "cmyk8" else 3
        res[name]["store"] = {leg: dict(dcshift_mct_ms=stat(times[leg]),
                                        bytes=4 * h * w * ncomp + h * w * c * bufs[leg].element_size())
                              for leg, _, c, _ in legs}
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
