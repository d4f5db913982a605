"""The JP2 fixtures (scripts/make_golden_jp2.py) for the tests: files, the
reference's decodes, and the source planes of the files the reference encoded."""
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
MAN = json.load(open(os.path.join(GOLD, "manifest_jp2.json")))
A = sorted(t for t, r in MAN.items() if r["kind"] == "A")
B = sorted(t for t, r in MAN.items() if r["kind"] == "B")
C = sorted(t for t, r in MAN.items() if r["kind"] == "C")
PALETTE = sorted(t for t, r in MAN.items() if r["kind"] == "B" and r["palette"])
ICC300 = bytes((i * 7 + 3) & 0xFF for i in range(300))
_dec = {}


def load(tag):
    with open(os.path.join(GOLD, tag + ".jp2"), "rb") as f:
        return f.read()


def ref_planes(tag, variant=None):
    """the reference's decode: a list of int32 (h, w) planes, one per output channel"""
    if tag not in _dec:
        z = np.load(os.path.join(GOLD, tag + ".dec.npz"))
        _dec[tag] = {k: z[k].astype(np.int32) for k in z.files}
    pre = (variant + "_p") if variant else "p"
    n = len([k for k in _dec[tag] if k.startswith(pre) and k[len(pre):].isdigit()])
    return [_dec[tag][pre + str(k)] for k in range(n)]


def ref_image(tag, variant=None):
    """(c, h, w) int32 of a file whose channels share one grid"""
    return np.stack(ref_planes(tag, variant))


def option(args, name):
    return [int(v) for v in args[args.index(name) + 1].split(",")] if name in args else None


def source_planes(tag):
    """the planes the reference encoded into an A file (make_golden_jp2.a_planes)"""
    import synth
    spec = MAN[tag]["spec"]
    h, w, c, bits = spec["shape"]
    precs = option(spec["args"], "-prec") or [bits] * c
    img = synth.synth_image(h, w, c, max(precs), spec["seed"], "smooth")
    if spec["sgnd"]:
        img = img - (1 << (bits - 1))
    planes = []
    for k in range(c):
        dx, dy = spec["subsampling"][k] if spec["subsampling"] else (1, 1)
        planes.append(np.ascontiguousarray((img[k] >> (max(precs) - precs[k]))[::dy, ::dx]))
    return planes


def codec_args(args):
    """the driver options that are grk_compress's (CParams.from_cli)"""
    out, i = [], 0
    while i < len(args):
        if args[i] in ("-alpha", "-icc", "-prec", "-sub"):
            i += 2
            continue
        out.append(args[i])
        i += 1
    return out
