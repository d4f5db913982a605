"""The p_* fixture family (oracle/make_golden_prec.py, manifest_prec.json):
every precision 1 .. 16, signed samples, 1 .. 5 components, mixed components.
Shared by the CPU chain and the GPU tests."""
import json

import numpy as np

import synth
from conftest import GOLD

PREC = json.load(open(f"{GOLD}/manifest_prec.json"))
REFUSED = sorted(n for n, m in PREC.items() if m.get("ref_enc") == "refused")


def precs(m):
    return list(m.get("prec", [m["shape"][3]] * m["shape"][2]))


def sgnds(m):
    return [bool(s) for s in m.get("sgnd", [m["signed"]] * m["shape"][2])]


def image(m):
    """The case's source image, (c,h,w) int32."""
    h, w, c, bits = m["shape"]
    img = synth.synth_image_mixed(h, w, precs(m), sgnds(m), m["seed"], m["kind"])
    assert synth.image_sha256(img) == m["image_sha256"], "generator drift"
    img.setflags(write=False)
    return img


def stream(name):
    with open(f"{GOLD}/{name}.j2k", "rb") as f:
        return f.read()


def ref_decode(name, tag=""):
    """The reference's decode of the case's stream (a -l / -r variant with
    tag), int32: the stored .dec.npz, or -- a lossless case, dec_vs_src_maxabs
    0 -- the source image, either one checked against the manifest's hash."""
    m = PREC[name]
    if tag or m["dec_vs_src_maxabs"]:
        d = np.load(f"{GOLD}/{name}{'.' + tag if tag else ''}.dec.npz")["dec"].astype(np.int32)
    else:
        d = image(m)
    assert synth.image_sha256(d) == (m["variants"][tag] if tag else m)["dec_sha256"]
    return d


def ranges(m):
    """(min, max) of each component's sample range."""
    return [(-(1 << (p - 1)), (1 << (p - 1)) - 1) if s else (0, (1 << p) - 1) for p, s in zip(precs(m), sgnds(m))]
