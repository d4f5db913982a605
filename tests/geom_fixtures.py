"""The geometry sweep (oracle/make_golden_geom.py, manifest_geom.json): 256
machine-drawn small images, each pinned by the reference's codestream and
decode hashes alone.  Shared by the CPU chain (tests/test_oracle_golden.py)
and the GPU test (tests/test_gpu_geom.py); nothing here runs the sampler."""
import functools
import hashlib
import json

import numpy as np

import synth
from conftest import GOLD

GEOM = json.load(open(f"{GOLD}/manifest_geom.json"))
CASES = GEOM["cases"]
BY_NAME = {m["name"]: m for m in CASES}
CHUNK = 32
CODES = {"GRKGPU_EINVAL": -1, "GRKGPU_EUNSUPPORTED": -4}


def cd(a, b):
    return -(-a // b)


def opt(m, name, default=None):
    a = m["args"]
    return a[a.index(name) + 1] if name in a else default


def pair(v):
    return tuple(int(x) for x in v.split(","))


def offset(m):
    return pair(opt(m, "-d", "0,0"))


def subsampling(m):
    return [tuple(s) for s in m["subsampling"]] if m["subsampling"] else [(1, 1)] * m["comps"]


def planes_sha(planes):
    """The manifest's hash of a decode: the components' int32 planes one after the other."""
    return hashlib.sha256(b"".join(np.ascontiguousarray(p, dtype="<i4").tobytes() for p in planes)).hexdigest()


@functools.lru_cache(maxsize=None)
def _planes(name):
    m = BY_NAME[name]
    (x0, y0), (w, h) = offset(m), m["size"]
    out = [synth.synth_image(cd(y0 + h, dy) - cd(y0, dy), cd(x0 + w, dx) - cd(x0, dx), 1, m["bits"], m["seed"] + k,
                             m["kind"])[0] for k, (dx, dy) in enumerate(subsampling(m))]
    assert planes_sha(out) == m["src_sha256"], "generator drift"
    for p in out:
        p.setflags(write=False)
    return out


def planes(m):
    """The case's source planes, component k on its grid (read-only, computed once)."""
    return _planes(m["name"])


def image(m):
    """The source of a case without subsampling, (c,h,w) int32."""
    assert not m["subsampling"]
    a = np.stack(planes(m))
    a.setflags(write=False)
    return a


def narrow_dtype(m):
    """The narrowest numpy dtype holding the case's (unsigned) samples."""
    return np.uint8 if m["bits"] <= 8 else np.uint16


def variant_kw(v):
    a = v["args"]
    return {"reduce": int(a[1])} if a[0] == "-r" else {"window": pair(a[1])}


def tile_of(m, k, y, x):
    """The tile (index, column, row) holding sample (y, x) of component k's full-resolution plane."""
    (x0, y0), (w, h) = offset(m), m["size"]
    dx, dy = subsampling(m)[k]
    if "-t" not in m["args"]:
        return 0, 0, 0
    (tdx, tdy), (tx0, ty0) = pair(opt(m, "-t")), pair(opt(m, "-T", "0,0"))
    # component sample X lies in the tile column p with ceil(tile x0 / dx) <= X < ceil(tile x1 / dx)
    X, Y = x + cd(x0, dx), y + cd(y0, dy)
    tw = cd(x0 + w - tx0, tdx)
    p = max(i for i in range(tw) if cd(max(tx0 + i * tdx, x0), dx) <= X)
    q = max(j for j in range(cd(y0 + h - ty0, tdy)) if cd(max(ty0 + j * tdy, y0), dy) <= Y)
    return q * tw + p, p, q


def first_difference(m, got, ref):
    """'component k, y, x (tile t = column p, row q): got a, reference b' for the first differing sample."""
    for k, (a, b) in enumerate(zip(got, ref)):
        a, b = np.asarray(a), np.asarray(b)
        if a.shape != b.shape:
            return "component %d has shape %s, the reference %s" % (k, a.shape, b.shape)
        bad = np.argwhere(a != b)
        if len(bad):
            y, x = (int(v) for v in bad[0])
            return ("%d samples of component %d differ, first at y %d, x %d (tile %d = column %d, row %d): got %d, "
                    "reference %d" % ((len(bad), k, y, x) + tile_of(m, k, y, x) + (int(a[y, x]), int(b[y, x]))))
    return "no sample differs"
