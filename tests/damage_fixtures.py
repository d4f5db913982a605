"""The damaged-stream fixture (tests/golden/manifest_damage.json, written by
oracle/make_golden_damage.py with the reference) and the checks on the tables
the decoder's host half hands its device half (grkgpu_dec_tables_of), shared
by tests/test_damage_host.py and tests/test_gpu_damage.py."""
import json
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
OK, EINVAL, EHIP, EUNSUPPORTED, ECORRUPT = 0, -1, -3, -4, -5

_MAN = None


def manifest():
    global _MAN
    if _MAN is None:
        with open(os.path.join(GOLD, "manifest_damage.json")) as f:
            _MAN = json.load(f)
    return _MAN


STREAMS = sorted(manifest())


def clean(name):
    with open(os.path.join(GOLD, name + ".j2k"), "rb") as f:
        return f.read()


def patched(cs, patch):
    b = bytearray(cs)
    for off, val in patch:
        b[off] = val
    return bytes(b)


def cases(name):
    """(case record, damaged stream) of every case of stream `name` that is
    not a listed deviation."""
    cs = clean(name)
    return [(c, patched(cs, c["p"])) for c in manifest()[name]["cases"] if "deviation" not in c]


def error_code(exc):
    """the grkgpu code of a GrkGpuError ("grkgpu error -5: ...")"""
    return int(str(exc).split()[2].rstrip(":"))


def plan_problems(t):
    """What is wrong with the tables `t` of grk.dec_tables(): a list of
    strings, empty when every offset stays inside its buffer and the blocks'
    fields are ones the Tier-1, DWT and store kernels are written for."""
    b, s = t["blocks"], t["segs"]
    sf = t["seg_first"].astype(np.int64)
    nb, ns = len(b), len(s)
    bad = []

    def need(ok, what):
        ok = np.asarray(ok)
        if not ok.all():
            bad.append("%s (%d of %d, first %d)" % (what, int((~ok).sum()), ok.size, int(np.argmin(ok))))

    if len(sf) != nb + 1 or (nb >= 0 and (sf[0] != 0 or sf[-1] != ns)) or np.any(np.diff(sf) < 0):
        return ["seg_first is not a non-decreasing run from 0 to the segment count"]
    slen, spass, soff = s["len"].astype(np.int64), s["npasses"].astype(np.int64), s["data_off"].astype(np.int64)
    need(soff + slen <= t["data_bytes"], "a segment ends past the data buffer")
    clen, cpass = np.concatenate([[0], np.cumsum(slen)]), np.concatenate([[0], np.cumsum(spass)])
    blen = b["len"].astype(np.int64)
    npass, nbps = b["numpasses"].astype(np.int64), b["numbps"].astype(np.int64)
    need(clen[sf[1:]] - clen[sf[:-1]] == blen, "a block's len is not the sum of its segments'")
    need(cpass[sf[1:]] - cpass[sf[:-1]] >= npass, "a block has more passes than its segments")
    need(npass <= np.maximum(0, 3 * nbps - 2), "numpasses above 3 * numbps - 2")
    need((blen != 0) | (npass == 0), "passes in a block without bytes")
    need((npass == 0) | (nbps <= 30), "more than 30 bit-planes in a block that is decoded")
    w, h, ds = b["w"].astype(np.int64), b["h"].astype(np.int64), b["dstride"].astype(np.int64)
    need((w >= 1) & (w <= 64) & (h >= 1) & (h <= 64), "block size outside 1 .. 64")
    need(ds >= w, "dstride below the block's width")
    need(b["orient"] <= 3, "orient above 3")
    dst = b["dst_off"].astype(np.int64)
    need((dst >= 0) & (dst + (h - 1) * ds + w <= t["coef_elems"]), "a block ends past the coefficient arena")
    if bad:
        return bad
    hits = np.zeros(int(t["coef_elems"]), np.uint8)
    for i in range(nb):
        idx = dst[i] + np.arange(h[i])[:, None] * ds[i] + np.arange(w[i])[None, :]
        hits[idx] += 1
    if hits.size and hits.max() > 1:
        bad.append("blocks overlap in the coefficient arena (%d samples)" % int((hits > 1).sum()))
    return bad


def planes_sha(out):
    """sha256 of a decode as the manifest records it: the (c, h, w) int32
    image, or a subsampled stream's planes flattened one after the other."""
    import hashlib
    if isinstance(out, (list, tuple)):
        out = np.concatenate([np.asarray(p).ravel() for p in out])
    return hashlib.sha256(np.ascontiguousarray(out, dtype=np.int32).tobytes()).hexdigest()
