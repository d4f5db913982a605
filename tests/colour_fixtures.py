"""The colour steps of grk_decompress that the decode stores apply -- eYCC ->
RGB, CMYK -> RGB, force-RGB -- as numpy closed forms, and the seeded inputs on
which tests/golden/manifest_colour.json pins them to the reference
(scripts/make_golden_colour.py runs the reference's own color.cpp over the
same inputs and records a sha256 per case).

The closed forms restate include/grk_mi355x.h: float64 (eYCC) / float32
(CMYK) with every operation rounded on its own -- numpy never contracts --
and truncating conversions."""
import hashlib
import json
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MANIFEST = os.path.join(GOLD, "manifest_colour.json")


def eycc_to_rgb(y, cb, cr, prec, sgnd_cb=False, sgnd_cr=False):
    """color_esycc_to_rgb on int arrays of one shape -> (R, G, B) int32."""
    flip, top = 1 << (prec - 1), (1 << prec) - 1
    y = np.asarray(y, dtype=np.int64).astype(np.float64)
    cb = (np.asarray(cb, dtype=np.int64) - (0 if sgnd_cb else flip)).astype(np.float64)
    cr = (np.asarray(cr, dtype=np.int64) - (0 if sgnd_cr else flip)).astype(np.float64)
    r = ((y - 0.0000368 * cb) + 1.40199 * cr) + 0.5
    g = ((1.0003 * y - 0.344125 * cb) - 0.7141128 * cr) + 0.5
    b = ((0.999823 * y + 1.77204 * cb) - 0.000008 * cr) + 0.5
    return tuple(np.clip(np.trunc(v).astype(np.int64), 0, top).astype(np.int32) for v in (r, g, b))


def cmyk_to_rgb(planes, precs):
    """color_cmyk_to_rgb: planes[0 .. 3] the inks (precisions precs[0 .. 3]),
    any further planes passed through -> the list of len(planes) - 1 channels."""
    one, c255 = np.float32(1.0), np.float32(255.0)
    inv = []
    for k in range(4):
        s = one / np.float32((1 << precs[k]) - 1)  # one correctly rounded float32 division
        inv.append(one - np.asarray(planes[k]).astype(np.float32) * s)
    C, M, Y, K = inv
    rgb = [((c255 * v) * K).astype(np.int32) for v in (C, M, Y)]  # (astype truncates)
    return rgb + [np.asarray(p, dtype=np.int32) for p in planes[4:]]


def force_rgb(planes):
    """convert_gray_to_rgb: one or two channels -> the first three times, the second behind it."""
    return [planes[0]] * 3 + list(planes[1:]) if 1 <= len(planes) <= 2 else list(planes)


def clip_prec(v, p, signed=False):
    """grk_decompress -p N (clip)"""
    return np.clip(v, -(1 << (p - 1)) if signed else 0, ((1 << (p - 1)) if signed else (1 << p)) - 1)


def scale_prec(v, p, q, signed=False):
    """grk_decompress -p NS (scale) of a component of precision q"""
    v = np.asarray(v).astype(np.int64)
    if p == q:
        return v
    if p < q:
        return v >> (q - p)
    return v * (1 << (p - q)) if signed else v * ((1 << p) - 1) // ((1 << q) - 1)


# ---------------------------------------------------------------------------
# the pinned cases: name -> (kind, precs, sgnds, planes), regenerated from seeds
# ---------------------------------------------------------------------------
N_RANDOM = 20000


def _unsigned(rs, prec, n):
    return rs.randint(0, 1 << prec, size=n).astype(np.int32)


def _signed(rs, prec, n):
    return rs.randint(-(1 << (prec - 1)), 1 << (prec - 1), size=n).astype(np.int32)


def cases():
    out = {}
    cb, cr = [a.ravel().astype(np.int32) for a in np.meshgrid(np.arange(256), np.arange(256), indexing="ij")]
    for yv in (0, 128, 255):
        out["eycc_p8_grid_y%d" % yv] = ("eycc", [8] * 3, [0, 0, 0], [np.full(65536, yv, np.int32), cb, cr])
    for i, prec in enumerate((8, 10, 12, 16)):
        for sg in (0, 1):
            rs = np.random.RandomState(7100 + 2 * i + sg)
            chroma = _signed if sg else _unsigned
            out["eycc_p%d_%s" % (prec, "signed" if sg else "unsigned")] = (
                "eycc", [prec] * 3, [0, sg, sg],
                [_unsigned(rs, prec, N_RANDOM), chroma(rs, prec, N_RANDOM), chroma(rs, prec, N_RANDOM)])
    ink, k = cb, cr
    out["cmyk_q8_grid"] = ("cmyk", [8] * 4, [0] * 4, [ink, (ink * 7 + 3) & 255, 255 - ink, k])
    for i, precs in enumerate(([8, 8, 12, 16], [12, 12, 12, 12], [16, 1, 8, 10])):
        rs = np.random.RandomState(7200 + i)
        out["cmyk_q%s" % "_".join(str(p) for p in precs)] = (
            "cmyk", precs, [0] * 4, [_unsigned(rs, p, N_RANDOM) for p in precs])
    rs = np.random.RandomState(7300)
    out["cmyk_5comp"] = ("cmyk", [8, 8, 8, 8, 12], [0, 0, 0, 0, 1],
                         [_unsigned(rs, 8, N_RANDOM) for _ in range(4)] + [_signed(rs, 12, N_RANDOM)])
    return out


def closed_form(kind, precs, sgnds, planes):
    """-> (output planes, [(prec, sgnd), ...] as this project reports them)"""
    if kind == "eycc":
        return list(eycc_to_rgb(planes[0], planes[1], planes[2], precs[0], sgnds[1], sgnds[2])), [(precs[0], 0)] * 3
    chans = [(8, 0)] * 3 + [(p, s) for p, s in zip(precs[4:], sgnds[4:])]
    return cmyk_to_rgb(planes, precs), chans


def digest(planes):
    h = hashlib.sha256()
    for p in planes:
        h.update(np.ascontiguousarray(p, dtype="<i4").tobytes())
    return h.hexdigest()


def manifest():
    with open(MANIFEST) as f:
        return json.load(f)
