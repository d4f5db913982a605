"""A seeded sweep of odd geometries, pinned by the REFERENCE by hashes alone
(oracle/_ref/ref_driver; no .j2k / .npy is stored, as manifest_large.json).

256 small images are drawn by random.Random(SEED): image origin and size,
tile grid and its origin, resolutions, wavelet, MCT, code-block and precinct
sizes, progression, two-layer rate control, per-component subsampling.  From
the geometry alone every case is sorted into the edge classes below; the
draw is steered (a focus per draw, rejection against classes_of) until every
class has MIN_CLASS members.  A case the reference does not encode is
dropped, never recorded; at most MAX_DROP of the cases handed to it may be.

 a    a tile-component with an empty resolution that another tile has samples in
 b    a tile-component 1 sample wide or high
 c    first tile column / row clipped to 1 sample by the image origin
 d    last tile column / row 1 sample wide
 e<xy> origin parity (x0 & 1, y0 & 1) with numres >= 3, each of the four
 f    a precinct smaller than the nominal code-block at some resolution
 g    a precinct that holds no code-block of some band
 h<P> RPCL / PCRL / CPRL, >= 2 tiles, >= 2 components, precincts, odd tile origin
 i<P> the same with subsampled components
 j    a lowest resolution of 1 x 1
 k    numres = 1 with >= 2 tiles
 l<wxh> code-block 4x4, 64x4, 4x64
 m    a tile in which a subsampled component has no sample: LEFT OUT -- the
      reference refuses every such image ("Error allocating tile component
      data"); M_PROBES below are handed to it on every run to show that.
 l1024x4 / l4x1024: the reference codes them, the library refuses code-block
      sides above 64 (GRKGPU_EINVAL); N_WIDE of each are kept as refusal cases
      ("refuse" in the manifest), which is what the 5 % bound on refusals leaves
      room for -- they are no class of MIN_CLASS members.

Each kept case records the reference's codestream hash and length and the hash
of its decode (planes_sha: the components' int32 planes one after the other);
a seeded half also one -r decode (hash of the decoded samples: with an origin
that is no multiple of 2^r the reference sizes the plane one row / column
larger and leaves that uninitialised, make_golden.py DEC_VARIANTS) and one -d
window through a tile seam.  Component k's source plane is
synth.synth_image(h_k, w_k, 1, bits, seed + k, kind)[0].

Writes tests/golden/manifest_geom.json.
  python oracle/make_golden_geom.py [--check]"""
import json
import os
import random
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE]

import numpy as np  # noqa: E402

import make_golden as mg  # noqa: E402
from make_golden_sub import planes_sha, sub_arg  # noqa: E402

SEED = 20260
N_CASES = 256
MIN_CLASS = 8
N_WIDE = 4          # kept cases of each of -b 1024,4 and -b 4,1024 (library refusals)
MAX_DROP = 0.10     # share of the cases handed to the reference that it may refuse
DRAW_LIMIT = 400000  # sampler draws (geometry only) before the generator gives up
PROGS = ["LRCP", "RLCP", "RPCL", "PCRL", "CPRL"]
TILE_SIDES = [1, 2, 3, 17, 33, 48, 64, 100]
CBLKS = [(32, 32), (16, 16), (8, 8), (4, 4), (64, 4), (4, 64), (16, 64), (64, 16), (8, 32), (32, 8)]
REQUIRED = (["a", "b", "c", "d", "e00", "e01", "e10", "e11", "f", "g"] + ["h" + p[0] for p in PROGS[2:]] +
            ["i" + p[0] for p in PROGS[2:]] + ["j", "k", "l4x4", "l64x4", "l4x64"])
LEFT_OUT = {"m": "the reference refuses every image in which a tile-component has no sample "
                 "(\"Error allocating tile component data\")"}
# (w, h), components' (dx, dy), options: a tile without a sample of the subsampled component
M_PROBES = [((20, 10), [(1, 1), (4, 1)], ["-t", "3,10", "-n", "1"]),
            ((20, 10), [(1, 1), (1, 2)], ["-t", "20,1", "-n", "1"]),
            ((20, 10), [(3, 1), (1, 1)], ["-t", "2,10", "-n", "2"]),
            ((9, 9), [(1, 1), (2, 2), (2, 2)], ["-t", "1,1", "-n", "1", "-d", "2,2", "-T", "2,2"])]


def cd(a, b):
    return -(-a // b)


def opt(args, name, default=None):
    return args[args.index(name) + 1] if name in args else default


def pair(v):
    return tuple(int(x) for x in v.split(","))


def precinct_exps(args, numres):
    """log2 precinct size per resolution as j2k.cpp:1989-2041 derives it from -c
    (entry q is resolution numres - 1 - q; the last entry halves from there on);
    None where a size falls below 2 (1 at resolution 0), which nothing codes."""
    if "-c" not in args:
        return [(15, 15)] * numres
    sizes = [pair(t.strip("[]")) for t in opt(args, "-c").replace("],[", "];[").split(";")]
    out = [None] * numres
    for q in range(numres):
        w, h = sizes[q] if q < len(sizes) else tuple(v >> (q - (len(sizes) - 1)) for v in sizes[-1])
        r = numres - 1 - q
        if min(w, h) < (2 if r else 1):
            return None
        out[r] = (w.bit_length() - 1, h.bit_length() - 1)
    return out


def geometry(case):
    """Tile grid and per tile-component rectangles of a case, None when some
    tile-component is empty or the options are not valid."""
    w, h = case["size"]
    args = case["args"]
    c = case["comps"]
    subs = [tuple(s) for s in case["subsampling"]] if case.get("subsampling") else [(1, 1)] * c
    x0, y0 = pair(opt(args, "-d", "0,0"))
    x1, y1 = x0 + w, y0 + h
    numres = int(opt(args, "-n", "6"))
    tx0, ty0 = pair(opt(args, "-T", "0,0"))
    if tx0 > x0 or ty0 > y0:
        return None
    tiled = "-t" in args
    tdx, tdy = pair(opt(args, "-t")) if tiled else (x1 - tx0, y1 - ty0)
    if tx0 + tdx <= x0 or ty0 + tdy <= y0:
        return None
    tw, th = cd(x1 - tx0, tdx), cd(y1 - ty0, tdy)
    pp = precinct_exps(args, numres)
    if pp is None:
        return None
    # the reference reads a component's source rows ceil(w / dx) samples apart
    # (TileComponent::get_dimensions); where the component is
    # ceil(x1 / dx) - ceil(x0 / dx) != that wide it codes a skewed picture or
    # reads past the plane, and its codestream differs from run to run
    if any(cd(w, dx) != cd(x1, dx) - cd(x0, dx) for dx, dy in subs):
        return None
    tiles = []
    for q in range(th):
        for p in range(tw):
            t = (max(tx0 + p * tdx, x0), max(ty0 + q * tdy, y0), min(tx0 + (p + 1) * tdx, x1), min(ty0 + (q + 1) * tdy, y1))
            comps = []
            for dx, dy in subs:
                r = (cd(t[0], dx), cd(t[1], dy), cd(t[2], dx), cd(t[3], dy))
                if r[2] <= r[0] or r[3] <= r[1]:
                    return None
                comps.append(r)
            tiles.append((t, comps))
    return dict(x0=x0, y0=y0, x1=x1, y1=y1, numres=numres, tx0=tx0, ty0=ty0, tdx=tdx, tdy=tdy, tw=tw, th=th,
                tiled=tiled, pp=pp, tiles=tiles, subs=subs)


def classes_of(case):
    """The edge classes of a case (see the module's text), from its geometry alone; None: not codable."""
    g = geometry(case)
    if g is None:
        return None
    args = case["args"]
    numres, pp = g["numres"], g["pp"]
    cbw, cbh = pair(opt(args, "-b", "64,64"))
    cbw, cbh = cbw.bit_length() - 1, cbh.bit_length() - 1
    out = set()
    ntiles = g["tw"] * g["th"]
    has_res = {}  # (component, resolution) -> {is it empty, per tile}
    for t, comps in g["tiles"]:
        for k, (cx0, cy0, cx1, cy1) in enumerate(comps):
            if cx1 - cx0 == 1 or cy1 - cy0 == 1:
                out.add("b")
            for r in range(numres):
                lvl = numres - 1 - r
                rx0, ry0, rx1, ry1 = (cd(v, 1 << lvl) for v in (cx0, cy0, cx1, cy1))
                empty = rx1 <= rx0 or ry1 <= ry0
                has_res.setdefault((k, r), set()).add(empty)
                if r == 0 and rx1 - rx0 == 1 and ry1 - ry0 == 1:
                    out.add("j")
                if empty:
                    continue
                ppx, ppy = pp[r]
                if "-c" in args and (ppx - (r > 0) < cbw or ppy - (r > 0) < cbh):
                    out.add("f")
                if "g" in out:
                    continue
                gx0, gy0 = (rx0 >> ppx) << ppx, (ry0 >> ppy) << ppy
                npx, npy = cd(rx1 - gx0, 1 << ppx), cd(ry1 - gy0, 1 << ppy)
                nb = lvl + (r > 0)
                for xob, yob in ([(0, 0)] if r == 0 else [(1, 0), (0, 1), (1, 1)]):
                    bx0, bx1 = (cd(v - (xob << (nb - 1) if nb else 0), 1 << nb) for v in (cx0, cx1))
                    by0, by1 = (cd(v - (yob << (nb - 1) if nb else 0), 1 << nb) for v in (cy0, cy1))
                    xs = [min(((gx0 + ((i + 1) << ppx)) >> (r > 0)), bx1) - max((gx0 + (i << ppx)) >> (r > 0), bx0)
                          for i in range(npx)]
                    ys = [min(((gy0 + ((j + 1) << ppy)) >> (r > 0)), by1) - max((gy0 + (j << ppy)) >> (r > 0), by0)
                          for j in range(npy)]
                    if min(xs) <= 0 or min(ys) <= 0:
                        out.add("g")
    if any(len(v) == 2 for v in has_res.values()):
        out.add("a")
    if g["tiled"]:
        if g["tw"] >= 2 and g["tx0"] < g["x0"] and g["tx0"] + g["tdx"] - g["x0"] == 1:
            out.add("c")
        if g["th"] >= 2 and g["ty0"] < g["y0"] and g["ty0"] + g["tdy"] - g["y0"] == 1:
            out.add("c")
        if g["tw"] >= 2 and g["x1"] - (g["tx0"] + (g["tw"] - 1) * g["tdx"]) == 1:
            out.add("d")
        if g["th"] >= 2 and g["y1"] - (g["ty0"] + (g["th"] - 1) * g["tdy"]) == 1:
            out.add("d")
        if numres == 1 and ntiles >= 2:
            out.add("k")
    if numres >= 3:
        out.add("e%d%d" % (g["x0"] & 1, g["y0"] & 1))
    prog = opt(args, "-p", "LRCP")
    if (prog in PROGS[2:] and ntiles >= 2 and case["comps"] >= 2 and "-c" in args and g["tiled"]
            and (g["tx0"] | g["ty0"]) & 1):
        out.add(("i" if case.get("subsampling") else "h") + prog[0])
    b = opt(args, "-b")
    if b in ("4,4", "64,4", "4,64", "1024,4", "4,1024"):
        out.add("l" + b.replace(",", "x"))
    return sorted(out)


def draw(rng, focus):
    """One case from the sampler; `focus` (a class tag or None) bends the draw towards that class."""
    f = focus or ""
    sub = rng.random() < 0.125 if not f else f[0] == "i"
    c = rng.choice([1, 1, 2, 3, 3, 4])
    if f[:1] in ("h", "i") or sub:
        c = rng.choice([2, 3, 3, 4])
    bits = rng.choice([8, 12, 16])
    kind = rng.choice(["smooth", "uniform"])
    x0, y0 = (rng.choice([0, rng.randint(0, 70)]) for _ in range(2))

    def side():
        u = rng.random()
        return 1 if u < 0.08 else rng.randint(2, 8) if u < 0.25 else rng.randint(9, 160)
    w, h = side(), side()
    args = []
    tiled = rng.random() < 0.55 or f[:1] in ("c", "d", "h", "i", "k")
    tdx = tdy = 0
    if tiled:
        pool = ([t for t in TILE_SIDES if t >= 17] if f[:1] in ("h", "i") else
                [t for t in TILE_SIDES if t <= 64] if f == "c" else TILE_SIDES)
        tdx, tdy = rng.choice(pool), rng.choice(pool)
        w, h = min(w, tdx * rng.randint(1, 6)), min(h, tdy * rng.randint(1, 6))
        tx0, ty0 = rng.randint(max(0, x0 - tdx + 1), x0), rng.randint(max(0, y0 - tdy + 1), y0)
        if f == "c":  # the first column / row keeps one sample
            if rng.random() < 0.5 and tdx > 1:
                x0 = max(x0, tdx - 1)
                tx0, w = x0 - tdx + 1, max(w, 2)
            elif tdy > 1:
                y0 = max(y0, tdy - 1)
                ty0, h = y0 - tdy + 1, max(h, 2)
        if f == "d":
            if rng.random() < 0.5:
                w = tx0 + tdx * rng.randint(1, 4) + 1 - x0
            else:
                h = ty0 + tdy * rng.randint(1, 4) + 1 - y0
        if f[:1] in ("h", "i"):
            if rng.random() < 0.5:
                x0 = min(x0 | 1, 69)
                tx0 = min(x0, tx0 | 1)
            else:
                y0 = min(y0 | 1, 69)
                ty0 = min(y0, ty0 | 1)
            w, h = max(w, tdx + 2), max(h, 2)
        args += ["-t", "%d,%d" % (tdx, tdy)]
        if (tx0, ty0) != (0, 0) or rng.random() < 0.2:
            args += ["-T", "%d,%d" % (tx0, ty0)]
    if (x0, y0) != (0, 0):
        args += ["-d", "%d,%d" % (x0, y0)]
    numres = 1 if f == "k" else rng.choice([1, 2, 2, 3, 3, 4, 4, 5, 6, 6, 7, 8, 9])
    if f[:1] == "e":
        numres = max(numres, 3)
    if numres != 6 or rng.random() < 0.5:
        args += ["-n", str(numres)]
    if rng.random() < 0.35:
        args.append("-I")
    if c >= 3 and rng.random() < 0.6:
        args += ["-Y", str(rng.randint(0, 1))]
    if f[:1] == "l":
        args += ["-b", f[1:].replace("x", ",")]
    elif rng.random() < 0.6:
        args += ["-b", "%d,%d" % rng.choice(CBLKS)]
    if rng.random() < 0.45 or f[:1] in ("f", "g", "h", "i"):
        n = rng.randint(1, numres)
        lo = rng.choice([1, 2, 3, 3])
        args += ["-c", ",".join("[%d,%d]" % (1 << rng.randint(lo, 7), 1 << rng.randint(lo, 7)) for _ in range(n))]
    if f[:1] in ("h", "i"):
        args += ["-p", {"R": "RPCL", "P": "PCRL", "C": "CPRL"}[f[1]]]
    elif rng.random() < 0.7:
        args += ["-p", rng.choice(PROGS)]
    if rng.random() < 0.125:
        args += ["-r", "%d,1" % rng.choice([40, 20, 10, 5])]
    subs = None
    if sub:
        subs = [[rng.randint(1, 4), rng.randint(1, 4)] for _ in range(c)]
        if rng.random() < 0.6:
            subs[0] = [1, 1]
        if c >= 3 and rng.random() < 0.4:
            subs[2] = subs[1]
        if all(v == [1, 1] for v in subs):
            subs[-1] = [2, rng.randint(1, 4)]
    return dict(size=[w, h], comps=c, bits=bits, kind=kind, seed=rng.randint(1, 4000), subsampling=subs, args=args)


def planes_of(case):
    """The source planes: component k on its grid, synth seed + k."""
    g = geometry(case)
    return [mg.synth.synth_image(cd(g["y1"], dy) - cd(g["y0"], dy), cd(g["x1"], dx) - cd(g["x0"], dx), 1,
                                 case["bits"], case["seed"] + k, case["kind"])[0] for k, (dx, dy) in enumerate(g["subs"])]


def ref_encode(case, tmp):
    """The reference's codestream, or None where it refuses (or runs out of 4 GiB, or of a minute)."""
    src = os.path.join(tmp, "in.i32")
    out = os.path.join(tmp, "out.j2k")
    with open(src, "wb") as f:
        for p in planes_of(case):
            f.write(np.ascontiguousarray(p, dtype="<i4").tobytes())
    if os.path.exists(out):
        os.remove(out)
    cmd = ([mg.DRIVER, "enc", src, out, str(case["size"][0]), str(case["size"][1]), str(case["comps"]),
            str(case["bits"]), "0"] + list(case["args"]) + (sub_arg([tuple(s) for s in case["subsampling"]])
                                                           if case["subsampling"] else []))
    try:
        r = subprocess.run(["sh", "-c", 'ulimit -v 4194304; exec "$@"', "sh"] + cmd, capture_output=True, text=True,
                           timeout=60)
    except subprocess.TimeoutExpired:
        return None, "timeout"
    if r.returncode != 0 or not os.path.exists(out):
        return None, (r.stderr.strip().splitlines() or ["exit %d" % r.returncode])[0][:100]
    with open(out, "rb") as f:
        return f.read(), ""


def draw_variants(rng, case):
    """One -r and one -d decode of a case: [args, ...]."""
    g = geometry(case)
    out = []
    if g["numres"] >= 2:
        out.append(["-r", str(rng.randint(1, min(g["numres"] - 1, 5)))])
    mx, my = (max(s[i] for s in g["subs"]) for i in (0, 1))

    def span(a0, a1, t0, td, m):
        if a1 - a0 < 2 * m + 2:
            return a0, a1
        seams = [s for s in range(t0 + td, a1, td) if a0 + m <= s <= a1 - m] if g["tiled"] else []
        if seams:
            s = rng.choice(seams)
            return rng.randint(a0, s - m), rng.randint(s + m, a1)
        lo = rng.randint(a0, a1 - m - 1)
        return lo, rng.randint(lo + m, a1)
    wx0, wx1 = span(g["x0"], g["x1"], g["tx0"], g["tdx"], mx)
    wy0, wy1 = span(g["y0"], g["y1"], g["ty0"], g["tdy"], my)
    if (wx0, wy0, wx1, wy1) != (g["x0"], g["y0"], g["x1"], g["y1"]):
        out.append(["-d", "%d,%d,%d,%d" % (wx0, wy0, wx1, wy1)])
    return out


def valid_dims(case, reduce):
    """Decoded samples of a whole-image -r decode, (h, w) per component."""
    g = geometry(case)
    R = 1 << reduce
    return [[cd(cd(g["y1"], dy), R) - cd(cd(g["y0"], dy), R), cd(cd(g["x1"], dx), R) - cd(cd(g["x0"], dx), R)]
            for dx, dy in g["subs"]]


def refusal_of(case):
    """The library's refusal of a case the reference codes (a GRKGPU_E* name), or None."""
    if max(pair(opt(case["args"], "-b", "64,64"))) > 64:
        return "GRKGPU_EINVAL"
    return None


def vtag(a):
    return "".join(x.strip("-").replace(",", "_") for x in a)


def generate(log=print):
    rng = random.Random(SEED)
    counts = {t: 0 for t in REQUIRED + ["l1024x4", "l4x1024"]}
    need = {t: MIN_CLASS for t in REQUIRED}
    need.update({"l1024x4": N_WIDE, "l4x1024": N_WIDE})
    cases, draws, handed, dropped, reasons = [], 0, 0, 0, {}
    with tempfile.TemporaryDirectory() as tmp:
        for size, subs, args in M_PROBES:
            assert geometry(dict(size=list(size), comps=len(subs), subsampling=subs, args=args)) is None
            x0, y0 = pair(opt(args, "-d", "0,0"))
            with open(os.path.join(tmp, "in.i32"), "wb") as f:
                for dx, dy in subs:
                    f.write(np.zeros((cd(y0 + size[1], dy) - cd(y0, dy)) * (cd(x0 + size[0], dx) - cd(x0, dx)), "<i4").tobytes())
            r = subprocess.run([mg.DRIVER, "enc", os.path.join(tmp, "in.i32"), os.path.join(tmp, "m.j2k"), str(size[0]),
                                str(size[1]), str(len(subs)), "8", "0"] + args + sub_arg(subs), capture_output=True,
                               text=True)
            assert r.returncode != 0 and "Error allocating tile component data" in r.stderr, \
                "class m: the reference now codes %s %s %s -- put the class back" % (size, subs, args)
        log("class m: the reference refuses %d of %d probes; left out" % (len(M_PROBES), len(M_PROBES)))
        while len(cases) < N_CASES:
            unmet = [t for t in need if counts[t] < need[t]]
            left = N_CASES - len(cases)
            # steer once the free draws could no longer leave room for the classes still short
            focus = unmet[0] if unmet and left <= 2 * sum(need[t] - counts[t] for t in unmet) + 8 else None
            while True:
                draws += 1
                assert draws <= DRAW_LIMIT, "draw limit reached with %s short" % unmet
                case = draw(rng, focus)
                cl = classes_of(case)
                if cl is None or (focus and focus not in cl):
                    continue
                # the refusal cases are the N_WIDE of each and no more
                if any(t in cl and counts[t] >= need[t] for t in ("l1024x4", "l4x1024")):
                    continue
                break
            handed += 1
            cs, why = ref_encode(case, tmp)
            if cs is None:
                dropped += 1
                reasons[why] = reasons.get(why, 0) + 1
                continue
            try:
                dec, dsubs = mg.ref_decode_planes(cs, tmp)
            except subprocess.CalledProcessError:
                dropped += 1
                reasons["decode failed"] = reasons.get("decode failed", 0) + 1
                continue
            if "-I" not in case["args"] and not all(np.array_equal(a, b) for a, b in zip(dec, planes_of(case))):
                dropped += 1
                reasons["5/3 decode differs from the source"] = reasons.get("5/3 decode differs from the source", 0) + 1
                log("  not lossless:", case)
                continue
            g = geometry(case)
            assert dsubs == g["subs"] and [p.shape for p in dec] == [p.shape for p in planes_of(case)]
            rec = dict(name="geom_%03d" % len(cases), **case)
            rec.update(classes=cl, src_sha256=planes_sha(planes_of(case)), j2k_len=len(cs), j2k_sha256=mg.sha(cs), dec_sha256=planes_sha(dec))
            if refusal_of(case):
                rec["refuse"] = refusal_of(case)
            flags = [n for n, p in (("device", 0.25), ("narrow", 0.25), ("forced", 0.125)) if rng.random() < p]
            rec["flags"] = flags
            if rng.random() < 0.5:
                for va in draw_variants(rng, case):
                    try:
                        vd, _ = mg.ref_decode_planes(cs, tmp, va)
                    except subprocess.CalledProcessError:
                        continue
                    v = {"args": va}
                    if va[0] == "-r":
                        v["valid"] = valid_dims(case, int(va[1]))
                        if any(p.shape[0] < hh or p.shape[1] < ww for p, (hh, ww) in zip(vd, v["valid"])):
                            continue
                        # several tiles: each is copied to its place in the plane and the
                        # last row / column is uninitialised; one tile: its samples lie
                        # packed at the plane's start, uninitialised behind them
                        if g["tw"] * g["th"] > 1:
                            vd = [p[:hh, :ww] for p, (hh, ww) in zip(vd, v["valid"])]
                        else:
                            vd = [p.ravel()[:hh * ww].reshape(hh, ww) for p, (hh, ww) in zip(vd, v["valid"])]
                    v["shapes"] = [list(p.shape) for p in vd]
                    v["dec_sha256"] = planes_sha(vd)
                    rec.setdefault("variants", {})[vtag(va)] = v
            for t in cl:
                if t in counts:
                    counts[t] += 1
            cases.append(rec)
    share = dropped / float(handed)
    log("drawn %d  dropped %d (%.1f %%)  kept %d  (sampler draws %d)" % (handed, dropped, 100 * share, len(cases), draws))
    for why, n in sorted(reasons.items()):
        log("  dropped %3d: %s" % (n, why))
    allc = {}
    for rec in cases:
        for t in rec["classes"]:
            allc[t] = allc.get(t, 0) + 1
    log("class  cases")
    for t in sorted(allc):
        log("%-8s %4d%s" % (t, allc[t], "" if t in REQUIRED else "  (library refusals)"))
    log("%-8s %4d  left out: %s" % ("m", 0, LEFT_OUT["m"]))
    assert share <= MAX_DROP, "the reference refused more than %d %% of the cases: narrow the sampler" % (100 * MAX_DROP)
    assert all(allc.get(t, 0) >= MIN_CLASS for t in REQUIRED), "a class is short"
    nref = sum("refuse" in rec for rec in cases)
    assert nref <= 0.05 * len(cases), "more than 5 % library refusals"
    log("subsampled %d  rate-controlled %d  with variants %d  library refusals %d"
        % (sum(bool(r["subsampling"]) for r in cases), sum("-r" in r["args"] for r in cases),
           sum("variants" in r for r in cases), nref))
    return dict(seed=SEED, drawn=handed, dropped=dropped, kept=len(cases), sampler_draws=draws, classes=allc,
                left_out=LEFT_OUT, cases=cases)


def main():
    check = "--check" in sys.argv
    mg.build_ref()
    mpath = os.path.join(mg.GOLD, "manifest_geom.json")
    man = generate()
    if check:
        old = json.load(open(mpath)) if os.path.exists(mpath) else {}
        new = json.loads(json.dumps(man))
        bad = sum(a != b for a, b in zip(old.get("cases", []), new["cases"]))
        bad += abs(len(old.get("cases", [])) - len(new["cases"]))
        bad += any(old.get(k) != new[k] for k in new if k != "cases")
        print("mismatches", bad)
        sys.exit(1 if bad else 0)
    with open(mpath, "w") as f:
        # one case a line
        head = {k: v for k, v in man.items() if k != "cases"}
        f.write(json.dumps(head, indent=1)[:-2] + ',\n "cases": [\n')
        f.write(",\n".join("  " + json.dumps(rec, separators=(",", ":")) for rec in man["cases"]))
        f.write("\n ]\n}\n")
    print("ok", len(man["cases"]))


if __name__ == "__main__":
    main()
