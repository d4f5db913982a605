"""Damaged-stream fixtures: committed goldens with 1 to 3 bytes replaced inside
the tile-parts (SOT fields, tile-part marker segments, the bytes behind SOD,
SOP / EPH markers, packed packet headers, tile data, the tail of a tile-part),
decoded by the reference itself (oracle/_ref/ref_driver, Grok 5.1.0 built from
/root/reference).  A decode of such a stream must return what Grok returns --
the same image, or a refusal where Grok refuses.

The offsets come from a marker walk of the clean stream written here
(structure(): make_golden_cut.layout() for the tile-parts, then the marker
segments of each tile-part header, the PPM segments of the main header and
the FF91 / FF92 patterns of streams written with SOP / EPH -- a bit-stuffed
packet header or code-block byte never holds FF followed by 9x), never from
the library under test.  Cases are drawn per stream from a seeded generator,
the strata in turn.

Every case is decoded twice by the reference, each run under a 30 s limit; a
case that ends in a signal, a timeout or two different results is left out
(counted by reason in the manifest; more than 1 % of a stream's draws fails
the generator).  Per stream at least 15 % of the kept cases are refusals and
at least 30 % decodes, and every stratum the stream has the structure for
holds a case: asserted here.

Writes tests/golden/manifest_damage.json: per stream its length and hash, the
counts, and one line per case: {"p": [[offset, value], ...], "s": stratum,
"r": "error" or the sha256 of the reference's decoded planes (the cut
manifest's convention: the (c, h, w) int32 image, or the planes of a
subsampled stream flattened one after the other), "t": tiles holding a
non-zero sample (absent for subsampled streams and refusals)}.  No stream is
stored.  TEST INFRASTRUCTURE ONLY.
  python oracle/make_golden_damage.py [--check] [--only NAME ...]"""
import concurrent.futures
import json
import os
import subprocess
import sys
import tempfile
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE]

import numpy as np  # noqa: E402

import make_golden as mg  # noqa: E402
import make_golden_cut as cut  # noqa: E402

STREAMS = cut.STREAMS + ["mk_tile_coc", "mk_main_coc", "mk_mixed_cblksty", "g8_M4_termall", "g12_M63"]
NCASES = 120
LIMIT_S = 30
MAX_LEFT_OUT = 0.01
MIN_REFUSED, MIN_DECODED = 0.15, 0.30
# named deviations: cases where the reference's result rests on memory it never
# wrote or on a read past a buffer (shown from its source); at most 8
DEVIATIONS = {}

# cases found by hand where the decoder once disagreed with the reference,
# kept behind the drawn ones (stratum "listed"): a packet header's bytes behind
# an SOP, SOP bytes in tile data whose headers are packed, an EPH inside a PPT
# payload, Scoc and SPcoc / SPcod bytes of a tile-part COC / COD
LISTED = {
    "g8_sop_eph": [[[161, 0x4C]], [[165, 0x8D]]],
    "mk_ppm": [[[1919, 0xA7]], [[890, 0x51]]],
    "mk_ppt_tparts": [[[12602, 0xC0]]],
    "mk_tile_coc": [[[6908, 0xE4]], [[6912, 0x84]], [[6878, 0x47]], [[6878, 0x47], [6912, 0x84]]],
}

TPH = {0xFF52: "COD", 0xFF53: "COC", 0xFF5C: "QCD", 0xFF5D: "QCC", 0xFF5E: "RGN", 0xFF5F: "POC", 0xFF61: "PPT"}
rd16, rd32 = cut.rd16, cut.rd32


def structure(cs):
    """Stratum -> sorted byte offsets of the clean stream `cs`."""
    siz, tps = cut.layout(cs)
    st = {}

    def add(name, offs):
        st.setdefault(name, set()).update(o for o in offs if 0 <= o < len(cs) - 2)

    # main header: PPM segments, and whether any COD asks for SOP / EPH
    sop = eph = False
    packed = []  # (start, end) of packed packet headers
    pos = 2
    while rd16(cs, pos) != 0xFF90:
        m, L = rd16(cs, pos), rd16(cs, pos + 2)
        if m == 0xFF52:
            sop, eph = sop or bool(cs[pos + 4] & 2), eph or bool(cs[pos + 4] & 4)
        if m == 0xFF60:  # PPM: Zppm, then Nppm / Ippm
            packed.append((pos + 5, pos + 2 + L))
        pos += 2 + L
    data = []  # (start, end) of each tile-part's data
    for sot, t, psot, sod in tps:
        end = sot + psot if psot else len(cs) - 2
        add("sot", range(sot + 4, sot + 12))  # Isot, Psot, TPsot, TNsot
        q = sot + 12
        while q < sod:
            m, L = rd16(cs, q), rd16(cs, q + 2)
            if m in TPH:
                add("tph_" + TPH[m], range(q + 2, q + 2 + L))  # Lxxx and the body
            if m == 0xFF52:
                sop, eph = sop or bool(cs[q + 4] & 2), eph or bool(cs[q + 4] & 4)
            if m == 0xFF61:  # PPT: Zppt, then Ippt
                packed.append((q + 5, q + 2 + L))
            q += 2 + L
        data.append((sod + 2, end))
        add("sod48", range(sod + 2, min(sod + 50, end)))
        add("tail16", range(max(end - 16, sod + 2), end))
    for a, b in packed:
        add("packed", range(a, b))
    span = [o for a, b in data for o in range(a, b)]
    add("uniform", span)
    if sop or eph:
        for a, b in data + packed:
            for o in range(a, b - 1):
                if cs[o] == 0xFF and ((sop and cs[o + 1] == 0x91) or (eph and cs[o + 1] == 0x92)):
                    n = 6 if cs[o + 1] == 0x91 else 2
                    add("sop_eph", range(o, min(o + n + 8, b)))
    return siz, tps, {k: sorted(v) for k, v in st.items() if v}


def draw(name, cs, strata):
    """NCASES patch lists, then the stream's LISTED ones: the strata in turn
    (the SOT fields twice), 1 to 3 bytes of one stratum no more than 16 apart,
    each set to another value."""
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    names = sorted(strata) + ["sot"]  # header-aimed: the SOT fields twice a round
    cases, seen = [], set()
    while len(cases) < NCASES:
        s = names[len(cases) % len(names)]
        offs = strata[s]
        o0 = offs[int(rng.integers(len(offs)))]
        near = [o for o in offs if abs(o - o0) <= 16]
        pick = {o0}
        for _ in range(int(rng.integers(1, 4)) - 1):
            pick.add(near[int(rng.integers(len(near)))])
        patch = []
        for o in sorted(pick):
            v = int(rng.integers(255))
            patch.append([o, v + (v >= cs[o])])
        key = json.dumps(patch)
        if key in seen:
            continue
        seen.add(key)
        cases.append((s, patch))
    return cases + [("listed", p) for p in LISTED.get(name, []) if json.dumps(p) not in seen]


def patched(cs, patch):
    b = bytearray(cs)
    for o, v in patch:
        b[o] = v
    return bytes(b)


def ref_run(data, path):
    """One reference decode: ("error",) | ("ok", stdout, samples) | ("signal" / "timeout",)."""
    src, out = path + ".j2k", path + ".i32"
    with open(src, "wb") as f:
        f.write(data)
    if os.path.exists(out):
        os.remove(out)
    try:
        r = subprocess.run([mg.DRIVER, "dec", src, out], capture_output=True, text=True, timeout=LIMIT_S)
    except subprocess.TimeoutExpired:
        return ("timeout",)
    if r.returncode < 0:
        return ("signal",)
    if r.returncode:
        return ("error",)
    return ("ok", r.stdout, np.fromfile(out, dtype="<i4"))


def ref_case(cs, patch, subs, siz, path):
    data = patched(cs, patch)
    a, b = ref_run(data, path), ref_run(data, path)
    for r in (a, b):
        if r[0] in ("signal", "timeout"):
            return {"left_out": r[0]}
    if a[0] != b[0] or (a[0] == "ok" and (a[1] != b[1] or not np.array_equal(a[2], b[2]))):
        return {"left_out": "unstable"}
    if a[0] == "error":
        return {"r": "error"}
    rec = {"r": mg.synth.image_sha256(a[2])}  # (flat samples hash as the (c, h, w) image does)
    if not subs:
        x0, y0, x1, y1, nc, prec, sgnd, cw, ch = map(int, a[1].splitlines()[0].split())
        rec["t"] = cut.tiles_nonzero(a[2].reshape(nc, ch, cw), siz)
    return rec


def run_stream(name, tmp, pool):
    cs = open(os.path.join(mg.GOLD, name + ".j2k"), "rb").read()
    siz, tps, strata = structure(cs)
    subs = siz["dx"] != [1] * len(siz["dx"]) or siz["dy"] != [1] * len(siz["dy"])
    cases = draw(name, cs, strata)
    clean = ref_case(cs, [], subs, siz, os.path.join(tmp, name + "_clean"))
    assert "r" in clean and clean["r"] != "error", name
    futs = [pool.submit(ref_case, cs, p, subs, siz, os.path.join(tmp, "%s_%d" % (name, i)))
            for i, (s, p) in enumerate(cases)]
    kept, left = [], {}
    for (s, p), f in zip(cases, futs):
        r = f.result()
        if "left_out" in r:
            left[r["left_out"]] = left.get(r["left_out"], 0) + 1
            continue
        kept.append(dict(p=p, s=s, **r))
    nref = sum(c["r"] == "error" for c in kept)
    nsame = sum(c["r"] == clean["r"] for c in kept)
    ndec = len(kept) - nref
    assert sum(left.values()) <= MAX_LEFT_OUT * len(cases), (name, left)
    assert nref >= MIN_REFUSED * len(kept) and ndec >= MIN_DECODED * len(kept), (name, nref, ndec)
    have = {c["s"] for c in kept}
    assert have - {"listed"} == set(strata), (name, sorted(set(strata) - have))
    # the strata a stream must have: every tile-part has SOT fields, data and a tail
    assert {"sot", "sod48", "uniform", "tail16"} <= have, name
    print(name, len(kept), "cases:", ndec, "decoded (%d as the clean stream)," % nsame, nref, "refused,",
          sum(left.values()), "left out;", " ".join(sorted(have)), flush=True)
    return {"len": len(cs), "j2k_sha256": mg.sha(cs), "clean": clean["r"], "drawn": len(cases), "decoded": ndec,
            "refused": nref, "same_as_clean": nsame, "left_out": left, "cases": kept}


def dumps(man):
    """One compact line per case."""
    out = ["{"]
    for i, name in enumerate(sorted(man)):
        rec = dict(man[name])
        cases = rec.pop("cases")
        head = json.dumps(rec, sort_keys=True)
        out.append(json.dumps(name) + ": " + head[:-1] + ', "cases": [')
        out += [json.dumps(c, sort_keys=True, separators=(",", ":")) + ("," if j + 1 < len(cases) else "")
                for j, c in enumerate(cases)]
        out.append("]}" + ("," if i + 1 < len(man) else ""))
    out.append("}")
    return "\n".join(out) + "\n"


def main():
    check = "--check" in sys.argv
    only = sys.argv[sys.argv.index("--only") + 1:] if "--only" in sys.argv else None
    mg.build_ref()
    assert len(DEVIATIONS) <= 8
    man = {}
    with tempfile.TemporaryDirectory() as tmp, concurrent.futures.ThreadPoolExecutor(8) as pool:
        for name in STREAMS:
            if only and name not in only:
                continue
            man[name] = run_stream(name, tmp, pool)
            for c in man[name]["cases"]:
                key = "%s %s" % (name, json.dumps(c["p"], separators=(",", ":")))
                if key in DEVIATIONS:
                    c["deviation"] = DEVIATIONS[key]
    path = os.path.join(mg.GOLD, "manifest_damage.json")
    if check:
        old = json.load(open(path))
        bad = sum(old.get(k) != v for k, v in man.items()) + (0 if only else len(set(old) - set(man)))
        print("mismatches", bad)
        sys.exit(1 if bad else 0)
    if only:
        old = json.load(open(path)) if os.path.exists(path) else {}
        old.update(man)
        man = old
    with open(path, "w") as f:
        f.write(dumps(man))


if __name__ == "__main__":
    main()
