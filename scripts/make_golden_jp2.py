"""JP2 file fixtures: tests/golden/jp2_*.jp2, jp2_*.dec.npz, manifest_jp2.json.

Three families, every one pinned by the REFERENCE (oracle/_ref/libgrok.so)
through tests/cpp/jp2_driver.cpp, which this script compiles into oracle/_ref/
(nothing compiled is committed):

  A  files the reference ENCODES (jp2_driver enc): this project's writer must
     produce the same bytes, its decoder the reference's decode of them
  B  files assembled here at the box level around reference-encoded
     codestreams (oracle/_ref/ref_driver enc), decoded by the reference:
     palettes, channel definitions, stray / repeated / oddly sized boxes
  C  files the reference REFUSES (the manifest says "error")

Per file the manifest keeps its sha256, the offset of the codestream, what
the reference's decode reported (colour space, ICC length and hash, and per
output channel w h dx dy prec sgnd alpha) and, for B, the palette as written.
jp2_<name>.dec.npz holds the reference's planes ("p0", "p1", ...; variants
such as -r 1 or a window as "<tag>_p0", ...).

  python scripts/make_golden_jp2.py [--check]"""
import hashlib
import json
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [os.path.join(ROOT, "oracle")]

import make_golden as mg  # noqa: E402

synth = mg.synth
DRIVER = os.path.join(ROOT, "oracle", "_ref", "jp2_driver")
GEN = os.path.join(ROOT, "oracle", "_ref", "gen")
REF_SRC = "/root/reference/src/lib/jp2"

# GRK_COLOR_SPACE
CS_UNKNOWN, CS_SRGB, CS_GRAY, CS_SYCC, CS_ICC = 0, 2, 3, 4, 9
ICC300 = bytes((i * 7 + 3) & 0xFF for i in range(300))


def build_driver():
    mg.build_ref()
    src = os.path.join(ROOT, "tests", "cpp", "jp2_driver.cpp")
    if os.path.exists(DRIVER) and os.path.getmtime(DRIVER) >= os.path.getmtime(src):
        return
    subprocess.run(["g++", "-std=c++17", "-O2", "-I" + REF_SRC, "-I" + GEN, "-o", DRIVER, src,
                    "-L" + os.path.dirname(DRIVER), "-lgrok", "-Wl,-rpath,$ORIGIN", "-lpthread"], check=True)


# ---------------------------------------------------------------------------
# boxes
# ---------------------------------------------------------------------------
def box(typ, payload=b""):
    return struct.pack(">I", 8 + len(payload)) + typ + payload


def xlbox(typ, payload=b""):
    return struct.pack(">I", 1) + typ + struct.pack(">Q", 16 + len(payload)) + payload


SIG = box(b"jP  ", b"\x0d\x0a\x87\x0a")
FTYP = box(b"ftyp", b"jp2 " + b"\0\0\0\0" + b"jp2 ")


def ihdr(h, w, nc, bpc):
    return box(b"ihdr", struct.pack(">IIHBBBB", h, w, nc, bpc, 7, 0, 0))


def colr(enumcs=None, meth=1, icc=b""):
    return box(b"colr", bytes([meth, 0, 0]) + (struct.pack(">I", enumcs) if meth == 1 else icc))


def pclr(entries, sizes, signs=None):
    """entries: (NE, NPC) ints; sizes: bits per column"""
    ne, npc = len(entries), len(sizes)
    out = struct.pack(">HB", ne, npc)
    for i, s in enumerate(sizes):
        out += bytes([(s - 1) | (0x80 if signs and signs[i] else 0)])
    for row in entries:
        for v, s in zip(row, sizes):
            out += int(v).to_bytes(min(4, (s + 7) // 8), "big")
    return box(b"pclr", out)


def cmap(triples):
    return box(b"cmap", b"".join(struct.pack(">HBB", *t) for t in triples))


def cdef(triples):
    return box(b"cdef", struct.pack(">H", len(triples)) + b"".join(struct.pack(">HHH", *t) for t in triples))


RES = box(b"res ", box(b"resc", struct.pack(">HHHHBB", 300, 1, 300, 1, 2, 2)))


def jp2(header_boxes, cs, before=b"", between=b"", jp2c=None):
    head = SIG + FTYP + before + box(b"jp2h", b"".join(header_boxes)) + between
    return head + (jp2c if jp2c is not None else box(b"jp2c", cs)), len(head) + 8


# ---------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------
def ref_jp2_encode(planes, w, h, bits, signed, args, tmp):
    src, out = os.path.join(tmp, "in.i32"), os.path.join(tmp, "out.jp2")
    np.concatenate([np.ascontiguousarray(p, dtype="<i4").ravel() for p in planes]).tofile(src)
    subprocess.run([DRIVER, "enc", src, out, str(w), str(h), str(len(planes)), str(bits), str(int(signed))] + args,
                   check=True, stdout=subprocess.DEVNULL)
    with open(out, "rb") as f:
        return f.read()


def ref_jp2_decode(data, tmp, extra=()):
    """None when the reference refuses; else (meta dict, [planes])"""
    src, out = os.path.join(tmp, "in.jp2"), os.path.join(tmp, "out.i32")
    with open(src, "wb") as f:
        f.write(data)
    r = subprocess.run([DRIVER, "dec", src, out] + list(extra), capture_output=True, text=True)
    if r.returncode == 1 and r.stdout.strip().endswith("error"):
        return None
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith(("image", "comp"))]
    x0, y0, x1, y1, nc, cs, icc_len = map(int, lines[0][1:])
    raw = np.fromfile(out, dtype="<i4")
    with open(out + ".icc", "rb") as f:
        icc = f.read()
    comps, planes, off = [], [], 0
    for ln in lines[1:]:
        w, h, dx, dy, prec, sgnd, alpha = map(int, ln[1:])
        comps.append(dict(w=w, h=h, dx=dx, dy=dy, prec=prec, sgnd=sgnd, alpha=alpha))
        planes.append(raw[off:off + w * h].reshape(h, w).copy())
        off += w * h
    assert off == raw.size and len(comps) == nc
    meta = dict(rect=[x0, y0, x1, y1], colour_space=cs, icc_len=icc_len,
                icc_sha256=hashlib.sha256(icc).hexdigest() if icc_len else None, comps=comps)
    return meta, planes


def image(h, w, c, bits, seed, signed=False, kind="smooth"):
    img = synth.synth_image(h, w, c, bits, seed, kind)
    return img - (1 << (bits - 1)) if signed else img


# ---------------------------------------------------------------------------
# A: reference encodes.  name -> (h, w, c, bits, signed, seed, colour space, driver args, subsampling)
# ---------------------------------------------------------------------------
A_CASES = [
    ("a_gray8", (48, 64, 1, 8, 0), 901, CS_GRAY, [], None),
    ("a_rgb8_I_tiles", (43, 61, 3, 8, 0), 902, CS_SRGB, ["-I", "-t", "32,32"], None),
    ("a_sycc420_12", (48, 64, 3, 12, 0), 903, CS_SYCC, ["-sub", "1,1/2,2/2,2"], [(1, 1), (2, 2), (2, 2)]),
    ("a_rgba_typ1", (40, 52, 4, 8, 0), 904, CS_SRGB, ["-alpha", "0,0,0,1"], None),
    ("a_rgba_typ2", (40, 52, 4, 8, 0), 905, CS_SRGB, ["-alpha", "0,0,0,2"], None),
    ("a_graya", (40, 52, 2, 8, 0), 906, CS_GRAY, ["-alpha", "0,1"], None),
    ("a_prec_8_10_12", (40, 52, 3, 8, 0), 907, CS_SRGB, ["-prec", "8,10,12", "-Y", "0"], None),
    ("a_gray_s16", (40, 52, 1, 16, 1), 908, CS_GRAY, [], None),
    ("a_unknown", (40, 52, 3, 8, 0), 909, CS_UNKNOWN, [], None),
    ("a_icc", (40, 52, 3, 8, 0), 910, CS_ICC, ["-icc", "@ICC"], None),
    ("a_two_alpha", (40, 52, 4, 8, 0), 911, CS_SRGB, ["-alpha", "0,0,1,1"], None),
]


def a_planes(case):
    """the source planes of an A case (the tests rebuild them from the manifest's spec)"""
    name, (h, w, c, bits, signed), seed, cs, args, sub = case
    precs = [int(v) for v in args[args.index("-prec") + 1].split(",")] if "-prec" in args else [bits] * c
    img = image(h, w, c, max(precs), seed, bool(signed))
    planes = []
    for k in range(c):
        p = img[k] >> (max(precs) - precs[k])
        dx, dy = sub[k] if sub else (1, 1)
        planes.append(np.ascontiguousarray(p[::dy, ::dx]))
    return planes


# ---------------------------------------------------------------------------
# B and C: assembled files
# ---------------------------------------------------------------------------
def rnd_palette(ne, sizes, seed):
    r = np.random.RandomState(seed)
    return [[int(r.randint(0, 1 << s)) for s in sizes] for _ in range(ne)]


def build_bc(tmp):
    """-> list of (name, kind, file bytes, codestream offset, palette record or None, decode variants)"""
    out = []
    enc = lambda img, bits, args=(), signed=False: mg.ref_encode(img, bits, list(args), tmp, signed=signed)  # noqa: E731
    g8 = image(40, 52, 1, 8, 921)
    cs_g8 = enc(g8, 8)
    H8 = [ihdr(40, 52, 1, 7), colr(17)]
    CM3 = [(0, 1, 0), (0, 1, 1), (0, 1, 2)]

    def add(name, kind, data_off, pal=None, variants=()):
        data, off = data_off
        out.append((name, kind, data, off, pal, list(variants)))

    def palrec(entries, sizes, cm):
        return dict(ne=len(entries), npc=len(sizes), sizes=list(sizes), cmap=[list(t) for t in cm],
                    entries_sha256=hashlib.sha256(np.asarray(entries, dtype="<u2").tobytes()).hexdigest())

    # --- B ---
    p8 = rnd_palette(256, [8, 8, 8], 1)
    add("b_pal8", "B", jp2(H8[:1] + [colr(16), pclr(p8, [8, 8, 8]), cmap(CM3)], cs_g8), palrec(p8, [8, 8, 8], CM3))
    g4 = image(40, 52, 1, 4, 922)
    p4 = rnd_palette(16, [5, 6, 5], 2)
    add("b_pal4_565", "B", jp2([ihdr(40, 52, 1, 3), colr(16), pclr(p4, [5, 6, 5]), cmap(CM3)], enc(g4, 4)),
        palrec(p4, [5, 6, 5], CM3))
    g10 = image(40, 52, 1, 10, 923, kind="uniform")
    p10 = rnd_palette(700, [12, 12, 12], 3)
    assert int(g10.max()) > 699
    add("b_pal10_ne700", "B", jp2([ihdr(40, 52, 1, 9), colr(16), pclr(p10, [12, 12, 12]), cmap(CM3)], enc(g10, 10)),
        palrec(p10, [12, 12, 12], CM3))
    s8 = image(40, 52, 1, 8, 924, signed=True)
    assert int(s8.min()) < 0
    p100 = rnd_palette(100, [8, 8, 8], 4)
    add("b_pal_signed_index", "B", jp2([ihdr(40, 52, 1, 0x87), colr(16), pclr(p100, [8, 8, 8]), cmap(CM3)],
                                       enc(s8, 8, signed=True)), palrec(p100, [8, 8, 8], CM3))
    p1 = rnd_palette(1, [8, 8, 8], 5)
    add("b_pal_ne1", "B", jp2(H8[:1] + [colr(16), pclr(p1, [8, 8, 8]), cmap(CM3)], cs_g8), palrec(p1, [8, 8, 8], CM3))
    ga = image(40, 52, 2, 8, 925)
    pa = rnd_palette(256, [8, 8, 8, 8], 6)
    cma = [(0, 1, 0), (0, 1, 1), (0, 1, 2), (1, 0, 0)]
    add("b_pal_direct_alpha", "B", jp2([ihdr(40, 52, 2, 7), colr(16), pclr(pa, [8, 8, 8, 8]), cmap(cma),
                                        cdef([(0, 0, 1), (1, 0, 2), (2, 0, 3), (3, 1, 0)])], enc(ga, 8)),
        palrec(pa, [8, 8, 8, 8], cma))
    weird = [(0, 0, 0)] * 3
    add("b_pal_weird_cmap", "B", jp2(H8[:1] + [colr(16), pclr(p8, [8, 8, 8]), cmap(weird)], cs_g8),
        palrec(p8, [8, 8, 8], CM3))
    add("b_pclr_no_cmap", "B", jp2(H8 + [pclr(p8, [8, 8, 8])], cs_g8))
    rgb = image(40, 52, 3, 8, 926)
    cs_rgb = enc(rgb, 8)
    HRGB = [ihdr(40, 52, 3, 7), colr(16)]
    BGR = [(0, 0, 3), (1, 0, 2), (2, 0, 1)]
    add("b_cdef_bgr", "B", jp2(HRGB + [cdef(BGR)], cs_rgb))
    add("b_pal8_cdef_swap", "B", jp2(H8[:1] + [colr(16), pclr(p8, [8, 8, 8]), cmap(CM3), cdef(BGR)], cs_g8),
        palrec(p8, [8, 8, 8], CM3))
    gt = image(64, 128, 1, 8, 927)
    cs_gt = enc(gt, 8, ["-t", "64,64", "-I", "-n", "6", "-r", "20,5"])
    add("b_pal8_tiles_I", "B", jp2([ihdr(64, 128, 1, 7), colr(16), pclr(p8, [8, 8, 8]), cmap(CM3)], cs_gt),
        palrec(p8, [8, 8, 8], CM3),
        variants=[["-r", "1"], ["-l", "1"], ["-d", "0,0,1,1"], ["-d", "127,63,128,64"], ["-d", "60,20,70,41"],
                  ["-d", "0,63,1,64"], ["-d", "127,0,128,1"], ["-d", "17,9,101,50"], ["-d", "63,0,65,64"],
                  ["-d", "1,1,64,33"], ["-d", "64,31,127,63"]])
    # the same file cut where its second tile's tile-part would start: that tile is never reached
    d, off = jp2([ihdr(64, 128, 1, 7), colr(16), pclr(p8, [8, 8, 8]), cmap(CM3)], cs_gt)
    add("b_pal8_tiles_cut", "B", (d[:off + cs_gt.index(b"\xff\x90", cs_gt.index(b"\xff\x90") + 2)], off),
        palrec(p8, [8, 8, 8], CM3))
    go = image(17, 33, 1, 8, 928)
    add("b_pal8_odd_origin", "B", jp2([ihdr(17, 33, 1, 7), colr(16), pclr(p8, [8, 8, 8]), cmap(CM3)],
                                      enc(go, 8, ["-d", "5,3", "-n", "3"])), palrec(p8, [8, 8, 8], CM3))
    junk = box(b"xml ", b"<a/>") + box(b"uuid", bytes(range(16)) + b"payload") + box(b"abcd", b"\1\2\3")
    add("b_extra_boxes", "B", jp2(H8 + [RES, box(b"wxyz", b"zz")], cs_g8, before=RES + junk, between=junk + RES))
    add("b_second_colr", "B", jp2([ihdr(40, 52, 3, 7), colr(16), colr(17)], cs_rgb))
    add("b_colr_meth3", "B", jp2([ihdr(40, 52, 3, 7), colr(meth=3, icc=b"\1\2\3\4")], cs_rgb))
    add("b_colr_meth3_then_1", "B", jp2([ihdr(40, 52, 3, 7), colr(meth=3, icc=b"\1\2\3\4"), colr(16)], cs_rgb))
    add("b_jp2c_lbox0", "B", jp2(H8, cs_g8, jp2c=struct.pack(">I", 0) + b"jp2c" + cs_g8))
    d, off = jp2(H8, cs_g8, jp2c=xlbox(b"jp2c", cs_g8))
    add("b_jp2c_xl", "B", (d, off + 8))
    add("b_colr_after_jp2h", "B", jp2([ihdr(40, 52, 3, 7)], cs_rgb, between=colr(16)))
    add("b_icc_meth2", "B", jp2([ihdr(40, 52, 3, 7), colr(meth=2, icc=ICC300[:64])], cs_rgb))
    add("b_cielab_default", "B", jp2([ihdr(40, 52, 3, 7), colr(14)], cs_rgb))

    # --- C ---
    ok_h = H8
    add("c_no_signature", "C", (FTYP + box(b"jp2h", b"".join(ok_h)) + box(b"jp2c", cs_g8), 0))
    add("c_no_ftyp", "C", (SIG + box(b"jp2h", b"".join(ok_h)) + box(b"jp2c", cs_g8), 0))
    add("c_jp2c_before_jp2h", "C", (SIG + FTYP + box(b"jp2c", cs_g8) + box(b"jp2h", b"".join(ok_h)), 0))
    add("c_no_ihdr", "C", jp2([colr(17)], cs_g8))
    add("c_ihdr_13", "C", jp2([box(b"ihdr", struct.pack(">IIHBBB", 40, 52, 1, 7, 7, 0)), colr(17)], cs_g8))
    add("c_cmap_before_pclr", "C", jp2(H8 + [cmap(CM3), pclr(p8, [8, 8, 8])], cs_g8))
    add("c_two_cmap", "C", jp2(H8 + [pclr(p8, [8, 8, 8]), cmap(CM3), cmap(CM3)], cs_g8))
    add("c_ne0", "C", jp2(H8 + [box(b"pclr", struct.pack(">HB", 0, 3) + b"\7\7\7"), cmap(CM3)], cs_g8))
    add("c_ne1025", "C", jp2(H8 + [box(b"pclr", struct.pack(">HB", 1025, 1) + b"\7" + bytes(1025)),
                                   cmap([(0, 1, 0)])], cs_g8))
    add("c_npc0", "C", jp2(H8 + [box(b"pclr", struct.pack(">HB", 4, 0)), cmap([])], cs_g8))
    add("c_cdef_incomplete", "C", jp2(HRGB + [cdef([(0, 0, 1), (1, 0, 2)])], cs_rgb))
    add("c_cdef_cn_range", "C", jp2(HRGB + [cdef([(0, 0, 1), (1, 0, 2), (2, 0, 3), (3, 1, 0)])], cs_rgb))
    add("c_cmap_comp_range", "C", jp2(H8 + [pclr(p8, [8, 8, 8]), cmap([(0, 1, 0), (1, 1, 1), (0, 1, 2)])], cs_g8))
    add("c_column_twice", "C", jp2(H8 + [pclr(p8, [8, 8, 8]), cmap([(0, 1, 0), (0, 1, 0), (0, 1, 2)])], cs_g8))
    add("c_mtyp2", "C", jp2(H8 + [pclr(p8, [8, 8, 8]), cmap([(0, 1, 0), (0, 2, 1), (0, 1, 2)])], cs_g8))
    add("c_direct_pcol1", "C", jp2([ihdr(40, 52, 2, 7), colr(16), pclr(pa, [8, 8, 8, 8]),
                                    cmap([(0, 1, 0), (0, 1, 1), (0, 1, 2), (1, 0, 1)])], enc(ga, 8)))
    add("c_meth2_empty", "C", jp2([ihdr(40, 52, 1, 7), colr(meth=2)], cs_g8))
    bad = ihdr(40, 52, 1, 7) + struct.pack(">I", 100) + b"colr" + bytes([1, 0, 0]) + struct.pack(">I", 17)
    add("c_box_past_jp2h", "C", (SIG + FTYP + box(b"jp2h", bad) + box(b"jp2c", cs_g8), 0))
    small = ihdr(40, 52, 1, 7) + struct.pack(">I", 7) + b"colr" + bytes([1, 0, 0]) + struct.pack(">I", 17)
    add("c_box_below_8", "C", (SIG + FTYP + box(b"jp2h", small) + box(b"jp2c", cs_g8), 0))
    return out


def vtag(args):
    return "".join(a.lstrip("-") for a in args).replace(",", "_")


def main():
    check = "--check" in sys.argv
    build_driver()
    path = os.path.join(mg.GOLD, "manifest_jp2.json")
    old = json.load(open(path)) if os.path.exists(path) else {}
    man, bad = {}, 0
    files, decs = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        icc_path = os.path.join(tmp, "profile.icc")
        with open(icc_path, "wb") as f:
            f.write(ICC300)
        todo = []
        for case in A_CASES:
            name, (h, w, c, bits, signed), seed, cs, args, sub = case
            dargs = ["-cs", str(cs)] + [icc_path if a == "@ICC" else a for a in args]
            data = ref_jp2_encode(a_planes(case), w, h, bits, signed, dargs, tmp)
            off = data.index(b"jp2c") + 4
            spec = dict(shape=[h, w, c, bits], sgnd=signed, seed=seed, colour_space=cs, args=args,
                        subsampling=[list(s) for s in sub] if sub else None)
            todo.append((name, "A", data, off, None, [], spec))
        for name, kind, data, off, pal, variants in build_bc(tmp):
            todo.append((name, kind, data, off, pal, variants, None))
        for name, kind, data, off, pal, variants, spec in todo:
            tag = "jp2_" + name
            r = ref_jp2_decode(data, tmp)
            rec = dict(kind=kind, sha256=hashlib.sha256(data).hexdigest(), len=len(data))
            arrays = {}
            if kind == "C":
                assert r is None, "%s: the reference decodes it" % tag
                rec["expect"] = "error"
            else:
                assert r is not None, "%s: the reference refuses it" % tag
                meta, planes = r
                rec.update(expect=meta, cs_offset=off, palette=pal, spec=spec, variants={})
                for k, p in enumerate(planes):
                    arrays["p%d" % k] = p
                for v in variants:
                    rv = ref_jp2_decode(data, tmp, v)
                    assert rv is not None, (tag, v)
                    rec["variants"][vtag(v)] = dict(args=v, rect=rv[0]["rect"], comps=rv[0]["comps"])
                    for k, p in enumerate(rv[1]):
                        arrays["%s_p%d" % (vtag(v), k)] = p
                rec["dec_sha256"] = {k: hashlib.sha256(np.ascontiguousarray(a, dtype="<i4").tobytes()).hexdigest()
                                     for k, a in arrays.items()}
            man[tag] = rec
            files[tag], decs[tag] = data, arrays
            if check:
                ok = old.get(tag) == json.loads(json.dumps(rec))
                fp = os.path.join(mg.GOLD, tag + ".jp2")
                ok = ok and os.path.exists(fp) and open(fp, "rb").read() == data
                if arrays:
                    z = np.load(os.path.join(mg.GOLD, tag + ".dec.npz"))
                    ok = ok and sorted(z.files) == sorted(arrays) and all(np.array_equal(z[k], arrays[k]) for k in arrays)
                print(tag, "ok" if ok else "MISMATCH", flush=True)
                bad += not ok
            else:
                print(tag, kind, len(data), flush=True)
    if check:
        bad += len(set(old) - set(man))
        print("mismatches", bad)
        sys.exit(1 if bad else 0)
    for tag, data in files.items():
        with open(os.path.join(mg.GOLD, tag + ".jp2"), "wb") as f:
            f.write(data)
        if decs[tag]:
            small = {k: (a.astype(np.int16) if a.min() >= -32768 and a.max() <= 32767 else a) for k, a in decs[tag].items()}
            np.savez_compressed(os.path.join(mg.GOLD, tag + ".dec.npz"), **small)
    with open(path, "w") as f:
        json.dump(man, f, indent=1)


if __name__ == "__main__":
    main()
