"""Precision fixtures: every sample precision 1 .. 16, signed and unsigned
samples, 1 .. 5 components and components of mixed precision / signedness,
encoded AND decoded by the REFERENCE (oracle/_ref/ref_driver, Grok 5.1.0 built
from /root/reference).  The precision and the sign reach the DC shift
(0 for signed, 2^(prec-1) otherwise), the decode clamp, the quantisation
(reversible exponents prec + gain, irreversible base step 2^-(prec + sgnd)),
the rate control's byte budgets and the SIZ Ssiz byte.

Four families:
  1  sweep     37 x 45, -n 3: gray at every precision, RGB (RCT / ICT) at
               eleven, both signs, 5/3 and 9/7; `uniform` 9/7 images whose
               decoded overshoot reaches both clamps
  2  crosses   70 x 90: precision / sign / component count crossed with rate
               control, -q, -M, tiles, ROI, precincts; -l / -r decode variants
  3  mixed     components of different precision and sign in one image (the
               driver's -prec / -sgnd lists)
  4  refused   busy low-precision images the reference refuses to ENCODE
               (T2.cpp:1094 "Code block layer size N exceeds number of
               available bytes M in tile buffer": its tile buffer holds about
               0.1625 bytes per sample-bit).  Recorded as "ref_enc": "refused";
               the stored stream is the CPU oracle's (oracle/pyoracle.py, byte
               for byte the reference's wherever the reference encodes), and
               the stored decode is the reference's decode of that stream.  A
               refusal is accepted only below 6 bits and for at most 10 % of
               the cases, so a broken driver cannot turn the family into
               oracle-only fixtures.

Writes tests/golden/p_<name>.j2k, p_<name>.dec.npz (array "dec": the
reference's decode in the narrowest integer type holding it, lossy cases only
-- a lossless case's decode is the synth image, dec_vs_src_maxabs == 0),
p_<name>.<variant>.dec.npz for -l / -r decodes and manifest_prec.json.
  python oracle/make_golden_prec.py [--check]"""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE]

import numpy as np  # noqa: E402

import make_golden as mg  # noqa: E402
import pyoracle  # noqa: E402

REFUSAL = "exceeds number of available bytes"


def _cases():
    """name -> (h, w, precs, sgnds, kind, args); seeds follow the order."""
    out = []

    def add(name, hw, precs, sgnds, kind, args):
        out.append(("p_" + name, hw[0], hw[1], list(precs), [int(s) for s in sgnds], kind, list(args)))

    small, n3 = (37, 45), ["-n", "3"]
    su = (("u", 0), ("s", 1))
    # family 1: sweep
    for prec in range(1, 17):
        for tag, s in su:
            add("g%d%s" % (prec, tag), small, [prec], [s], "smooth", n3)
            add("g%d%s_I" % (prec, tag), small, [prec], [s], "smooth", n3 + ["-I"])
    for prec in (1, 2, 3, 5, 7, 9, 11, 13, 14, 15, 16):
        for tag, s in su:
            add("rgb%d%s" % (prec, tag), small, [prec] * 3, [s] * 3, "smooth", n3)
            add("rgb%d%s_I" % (prec, tag), small, [prec] * 3, [s] * 3, "smooth", n3 + ["-I"])
    for prec in (3, 7, 9, 13, 16):
        for tag, s in su:
            add("g%d%s_uni_I" % (prec, tag), small, [prec], [s], "uniform", n3 + ["-I"])
            add("rgb%d%s_uni_I" % (prec, tag), small, [prec] * 3, [s] * 3, "uniform", n3 + ["-I"])
    # family 2: crosses
    big = (70, 90)
    for name, c, prec, s, kind, args in [
        ("x_rgb5u_I_r10_3", 3, 5, 0, "smooth", ["-I", "-r", "10,3"]),
        ("x_rgb9s_I_r20_5", 3, 9, 1, "smooth", ["-I", "-r", "20,5"]),
        ("x_g14s_uni_I_r6", 1, 14, 1, "uniform", ["-I", "-r", "6"]),
        ("x_rgb7s_q30_40", 3, 7, 1, "smooth", ["-q", "30,40"]),
        ("x_g3u_I_q25", 1, 3, 0, "smooth", ["-I", "-q", "25"]),
        ("x_rgb12s_r12_4_A1", 3, 12, 1, "smooth", ["-r", "12,4", "-A", "1"]),
        ("x_c4_8u", 4, 8, 0, "smooth", []),
        ("x_c4_8u_I_r15_5", 4, 8, 0, "smooth", ["-I", "-r", "15,5"]),
        ("x_c2_10s_I", 2, 10, 1, "smooth", ["-I"]),
        ("x_c5_8u_r10", 5, 8, 0, "smooth", ["-r", "10"]),
        ("x_c4_12s_uni_I_q35", 4, 12, 1, "uniform", ["-I", "-q", "35"]),
        ("x_rgb16s_uni_I_r4", 3, 16, 1, "uniform", ["-I", "-r", "4"]),
        ("x_rgb15s_uni_M63_tiles", 3, 15, 1, "uniform", ["-M", "63", "-t", "64,64"]),
        ("x_g4s_roi_U4", 1, 4, 1, "smooth", ["-R", "c=0,U=4"]),
        ("x_rgb6s_prec_rpcl_r8_2", 3, 6, 1, "smooth", ["-c", "[32,32],[16,16]", "-p", "RPCL", "-r", "8,2"]),
    ]:
        add(name, big, [prec] * c, [s] * c, kind, args)
    # family 3: mixed components
    add("mix_8u8u8u1u", small, [8, 8, 8, 1], [0, 0, 0, 0], "smooth", n3)
    add("mix_12s8u", small, [12, 8], [1, 0], "smooth", n3)
    add("mix_16u10s5u", small, [16, 10, 5], [0, 1, 0], "smooth", n3 + ["-Y", "0"])
    add("mix_16u10s5u_I", small, [16, 10, 5], [0, 1, 0], "smooth", n3 + ["-Y", "0", "-I"])
    # family 4: busy low-precision images (1-bit gray / RGB `smooth` are family 1's g1u / rgb1u)
    add("g1u_uni", small, [1], [0], "uniform", n3)
    add("g2s_uni", small, [2], [1], "uniform", n3)
    add("g5s_uni_I", small, [5], [1], "uniform", n3 + ["-I"])
    return [cs + (1000 + i,) for i, cs in enumerate(out)]


CASES = _cases()
VARIANTS = {
    "p_x_rgb5u_I_r10_3": [["-l", "1"]],
    "p_x_rgb9s_I_r20_5": [["-l", "1"]],
    "p_x_rgb7s_q30_40": [["-l", "1"]],
    "p_x_rgb12s_r12_4_A1": [["-l", "1"]],
    "p_x_c4_8u_I_r15_5": [["-l", "1"], ["-r", "1"]],
    "p_x_rgb6s_prec_rpcl_r8_2": [["-l", "1"]],
    "p_x_rgb15s_uni_M63_tiles": [["-r", "1"]],
}


def image_of(case):
    name, h, w, precs, sgnds, kind, args, seed = case
    return mg.synth.synth_image_mixed(h, w, precs, sgnds, seed, kind)


def clamp_hits(dec, precs, sgnds):
    """[the decode holds a component's range minimum, ... its range maximum]"""
    lo = hi = False
    for k, (p, s) in enumerate(zip(precs, sgnds)):
        mn, mx = (-(1 << (p - 1)), (1 << (p - 1)) - 1) if s else (0, (1 << p) - 1)
        lo = lo or bool((dec[k] == mn).any())
        hi = hi or bool((dec[k] == mx).any())
    return [lo, hi]


def run_case(case, tmp):
    """-> (manifest record, codestream, {"": decode, variant tag: decode})"""
    name, h, w, precs, sgnds, kind, args, seed = case
    img = image_of(case)
    mixed = len(set(precs)) > 1 or len(set(sgnds)) > 1
    extra = ["-prec", ",".join(map(str, precs)), "-sgnd", ",".join(map(str, sgnds))] if mixed else []
    rec = dict(shape=[h, w, len(precs), precs[0]], kind=kind, seed=seed, signed=bool(sgnds[0]), args=args)
    if mixed:
        rec.update(prec=precs, sgnd=sgnds)
    try:
        cs = mg.ref_encode(img, precs[0], args + extra, tmp, signed=bool(sgnds[0]), stderr=subprocess.PIPE)
    except subprocess.CalledProcessError as e:
        if REFUSAL not in (e.stderr or ""):
            raise
        # the reference accepts every image of 6 or more bits
        assert min(precs) < 6, (name, e.stderr)
        rec["ref_enc"] = "refused"
        cs = pyoracle.encode(img, precs, pyoracle.params_from_args(args), sgnd=sgnds)
    dec, hdr = mg.ref_decode(cs, tmp)
    assert hdr == (0, 0, w, h, precs[0], sgnds[0]), (name, hdr)
    diff = np.abs(dec.astype(np.int64) - img)
    rec.update(image_sha256=mg.synth.image_sha256(img), j2k_sha256=mg.sha(cs), j2k_len=len(cs),
               dec_sha256=mg.synth.image_sha256(dec), dec_vs_src_maxabs=int(diff.max()),
               clamp_hits=clamp_hits(dec, precs, sgnds))
    decs = {"": dec}
    for va in VARIANTS.get(name, []):
        vd, vh = mg.ref_decode(cs, tmp, va)
        tag = mg.variant_tag(va)
        decs[tag] = vd
        rec.setdefault("variants", {})[tag] = dict(args=va, dec_sha256=mg.synth.image_sha256(vd), header=list(vh))
    return rec, cs, decs


def narrow(d):
    """d in the narrowest integer type that holds it (the .npz stays small; readers widen to int32)"""
    for dt in (np.uint8, np.int8, np.uint16, np.int16):
        if np.iinfo(dt).min <= d.min() and d.max() <= np.iinfo(dt).max:
            return d.astype(dt)
    return d.astype(np.int32)


def dec_path(name, tag):
    return os.path.join(mg.GOLD, "%s%s.dec.npz" % (name, "." + tag if tag else ""))


def main():
    check = "--check" in sys.argv
    mg.build_ref()
    pyoracle.build()
    mpath = os.path.join(mg.GOLD, "manifest_prec.json")
    old = json.load(open(mpath)) if os.path.exists(mpath) else {}
    man, bad = {}, 0
    assert len({cs[0] for cs in CASES}) == len(CASES)
    assert all(n in {cs[0] for cs in CASES} for n in VARIANTS)
    with tempfile.TemporaryDirectory() as tmp:
        for case in CASES:
            name = case[0]
            rec, cs, decs = run_case(case, tmp)
            man[name] = rec
            lossless = rec["dec_vs_src_maxabs"] == 0
            if check:
                ok = old.get(name) == rec and os.path.exists(os.path.join(mg.GOLD, name + ".j2k")) and \
                    open(os.path.join(mg.GOLD, name + ".j2k"), "rb").read() == cs
                for tag, d in decs.items():
                    if tag == "" and lossless:
                        ok = ok and not os.path.exists(dec_path(name, tag))
                        continue
                    ok = ok and os.path.exists(dec_path(name, tag))
                    if ok:
                        z = np.load(dec_path(name, tag))["dec"]
                        ok = z.dtype == narrow(d).dtype and z.shape == d.shape and np.array_equal(z, d)
                print(name, "ok" if ok else "MISMATCH", flush=True)
                bad += not ok
                continue
            with open(os.path.join(mg.GOLD, name + ".j2k"), "wb") as f:
                f.write(cs)
            for tag, d in decs.items():
                if tag or not lossless:
                    np.savez_compressed(dec_path(name, tag), dec=narrow(d))
            print(name, len(cs), "lossless" if lossless else "lossy", rec.get("ref_enc", ""), flush=True)
    refused = [n for n, r in man.items() if r.get("ref_enc") == "refused"]
    assert 10 * len(refused) <= len(man), refused
    if check:
        stale = sorted(set(old) - set(man))
        for n in stale:
            print(n, "MISMATCH (not a case)", flush=True)
        print("mismatches", bad + len(stale))
        sys.exit(1 if bad or stale else 0)
    with open(mpath, "w") as f:
        json.dump(man, f, indent=1)
    print("ok", len(man), "refused by the reference:", " ".join(refused))


if __name__ == "__main__":
    main()
