"""Foreign-byte fixtures: reference-encoded streams (SOP + EPH) whose packet
bodies are overwritten in place (tests/foreign_bytes.py overwrite_bodies:
noise, sparse, tailff), decoded by the reference itself (oracle/_ref/ref_driver,
Grok 5.1.0 as oracle/ref.mk builds it).  Every header and every length stays
as the encoder wrote it, so the streams are well-formed down to the packet
headers while their code-block bytes are ones no Grok encoder writes: markers
inside segments, segments that end before the decoder stops reading, raw
(BYPASS) segments holding FF 80..8F pairs -- through the segment cursor, the raw
reader, TERMALL's segment per pass, RESET and segments split over layers, which
the block oracle does not have.  A decode must return what Grok returns.

Writes tests/golden/fg_*.j2k (the clean bases), fg_*.<pattern>.dec.npy (the
reference's decode of the overwritten base) and tests/golden/manifest_foreign.json;
the overwritten streams are rebuilt from the bases by the test, so none is
stored, and the two bases of more than 4,096 code-blocks are kept as hashes
only.  TEST INFRASTRUCTURE ONLY.
  python oracle/make_golden_foreign.py [--check]"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.join(os.path.dirname(HERE), "tests")]

import numpy as np  # noqa: E402

import make_golden as mg  # noqa: E402
import foreign_bytes as fb  # noqa: E402

SE = ["-S", "-E"]
# name, (h, w, c, bits), kind, seed, grk_compress args.  The images are chosen
# so that tailff changes the decode: with TERMALL on one lossless component the
# last byte of a packet body is never consumed (RGB bases there), and a 9/7
# decode of a 12- or 16-bit image rounds a last byte's change away (8 bits there).
SMALL = [
    ("fg_M0", (96, 128, 1, 8), "smooth", 201, SE + ["-M", "0"]),
    ("fg_M1_I", (96, 128, 1, 8), "smooth", 202, SE + ["-M", "1", "-I"]),
    ("fg_M5", (64, 80, 3, 8), "smooth", 203, SE + ["-M", "5"]),
    ("fg_M4_b32", (64, 80, 3, 8), "smooth", 204, SE + ["-M", "4", "-b", "32,32"]),
    ("fg_M10", (77, 100, 1, 8), "uniform", 205, SE + ["-M", "10"]),
    ("fg_M63_r", (96, 128, 3, 8), "smooth", 206, SE + ["-M", "63", "-r", "20,5"]),
]
# more than 4,096 code-blocks in one call (the size of make_golden.py's m_rgb12u_640_b16_*)
MANY = [
    ("fgm_rgb12u_640_b16_M1", (640, 640, 3, 12), "uniform", 3, SE + ["-b", "16,16", "-M", "1"]),
    ("fgm_rgb12u_640_b16_M63", (640, 640, 3, 12), "uniform", 3, SE + ["-b", "16,16", "-M", "63"]),
]
# the overwrite's seed per (base, pattern): 1000 * position + pattern index
# unless listed here (a stream the reference refused would get another seed)
SEEDS = {}


def seed_of(k, name, pattern):
    return SEEDS.get((name, pattern), 1000 * (k + 1) + fb.PATTERNS.index(pattern))


def run(k, name, shape, kind, seed, args, patterns, tmp, keep):
    h, w, c, bits = shape
    img = mg.synth.synth_image(h, w, c, bits, seed, kind)
    base = mg.ref_encode(img, bits, args, tmp)
    clean, _ = mg.ref_decode(base, tmp)
    rec = dict(shape=[h, w, c, bits], kind=kind, seed=seed, args=args, image_sha256=mg.synth.image_sha256(img),
               j2k_sha256=mg.sha(base), j2k_len=len(base), bodies=sum(e > s for s, e in fb.packet_bodies(base)),
               patterns={})
    if keep:
        with open(os.path.join(keep, name + ".j2k"), "wb") as f:
            f.write(base)
    for pat in patterns:
        ps = seed_of(k, name, pat)
        cs = fb.overwrite_bodies(base, pat, ps)
        assert len(cs) == len(base) and cs != base, (name, pat)
        dec, _ = mg.ref_decode(cs, tmp)  # a refusal ends the run (check=True): never dropped
        assert dec.shape == clean.shape and np.any(dec), (name, pat, "an all-zero decode")
        assert not np.array_equal(dec, clean), (name, pat, "the overwrite changed nothing")
        rec["patterns"][pat] = dict(seed=ps, j2k_sha256=mg.sha(cs), dec_sha256=mg.synth.image_sha256(dec),
                                    differs=int(np.count_nonzero(dec != clean)))
        if keep:
            np.save(os.path.join(keep, "%s.%s.dec.npy" % (name, pat)), dec.astype(np.int32))
    return rec


def main():
    check = "--check" in sys.argv
    mg.build_ref()
    path = os.path.join(mg.GOLD, "manifest_foreign.json")
    man = {"small": {}, "many": {}}
    with tempfile.TemporaryDirectory() as tmp, tempfile.TemporaryDirectory() as out:
        keep = out if check else mg.GOLD
        for k, case in enumerate(SMALL):
            man["small"][case[0]] = run(k, *case, fb.PATTERNS, tmp, keep)
            print(case[0], man["small"][case[0]]["j2k_len"], flush=True)
        for k, case in enumerate(MANY):
            man["many"][case[0]] = run(100 + k, *case, ("noise", "sparse"), tmp, None)
            print(case[0], man["many"][case[0]]["j2k_len"], flush=True)
        if check:
            old = json.load(open(path))
            bad = int(old != json.loads(json.dumps(man)))
            for name, rec in man["small"].items():
                with open(os.path.join(mg.GOLD, name + ".j2k"), "rb") as f:
                    bad += mg.sha(f.read()) != rec["j2k_sha256"]
                for pat, p in rec["patterns"].items():
                    d = np.load(os.path.join(mg.GOLD, "%s.%s.dec.npy" % (name, pat)))
                    bad += mg.synth.image_sha256(d) != p["dec_sha256"]
            print("mismatches", bad)
            sys.exit(1 if bad else 0)
    with open(path, "w") as f:
        json.dump(man, f, indent=1)
    print("ok", len(SMALL) + len(MANY))


if __name__ == "__main__":
    main()
