"""The CPU oracle is pinned against reference-generated codestreams.

tests/golden/*.j2k were written by the reference grk_compress (Grok v5.1.0)
from tests/golden/synth.py images (oracle/make_golden.py); *.dec.npy are the
reference grk_decompress outputs.  The oracle must reproduce both exactly.
"""
import functools
import hashlib

import numpy as np
import pytest

import geom_fixtures
import prec_fixtures
import synth
from conftest import GOLD, load_manifest, oracle_supported

MAN = {k: v for k, v in load_manifest().items() if oracle_supported(v["args"])}


@pytest.mark.parametrize("name", sorted(MAN))
def test_oracle_encode_matches_reference(oracle, name):
    m = MAN[name]
    h, w, c, bits = m["shape"]
    img = synth.synth_image(h, w, c, bits, m["seed"], m["kind"])
    assert synth.image_sha256(img) == m["image_sha256"], "generator drift"
    p = oracle.params_from_args(m["args"], nthreads=4)
    b = oracle.encode(img, bits, p, oracle.image_offset_from_args(m["args"]))
    gold = open(f"{GOLD}/{name}.j2k", "rb").read()
    assert hashlib.sha256(gold).hexdigest() == m["j2k_sha256"]
    assert b == gold


@pytest.mark.parametrize("name", sorted(MAN))
def test_oracle_decode_matches_reference(oracle, name):
    gold = open(f"{GOLD}/{name}.j2k", "rb").read()
    ref = np.load(f"{GOLD}/{name}.dec.npy")
    d = oracle.decode(gold, nthreads=4)
    assert d.shape == ref.shape
    assert np.array_equal(d, ref)


PMAN = {k: v for k, v in prec_fixtures.PREC.items() if oracle_supported(v["args"])}


@pytest.mark.parametrize("name", sorted(PMAN))
def test_oracle_encode_matches_precision_fixtures(oracle, name):
    """The p_* family (oracle/make_golden_prec.py): every precision 1 .. 16,
    signed samples, 2 / 4 components, components of mixed precision and sign.
    Where the reference refuses the image ("ref_enc": "refused") the fixture IS
    the oracle's stream; its decode below is still the reference's."""
    m = PMAN[name]
    p = oracle.params_from_args(m["args"], nthreads=4)
    b = oracle.encode(prec_fixtures.image(m), prec_fixtures.precs(m), p, sgnd=prec_fixtures.sgnds(m))
    gold = prec_fixtures.stream(name)
    assert hashlib.sha256(gold).hexdigest() == m["j2k_sha256"] and len(gold) == m["j2k_len"]
    assert b == gold


@pytest.mark.parametrize("name", sorted(PMAN))
def test_oracle_decode_matches_precision_fixtures(oracle, name):
    ref = prec_fixtures.ref_decode(name)
    d = oracle.decode(prec_fixtures.stream(name), nthreads=4)
    assert d.shape == ref.shape
    assert np.array_equal(d, ref)


def test_precision_fixtures_reach_the_clamps():
    """A clamp is tested only by a decode that reaches it: lossy 9/7 decodes
    holding both ends of the range exist for signed and unsigned, gray and
    ICT images; and every family is present."""
    P = prec_fixtures.PREC
    for signed in (False, True):
        for c in (1, 3):
            both = [n for n, m in P.items() if m["clamp_hits"] == [True, True] and m["dec_vs_src_maxabs"]
                    and m["signed"] == signed and m["shape"][2] == c and "prec" not in m and "-I" in m["args"]]
            assert len(both) >= 3, (signed, c, both)
    gray = {(m["shape"][3], m["signed"], "-I" in m["args"]) for m in P.values() if m["shape"][2] == 1}
    assert all((p, s, i) in gray for p in range(1, 17) for s in (False, True) for i in (False, True))
    assert {m["shape"][2] for m in P.values()} == {1, 2, 3, 4, 5} and sum("prec" in m for m in P.values()) == 4
    assert len(PMAN) >= 130


def test_oracle_lossless_roundtrip_random(oracle):
    rng = np.random.default_rng(7)
    for (h, w, c, bits) in [(33, 47, 1, 8), (19, 70, 3, 12), (64, 64, 3, 16)]:
        img = rng.integers(0, 1 << bits, size=(c, h, w)).astype(np.int32)
        b = oracle.encode(img, bits, oracle.params(numres=4))
        assert np.array_equal(oracle.decode(b), img)


def _ceil_pow2(v, r):
    return -(-v >> r)


REDUCE_CASES = [n for n in sorted(MAN) if "-I" not in MAN[n]["args"] and "-t" not in MAN[n]["args"]]


@pytest.mark.parametrize("name", REDUCE_CASES)
def test_oracle_reduce_is_forward_ll(oracle, name):
    """Reduced-resolution decode (grk_decompress -r) of a lossless stream is
    the image's own LL band after `reduce` forward levels, run back through
    the inverse RCT and the DC shift + clamp (TileProcessor.cpp:1165 stops
    the inverse DWT at minimum_num_resolutions; :1303-1432 run on the reduced
    buffers).  Parity is unpinned by reference fixtures (none exist for -r);
    this property pins it for 5/3."""
    m = MAN[name]
    h, w, c, bits = m["shape"]
    img = synth.synth_image(h, w, c, bits, m["seed"], m["kind"])
    gold = open(f"{GOLD}/{name}.j2k", "rb").read()
    args = m["args"]
    numres = int(args[args.index("-n") + 1]) if "-n" in args else 6
    mct = 0 if ("-Y" in args and args[args.index("-Y") + 1] == "0") or c < 3 else 1
    x0, y0 = map(int, args[args.index("-d") + 1].split(",")) if "-d" in args else (0, 0)
    shift = 1 << (bits - 1)
    fwd = oracle.dcshift_mct_fwd(list(img), [shift] * c, mct, False)
    for r in range(1, numres):
        red = oracle.decode(gold, reduce=r)
        rh = _ceil_pow2(y0 + h, r) - _ceil_pow2(y0, r)
        rw = _ceil_pow2(x0 + w, r) - _ceil_pow2(x0, r)
        assert red.shape == (c, rh, rw)
        ll = np.stack([oracle.dwt_fwd(p, x0, y0, r + 1, False)[:rh, :rw] for p in fwd])
        if mct:
            y, u, v = ll[0].astype(np.int64), ll[1].astype(np.int64), ll[2].astype(np.int64)
            g = y - ((u + v) >> 2)
            ll = np.stack([v + g, g, u + g])
        exp = np.clip(ll.astype(np.int64) + shift, 0, (1 << bits) - 1)
        assert np.array_equal(red, exp), (name, r)
    with pytest.raises(RuntimeError):
        oracle.decode(gold, reduce=numres)


# ---- the geometry sweep (oracle/make_golden_geom.py): reference == manifest == oracle ----
GEOM_ORACLE = [m["name"] for m in geom_fixtures.CASES if oracle_supported(m["args"]) and not m["subsampling"]]


@functools.lru_cache(maxsize=None)
def geom_oracle_stream(name):
    """The oracle's codestream of a sweep case (no stream is committed: the
    manifest holds the reference's hash of it)."""
    import pyoracle
    m = geom_fixtures.BY_NAME[name]
    p = pyoracle.params_from_args(m["args"], nthreads=4)
    return pyoracle.encode(geom_fixtures.image(m), m["bits"], p, pyoracle.image_offset_from_args(m["args"]))


def test_geom_sweep_reaches_the_oracle():
    """Enough of the sweep is within the options the oracle restates, and it
    holds tiled, offset, one-sample and deep-resolution cases."""
    cl = [set(geom_fixtures.BY_NAME[n]["classes"]) for n in GEOM_ORACLE]
    assert len(GEOM_ORACLE) >= 30
    for t in "abcdjk":
        assert sum(t in c for c in cl) >= 2, t


@pytest.mark.parametrize("name", GEOM_ORACLE)
def test_oracle_matches_reference_on_geom_sweep(oracle, name):
    """Encode: the recorded length and hash of the reference's codestream.
    Decode of those bytes: the recorded hash of the reference's decode, and of
    its -r decode where the case has one (the decoded samples, as
    oracle.decode returns them)."""
    m = geom_fixtures.BY_NAME[name]
    b = geom_oracle_stream(name)
    assert len(b) == m["j2k_len"]
    assert hashlib.sha256(b).hexdigest() == m["j2k_sha256"]
    d = oracle.decode(b, nthreads=4)
    assert geom_fixtures.planes_sha(list(d)) == m["dec_sha256"]
    for tag, v in m.get("variants", {}).items():
        if v["args"][0] != "-r":
            continue
        r = oracle.decode(b, nthreads=4, reduce=int(v["args"][1]))
        assert [list(p.shape) for p in r] == v["shapes"], tag
        assert geom_fixtures.planes_sha(list(r)) == v["dec_sha256"], tag
