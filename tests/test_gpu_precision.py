"""Every sample precision 1 .. 16, signed samples and 1 .. 5 components
(mixed ones included) against the REFERENCE: the p_* fixtures of
oracle/make_golden_prec.py.  Tolerance 0 on codestream bytes and on decoded
samples.

The precision and the sign reach the DC shift (k_dcshift_mct_fwd*, the fused
level-0 loads of k_dwt_fwd_mct3, k_mct_inv_dcshift*), the decode clamp, the
quantisation (reversible exponents, the irreversible base step
2^-(prec + sgnd), the bit-plane count of every band), the rate control's byte
budgets and PSNR targets, the SIZ Ssiz byte and the narrowing stores.  A
mistake that is symmetric between our encoder and our decoder round-trips
perfectly; only another codec's bytes show it.

Images the reference refuses to encode ("ref_enc": "refused", busy images of
less than 6 bits: its tile buffer holds about 0.1625 bytes per sample-bit)
are pinned to the CPU oracle's stream and the reference's decode of it; see
test_refused_by_reference.
"""
import numpy as np
import pytest

import synth
from conftest import GOLD, load_manifest
from prec_fixtures import PREC, REFUSED, image, precs, ranges, ref_decode, sgnds, stream
from test_gpu_decode_formats import check_all, formats

pytestmark = pytest.mark.gpu

NAMES = sorted(PREC)


def _params(m):
    import grokimagecompression_amd as grk
    return grk.CParams.from_cli(m["args"])


def _scalar_or_list(v):
    return v[0] if len(set(v)) == 1 else v


def _compress(codec, m, img, layout="chw"):
    p, off = _params(m)
    return codec.compress(img, _scalar_or_list(precs(m)), p, offset=off, sgnd=_scalar_or_list(sgnds(m)), layout=layout)


def _dtypes(m):
    """The output / input dtypes that hold every component of the case (int32 last)."""
    per = [formats(p, s) for p, s in zip(precs(m), sgnds(m))]
    return [dt for dt in per[0] if all(dt in f for f in per)]


@pytest.mark.parametrize("name", NAMES)
def test_encode_matches_reference(codec, name):
    """int32 planes, and the narrowest numpy dtype holding the samples, planar
    and pixel-interleaved: the reference's bytes (for a refused case the
    oracle's, test_refused_by_reference)."""
    m = PREC[name]
    img = image(m)
    gold = stream(name)
    b = _compress(codec, m, img)
    assert len(b) == len(gold) == m["j2k_len"]
    assert b == gold
    dt = _dtypes(m)[0]
    assert dt is np.int32 or np.iinfo(dt).bits == (8 if max(precs(m)) <= 8 else 16)
    narrow = img.astype(dt)
    assert np.array_equal(narrow, img)
    assert _compress(codec, m, narrow) == gold
    assert _compress(codec, m, np.ascontiguousarray(narrow.transpose(1, 2, 0)), layout="hwc") == gold


def _assert_clamp_hits(m, d):
    """Where the reference's decode holds the range minimum / maximum, ours does."""
    lo = any((d[k] == mn).any() for k, (mn, mx) in enumerate(ranges(m)))
    hi = any((d[k] == mx).any() for k, (mn, mx) in enumerate(ranges(m)))
    assert [bool(lo), bool(hi)] == m["clamp_hits"]
    for k, (mn, mx) in enumerate(ranges(m)):
        assert mn <= d[k].min() and d[k].max() <= mx


def _variant_kw(args):
    return dict(reduce=int(args[args.index("-r") + 1]) if "-r" in args else 0,
                layers=int(args[args.index("-l") + 1]) if "-l" in args else 0)


@pytest.mark.parametrize("name", NAMES)
def test_decode_matches_reference(codec, name):
    m = PREC[name]
    cs = stream(name)
    ref = ref_decode(name)
    d = codec.decompress(cs)
    assert d.dtype == np.int32 and d.shape == ref.shape
    assert int(np.abs(d.astype(np.int64) - ref).max()) == 0
    _assert_clamp_hits(m, d)
    for tag, v in m.get("variants", {}).items():
        vref = ref_decode(name, tag)
        vd = codec.decompress(cs, **_variant_kw(v["args"]))
        assert vd.shape == vref.shape and np.array_equal(vd, vref), tag


@pytest.mark.parametrize("name", NAMES)
def test_decode_narrow_formats(codec, name):
    """Every dtype that holds the components (int8 at signed 1 .. 8 bits, int16
    at signed 9 .. 16, ...), planar and pixel-interleaved, host and device."""
    m = PREC[name]
    dts = _dtypes(m)
    if len(set(sgnds(m))) == 1:
        p, s = max(precs(m)), sgnds(m)[0]
        assert dts == formats(p, s) and len(dts) == (3 if p <= 8 else 2)
        assert (np.int8 if s else np.uint8) in dts or p > 8
    check_all(codec, stream(name), ref_decode(name), dts)


# What the encoder does with an image whose lossless stream exceeds the
# reference's tile-buffer bound ("Streams past the reference's
# tile-buffer bound"), pinned per case: "stream" = the whole stream, byte for
# byte the oracle's; "error" = a GrkGpuError.
REFUSED_OUTCOME = {
    "p_g1u": "stream", "p_g1s": "stream", "p_g1s_I": "stream", "p_rgb1u": "stream", "p_rgb1s": "stream",
    "p_g3s_uni_I": "stream", "p_g1u_uni": "stream", "p_g2s_uni": "stream", "p_g5s_uni_I": "stream",
}


def test_refused_cases_are_pinned():
    assert sorted(REFUSED_OUTCOME) == REFUSED
    for n in ("p_g1u", "p_g1u_uni", "p_rgb1u", "p_g2s_uni", "p_g5s_uni_I"):
        assert n in REFUSED
    assert all(min(precs(PREC[n])) < 6 for n in REFUSED) and 10 * len(REFUSED) <= len(PREC)


@pytest.mark.parametrize("name", REFUSED)
def test_refused_by_reference(codec, name):
    """An encode without -r / -q of an image the reference refuses ends in a
    GrkGpuError that leaves the codec usable, or in the oracle's stream, which
    decodes to the image (5/3) / to the reference's decode of it (9/7) --
    never in a stream cut to the tile bound that decodes to something else."""
    import grokimagecompression_amd as grk
    m = PREC[name]
    img = image(m)
    assert "-r" not in m["args"] and "-q" not in m["args"]
    try:
        b = _compress(codec, m, img)
    except grk.GrkGpuError:
        b = None
    assert ("error" if b is None else "stream") == REFUSED_OUTCOME[name]
    if b is None:
        g = load_manifest()["g8_64"]
        h, w, c, bits = g["shape"]
        gold = open(f"{GOLD}/g8_64.j2k", "rb").read()
        assert codec.compress(synth.synth_image(h, w, c, bits, g["seed"], g["kind"]), bits,
                              grk.CParams.from_cli(g["args"])[0]) == gold
        assert np.array_equal(codec.decompress(gold), np.load(f"{GOLD}/g8_64.dec.npy"))
    else:
        assert b == stream(name)
        d = codec.decompress(b)
        if "-I" not in m["args"]:
            assert np.array_equal(d, img)
    assert np.array_equal(codec.decompress(stream(name)), ref_decode(name))


# ---- encoder / decoder options ----
SIGNED_RGB = sorted(n for n, m in PREC.items() if m["signed"] and m["shape"][2] == 3 and "prec" not in m
                    and m["shape"][:2] == [37, 45] and m["kind"] == "smooth" and n not in REFUSED)


@pytest.mark.parametrize("fuse", [0, 1])
@pytest.mark.parametrize("name", SIGNED_RGB)
def test_encode_signed_fuse_level0(codec, name, fuse):
    """fuse_level0 = 1: the DC shift (0 for signed samples) and the RCT / ICT
    in the first DWT level's loads (k_dwt_fwd_mct3); 0: the separate
    k_dcshift_mct_fwd pass.  The reference's bytes either way."""
    import grokimagecompression_amd as grk
    m = PREC[name]
    with grk.dwt_options(fuse_level0=fuse):
        assert _compress(codec, m, image(m)) == stream(name)


T1_ORDER = ["p_g1u", "p_g1u_I", "p_g1s", "p_rgb1u", "p_rgb1s_I", "p_g1u_uni", "p_x_rgb15s_uni_M63_tiles", "p_g16s",
            "p_g16s_I", "p_rgb16s", "p_rgb16s_I", "p_g16s_uni_I", "p_rgb16s_uni_I", "p_x_rgb16s_uni_I_r4"]


@pytest.mark.parametrize("name", T1_ORDER)
def test_t1_lane_orders(codec, name):
    """The fewest and the most bit-planes (1-bit, 15-bit with every mode
    switch, 16-bit signed) with the Tier-1 lanes in the other block order /
    packing: t1_enc_sort = 0 on encode, t1_dec_sort = 1 with 16 blocks per
    wavefront on decode."""
    import grokimagecompression_amd as grk
    m = PREC[name]
    with grk.dwt_options(t1_enc_sort=0):
        assert _compress(codec, m, image(m)) == stream(name)
    with grk.dwt_options(t1_dec_sort=1, t1_dec_bpw=16):
        assert np.array_equal(codec.decompress(stream(name)), ref_decode(name))
