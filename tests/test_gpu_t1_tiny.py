"""TERMALL (-M 4 and its combinations) on code-blocks of one to a few samples,
through whole images (tests/golden/manifest_tiny.json: oracle/make_golden.py
--tiny, hashes of the reference's codestream and of its decode, pinned by
tests/test_ref_pinning.py).

Every terminated coding pass costs about two bytes whatever the block's
size, so a 1x1 block of 13 or more bit-planes holds more than w*h*4 + 64
bytes: the MQ output slab is laid out by t1_enc_slab_bytes (t1_lane.h), and
the two overflow checks (the host-formed pass records, and k_pass_records
under rate control: the -r / -q cases) use the same rule -- an encode the
reference performs must not be refused.  The cases take all three Tier-1
launch plans by block count (1 .. 16, 2,809 and 4,356 blocks), tiles, an odd
image origin and three components.

test_fixture_is_in_the_regime (CPU) keeps the fixtures honest: the
bottom-right 1x1 block of an -n 1 case (no DWT: its coefficient is the corner
sample less 2^15, after the reversible colour transform where there is one)
must take more than w*h*4 + 64 = 68 bytes in the host build of the encoder.
Three cases cannot (BYPASS at 16 bits, a corner block that is not 1x1, a
smooth corner under SEGSYM) and are listed in NOT_IN_REGIME with the reason;
they run on the GPU like the others.

Bar: the reference's bytes, the reference decoder's image.
"""
import functools
import hashlib
import json

import numpy as np
import pytest

import synth
import t1_host
from conftest import GOLD

TINY = json.load(open(f"{GOLD}/manifest_tiny.json"))
CHUNK = 64 * 1024

ENC_OPTS = [{}, dict(t1_lone=1), dict(t1_lone=-1), dict(t1_lone=-1, t1_enc_sort=1), dict(t1_lone=-1, t1_enc_bpw=16)]
DEC_OPTS = [{}, dict(t1_lone=1), dict(t1_lone=-1), dict(t1_lone=-1, t1_dec_sort=0), dict(t1_lone=-1, t1_dec_bpw=16)]

# -n 1 cases whose bottom-right block is not a 1x1 block past 68 bytes:
NOT_IN_REGIME = {
    # BYPASS codes the passes below the top four planes raw and terminates two of three: over all 65,536
    # coefficients of a 16-bit sample the 1x1 block's longest stream is 53 bytes (the sweep: past 68 from 21 planes)
    "t_g16_65_n1_M5": "TERMALL|BYPASS: at most 53 bytes at 16 bits",
    # x1 = 67, y1 = 68: the corner block is 3x4
    "t_g16_67x66_n1_M4_d11": "no 1x1 block",
    # TERMALL|SEGSYM passes 68 bytes for 681 of the 65,536 coefficients only, none of them within the smooth
    # field's range at this corner (its uniform-noise twin t_g16u_545_b16_n1_M36_r20_1 is in the regime)
    "t_g16_545_b16_n1_M36_r20_1": "smooth corner sample outside the few in-regime values of style 36",
}


def _arg(args, flag, default):
    return args[args.index(flag) + 1] if flag in args else default


@functools.lru_cache(maxsize=2)
def _synth(shape, kind, seed):
    h, w, c, bits = shape
    img = synth.synth_image(h, w, c, bits, seed, kind)
    img.setflags(write=False)  # shared by the cases of one base
    return img


def _n1_cases():
    return sorted(n for n, m in TINY.items() if _arg(m["args"], "-n", "6") == "1")


def test_manifest_lists_the_cases():
    """The list as oracle/make_golden.py TINY has it: the three block-count
    ranges, tiles, an odd origin, three components, -r and -q, SEGSYM and
    BYPASS next to TERMALL."""
    assert len(TINY) >= 16
    sizes = {m["shape"][0] for m in TINY.values()}
    assert {65, 98, 129, 545, 833, 1041} <= sizes
    flags = {a for m in TINY.values() for a in m["args"]}
    assert {"-t", "-d", "-r", "-q", "-b"} <= flags
    modes = {int(_arg(m["args"], "-M", "0")) for m in TINY.values()}
    assert {4, 5, 6, 12, 36} <= modes and all(md & 4 for md in modes)
    assert len(_n1_cases()) - len(NOT_IN_REGIME) >= 9 and set(NOT_IN_REGIME) <= set(_n1_cases())


@pytest.fixture(scope="module")
def host_encoder(tmp_path_factory):
    return t1_host.build(tmp_path_factory.mktemp("t1tiny"))


@pytest.mark.parametrize("name", _n1_cases())
def test_fixture_is_in_the_regime(host_encoder, name):
    m = TINY[name]
    h, w, c, bits = m["shape"]
    a = m["args"]
    sty = int(_arg(a, "-M", "0"))
    x0, y0 = (int(v) for v in _arg(a, "-d", "0,0").split(","))
    cbw, cbh = (int(v) for v in _arg(a, "-b", "64,64").split(","))
    # with one resolution the code-block grid is the canvas grid: the bottom-right block is
    # [x1 - x1 % cbw .. x1) wide unless x1 is a multiple (tile edges here never cut it shorter)
    is_1x1 = (x0 + w) % cbw == 1 and (y0 + h) % cbh == 1
    px = [int(_synth(tuple(m["shape"]), m["kind"], m["seed"])[k, h - 1, w - 1]) - (1 << (bits - 1)) for k in range(c)]
    if c == 3 and _arg(a, "-Y", "1") != "0":  # the reversible colour transform
        r, g, b = px
        px = [(r + 2 * g + b) >> 2, b - g, r - g]
    lens = [len(host_encoder([(1, 1, 0, 1, 0, np.array([[v]], np.int32))], sty)[0][3]) for v in px]
    print(name, "corner coefficients", px, "bytes", lens)
    if name in NOT_IN_REGIME:
        assert not is_1x1 or min(lens) <= 68, "in the regime after all: take it off NOT_IN_REGIME"
        return
    assert is_1x1, name
    assert min(lens) > 1 * 1 * 4 + 64, (name, px, lens)


def _first_bad_chunk(b, m):
    for k, want in enumerate(m["chunk_sha256"]):
        if hashlib.sha256(b[k * CHUNK:(k + 1) * CHUNK]).hexdigest() != want:
            return k
    return len(m["chunk_sha256"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(TINY))
def test_tiny_block_images(codec, name):
    import grokimagecompression_amd as grk
    m = TINY[name]
    img = _synth(tuple(m["shape"]), m["kind"], m["seed"])
    bits = m["shape"][3]
    assert synth.image_sha256(img) == m["image_sha256"]
    p, off = grk.CParams.from_cli(m["args"])
    lossless = m["dec_vs_src_maxabs"] == 0  # also -r ..,1: the last layer holds every pass
    assert lossless or "-r" in m["args"] or "-q" in m["args"]  # 5/3 with no rate or quality target is lossless
    stream = None
    for opts in ENC_OPTS:
        with grk.dwt_options(**opts):
            b = codec.compress(img, bits, p, offset=off)
        if len(b) != m["j2k_len"] or hashlib.sha256(b).hexdigest() != m["j2k_sha256"]:
            bad = _first_bad_chunk(b, m)
            pytest.fail("%s encode %s: %d bytes (reference %d), first differing 64 KiB chunk %d (byte offset %d)"
                        % (name, opts, len(b), m["j2k_len"], bad, bad * CHUNK))
        stream = b
    for opts in DEC_OPTS:
        with grk.dwt_options(**opts):
            d = codec.decompress(stream)
        if lossless and not np.array_equal(d, img):
            ys = np.argwhere(np.asarray(d) != img)
            pytest.fail("%s decode %s: %d samples differ from the image, first at (c, y, x) = %s"
                        % (name, opts, len(ys), tuple(ys[0])))
        assert synth.image_sha256(d) == m["dec_sha256"], (name, opts)
