"""Code-block mode switches (-M, cblk_sty) through the Tier-1 kernels that are
picked by block count: every case of tests/golden/manifest_many.json has more
than 4,096 code-blocks of one style in one call (oracle/make_golden.py --many;
hashes of the reference's codestream and of its decode, pinned by
tests/test_ref_pinning.py).

Block-count ranges of the T1 selectors (kernels.hip launch_t1_encode /
launch_t1_decode) and who runs them:
  n <= 1,024         one block per wavefront          the goldens (test_gpu_parity.py)
  1,024 < n <= 4,096 2-32 blocks per wavefront        test_mid_size_blocks_per_wave (-M 0)
  n > 4,096          k_t1_decode_ub in 4-wavefront workgroups (128-VGPR cap,
                     shared LDS tables and rings), with and without BYPASS;
                     batch plan: k_t1_unstuff (lane per block, here with
                     several segments per block) and the wide MQ coder
                     k_t1_mq<64, 1, LAZY, MQ_WAVES, 19>         this file

The batch plan is what a call takes while others are in progress; t1_lone = -1
(grkgpu_dwt_options) gives it to a call that is alone, t1_lone = 1 the lone
plan.  Bar: the reference's bytes, the reference decoder's image.
"""
import functools
import hashlib
import json

import numpy as np
import pytest

import synth
from conftest import GOLD

pytestmark = pytest.mark.gpu
MANY = json.load(open(f"{GOLD}/manifest_many.json"))
CHUNK = 64 * 1024

ENC_OPTS = [{}, dict(t1_lone=1), dict(t1_lone=-1), dict(t1_lone=-1, t1_enc_sort=1), dict(t1_lone=-1, t1_enc_bpw=16)]
DEC_OPTS = [{}, dict(t1_lone=1), dict(t1_lone=-1), dict(t1_lone=-1, t1_dec_sort=0), dict(t1_lone=-1, t1_dec_bpw=16)]


@functools.lru_cache(maxsize=2)
def _synth(shape, kind, seed):
    h, w, c, bits = shape
    img = synth.synth_image(h, w, c, bits, seed, kind)
    img.setflags(write=False)  # shared by the cases of one base
    return img


def _first_bad_chunk(b, m):
    for k, want in enumerate(m["chunk_sha256"]):
        if hashlib.sha256(b[k * CHUNK:(k + 1) * CHUNK]).hexdigest() != want:
            return k
    return len(m["chunk_sha256"])


def test_manifest_covers_the_matrix():
    """The matrix as oracle/make_golden.py MANY lists it: every combination of
    the six switches on one base, the other bases' styles, one layers and
    one reduce variant."""
    assert len(MANY) >= 81
    modes = {int(m["args"][m["args"].index("-M") + 1]) for m in MANY.values()}
    assert set(range(1, 64)) <= modes
    for n in ("m_rgb12u_640_b16_M17", "m_rgb12u_640_b16_I_r_M62", "m_rgb12u_640_b16_r_M5", "m_g8_1100_b16_t256_M46",
              "m_g12u_2100_b32_M1", "m_g12u_2100_b32_M63", "m_g16_1300_b16_d53_M21"):
        assert n in MANY
    tags = [(n, t) for n in MANY for t in MANY[n].get("variants", {})]
    assert any(t.startswith("l") for _, t in tags) and any(t.startswith("r") for _, t in tags)


@pytest.mark.parametrize("name", sorted(MANY))
def test_many_block_mode_switches(codec, name):
    import grokimagecompression_amd as grk
    m = MANY[name]
    img = _synth(tuple(m["shape"]), m["kind"], m["seed"])
    bits = m["shape"][3]
    assert synth.image_sha256(img) == m["image_sha256"]
    p, off = grk.CParams.from_cli(m["args"])
    lossless = "-I" not in m["args"] and "-r" not in m["args"]  # 5/3 with no rate target
    assert not lossless or m["dec_vs_src_maxabs"] == 0
    stream = None
    for k, opts in enumerate(ENC_OPTS):
        with grk.dwt_options(**opts):
            b = codec.compress(img, bits, p, offset=off)
        if k == 0:  # the coverage condition: the kernels picked from 4,096 blocks on
            assert codec.stats()["num_cblks"] > 4096, (name, codec.stats()["num_cblks"])
        if len(b) != m["j2k_len"] or hashlib.sha256(b).hexdigest() != m["j2k_sha256"]:
            bad = _first_bad_chunk(b, m)
            pytest.fail("%s encode %s: %d bytes (reference %d), first differing 64 KiB chunk %d (byte offset %d)"
                        % (name, opts, len(b), m["j2k_len"], bad, bad * CHUNK))
        stream = b
    for k, opts in enumerate(DEC_OPTS):
        with grk.dwt_options(**opts):
            d = codec.decompress(stream)
        if k == 0:
            assert codec.stats()["num_cblks"] > 4096, (name, codec.stats()["num_cblks"])
        if lossless and not np.array_equal(d, img):
            ys = np.argwhere(np.asarray(d) != img)
            pytest.fail("%s decode %s: %d samples differ from the image, first at (c, y, x) = %s"
                        % (name, opts, len(ys), tuple(ys[0])))
        assert synth.image_sha256(d) == m["dec_sha256"], (name, opts)
    for tag, v in m.get("variants", {}).items():
        a = v["args"]
        reduce = int(a[a.index("-r") + 1]) if "-r" in a else 0
        layers = int(a[a.index("-l") + 1]) if "-l" in a else 0
        for opts in ({}, dict(t1_lone=-1)):
            with grk.dwt_options(**opts):
                d = codec.decompress(stream, reduce=reduce, layers=layers)
            assert synth.image_sha256(d) == v["dec_sha256"], (name, tag, opts)
