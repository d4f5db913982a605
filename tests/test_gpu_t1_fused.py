"""The T1 decoder's column step on the GPU (t1_dec.h d3_column: one step per
sample, a sample's significance and sign decision in the same step), on the two
launch shapes of k_t1_decode_ub:

  260 x 288 gray 12-bit, 4x4 code-blocks, one resolution: 4,680 blocks, so the
      4-wavefront 128-VGPR kernel runs (num_cblks > 4096 is asserted, as in
      tests/test_gpu_t1_many.py); the blocks are the image's own samples less
      the DC shift, so the dense content below reaches the block coder as it is
  130 x 67, 64x64 code-blocks, two resolutions: eight blocks of odd sizes, one
      block per wavefront

Content: "dense" -- every sample 512..1023 away from mid-grey, the sign
alternating in the left half and random in the right, so every sample turns
significant in one plane and a column yields 4 ZC + 4 SC decisions -- and
synth "uniform" noise.  Styles -M 0, 1 (BYPASS), 8 (VSC), 63 (all six
switches); 5/3 and 9/7; each stream decoded under the default plan and under
t1_lone = -1 (the batch plan).

Bar: the 5/3 decode is the image; every decode equals the C oracle's decode
sample for sample; two consecutive decodes of one stream are identical.  The
oracle's decoder reads cblksty == 0 streams only (oracle/grk_oracle.c), so the
oracle's decode of the -M 0 stream of the same image and wavelet stands for the
styled streams too: no layer or rate cut is set, every pass of every block is
in each stream, and the mode switches change the bytes, never the fully decoded
coefficients (tests/cpp/test_t1_modes.cpp holds the block coder to the same).
"""
import functools

import numpy as np
import pytest

import synth

pytestmark = pytest.mark.gpu

SIZES = {"b4": ((260, 288), ["-b", "4,4", "-n", "1"]), "b64": ((67, 130), ["-b", "64,64", "-n", "2"])}


@functools.lru_cache(maxsize=None)
def _image(size, content):
    h, w = SIZES[size][0]
    if content == "uniform":
        img = synth.synth_image(h, w, 1, 12, 7, "uniform")
    else:
        rs = np.random.RandomState(11)
        mag = 512 + rs.randint(0, 512, size=(h, w))
        yy, xx = np.mgrid[0:h, 0:w]
        sign = np.where((xx + yy) & 1, -1, 1)
        sign[:, w // 2:] = np.where(rs.randint(0, 2, size=(h, w - w // 2)), -1, 1)
        img = (2048 + sign * mag).astype(np.int32)[None]
    img.setflags(write=False)
    return img


def _params(size, irrev, sty):
    import grokimagecompression_amd as grk
    args = SIZES[size][1] + (["-I"] if irrev else []) + (["-M", str(sty)] if sty else [])
    return grk.CParams.from_cli(args)


@functools.lru_cache(maxsize=None)
def _reference(codec, size, content, irrev):
    """the C oracle's decode of the -M 0 stream (computed once per image and wavelet)"""
    import pyoracle
    p, off = _params(size, irrev, 0)
    ref = pyoracle.decode(codec.compress(_image(size, content), 12, p, offset=off), nthreads=4)
    ref.setflags(write=False)
    return ref


@pytest.mark.parametrize("sty", [0, 1, 8, 63])
@pytest.mark.parametrize("irrev", [False, True], ids=["53", "97"])
@pytest.mark.parametrize("content", ["dense", "uniform"])
@pytest.mark.parametrize("size", sorted(SIZES))
def test_fused_column_step(codec, oracle, size, content, irrev, sty):
    import grokimagecompression_amd as grk
    import pyoracle
    img = _image(size, content)
    p, off = _params(size, irrev, sty)
    stream = codec.compress(img, 12, p, offset=off)
    if size == "b4":  # the coverage condition: the kernels picked from 4,096 blocks on
        assert codec.stats()["num_cblks"] > 4096, codec.stats()["num_cblks"]
    else:
        assert codec.stats()["num_cblks"] == 8, codec.stats()["num_cblks"]
    ref = _reference(codec, size, content, irrev)
    if sty == 0:  # the same stream through the oracle
        assert np.array_equal(pyoracle.decode(stream, nthreads=4), ref)
    for opts in ({}, dict(t1_lone=-1)):
        with grk.dwt_options(**opts):
            d1 = np.array(codec.decompress(stream))
            if size == "b4":
                assert codec.stats()["num_cblks"] > 4096
            d2 = np.array(codec.decompress(stream))
        assert np.array_equal(d1, d2), "two decodes of one stream differ (%s)" % (opts,)
        if not np.array_equal(d1, ref):
            ys = np.argwhere(d1 != ref)
            pytest.fail("decode %s: %d samples differ from the oracle's decode, first at (c, y, x) = %s"
                        % (opts, len(ys), tuple(ys[0])))
        if not irrev:
            assert np.array_equal(d1, img), "the 5/3 decode is not the image (%s)" % (opts,)
