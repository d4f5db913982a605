"""Decode straight to 8 / 16-bit and pixel-interleaved samples
(grkgpu_decompress_to, Codec.decompress(dtype=, layout=)): every value is the
reference's -- the committed fixtures tests/golden/<case>.dec.npy, or the int32
decode of the same stream (pinned to the reference with max-abs 0 by
test_gpu_parity.py) -- cast to the output type, tolerance 0."""
import json

import numpy as np
import pytest

from conftest import GOLD

pytestmark = pytest.mark.gpu

MAN = json.load(open(f"{GOLD}/manifest.json"))
NARROW = (np.uint8, np.int8, np.uint16, np.int16)


def formats(prec, sgnd=False):
    """The output dtypes holding a (prec, sgnd) component, int32 included."""
    return [dt for dt in NARROW if (np.iinfo(dt).min < 0) == bool(sgnd) and np.iinfo(dt).bits >= prec] + [np.int32]


def to_numpy(x):
    return x if isinstance(x, np.ndarray) else x.cpu().numpy()


def assert_is(got, ref, dtype, layout):
    """got == ref (the (c,h,w) int32 reference) in dtype and layout, exactly."""
    info = np.iinfo(dtype)
    assert info.min <= ref.min() and ref.max() <= info.max  # the cast cannot wrap
    want = ref.astype(dtype)
    if layout == "hwc":
        want = want.transpose(1, 2, 0)
    got = to_numpy(got)
    assert got.dtype == np.dtype(dtype) and got.shape == want.shape
    assert np.array_equal(got, want), (dtype, layout, int(np.argmax(got != want)))


def check_all(codec, cs, ref, dtypes, **kw):
    """Every dtype x layout x (host numpy, cuda tensor) of one stream."""
    for dt in dtypes:
        for layout in ("chw", "hwc"):
            for dev in (False, True):
                got = codec.decompress(cs, dtype=dt, layout=layout, device_out=dev, **kw)
                assert isinstance(got, np.ndarray) != dev
                assert_is(got, ref, dt, layout)


def gold(name):
    return open(f"{GOLD}/{name}.j2k", "rb").read()


FIXTURES = ["g8_3x5", "g8_1x37", "g8_45x1", "g8_100x77", "g8_off35", "g8_off_tiles", "rgb8_128x96", "rgb8_I",
            "rgb8_nomct", "rgb12_96x80", "rgb12_I", "rgb12_tiles_I", "rgb16_64", "g16_128"]


@pytest.mark.parametrize("name", FIXTURES)
def test_golden_fixture_in_every_format(codec, name):
    ref = np.load(f"{GOLD}/{name}.dec.npy")
    check_all(codec, gold(name), ref, formats(MAN[name]["shape"][3]))


@pytest.mark.parametrize("name,tag,dtype,kw", [
    ("rgb12_I", "r2", np.uint16, dict(reduce=2)),
    ("rgb12_I", "r1d9_13_70_61", np.uint16, dict(reduce=1, window=(9, 13, 70, 61))),
    ("g8_off_tiles", "r2", np.uint8, dict(reduce=2)),  # odd origin: the plane's margin must be zero
    ("rgb8_rlcp_layers", "l1", np.uint8, dict(layers=1)),
])
def test_decode_options_in_narrow_formats(codec, name, tag, dtype, kw):
    ref = np.load(f"{GOLD}/{name}.{tag}.dec.npy")
    cs = gold(name)
    for layout in ("chw", "hwc"):
        for dev in (False, True):
            # a pre-filled output: the zero margin of a reduced decode has to be written
            shape = ref.shape if layout == "chw" else (ref.shape[1], ref.shape[2], ref.shape[0])
            out = np.full(shape, 0x5A, dtype=dtype)
            if dev:
                import torch
                out = torch.from_numpy(out).cuda()
            got = codec.decompress(cs, out=out, layout=layout, **kw)
            assert got is out
            assert_is(got, ref, dtype, layout)


def test_alignment_sweep(codec):
    """Rows of 1 .. 9 and 63 .. 65 three-byte pixels: every row start of the
    second row falls on another byte offset, heads and tails of every length."""
    import grokimagecompression_amd as grk
    rng = np.random.default_rng(7)
    for w in list(range(1, 10)) + [63, 64, 65]:
        img = rng.integers(0, 256, size=(3, 2, w)).astype(np.int32)
        cs = codec.compress(img, 8, grk.CParams.make(numresolution=1))
        ref = codec.decompress(cs)
        assert np.array_equal(ref, img)
        for layout in ("hwc", "chw"):
            assert_is(codec.decompress(cs, dtype=np.uint8, layout=layout), ref, np.uint8, layout)
            assert_is(codec.decompress(cs, dtype=np.uint8, layout=layout, device_out=True), ref, np.uint8, layout)


@pytest.fixture(scope="module")
def odd_tiles(codec):
    """101 x 67 at offset (3,5) in tiles of 37 x 29: 8-bit 5/3 and 12-bit 9/7
    streams with their int32 decodes."""
    import grokimagecompression_amd as grk
    import synth
    out = {}
    for bits, args in ((8, []), (12, ["-I"])):
        img = synth.synth_image(67, 101, 3, bits, 900 + bits)
        p, off = grk.CParams.from_cli(["-t", "37,29", "-d", "3,5"] + args)
        cs = codec.compress(img, bits, p, offset=off)
        ref = codec.decompress(cs)
        ref.setflags(write=False)
        if not args:
            assert np.array_equal(ref, img)
        out[bits] = (cs, ref)
    return out


@pytest.mark.parametrize("bits", [8, 12])
def test_odd_tiles(codec, odd_tiles, bits):
    cs, ref = odd_tiles[bits]
    check_all(codec, cs, ref, formats(bits))


def test_signed_samples(codec):
    import grokimagecompression_amd as grk
    import synth
    for bits, dt in ((8, np.int8), (12, np.int16)):
        img = synth.synth_image(17, 33, 1, bits, 60 + bits, signed=True)
        assert img.min() < 0
        cs = codec.compress(img, bits, grk.CParams.make(numresolution=3), sgnd=True)
        ref = codec.decompress(cs)
        assert np.array_equal(ref, img)
        check_all(codec, cs, ref, [dt])


def test_four_components(codec):
    """MCT over the first three components, the fourth passes through."""
    import grokimagecompression_amd as grk
    import synth
    img = synth.synth_image(24, 40, 4, 8, 77)
    cs = codec.compress(img, 8, grk.CParams.make(numresolution=3, mct=1))
    ref = codec.decompress(cs)
    assert np.array_equal(ref, img)
    check_all(codec, cs, ref, [np.uint8, np.uint16])


def test_five_components_interleaved(codec):
    """A component count without a packed-store kernel (one store per sample)."""
    import grokimagecompression_amd as grk
    import synth
    img = synth.synth_image(9, 21, 5, 8, 78)
    cs = codec.compress(img, 8, grk.CParams.make(numresolution=2, mct=1))
    ref = codec.decompress(cs)
    assert np.array_equal(ref, img)
    check_all(codec, cs, ref, [np.uint8])


def test_tile_shards(codec, odd_tiles):
    """decompress_tiles into uint8: the range's samples, every other sample untouched."""
    import torch
    cs, ref = odd_tiles[8]
    c, h, w = ref.shape
    tiles = []  # tile rectangles on the image's own grid (origin 3,5; tiles 37 x 29 from 0,0)
    for ty in range(3):
        for tx in range(3):
            tiles.append((max(37 * tx, 3) - 3, max(29 * ty, 5) - 5, min(37 * (tx + 1), 104) - 3,
                          min(29 * (ty + 1), 72) - 5))
    for b, e in ((0, 1), (1, 4), (8, 9)):
        want = np.full((c, h, w), 0xA5, dtype=np.uint8)
        for x0, y0, x1, y1 in tiles[b:e]:
            want[:, y0:y1, x0:x1] = ref[:, y0:y1, x0:x1]
        for layout in ("chw", "hwc"):
            wl = want if layout == "chw" else want.transpose(1, 2, 0)
            for dev in (False, True):
                out = np.full(wl.shape, 0xA5, dtype=np.uint8)
                if dev:
                    out = torch.from_numpy(out).cuda()
                codec.decompress_tiles(cs, b, e, out, layout=layout)
                assert np.array_equal(to_numpy(out), wl), (b, e, layout, dev)


def test_missing_tiles_are_zero(codec):
    """A stream cut before its later tiles: they decode to zero in every format."""
    cuts = json.load(open(f"{GOLD}/manifest_cut.json"))["rgb8_r10_tiles"]["cuts"]
    n = max(int(k) for k, v in cuts.items() if v != "error" and v["tiles"] == [0, 1])
    cs = gold("rgb8_r10_tiles")[:n]
    ref = codec.decompress(cs)
    assert ref.any() and not ref[:, -8:, -8:].any()  # the last tile was never reached
    for layout in ("chw", "hwc"):
        for dev in (False, True):
            shape = ref.shape if layout == "chw" else (ref.shape[1], ref.shape[2], ref.shape[0])
            out = np.full(shape, 0x5A, dtype=np.uint8)
            if dev:
                import torch
                out = torch.from_numpy(out).cuda()
            assert_is(codec.decompress(cs, out=out, layout=layout), ref, np.uint8, layout)


@pytest.mark.parametrize("irrev", [False, True])
def test_stage_entry_point(irrev):
    """grkgpu_mct_inv_dcshift_to against grkgpu_mct_inv_dcshift on a copy, the
    destination starting 1, 2 and 3 samples past an aligned base; the samples
    around the destination stay untouched."""
    import torch
    import grokimagecompression_amd as grk
    rng = np.random.default_rng(11)
    for (w, h) in ((1, 1), (5, 3), (67, 9), (130, 4)):
        for prec, sgnd, tdt in ((8, False, torch.uint8), (12, True, torch.int16), (12, False, torch.uint16)):
            stride = w + 5
            lim = 3 << (prec - 1)  # past the component's range on both sides: the clamp works
            a = rng.integers(-lim, lim, size=(3, h, stride))
            src = (a.astype(np.float32) * 0.75).view(np.int32) if irrev else a.astype(np.int32)
            src = torch.from_numpy(np.ascontiguousarray(src)).cuda()
            want = grk.mct_inv_dcshift(src[:, :, :w].contiguous(), prec, sgnd, 1, irrev).cpu().numpy()
            npdt = np.dtype(str(tdt).replace("torch.", ""))
            for layout in ("chw", "hwc"):
                exp = want.astype(npdt) if layout == "chw" else want.astype(npdt).transpose(1, 2, 0)
                for off in (1, 2, 3):
                    for pad in (0, 3):
                        row = (w if layout == "chw" else 3 * w) + pad
                        rows = 3 * h if layout == "chw" else h
                        base = torch.from_numpy(np.full(off + rows * row + 16, 0x5A, dtype=npdt)).cuda()
                        grk.mct_inv_dcshift_to(src, base[off:], w, prec, sgnd, 1, irrev, layout=layout,
                                               dst_stride=row)
                        got = base.cpu().numpy()
                        body = got[off:off + rows * row].reshape(rows, row)
                        used = row - pad
                        assert np.array_equal(body[:, :used].reshape(exp.shape), exp), (w, h, tdt, layout, off, pad)
                        assert (body[:, used:] == 0x5A).all() and (got[:off] == 0x5A).all()
                        assert (got[off + rows * row:] == 0x5A).all()


def test_refusals_leave_the_context_usable(codec):
    import grokimagecompression_amd as grk
    import synth
    good = gold("rgb8_128x96")
    good_ref = np.load(f"{GOLD}/rgb8_128x96.dec.npy")

    def refused(code, cs, **kw):
        with pytest.raises(grk.GrkGpuError, match="grkgpu error %d:" % code):
            codec.decompress(cs, **kw)
        assert_is(codec.decompress(good, dtype=np.uint8, layout="hwc"), good_ref, np.uint8, "hwc")

    refused(-1, gold("rgb12_I"), dtype=np.uint8)        # GRKGPU_EINVAL: 12 bits in 8
    refused(-1, gold("rgb16_64"), dtype=np.int16)       # unsigned 16-bit in int16
    simg = synth.synth_image(17, 33, 1, 8, 68, signed=True)
    refused(-1, codec.compress(simg, 8, grk.CParams.make(numresolution=3), sgnd=True), dtype=np.uint16)
    sub = gold("sub_420_rgb8")
    refused(-4, sub, layout="hwc")                      # GRKGPU_EUNSUPPORTED: no pixels on mixed grids
    z = np.load(f"{GOLD}/sub_420_rgb8.dec.npz")
    planes = codec.decompress(sub, dtype=np.uint8)
    assert len(planes) == 3
    for k, p in enumerate(planes):
        assert p.dtype == np.uint8 and p.shape == z["c%d" % k].shape and np.array_equal(p, z["c%d" % k])


@pytest.mark.parametrize("name", ["g8_off_tiles", "rgb12_I", "rgb16_64"])
def test_default_path_unchanged(codec, name):
    ref = np.load(f"{GOLD}/{name}.dec.npy")
    d = codec.decompress(gold(name))
    assert isinstance(d, np.ndarray) and d.dtype == np.int32 and d.shape == ref.shape and np.array_equal(d, ref)
