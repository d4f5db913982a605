"""Decode straight to normalised float32 / float16 / bfloat16 samples
(grkgpu_decompress_float, Codec.decompress_float).  The expected value is always
float_fixtures.normalise() -- the two-rounding definition in numpy -- of the
int32 decode with the same arguments, which the other suites pin to the
reference; bit patterns are compared, not values."""
import numpy as np
import pytest

from conftest import GOLD
from float_fixtures import FLOATS, bits, normalise, same_bits

pytestmark = pytest.mark.gpu

WIDTHS = (1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 33)
HEIGHTS = (1, 3)


def _grk():
    import grokimagecompression_amd as grk
    return grk


def gold(name):
    return open(f"{GOLD}/{name}.j2k", "rb").read()


def image(c, h, w, prec, sgnd=False, seed=1):
    rs = np.random.RandomState(seed + 31 * c + 7 * w + h)
    lo, hi = (-(1 << (prec - 1)), 1 << (prec - 1)) if sgnd else (0, 1 << prec)
    return rs.randint(lo, hi, (c, h, w)).astype(np.int32)


def encode(codec, img, prec, sgnd=False, offset=(0, 0), **pk):
    grk = _grk()
    return codec.compress(np.ascontiguousarray(img), prec, grk.CParams.make(**{"numresolution": 2, "mct": 0, **pk}),
                          offset=offset, sgnd=sgnd)


def norm_for(c, k=0):
    """a different scale and a non-zero bias per channel, none of them a power of two"""
    scale = [(1.0 + 0.37 * ((ch + k) % 5)) / 255.0 for ch in range(c)]
    bias = [-0.485 / 0.229 + 0.61 * ((ch + 2 * k) % 4) for ch in range(c)]
    return np.array(scale), np.array(bias)


def nch(ref, layout):
    return len(ref) if isinstance(ref, list) else (ref.shape[0] if layout == "chw" else ref.shape[-1])


def check(codec, cs, names=FLOATS, layouts=("chw", "hwc"), dests=(True,), norm=None, **kw):
    """decompress_float against the restated int32 decode, for every format x layout x destination asked for"""
    n = 0
    for layout in layouts:
        ref = codec.decompress(cs, layout=layout, **kw)
        scale, bias = norm if norm is not None else norm_for(nch(ref, layout))
        for name in names:
            want = normalise(ref, scale, bias, name, layout)
            for dev in dests:
                dev = dev and not isinstance(ref, list)  # (a list of planes lives on the host)
                got = codec.decompress_float(cs, dtype=name, scale=scale, bias=bias, layout=layout, device_out=dev, **kw)
                if not isinstance(ref, list):
                    assert isinstance(got, np.ndarray) == (not dev and name != "bfloat16"), (name, dev, type(got))
                    assert bool(getattr(got, "is_cuda", False)) == dev
                assert same_bits(got, want), (name, layout, dev, kw)
                n += 1
    return n


# ---------------------------------------------------------------------------
# run geometry: the lead run, the cut last run, every run length
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("c", [1, 2, 3, 4, 5])
def test_run_geometry(codec, c):
    n = 0
    for irrev in (False, True):
        for mct in ((0, 1) if c >= 3 else (0,)):
            for h in HEIGHTS:
                for w in WIDTHS:
                    cs = encode(codec, image(c, h, w, 8), 8, irreversible=irrev, mct=mct,
                                numresolution=1 if min(w, h) < 4 else 2)
                    n += check(codec, cs)
    assert n == 2 * (2 if c >= 3 else 1) * len(HEIGHTS) * len(WIDTHS) * 6


# ---------------------------------------------------------------------------
# destination alignment: every 16-byte, 4-byte and odd start, canaries around it
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", FLOATS)
def test_destination_alignment(codec, name):
    import torch
    tdt = getattr(torch, name)
    per16 = 16 // torch.empty(0, dtype=tdt).element_size()
    for c, w, h in ((1, 33, 3), (3, 33, 3), (4, 17, 3), (2, 9, 3), (5, 16, 1)):
        cs = encode(codec, image(c, h, w, 8), 8)
        scale, bias = norm_for(c)
        for layout in ("chw", "hwc"):
            ref = codec.decompress(cs, layout=layout)
            want = bits(normalise(ref, scale, bias, name, layout))
            for off in range(per16):
                base = torch.full((off + c * h * w + 2 * per16,), 1.5, dtype=tdt, device="cuda:0")
                canary = int(bits(base[:1])[0])
                view = base[off:off + c * h * w].view(ref.shape)
                assert view.is_contiguous() and view.data_ptr() == base.data_ptr() + off * base.element_size()
                got = codec.decompress_float(cs, dtype=name, scale=scale, bias=bias, layout=layout, out=view)
                assert got is view
                b = bits(base)
                assert np.array_equal(b[off:off + c * h * w].reshape(want.shape), want), (c, w, layout, off)
                assert (b[:off] == canary).all() and (b[off + c * h * w:] == canary).all(), (c, w, layout, off)


# ---------------------------------------------------------------------------
# the conversions in front of the normalisation
# ---------------------------------------------------------------------------
def test_upsample_and_sycc_420(codec):
    cs = gold("sub_420_rgb8")  # 97 x 75, 4:2:0
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    norm = _grk().norm_scale_bias(8, mean, std)
    for kw in (dict(upsample=True), dict(colour="sycc")):
        assert check(codec, cs, names=("float16",), layouts=("hwc",), norm=norm, **kw) == 1
        assert check(codec, cs, **kw) == 6
    got = codec.decompress_float(cs, dtype="float16", scale=norm[0], bias=norm[1], layout="hwc", colour="sycc",
                                 device_out=True)
    assert tuple(got.shape) == (75, 97, 3) and str(got.dtype) == "torch.float16"
    # on the components' own grids: a list of host planes, each normalised with its channel's pair
    assert check(codec, cs, layouts=("chw",)) == 3


def test_precision_op_12_to_8(codec):
    cs = gold("rgb12_96x80")
    assert check(codec, cs, out_prec=8, prec_mode="scale") == 6
    assert check(codec, cs, out_prec=8, prec_mode="clip") == 6
    assert check(codec, cs) == 6  # (the identity precision op: plain normalisation of 12-bit samples)


@pytest.mark.parametrize("c", [4, 5, 6])
def test_cmyk(codec, c):
    cs = encode(codec, image(c, 9, 37, 8), 8)
    ref = codec.decompress(cs, colour="cmyk")
    assert ref.shape[0] == c - 1
    assert check(codec, cs, colour="cmyk") == 6
    assert check(codec, cs, colour="cmyk", out_prec=5, prec_mode="scale") == 6


def test_eycc(codec):
    cs = encode(codec, image(3, 9, 37, 8), 8)
    assert check(codec, cs, colour="eycc") == 6


def test_signed_12_bit(codec):
    img = image(3, 7, 21, 12, sgnd=True)
    img[0, 0, :4] = (-2048, 2047, -1, 0)
    for irrev in (False, True):
        cs = encode(codec, img, 12, sgnd=True, irreversible=irrev)
        ref = codec.decompress(cs)
        assert ref.min() < 0 and (irrev or np.array_equal(ref, img))
        assert check(codec, cs) == 6


def test_16_bit_to_float16_subnormals_and_inf(codec):
    img = image(3, 8, 33, 16)
    img[0, 0, :8] = (0, 1, 2, 3, 65519, 65520, 65535, 40000)
    img[1, 1, :4] = (65535, 65521, 32768, 1)
    cs = encode(codec, img, 16)
    assert np.array_equal(codec.decompress(cs), img)
    # 1 / 65535: samples 0 .. 3 are float16 subnormals or zero and are kept
    small = (np.float32(1.0 / 65535.0), 0.0)
    assert check(codec, cs, norm=(np.float32(2.0 ** -24), 0.0)) == 6
    assert check(codec, cs, norm=small) == 6
    want = normalise(img, np.float32(2.0 ** -24), 0.0, "float16")
    assert bits(want)[0, 0, :4].tolist() == [0, 1, 2, 3]
    # scale 1: 65520 and above are inf
    assert check(codec, cs, norm=(1.0, 0.0)) == 6
    want = normalise(img, 1.0, 0.0, "float16")
    assert bits(want)[0, 0, 4:7].tolist() == [0x7BFF, 0x7C00, 0x7C00] and np.isinf(want).sum() >= 4
    got = codec.decompress_float(cs, dtype="float16", device_out=True)
    assert same_bits(got, want)


# ---------------------------------------------------------------------------
# samples nothing decoded: the normalised zero
# ---------------------------------------------------------------------------
def test_reduced_decode_at_an_odd_origin(codec):
    for c in (1, 3, 4, 5):
        cs = encode(codec, image(c, 9, 21, 8), 8, offset=(5, 3), numresolution=3)
        plain = codec.decompress(cs, reduce=1)
        assert not plain[:, -1, :].any() and not plain[:, :, -1].any()  # the zero margin
        assert check(codec, cs, reduce=1, dests=(True, False)) == 12
        scale, bias = norm_for(c)
        got = codec.decompress_float(cs, scale=scale, bias=bias, reduce=1)
        for ch in range(c):
            assert (got[ch, -1, :] == np.float32(bias[ch])).all() and (got[ch, :, -1] == np.float32(bias[ch])).all()
    # with a colour step: the normalised conversion of zeros (CMYK of zeros is white)
    cs = encode(codec, image(4, 9, 21, 8), 8, offset=(5, 3), numresolution=3)
    assert check(codec, cs, reduce=1, colour="cmyk") == 6
    got = codec.decompress_float(cs, scale=2.0, bias=1.0, reduce=1, colour="cmyk")
    assert (got[:, -1, :] == 511.0).all()
    # components on different grids: each plane's margin on its own grid
    cd = lambda v, d: -(-v // d)  # noqa: E731  (the chroma grid of x 5 .. 26, y 3 .. 12 at (2,2): 10 x 4)
    ch, cw = cd(3 + 9, 2) - cd(3, 2), cd(5 + 21, 2) - cd(5, 2)
    planes = [image(1, 9, 21, 8)[0], image(1, ch, cw, 8, seed=2)[0], image(1, ch, cw, 8, seed=3)[0]]
    sub = codec.compress_subsampled(planes, 8, (21, 9), [(1, 1), (2, 2), (2, 2)], _grk().CParams.make(numresolution=3),
                                    offset=(5, 3))
    assert check(codec, sub, layouts=("chw",), reduce=1) == 3
    assert check(codec, sub, layouts=("chw",)) == 3


def test_window_with_odd_corners(codec):
    cs = encode(codec, image(3, 40, 61, 8), 8, offset=(3, 5), tiles=(32, 16))
    assert check(codec, cs, window=(11, 7, 57, 39)) == 6
    assert check(codec, gold("sub_420_rgb8"), window=(11, 7, 71, 61), upsample=True) == 6
    assert check(codec, gold("sub_420_rgb8"), layouts=("chw",), window=(11, 7, 71, 61)) == 3


def test_upsampled_stream_with_an_odd_origin(codec):
    cs = gold("sub_422_I_tiles")  # starts at X = 3 with dx = 2: a zero lead-in column in the chroma
    ref = codec.decompress(cs, upsample=True)
    assert not ref[1:, :, 0].any() and ref[1, :, 1].any()
    assert check(codec, cs, upsample=True, dests=(True, False)) == 12
    assert check(codec, cs, colour="sycc") == 6
    scale, bias = norm_for(3)
    got = codec.decompress_float(cs, scale=scale, bias=bias, upsample=True)
    assert (got[1, :, 0] == np.float32(bias[1])).all() and (got[2, :, 0] == np.float32(bias[2])).all()


def _cut_inside_second_tile(codec, cs):
    """cs cut inside its second tile-part where the integer decode accepts that, else in front of it"""
    grk = _grk()
    first = cs.index(b"\xff\x90")
    second = cs.index(b"\xff\x90", first + 2)
    for cut in (cs[:second + (len(cs) - second) // 2], cs[:second]):
        try:
            codec.decompress(cut)
            return cut
        except grk.GrkGpuError:
            pass
    raise AssertionError("the integer decode takes neither cut")


def test_tiles_a_cut_stream_never_reached(codec):
    grk = _grk()
    for c in (1, 3, 5):
        full = encode(codec, image(c, 8, 37, 8), 8, tiles=(32, 8))
        cut = _cut_inside_second_tile(codec, full)
        assert len(cut) < len(full)
        assert check(codec, cut, dests=(True, False)) == 12
        if len(grk.walk_tiles(cut)) < 2:  # the second tile was never reached: its samples are the bias
            scale, bias = norm_for(c)
            got = codec.decompress_float(cut, scale=scale, bias=bias, layout="hwc")
            assert not codec.decompress(cut)[:, :, 32:].any()
            assert np.array_equal(got[:, 32:, :], np.broadcast_to(bias.astype(np.float32), (8, 5, c)))
    # ... on components of different grids, and upsampled
    cs = gold("sub_cprl_tiles_layers")
    total = len(grk.walk_tiles(cs))
    assert total > 1
    cut = None
    for num in (5, 4, 6, 3, 7):
        try:
            if 0 < len(grk.walk_tiles(cs[:len(cs) * num // 10])) < total:
                cut = cs[:len(cs) * num // 10]
                break
        except grk.GrkGpuError:
            pass
    assert cut is not None
    ref = codec.decompress(cut)
    assert check(codec, cut, layouts=("chw",)) == 3
    if isinstance(ref, list):
        assert check(codec, cut, upsample=True) == 6


def test_host_destination(codec):
    import torch
    cs = encode(codec, image(3, 9, 37, 8), 8)
    scale, bias = norm_for(3)
    for name in FLOATS:
        for layout in ("chw", "hwc"):
            ref = codec.decompress(cs, layout=layout)
            want = normalise(ref, scale, bias, name, layout)
            got = codec.decompress_float(cs, dtype=name, scale=scale, bias=bias, layout=layout)
            if name == "bfloat16":
                assert isinstance(got, torch.Tensor) and not got.is_cuda and got.dtype == torch.bfloat16
                out = torch.zeros(ref.shape, dtype=torch.bfloat16)
            else:
                assert isinstance(got, np.ndarray) and got.dtype == np.dtype(name)
                out = np.zeros(ref.shape, dtype=name)
            assert same_bits(got, want)
            assert codec.decompress_float(cs, dtype=name, scale=scale, bias=bias, layout=layout, out=out) is out
            assert same_bits(out, want)
    # the defaults: float32, scale 1, bias 0 -- the integer decode's values, exactly
    assert np.array_equal(codec.decompress_float(cs), codec.decompress(cs).astype(np.float32))
    # the torch and numpy spellings of the dtype
    a = codec.decompress_float(cs, dtype=torch.float16, scale=scale, bias=bias)
    b = codec.decompress_float(cs, dtype=np.float16, scale=scale, bias=bias)
    assert same_bits(a, b) and same_bits(a, normalise(codec.decompress(cs), scale, bias, "float16"))
