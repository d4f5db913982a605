"""eYCC -> RGB, CMYK -> RGB and force-RGB in the store of the last decode kernel
(Codec.decompress(colour="eycc" | "cmyk", force_rgb=), decompress_jp2(colour=
"auto_rgb"), grk.convert_to).  Every expected value is this codec's plain int32
decode of the same stream with the same window / reduce / layers -- which
test_gpu_parity.py and its neighbours pin to the reference, and which for the
lossless 5/3 streams encoded here is the source itself -- pushed through the
numpy closed forms of tests/colour_fixtures.py, which
test_decode_colour_host.py pins to the reference's color.cpp.  Tolerance 0.

The shapes are the smallest at which the stores can go wrong: a lane owns 16
destination bytes on the destination's 16-byte grid, so widths 1 / 15 / 17 /
37, 3- and 4-byte pixels, and a tile seam off that grid."""
import numpy as np
import pytest

import colour_fixtures as cf
from test_decode_colour_host import cdef, jp2_file
from test_gpu_decode_convert import to_prec

pytestmark = pytest.mark.gpu

NARROW = (np.uint8, np.int8, np.uint16, np.int16)


def _grk():
    import grokimagecompression_amd as grk
    return grk


def image(c, h, w, precs, sgnds=None, seed=1):
    precs = precs if isinstance(precs, list) else [precs] * c
    sgnds = sgnds or [False] * c
    rs = np.random.RandomState(seed + 31 * c + w)
    return np.stack([rs.randint(-(1 << (p - 1)) if s else 0, (1 << (p - 1)) if s else (1 << p), (h, w))
                     for p, s in zip(precs, sgnds)]).astype(np.int32)


def encode(codec, img, precs, sgnds=False, offset=(0, 0), **pk):
    grk = _grk()
    return codec.compress(np.ascontiguousarray(img), precs, grk.CParams.make(**{"numresolution": 3, "mct": 0, **pk}),
                          offset=offset, sgnd=sgnds)


def expected(codec, cs, colour=None, force_rgb=False, out_prec=None, prec_mode="clip", **dk):
    """forcergb(precision(colour(plain decode))) -> ((c,h,w) int64, [(prec, sgnd), ...])"""
    grk = _grk()
    base = codec.decompress(cs, **dk)
    planes = [np.asarray(p) for p in base]
    d = grk._read_mct(cs)[0] if dk.get("custom_mct") else grk.read_header(cs)  # (read_header refuses MCT = 2)
    precs, sgnds = [d.prec[k] for k in range(d.numcomps)], [d.sgnd[k] for k in range(d.numcomps)]
    if colour == "eycc":
        planes = list(cf.eycc_to_rgb(planes[0], planes[1], planes[2], precs[0], sgnds[1], sgnds[2]))
        chans = [(precs[0], 0)] * 3
    elif colour == "cmyk":
        planes = cf.cmyk_to_rgb(planes, precs)
        chans = [(8, 0)] * 3 + list(zip(precs[4:], sgnds[4:]))
    else:
        chans = list(zip(precs, sgnds))
    if out_prec:
        planes = [to_prec(p, q, s, out_prec, prec_mode) for p, (q, s) in zip(planes, chans)]
        chans = [(out_prec, s) for _, s in chans]
    if force_rgb:
        planes, chans = cf.force_rgb(planes), cf.force_rgb(chans)
    return np.stack(planes).astype(np.int64), chans


def dtypes(chans):
    return [dt for dt in NARROW if all((np.iinfo(dt).min < 0) == bool(s) and np.iinfo(dt).bits >= p for p, s in chans)] \
        + [np.int32]


def check(codec, cs, dests=("host", "device"), layouts=("chw", "hwc"), only=None, **kw):
    """every format the output admits x both layouts x host and device destinations"""
    dk = {k: kw[k] for k in ("reduce", "window", "layers", "upsample", "custom_mct") if k in kw}
    ref, chans = expected(codec, cs, **kw)
    n = 0
    for dt in only or dtypes(chans):
        want = ref.astype(dt)
        assert np.array_equal(want, ref)
        for layout in layouts:
            w = want.transpose(1, 2, 0) if layout == "hwc" else want
            for dest in dests:
                got = codec.decompress(cs, dtype=dt, layout=layout, device_out=dest == "device",
                                       **{k: v for k, v in kw.items() if k not in dk}, **dk)
                got = got if isinstance(got, np.ndarray) else got.cpu().numpy()
                assert got.dtype == np.dtype(dt) and got.shape == w.shape, (dt, layout, dest, got.shape, w.shape)
                assert np.array_equal(got, w), (dt, layout, dest, kw, int(np.argmax(got != w)))
                n += 1
    return n


CONVERSIONS = {
    "eycc8": (3, 8, None, dict(colour="eycc")),
    "cmyk4": (4, 8, None, dict(colour="cmyk")),
    "cmyk5": (5, [8, 8, 8, 8, 8], None, dict(colour="cmyk")),
    "cmyk6": (6, [8, 8, 8, 8, 8, 8], None, dict(colour="cmyk")),
    "gray": (1, 8, None, dict(force_rgb=True)),
    "graya": (2, 8, None, dict(force_rgb=True)),
}


@pytest.mark.parametrize("w", [1, 15, 17, 37])
@pytest.mark.parametrize("conv", sorted(CONVERSIONS))
def test_widths(codec, conv, w):
    c, precs, sgnds, kw = CONVERSIONS[conv]
    img = image(c, 5, w, precs, sgnds)
    cs = encode(codec, img, precs, numresolution=1)
    assert np.array_equal(codec.decompress(cs), img)  # lossless: the decode is the source
    assert check(codec, cs, **kw) >= 8


@pytest.mark.parametrize("conv", sorted(CONVERSIONS))
def test_tile_seam_off_the_16_byte_grid(codec, conv):
    """45 x 11 at (3, 2) under 32 x 8 tiles: unaligned row starts, a seam at x = 32 - 3"""
    c, precs, sgnds, kw = CONVERSIONS[conv]
    img = image(c, 11, 45, precs, sgnds)
    cs = encode(codec, img, precs, offset=(3, 2), tiles=(32, 8), numresolution=2)
    check(codec, cs, **kw)


@pytest.mark.parametrize("prec", [8, 12, 16])
@pytest.mark.parametrize("signed_chroma", [False, True])
def test_eycc_precisions_signs_and_mct(codec, prec, signed_chroma):
    sg = [False, signed_chroma, signed_chroma]
    img = image(3, 9, 37, prec, sg)
    # the extremes of every component, next to each other
    lo = [-(1 << (prec - 1)) if s else 0 for s in sg]
    hi = [(1 << (prec - 1)) - 1 if s else (1 << prec) - 1 for s in sg]
    for i in range(8):
        img[:, 0, i] = [hi[k] if (i >> k) & 1 else lo[k] for k in range(3)]
    check(codec, encode(codec, img, prec, sg), colour="eycc")
    if not signed_chroma:  # (the MCT needs one sign) RCT, lossless; ICT, where the decode differs from the source
        check(codec, encode(codec, img, prec, sg, mct=1), colour="eycc", dests=("host",))
        check(codec, encode(codec, img, prec, sg, mct=1, irreversible=True), colour="eycc", dests=("host",))


@pytest.mark.parametrize("precs", [[16, 8, 12, 8], [12, 12, 12, 12], [16, 1, 8, 10], [12, 8, 8, 8, 12, 5]])
def test_cmyk_mixed_precisions(codec, precs):
    """(the widest component first: the encoder here writes one QCD, sized by component 0)"""
    c = len(precs)
    sg = [False] * 4 + [True, False][:c - 4]
    img = image(c, 7, 37, precs, sg)
    for k in range(4):
        img[k, 0, :4] = [0, (1 << precs[k]) - 1, 0, (1 << precs[k]) - 1]
    img[3, 0, :4] = [0, 0, (1 << precs[3]) - 1, (1 << precs[3]) - 1]
    check(codec, encode(codec, img, precs, sg), colour="cmyk")


@pytest.mark.parametrize("c", [4, 5, 6])
def test_cmyk_behind_an_mct(codec, c):
    img = image(c, 7, 37, 8)
    check(codec, encode(codec, img, 8, mct=1), colour="cmyk")
    check(codec, encode(codec, img, 8, mct=1, irreversible=True), colour="cmyk", dests=("host",))


COMBOS = [("eycc", 3, 12), ("cmyk", 4, 12), ("cmyk", 5, 12)]


@pytest.mark.parametrize("colour,c,prec", COMBOS)
def test_with_the_precision_op(codec, colour, c, prec):
    cs = encode(codec, image(c, 9, 37, prec), prec)
    for out_prec, mode in ((8, "clip"), (8, "scale"), (10, "scale"), (16, "scale"), (6, "clip")):
        check(codec, cs, colour=colour, out_prec=out_prec, prec_mode=mode, dests=("host",))


@pytest.mark.parametrize("colour,c,prec", COMBOS)
def test_with_window_reduce_and_layers(codec, colour, c, prec):
    grk = _grk()
    img = image(c, 40, 53, prec)
    cs = encode(codec, img, prec, tiles=(32, 32), offset=(3, 2))
    check(codec, cs, colour=colour, window=(9, 5, 46, 37), dests=("host",))
    check(codec, cs, colour=colour, reduce=1, dests=("host",))
    p, off = grk.CParams.from_cli(["-r", "20,1", "-n", "3"])
    cs2 = codec.compress(img, prec, p)
    assert not np.array_equal(codec.decompress(cs2, layers=1), codec.decompress(cs2))
    check(codec, cs2, colour=colour, layers=1, dests=("host",))


@pytest.mark.parametrize("colour,c,prec", COMBOS)
def test_all_subsampled_alike(codec, colour, c, prec):
    """every component at (2,2): converted on its grid without the upsample flag, replicated first with it"""
    w, h = 37, 11
    planes = [p for p in image(c, (h + 1) // 2, (w + 1) // 2, prec)]
    cs = codec.compress_subsampled(planes, prec, (w, h), [(2, 2)] * c)
    check(codec, cs, colour=colour, upsample=True)
    ref, chans = expected(codec, cs, colour=colour)
    for dt in dtypes(chans):
        got = codec.decompress(cs, colour=colour, dtype=dt)
        assert isinstance(got, list) and len(got) == len(ref)
        for g, r in zip(got, ref):
            assert g.dtype == np.dtype(dt) and np.array_equal(g, r)


@pytest.mark.parametrize("colour,c,prec", COMBOS)
def test_behind_a_custom_mct(codec, colour, c, prec):
    grk = _grk()
    rs = np.random.RandomState(c)
    m = np.eye(c, dtype=np.float32) + rs.uniform(-0.2, 0.2, (c, c)).astype(np.float32)
    p = grk.CParams.make(numresolution=3, irreversible=True).set_mct(m, [1 << (prec - 1)] * c)
    cs = codec.compress(image(c, 9, 37, prec), prec, p)
    check(codec, cs, colour=colour, custom_mct=True)


def _cut_before_second_tile(cs):
    first = cs.index(b"\xff\x90")
    return cs[:cs.index(b"\xff\x90", first + 2)]


@pytest.mark.parametrize("conv", ["eycc8", "cmyk4", "cmyk5", "cmyk6"])
def test_zero_fills_are_converted(codec, conv):
    c, precs, sgnds, kw = CONVERSIONS[conv]
    img = image(c, 8, 37, precs)
    cut = _cut_before_second_tile(encode(codec, img, precs, tiles=(32, 8), numresolution=2))
    ref, _ = expected(codec, cut, **kw)
    zero = np.stack(cf.closed_form(kw["colour"], [8] * c, [0] * c, [np.zeros(1, np.int32)] * c)[0])[:, 0]
    assert np.array_equal(codec.decompress(cut)[:, :, 32:], np.zeros((c, 8, 5)))  # the tile never reached
    assert (ref[:, :, 32:] == zero[:, None, None]).all() and zero[:3].any()
    check(codec, cut, **kw)
    # a reduced decode at an odd origin: a zero row and column behind the decoded samples
    odd = encode(codec, image(c, 9, 21, precs), precs, offset=(5, 3))
    plain = codec.decompress(odd, reduce=1)
    assert not plain[:, -1, :].any() and not plain[:, :, -1].any()
    check(codec, odd, reduce=1, **kw)


def test_force_rgb(codec):
    grk = _grk()
    g12 = encode(codec, image(1, 9, 37, 12), 12)
    ga = encode(codec, image(2, 9, 37, [12, 8]), [12, 8])
    gs = encode(codec, image(1, 9, 37, 8, [True]), 8, [True])
    for cs, nch in ((g12, 3), (ga, 4), (gs, 3)):
        ref, _ = expected(codec, cs, force_rgb=True)
        assert ref.shape[0] == nch and np.array_equal(ref[0], ref[1]) and np.array_equal(ref[0], ref[2])
        check(codec, cs, force_rgb=True)
    check(codec, g12, force_rgb=True, out_prec=8, prec_mode="scale")
    check(codec, ga, force_rgb=True, out_prec=8, prec_mode="clip", dests=("host",))
    # three or more channels: nothing after a conversion, refused without one
    rgb = encode(codec, image(3, 9, 37, 8), 8)
    check(codec, rgb, colour="eycc", force_rgb=True, dests=("host",))
    check(codec, encode(codec, image(4, 9, 37, 8), 8), colour="cmyk", force_rgb=True, dests=("host",))
    with pytest.raises(grk.GrkGpuError, match="don't know how to convert"):
        codec.decompress(rgb, force_rgb=True)
    # subsampled gray: not taken
    sub = codec.compress_subsampled([image(1, 5, 19, 8)[0]], 8, (37, 9), [(2, 2)])
    with pytest.raises(grk.GrkGpuError, match="grkgpu error -4"):
        codec.decompress(sub, force_rgb=True, upsample=True)


def test_jp2_auto_rgb(codec):
    grk = _grk()
    h, w = 9, 37
    cmyk = encode(codec, image(4, h, w, 8), 8)
    ycc = encode(codec, image(3, h, w, 8), 8)
    f12, f24, f18, f16 = (jp2_file(cmyk, h, w, 4, 12), jp2_file(ycc, h, w, 3, 24), jp2_file(ycc, h, w, 3, 18),
                          jp2_file(ycc, h, w, 3, 16))
    for data, cs, colour in ((f12, cmyk, "cmyk"), (f24, ycc, "eycc"), (f18, ycc, "sycc"), (f16, ycc, None)):
        want = (codec.decompress(cs, colour=colour, dtype=np.uint8, layout="hwc") if colour
                else codec.decompress(cs, dtype=np.uint8, layout="hwc"))
        if colour in ("cmyk", "eycc"):
            assert np.array_equal(want.transpose(2, 0, 1), expected(codec, cs, colour=colour)[0])
        for dev in (False, True):
            got, info = codec.decompress_jp2(data, colour="auto_rgb", dtype=np.uint8, layout="hwc", device_out=dev)
            got = got if isinstance(got, np.ndarray) else got.cpu().numpy()
            assert got.shape == (h, w, 3) and np.array_equal(got, want), (colour, dev)
        # "auto" keeps meaning sYCC only: CMYK and eYCC files come back as their components
        got, info = codec.decompress_jp2(data, colour="auto", dtype=np.uint8)
        plain = codec.decompress(cs, colour="sycc" if colour == "sycc" else None, dtype=np.uint8)
        assert np.array_equal(got, plain)
    # force-RGB: a gray file -> three channels; an sRGB file is left alone; an eYCC file without conversion is refused
    gray = encode(codec, image(1, h, w, 8), 8)
    got, _ = codec.decompress_jp2(jp2_file(gray, h, w, 1, 17), force_rgb=True, dtype=np.uint8)
    assert np.array_equal(got, np.repeat(codec.decompress(gray, dtype=np.uint8), 3, axis=0))
    got, _ = codec.decompress_jp2(f16, force_rgb=True, dtype=np.uint8)
    assert np.array_equal(got, codec.decompress(ycc, dtype=np.uint8))
    got, _ = codec.decompress_jp2(f12, colour="auto_rgb", force_rgb=True, dtype=np.uint8)
    assert np.array_equal(got, codec.decompress(cmyk, colour="cmyk", dtype=np.uint8))
    with pytest.raises(grk.GrkGpuError, match="don't know how to convert"):
        codec.decompress_jp2(f24, colour="auto", force_rgb=True)
    # behind a channel swap the conversions are refused
    with pytest.raises(grk.GrkGpuError, match="grkgpu error -4"):
        codec.decompress_jp2(jp2_file(ycc, h, w, 3, 24, extra=[cdef([(0, 0, 3), (1, 0, 2), (2, 0, 1)])]), colour="auto_rgb")


def _stage(planes, subs, precs, sgnds, dst_dt, layout, nch, rect=None, **ops):
    import torch
    grk = _grk()
    h, w = planes[0].shape
    rect = rect or (0, 0, w * subs[0][0], h * subs[0][1])
    W, H = rect[2] - rect[0], rect[3] - rect[1]
    off, pad = 3, 5
    row = (W * nch if layout == "hwc" else W) + pad
    rows = H if layout == "hwc" else nch * H
    base = torch.from_numpy(np.full(off + rows * row + 16, 0x5A, dtype=dst_dt)).cuda()
    src = [torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in planes]
    grk.convert_to(src, base[off:], rect, subs, precs, sgnds, layout=layout, dst_stride=row, **ops)
    got = base.cpu().numpy()
    body = got[off:off + rows * row].reshape(rows, row)
    assert (body[:, row - pad:] == 0x5A).all() and (got[:off] == 0x5A).all() and (got[off + rows * row:] == 0x5A).all()
    body = body[:, :row - pad]
    return body.reshape(H, W, nch).transpose(2, 0, 1) if layout == "hwc" else body.reshape(nch, H, W)


@pytest.mark.parametrize("layout", ["chw", "hwc"])
def test_stage_call(layout):
    h, w = 5, 37
    for src_dt, subs1 in ((np.int32, (1, 1)), (np.uint16, (1, 1)), (np.uint16, (2, 2))):
        up = lambda p: np.repeat(np.repeat(p, subs1[1], axis=0), subs1[0], axis=1)  # noqa: E731
        # eYCC, 12 bits
        ycc = image(3, h, w, 12)
        want = np.stack(cf.eycc_to_rgb(*[up(p) for p in ycc], 12))
        for dt in (np.uint16, np.int32):
            got = _stage([p.astype(src_dt) for p in ycc], [subs1] * 3, 12, False, dt, layout, 3, colour="eycc")
            assert np.array_equal(got, want), (src_dt, subs1, dt)
        # CMYK, 4 -> 3, 5 -> 4 and 6 -> 5
        for c in (4, 5, 6):
            precs = [8, 12, 16, 10] + [8] * (c - 4)
            inks = image(c, h, w, precs)
            want = np.stack(cf.cmyk_to_rgb([up(p) for p in inks], precs))
            for dt in (np.uint8, np.uint16, np.int32):
                got = _stage([p.astype(src_dt) for p in inks], [subs1] * c, precs, False, dt, layout, c - 1,
                             colour="cmyk")
                assert np.array_equal(got, want), (src_dt, subs1, dt, c)
    # force-RGB on finished int32 planes
    g = image(2, h, w, [12, 8])
    for c in (1, 2):
        got = _stage(list(g[:c]), [(1, 1)] * c, [12, 8][:c], False, np.uint16, layout, c + 2, force_rgb=True)
        assert np.array_equal(got, np.stack(cf.force_rgb(list(g[:c]))))


def test_dirty_context_and_a_call_of_another_kind():
    """each conversion on scratch an earlier, larger call left behind and debug_fill(0xFF) overwrote"""
    grk = _grk()
    own = grk.Codec(0)
    try:
        big = image(3, 96, 128, 12, seed=9)
        streams = {}
        for conv in sorted(CONVERSIONS):
            c, precs, sgnds, kw = CONVERSIONS[conv]
            streams[conv] = (encode(own, image(c, 11, 45, precs), precs, tiles=(32, 8), numresolution=2), kw)
        fresh = {conv: own.decompress(cs, layout="hwc", **kw) for conv, (cs, kw) in streams.items()}
        for conv, (cs, kw) in streams.items():
            ref, _ = expected(own, cs, **kw)
            assert np.array_equal(fresh[conv].transpose(2, 0, 1), ref)
            own.compress(big, 12, grk.CParams.make(irreversible=True))  # a call of another kind, on larger buffers
            assert own.debug_fill(0xFF) > 0
            assert np.array_equal(own.decompress(cs, layout="hwc", **kw), fresh[conv]), conv
            own.decompress(encode(own, big, 12), colour="sycc", dtype=np.uint16)
            assert np.array_equal(own.decompress(cs, layout="hwc", **kw), fresh[conv]), conv
    finally:
        own.close()
