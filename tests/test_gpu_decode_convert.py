"""sYCC -> RGB and the output precision in the store of the last decode kernel
(grkgpu_decompress_convert, Codec.decompress(colour=, out_prec=, prec_mode=),
grk.convert_to): every expected value is a reference-pinned decode -- the
reference's own planes under tests/golden, or this codec's planar decode, which
test_gpu_parity.py pins to them -- pushed through upsample() and the numpy
closed forms of color_sycc_to_rgb / clip_component / scale_component below,
tolerance 0."""
import ctypes
import functools

import numpy as np
import pytest

from conftest import GOLD
from test_gpu_decode_upsample import SUB, assert_is, expected, formats, gold, image_rect, to_numpy, upsample

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------
# the closed forms (pure numpy: test_decode_convert_host.py checks them against
# values worked by hand from the reference's loops)
# ---------------------------------------------------------------------------
def sycc_to_rgb(ycc, prec):
    """sycc_to_rgb (color.cpp:136-162) on full-size (3,h,w) planes.  float64
    products and their sum are separate numpy operations, each rounded on its
    own, and astype truncates toward zero -- the reference's C expression."""
    off, upb = 1 << (prec - 1), (1 << prec) - 1
    y = ycc[0].astype(np.int64)
    cb, cr = ycc[1].astype(np.float64) - off, ycc[2].astype(np.float64) - off
    r = y + (1.402 * cr).astype(np.int64)
    g = y - (0.344 * cb + 0.714 * cr).astype(np.int64)
    b = y + (1.772 * cb).astype(np.int64)
    return np.clip(np.stack([r, g, b]), 0, upb)


def to_prec(v, q, sgnd, p, mode):
    """clip_component / scale_component (convert.cpp:82-161): samples of
    precision q to precision p."""
    v = np.asarray(v).astype(np.int64)
    if p is None:
        return v
    if mode == "clip":
        return np.clip(v, -(1 << (p - 1)), (1 << (p - 1)) - 1) if sgnd else np.minimum(v, (1 << p) - 1)
    assert mode == "scale"
    if p == q:
        return v
    if p < q:
        return v >> (q - p)
    if sgnd:
        return v * (1 << (p - q))
    return (v * ((1 << p) - 1)) // ((1 << q) - 1)


def convert(planes, rect, subs, precs, sgnd=False, colour=None, out_prec=None, prec_mode="clip", up=True):
    """precision(colour(upsample(decode))) of per-component planes."""
    precs = [precs] * len(planes) if np.isscalar(precs) else list(precs)
    sg = [sgnd] * len(planes) if np.isscalar(sgnd) else list(sgnd)
    full = upsample(planes, rect, subs) if up else planes
    if colour == "sycc":
        full = sycc_to_rgb(full, precs[0])
    return [to_prec(full[k], precs[k], sg[k], out_prec, prec_mode) for k in range(len(planes))]


def narrowest(prec, sgnd=False):
    return formats(prec, sgnd)[0]


# ---------------------------------------------------------------------------
# the stage call
# ---------------------------------------------------------------------------
def _plane(torch, a, off=0, pad=0):
    """a on the device as a view starting `off` samples past an aligned
    address, its rows `pad` samples longer than a's."""
    h, w = a.shape
    flat = np.zeros(off + h * (w + pad) + 8, a.dtype)
    flat[off:off + h * (w + pad)].reshape(h, w + pad)[:, :w] = a
    t = torch.from_numpy(flat).cuda()
    return t[off:off + h * (w + pad)].view(h, w + pad)[:, :w]


def stage(grk, torch, planes, rect, subs, precs, dst_dt, layout, sgnd=False, off=0, pad=0, src_off=0, src_pad=0,
          **ops):
    """One grk.convert_to call against convert(); the guard samples around the
    destination and between its rows stay untouched."""
    x0, y0, x1, y1 = rect
    c, w, h = len(subs), x1 - x0, y1 - y0
    exp = np.stack(convert(planes, rect, subs, precs, sgnd, **ops))
    info = np.iinfo(dst_dt)
    assert info.min <= exp.min() and exp.max() <= info.max
    exp = exp.astype(dst_dt)
    if layout == "hwc":
        exp = exp.transpose(1, 2, 0)
    row = (w if layout == "chw" else c * w) + pad
    rows = c * h if layout == "chw" else h
    base = torch.from_numpy(np.full(off + rows * row + 16, 0x5A, dtype=dst_dt)).cuda()
    src = [_plane(torch, np.ascontiguousarray(q), src_off, src_pad) for q in planes]
    grk.convert_to(src, base[off:], rect, subs, precs, sgnd, layout=layout, dst_stride=row, **ops)
    got = base.cpu().numpy()
    body = got[off:off + rows * row].reshape(rows, row)
    used = row - pad
    where = (planes[0].dtype, dst_dt, subs, rect, layout, off, pad, src_off, src_pad, ops)
    assert np.array_equal(body[:, :used].reshape(exp.shape), exp), where
    assert (body[:, used:] == 0x5A).all() and (got[:off] == 0x5A).all(), where
    assert (got[off + rows * row:] == 0x5A).all(), where


def _grk_torch():
    import torch
    import grokimagecompression_amd as grk
    return grk, torch


S444, S422, S420 = [(1, 1)] * 3, [(1, 1), (2, 1), (2, 1)], [(1, 1), (2, 2), (2, 2)]


@pytest.mark.parametrize("dst_dt", [np.uint8, np.uint16, np.int32])
def test_stage_sycc_every_chroma_pair_at_8_bits(dst_dt):
    """All 65,536 (cb, cr) pairs -- Cb = row, Cr = column of a 256 x 256 chroma
    plane -- under Y = 0, 255 and a mixed luma; 4:4:4 from int32 planes (the
    inverse-MCT kernels' stores) and from uint8 planes (the general upsampling
    kernel), 4:2:0 and 4:2:2 under a 512 x 512 / 512 x 256 luma (k_upsample_420)."""
    grk, torch = _grk_torch()
    cb, cr = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    for subs, src_dts in ((S444, (np.int32, np.uint8)), (S420, (np.uint8,)), (S422, (np.uint8,))):
        dx, dy = subs[1]
        rect = (0, 0, 256 * dx, 256 * dy)
        mixed = upsample([(7 * cb + 13 * cr) & 255], rect, [subs[1]])[0]
        for luma in (np.zeros_like(mixed), np.full_like(mixed, 255), mixed):
            for src_dt in src_dts:
                planes = [luma.astype(src_dt), cb.astype(src_dt), cr.astype(src_dt)]
                for layout in ("chw", "hwc"):
                    stage(grk, torch, planes, rect, subs, 8, dst_dt, layout, colour="sycc")


@pytest.mark.parametrize("prec", [12, 16])
def test_stage_sycc_at_12_and_16_bits(prec):
    """65,536 random (cb, cr) pairs plus every corner of {0, off - 1, off, upb}^2,
    as 4:4:4 and as 4:2:2, into U16 and I32."""
    grk, torch = _grk_torch()
    rng = np.random.default_rng(41 + prec)
    off, upb = 1 << (prec - 1), (1 << prec) - 1
    corners = np.array([(a, b) for a in (0, off - 1, off, upb) for b in (0, off - 1, off, upb)])
    pairs = np.concatenate([rng.integers(0, upb + 1, size=(65536, 2)), corners, np.zeros((240, 2), np.int64)])
    cb, cr = pairs[:, 0].reshape(257, 256), pairs[:, 1].reshape(257, 256)
    for subs in (S444, S422):
        dx = subs[1][0]
        rect = (0, 0, 256 * dx, 257)
        for luma in (0, upb, None):
            y = rng.integers(0, upb + 1, size=(257, 256 * dx)) if luma is None else np.full((257, 256 * dx), luma)
            for src_dt, dst_dt, layout in ((np.int32, np.uint16, "hwc"), (np.uint16, np.int32, "chw"),
                                           (np.uint16, np.uint16, "chw")):
                stage(grk, torch, [y.astype(src_dt), cb.astype(src_dt), cr.astype(src_dt)], rect, subs, prec,
                      dst_dt, layout, colour="sycc")


SHAPES = {"sycc420": (S420, dict(colour="sycc")), "sycc422": (S422, dict(colour="sycc")),
          "prec_any": ([(1, 1), (3, 2), (2, 3)], dict(out_prec=5, prec_mode="scale")),
          "prec_420": (S420, dict(out_prec=7, prec_mode="clip"))}


@pytest.mark.parametrize("layout", ["chw", "hwc"])
@pytest.mark.parametrize("dst_dt", [np.uint8, np.uint16, np.int32])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_stage_runs_and_alignment(shape, dst_dt, layout):
    """Heads, tails and cut runs of every length: widths 1 .. 40 at x origins
    0 .. 3 and y origins 0, 1, the destination and the sources starting 0 .. 3
    samples off a 16-byte boundary (each offset with every width modulo 4),
    rows wider than the image between guard bands."""
    grk, torch = _grk_torch()
    subs, ops = SHAPES[shape]
    rng = np.random.default_rng(53)
    cd = lambda v, s: -(-v // s)  # noqa: E731
    src_dt = np.uint8 if dst_dt != np.int32 else np.uint16
    for w in range(1, 41):
        for ox in range(4):
            for oy in (0, 1):
                rect = (ox, oy, ox + w, oy + 3)
                planes = [rng.integers(0, 256, size=(cd(rect[3], dy) - cd(rect[1], dy),
                                                     cd(rect[2], dx) - cd(rect[0], dx))).astype(src_dt)
                          for dx, dy in subs]
                stage(grk, torch, planes, rect, subs, 8, dst_dt, layout, off=(w + ox) % 4, pad=3,
                      src_off=(w // 4 + ox + oy) % 4, src_pad=(w + oy) % 3, **ops)
    # the full product of the destination's and the sources' offsets at the widths around a run's length
    for w in (1, 15, 16, 17, 33):
        for ox in (0, 1):
            rect = (ox, 1, ox + w, 4)
            planes = [rng.integers(0, 256, size=(cd(rect[3], dy) - cd(rect[1], dy),
                                                 cd(rect[2], dx) - cd(rect[0], dx))).astype(src_dt)
                      for dx, dy in subs]
            for off in range(4):
                for src_off in range(4):
                    stage(grk, torch, planes, rect, subs, 8, dst_dt, layout, off=off, pad=3, src_off=src_off,
                          src_pad=1, **ops)


@pytest.mark.parametrize("sgnd", [False, True])
def test_stage_precision_every_value(sgnd):
    """Every representable value of every source precision 1 .. 16 to every
    output precision 1 .. 16, clip and scale; the sources in the narrowest type
    holding them (U16 -> U8 and the like: the launch reads one type and writes
    another) and, for the odd precisions, in int32 (the inverse-MCT kernels'
    planar store)."""
    grk, torch = _grk_torch()
    for q in range(1, 17):
        lo = -(1 << (q - 1)) if sgnd else 0
        vals = np.arange(lo, lo + (1 << q), dtype=np.int64).reshape(1, -1)
        src_dt = np.int32 if q % 2 else narrowest(q, sgnd)
        for p in range(1, 17):
            for mode in ("clip", "scale"):
                stage(grk, torch, [vals.astype(src_dt)], (0, 0, vals.size, 1), [(1, 1)], q, narrowest(p, sgnd), "chw",
                      sgnd=sgnd, out_prec=p, prec_mode=mode)
    # a wide source into the narrowest destination, interleaved
    vals = np.arange(1 << 12).reshape(64, 64)
    for src_dt in (np.uint16, np.int32):
        stage(grk, torch, [vals.astype(src_dt)] * 3, (0, 0, 64, 64), S444, 12, np.uint8, "hwc", out_prec=8,
              prec_mode="scale")


# ---------------------------------------------------------------------------
# the decode
# ---------------------------------------------------------------------------
def check_decode(codec, cs, ref, dtype, layouts=("chw", "hwc"), **kw):
    """codec.decompress(cs, **kw) == ref (the (c,h,w) reference) into pre-filled
    host arrays and cuda tensors, both layouts."""
    import torch
    ref = np.stack(ref)
    for layout in layouts:
        for dev in (False, True):
            shape = ref.shape if layout == "chw" else (ref.shape[1], ref.shape[2], ref.shape[0])
            out = np.full(shape, 0x5A, dtype=dtype)
            if dev:
                out = torch.from_numpy(out).cuda()
            got = codec.decompress(cs, out=out, layout=layout, **kw)
            assert got is out
            assert_is(got, ref, dtype, layout)


def sub_planes(tag, vt=None):
    """The reference's per-component planes of a subsampled fixture, its rect and subsampling."""
    subs = [tuple(s) for s in SUB[tag]["subsampling"]]
    ref, kw = expected(tag, vt)  # (the upsampled planes)
    return ref, subs, kw


@pytest.mark.parametrize("tag", ["sub_420_rgb8", "sub_422_I_tiles"])
def test_sycc_on_the_subsampled_reference_fixtures(codec, tag):
    bits = SUB[tag]["bits"]
    ref, subs, _ = sub_planes(tag)
    rgb = sycc_to_rgb(ref, bits)
    assert not np.array_equal(rgb, ref)
    for dt in formats(bits):
        check_decode(codec, gold(tag), rgb, dt, colour="sycc")
    # upsample=True alongside changes nothing; host-allocated outputs
    got = codec.decompress(gold(tag), dtype=formats(bits)[0], layout="hwc", colour="sycc", upsample=True)
    assert_is(got, rgb, formats(bits)[0], "hwc")


@pytest.mark.parametrize("tag,vt", [("sub_420_rgb8", "d10_7_71_60"), ("sub_422_I_tiles", "d40_30_120_95")])
def test_sycc_on_their_windows(codec, tag, vt):
    bits = SUB[tag]["bits"]
    ref, subs, kw = sub_planes(tag, vt)
    check_decode(codec, gold(tag), sycc_to_rgb(ref, bits), formats(bits)[0], colour="sycc", **kw)


@pytest.mark.parametrize("name,bits", [("rgb8_nomct", 8), ("rgb12_tiles_I", 12), ("rgb16_64", 16)])
def test_sycc_on_444_streams(codec, name, bits):
    """The inverse-MCT kernels' stores: without an MCT (rgb8_nomct), after the
    9/7 ICT in tiles, after the RCT at 16 bits."""
    ref = np.load(f"{GOLD}/{name}.dec.npy")
    rgb = sycc_to_rgb(ref, bits)
    for dt in formats(bits):
        check_decode(codec, gold(name), rgb, dt, colour="sycc")
    if name == "rgb12_tiles_I":  # both ops are per sample: a reduced decode takes them
        half = codec.decompress(gold(name), reduce=1)
        check_decode(codec, gold(name), sycc_to_rgb(half, bits), np.uint16, colour="sycc", reduce=1)
        check_decode(codec, gold(name), to_prec(sycc_to_rgb(half, bits), 12, False, 8, "scale"), np.uint8,
                     colour="sycc", reduce=1, out_prec=8, prec_mode="scale")


def _p_names():
    from prec_fixtures import PREC
    names = [f"p_g{n}{s}{i}" for n in range(1, 17) for s in "us" for i in ("", "_I")]
    assert len(names) == 64 and all(n in PREC for n in names)
    return names


@pytest.mark.parametrize("name", _p_names())
def test_every_precision_fixture_to_8_bits(codec, name):
    from prec_fixtures import PREC, precs, ref_decode, sgnds, stream
    m = PREC[name]
    q, sg = precs(m)[0], sgnds(m)[0]
    ref = ref_decode(name)
    for mode in ("clip", "scale"):
        check_decode(codec, stream(name), to_prec(ref, q, sg, 8, mode), narrowest(8, sg), out_prec=8, prec_mode=mode)


def test_precision_of_the_plain_fixtures(codec):
    load = lambda n: np.load(f"{GOLD}/{n}.dec.npy")  # noqa: E731
    check_decode(codec, gold("rgb12_cinema2k"), to_prec(load("rgb12_cinema2k"), 12, False, 8, "scale"), np.uint8,
                 layouts=("hwc",), out_prec=8, prec_mode="scale")
    for mode in ("scale", "clip"):
        check_decode(codec, gold("g16_128"), to_prec(load("g16_128"), 16, False, 8, mode), np.uint8, out_prec=8,
                     prec_mode=mode)
    check_decode(codec, gold("rgb8_128x96"), to_prec(load("rgb8_128x96"), 8, False, 12, "scale"), np.uint16,
                 out_prec=12, prec_mode="scale")
    # uint8 still does not hold a 12-bit stream as it is
    import grokimagecompression_amd as grk
    with pytest.raises(grk.GrkGpuError, match="grkgpu error -1:.*does not hold"):
        codec.decompress(gold("rgb12_96x80"), dtype=np.uint8)
    with pytest.raises(grk.GrkGpuError, match="do not hold the output precision"):
        codec.decompress(gold("rgb12_96x80"), dtype=np.uint8, out_prec=9)


@pytest.mark.parametrize("tag,kw", [("sub_mixed_pcrl", {}), ("sub_gray_3x2_rpcl", {}),
                                    ("sub_cprl_tiles_layers", {"vt": "l1"})])
def test_precision_on_the_general_upsampling_path(codec, tag, kw):
    bits = SUB[tag]["bits"]
    ref, subs, dkw = sub_planes(tag, kw.get("vt"))
    for mode in ("clip", "scale"):
        check_decode(codec, gold(tag), to_prec(ref, bits, False, 4, mode), np.uint8, upsample=True, out_prec=4,
                     prec_mode=mode, **dkw)
    # precision alone, without the upsample flag: each plane on its own grid, converted
    z = np.load(f"{GOLD}/{tag}{'.' + kw['vt'] if kw.get('vt') else ''}.dec.npz")
    got = codec.decompress(gold(tag), dtype=np.uint8, out_prec=4, prec_mode="scale", **dkw)
    assert isinstance(got, list) and len(got) == len(subs)
    for k, g in enumerate(got):
        assert g.dtype == np.uint8 and np.array_equal(g, z["c%d" % k] >> (bits - 4))


@functools.lru_cache(maxsize=None)
def _seam_stream(bits):
    """test_seams_at_odd_tile_origins' streams: 101 x 67 at (3,5) in tiles of
    37 x 29 -- 8-bit 4:2:0 5/3, and 12-bit 4:2:2 9/7 -- and this codec's planar
    decode of them.  Tile origins that are no multiple of dx / dy: the chroma
    goes through the staging planes."""
    import grokimagecompression_amd as grk
    import synth
    cd = lambda v, s: -(-v // s)  # noqa: E731
    subs = S420 if bits == 8 else S422
    rect = (3, 5, 104, 72)
    planes = [synth.synth_image(cd(rect[3], dy) - cd(rect[1], dy), cd(rect[2], dx) - cd(rect[0], dx), 1, bits,
                                930 + bits + k)[0] for k, (dx, dy) in enumerate(subs)]
    p, off = grk.CParams.from_cli(["-t", "37,29", "-d", "3,5"] + (["-I"] if bits == 12 else []))
    codec = grk.Codec(0)
    try:
        cs = codec.compress_subsampled(planes, bits, (101, 67), subs, p, offset=off)
        dec = codec.decompress(cs)
    finally:
        codec.close()
    for d in dec:
        d.setflags(write=False)
    return cs, tuple(dec), rect, subs


def test_both_ops_on_the_staged_path(codec):
    cs, dec, rect, subs = _seam_stream(8)
    check_decode(codec, cs, convert(dec, rect, subs, 8, colour="sycc"), np.uint8, colour="sycc")
    # 12 bits staged, 8 stored: the staging planes keep the stream's precision
    cs, dec, rect, subs = _seam_stream(12)
    ref = convert(dec, rect, subs, 12, colour="sycc", out_prec=8, prec_mode="scale")
    assert not np.array_equal(ref, convert([d >> 4 for d in dec], rect, subs, 8, colour="sycc"))
    check_decode(codec, cs, ref, np.uint8, layouts=("hwc",), colour="sycc", out_prec=8, prec_mode="scale")
    check_decode(codec, cs, convert(dec, rect, subs, 12, out_prec=8, prec_mode="clip"), np.uint8, layouts=("chw",),
                 upsample=True, out_prec=8, prec_mode="clip")


def test_sycc_converts_the_zero_margin_of_a_reduced_decode(codec):
    """101 x 67 at (3, 5), reduce = 1: the planes are 51 x 34, one column and
    one row more than the decoded samples, zero in the plain decode -- and the
    conversion of zero samples, as the reference's colour step leaves them,
    with sYCC: (0, 135, 0) at 8 bits."""
    import grokimagecompression_amd as grk
    import synth
    p, off = grk.CParams.from_cli(["-t", "37,29", "-d", "3,5", "-Y", "0"])
    cs = codec.compress(synth.synth_image(67, 101, 3, 8, 77), 8, p, offset=off)
    half = codec.decompress(cs, reduce=1)  # the planar decode test_gpu_parity.py pins, zero margin included
    assert half.shape == (3, 34, 51) and not half[:, -1, :].any() and not half[:, :, -1].any()
    assert half[:, :-1, :-1].any()
    rgb = sycc_to_rgb(half, 8)
    assert rgb[:, -1, 0].tolist() == [0, 135, 0] and rgb[:, 0, -1].tolist() == [0, 135, 0]
    check_decode(codec, cs, rgb, np.uint8, colour="sycc", reduce=1)
    check_decode(codec, cs, rgb, np.int32, colour="sycc", reduce=1)
    check_decode(codec, cs, to_prec(rgb, 8, False, 12, "scale"), np.uint16, colour="sycc", reduce=1, out_prec=12,
                 prec_mode="scale")
    # precision alone: zero stays zero
    check_decode(codec, cs, to_prec(half, 8, False, 4, "scale"), np.uint8, reduce=1, out_prec=4, prec_mode="scale")
    assert np.array_equal(codec.decompress(cs, reduce=1), half)  # a clean decode on the same context


def test_sycc_converts_tiles_never_reached(codec):
    """rgb12_tiles_I (tiles of 64 x 64) cut after its fifth tile: the tiles the
    stream never reached are zero in the plain decode and sYCC(0, 0, 0) here."""
    import grokimagecompression_amd as grk
    cs = gold("rgb12_tiles_I")[:48890]
    assert grk.walk_tiles(cs) == [0, 1, 2, 3, 4]
    dec = codec.decompress(cs)  # today's planes: zero where no tile was decoded
    assert not dec[:, 64:128, 64:].any() and not dec[:, 128:, :].any() and dec[:, :64].any()
    rgb = sycc_to_rgb(dec, 12)
    assert rgb[:, 149, 199].tolist() == sycc_to_rgb(np.zeros((3, 1, 1), np.int64), 12)[:, 0, 0].tolist() != [0, 0, 0]
    for dt in (np.uint16, np.int32):
        check_decode(codec, cs, rgb, dt, colour="sycc")
    check_decode(codec, cs, to_prec(rgb, 12, False, 8, "scale"), np.uint8, colour="sycc", out_prec=8,
                 prec_mode="scale")
    check_decode(codec, cs, to_prec(dec, 12, False, 8, "clip"), np.uint8, out_prec=8, prec_mode="clip")
    assert np.array_equal(codec.decompress(cs), dec)  # a clean decode on the same context


def _raw_decode(grk, codec, entry, cs, out, fmt, layout, ops=None, dp=None, tiles=(0, 0xFFFFFFFF), desc=None):
    """grkgpu_decompress_to / _convert into the host array `out`; returns the return code."""
    op = grk.OutPlanes(sample_fmt=fmt, layout=layout, on_device=0)
    if layout & 1:
        op.planes[0] = out.ctypes.data
    else:
        for k in range(out.shape[0]):
            op.planes[k] = out[k].ctypes.data
    args = [codec._ctx, cs, len(cs), ctypes.byref(dp) if dp is not None else None, tiles[0], tiles[1],
            ctypes.byref(desc) if desc is not None else None, ctypes.byref(op)]
    if entry == "convert":
        return grk.lib().grkgpu_decompress_convert(*args, ctypes.byref(ops) if ops is not None else None)
    return grk.lib().grkgpu_decompress_to(*args)


@pytest.mark.parametrize("name,shape,fmt,layout", [("rgb12_tiles_I", (150 + 2, 200, 3), "U16", 1),
                                                   ("sub_420_rgb8", (3 + 1, 75, 97), "U8", 0x100)])
def test_no_ops_is_decompress_to_byte_for_byte(codec, name, shape, fmt, layout):
    """ops = NULL and zeroed ops against grkgpu_decompress_to, the bytes of a
    pre-filled output past the image included."""
    import grokimagecompression_amd as grk
    dt = np.uint16 if fmt == "U16" else np.uint8
    outs = []
    for entry, ops in (("to", None), ("convert", None), ("convert", grk.OutOps())):
        out = np.full(shape, 0x5A, dtype=dt)
        assert _raw_decode(grk, codec, entry, gold(name), out, getattr(grk, "SAMPLE_" + fmt), layout, ops) == 0
        outs.append(out)
    assert (outs[0].reshape(-1)[-shape[1] * shape[2]:] == 0x5A).all() and (outs[0] != 0x5A).any()
    assert outs[0].tobytes() == outs[1].tobytes() == outs[2].tobytes()


def test_image_descriptor_of_a_converted_decode(codec):
    """img receives the output precision, and dx = dy = 1 with sYCC."""
    import grokimagecompression_amd as grk
    ref, subs, _ = sub_planes("sub_422_I_tiles")
    out = np.empty(ref.shape, np.uint8)
    d = grk.ImageDesc()
    ops = grk.OutOps(colour=grk.COLOUR_SYCC, prec=8, prec_mode=grk.PREC_SCALE)
    assert _raw_decode(grk, codec, "convert", gold("sub_422_I_tiles"), out, grk.SAMPLE_U8, 0, ops, desc=d) == 0
    assert list(d.prec[:3]) == [8, 8, 8] and list(d.dx[:3]) == [1, 1, 1] and list(d.dy[:3]) == [1, 1, 1]
    assert_is(out, to_prec(sycc_to_rgb(ref, 12), 12, False, 8, "scale"), np.uint8, "chw")


def test_refusals_leave_the_context_usable(codec):
    import grokimagecompression_amd as grk
    good = gold("sub_420_rgb8")
    good_ref = sycc_to_rgb(expected("sub_420_rgb8")[0], 8)

    def still_good():
        assert_is(codec.decompress(good, dtype=np.uint8, layout="hwc", colour="sycc"), good_ref, np.uint8, "hwc")

    # one component, four components, (through the stage call) signed components
    for name, comps in (("g8_64", 1), ("p_x_c4_8u", 4)):
        assert grk.read_header(gold(name)).numcomps == comps
        with pytest.raises(grk.GrkGpuError, match="grkgpu error -1:.*3 components"):
            codec.decompress(gold(name), colour="sycc")
        still_good()
    with pytest.raises(grk.GrkGpuError, match="grkgpu error -1:.*upsampled output of a reduced decode"):
        codec.decompress(good, colour="sycc", reduce=1)
    still_good()
    cs = gold("sub_422_I_tiles")
    x0, y0, x1, y1 = image_rect("sub_422_I_tiles")
    out = np.empty((3, y1 - y0, x1 - x0), np.uint16)
    rc = _raw_decode(grk, codec, "convert", cs, out, grk.SAMPLE_U16, 0, grk.OutOps(colour=grk.COLOUR_SYCC),
                     tiles=(0, 1))
    assert rc == -4 and b"tile-range decode of subsampled images" in grk.lib().grkgpu_last_error()
    still_good()
    # the format has to hold the output precision, whatever the stream's
    out8 = np.empty((3, y1 - y0, x1 - x0), np.uint8)
    assert _raw_decode(grk, codec, "convert", cs, out8, grk.SAMPLE_U8, 0x100, grk.OutOps(colour=grk.COLOUR_SYCC)) == -1
    still_good()


def test_refusal_of_signed_sycc_through_the_stage_call():
    grk, torch = _grk_torch()
    src = [torch.zeros((4, 4), dtype=torch.int8, device="cuda") for _ in range(3)]
    dst = torch.zeros(48, dtype=torch.int8, device="cuda")
    with pytest.raises(grk.GrkGpuError, match="grkgpu error -1:.*unsigned"):
        grk.convert_to(src, dst, (0, 0, 4, 4), S444, 8, sgnd=True, colour="sycc")


def test_dirty_context(codec):
    """sYCC + scale of the 12-bit seam stream after every buffer of the context
    was filled with 0xFF, and after a call of a different kind (an encode)."""
    import synth
    cs, dec, rect, subs = _seam_stream(12)
    ref = np.stack(convert(dec, rect, subs, 12, colour="sycc", out_prec=8, prec_mode="scale"))
    kw = dict(dtype=np.uint8, layout="hwc", colour="sycc", out_prec=8, prec_mode="scale")
    assert_is(codec.decompress(cs, **kw), ref, np.uint8, "hwc")
    codec.debug_fill(0xFF)
    assert_is(codec.decompress(cs, **kw), ref, np.uint8, "hwc")
    codec.compress(synth.synth_image(96, 128, 3, 8, 7), 8)
    assert_is(codec.decompress(cs, device_out=True, **kw), ref, np.uint8, "hwc")
