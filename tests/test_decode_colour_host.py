"""Host side of the eYCC / CMYK / force-RGB decode stores (no GPU): the numpy
closed forms against what the reference's own color.cpp made of the pinned
inputs (tests/golden/manifest_colour.json), the exports and struct layouts,
every refusal -- returned before any device call, with a context that is never
dereferenced -- and the Python argument / shape / dtype checks."""
import ctypes
import os
import struct

import numpy as np
import pytest

import colour_fixtures as cf
from conftest import GOLD

EINVAL, EUNSUPPORTED = -1, -4


def _grk():
    import grokimagecompression_amd as grk
    if not os.path.exists(grk.LIB_PATH):
        grk.build()
    return grk


# ---------------------------------------------------------------------------
# the closed forms are the reference's loops
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cf.cases()))
def test_closed_form_equals_the_reference(name):
    kind, precs, sgnds, planes = cf.cases()[name]
    rec = cf.manifest()[name]
    assert (rec["kind"], rec["prec"], rec["sgnd"], rec["n"]) == (kind, precs, sgnds, planes[0].size)
    assert cf.digest(planes) == rec["in_sha256"], "the seeded recipe changed"
    out, chans = cf.closed_form(kind, precs, sgnds, planes)
    assert len(out) == len(rec["ref_comps"])
    assert cf.digest(out) == rec["ref_sha256"]
    # what the reference reports of its output: ours, except that eYCC's R, G, B are unsigned here
    for (p, s), (rp, rs) in zip(chans, rec["ref_comps"]):
        assert p == rp and (s == rs or kind == "eycc")
    if kind == "cmyk":  # never outside U8: no clamp is needed
        assert min(rec["ref_min"][:3]) >= 0 and max(rec["ref_max"][:3]) <= 255


def test_cmyk_stays_in_range_for_every_precision():
    """C in [0, 1] and every result in [0, 255] for in-range inks, q = 1 .. 16
    (all inks at q <= 8, the extremes and a random draw above)."""
    rs = np.random.RandomState(5)
    for q in range(1, 17):
        top = (1 << q) - 1
        v = np.arange(top + 1) if q <= 8 else np.concatenate([[0, 1, top - 1, top], rs.randint(0, top + 1, 4000)])
        a, k = [m.ravel() for m in np.meshgrid(v[:256], v[-256:], indexing="ij")]
        r, g, b = cf.cmyk_to_rgb([a, a[::-1], k, k], [q] * 4)
        for p in (r, g, b):
            assert p.min() >= 0 and p.max() <= 255
    z = np.zeros(4, np.int32)
    assert [int(p[0]) for p in cf.cmyk_to_rgb([z] * 5, [8] * 4)] == [255, 255, 255, 0]
    assert [int(p[0]) for p in cf.eycc_to_rgb(z, z, z, 8)] == [0, 135, 0]


def test_force_rgb_closed_form():
    a, b = np.arange(4), np.arange(4) + 10
    assert [p is a for p in cf.force_rgb([a])] == [True] * 3
    assert [id(p) for p in cf.force_rgb([a, b])] == [id(a)] * 3 + [id(b)]
    assert len(cf.force_rgb([a, b, a])) == 3


# ---------------------------------------------------------------------------
# ABI
# ---------------------------------------------------------------------------
def test_exports_and_layouts_are_unchanged():
    grk = _grk()
    for f in ("grkgpu_decompress_convert", "grkgpu_decompress_mct", "grkgpu_jp2_decompress", "grkgpu_convert_to"):
        assert hasattr(grk.lib(), f)
    assert (grk.COLOUR_NONE, grk.COLOUR_SYCC, grk.COLOUR_AUTO, grk.COLOUR_EYCC, grk.COLOUR_CMYK,
            grk.COLOUR_AUTO_RGB, grk.COLOUR_FORCE_RGB) == (0, 1, 2, 3, 4, 5, 0x100)
    assert ctypes.sizeof(grk.OutOps) == 16
    assert [getattr(grk.OutOps, f).offset for f in ("colour", "prec", "prec_mode", "reserved")] == [0, 4, 8, 12]
    assert ctypes.sizeof(grk.OutPlanes) == 16 * ctypes.sizeof(ctypes.c_void_p) + 16
    hdr = open(os.path.join(os.path.dirname(GOLD), "..", "include", "grk_mi355x.h")).read()
    for text in ("GRKGPU_COLOUR_EYCC = 3", "GRKGPU_COLOUR_CMYK = 4", "GRKGPU_COLOUR_FORCE_RGB 0x100u",
                 "GRKGPU_COLOUR_AUTO 2u", "GRKGPU_COLOUR_AUTO_RGB 5u"):
        assert text in hdr


# ---------------------------------------------------------------------------
# refusals, before any device call
# ---------------------------------------------------------------------------
def _stream(oracle, c, prec=8, sgnd=False, h=9, w=11):
    """a small lossless stream of c components, encoded on the CPU"""
    precs = prec if isinstance(prec, list) else [prec] * c
    sg = sgnd if isinstance(sgnd, list) else [sgnd] * c
    rs = np.random.RandomState(c)
    img = np.stack([rs.randint(0, 1 << (p - 1), (h, w)) for p in precs]).astype(np.int32)
    return oracle.encode(img, precs, oracle.params(numres=2, mct=0), sgnd=sg)


def _convert_rc(grk, cs, colour, fmt=None, entry="grkgpu_decompress_convert", **kw):
    L = grk.lib()
    ctx = ctypes.c_void_p(1)  # never dereferenced
    op = grk.OutPlanes(sample_fmt=grk.SAMPLE_I32 if fmt is None else fmt, layout=grk.LAYOUT_PLANAR)
    for k in range(16):
        op.planes[k] = 64
    ops = grk.OutOps(colour=colour, **kw)
    rc = getattr(L, entry)(ctx, cs, len(cs), None, 0, 0xFFFFFFFF, None, ctypes.byref(op), ctypes.byref(ops))
    return rc, L.grkgpu_last_error()


def test_eycc_shapes_refused(oracle):
    grk = _grk()
    E = grk.COLOUR_EYCC
    for entry in ("grkgpu_decompress_convert", "grkgpu_decompress_mct"):
        for cs, what in ((_stream(oracle, 2), b"exactly 3"), (_stream(oracle, 4), b"exactly 3"),
                         (_stream(oracle, 3, sgnd=[True, False, False]), b"unsigned component 0"),
                         (_stream(oracle, 3, prec=[8, 8, 10]), b"one precision"),
                         (open(f"{GOLD}/sub_420_rgb8.j2k", "rb").read(), b"one grid")):
            rc, msg = _convert_rc(grk, cs, E, entry=entry)
            assert rc == EINVAL and what in msg, (entry, what, rc, msg)
    # signed chroma is taken; the output is unsigned, so a signed format does not hold it
    rc, msg = _convert_rc(grk, _stream(oracle, 3, sgnd=[False, True, True]), E, fmt=grk.SAMPLE_I8)
    assert rc == EINVAL and b"sample format does not hold" in msg


def test_cmyk_shapes_refused(oracle):
    grk = _grk()
    C = grk.COLOUR_CMYK
    for cs, what in ((_stream(oracle, 3), b"at least 4"), (_stream(oracle, 1), b"at least 4"),
                     (_stream(oracle, 4, sgnd=[False, False, True, False]), b"unsigned inks"),
                     (_stream(oracle, 5, sgnd=[False, False, False, True, False]), b"unsigned inks")):
        rc, msg = _convert_rc(grk, cs, C)
        assert rc == EINVAL and what in msg, (what, rc, msg)
    # R, G, B are 8 bits unsigned; the fifth component keeps its 12 signed bits: only int32 holds both
    cs5 = _stream(oracle, 5, prec=[8, 8, 8, 8, 12], sgnd=[False] * 4 + [True])
    for fmt in (grk.SAMPLE_U8, grk.SAMPLE_U16, grk.SAMPLE_I16):
        rc, msg = _convert_rc(grk, cs5, C, fmt=fmt)
        assert rc == EINVAL and b"sample format does not hold" in msg, fmt
    rc, msg = _convert_rc(grk, _stream(oracle, 4, prec=12), C, fmt=grk.SAMPLE_I8)
    assert rc == EINVAL and b"sample format does not hold" in msg


def test_force_rgb_refused(oracle):
    grk = _grk()
    F = grk.COLOUR_FORCE_RGB
    for c in (3, 4, 5):  # a raw codestream has no colour space
        rc, msg = _convert_rc(grk, _stream(oracle, c), F)
        assert rc == EINVAL and b"don't know how to convert" in msg, (c, rc, msg)
    # no conversion takes one or two components: its own refusal, whatever the flag
    for col in (grk.COLOUR_SYCC, grk.COLOUR_EYCC, grk.COLOUR_CMYK):
        rc, msg = _convert_rc(grk, _stream(oracle, 2), col | F)
        assert rc == EINVAL and b"conversion needs" in msg, (col, rc, msg)
    # three channels of one component do not fit a format its precision does not fit
    rc, msg = _convert_rc(grk, _stream(oracle, 1, prec=12), F, fmt=grk.SAMPLE_U8)
    assert rc == EINVAL and b"sample format does not hold" in msg


def test_unknown_colour_values_still_refused(oracle):
    grk = _grk()
    cs = _stream(oracle, 3)
    for colour in (2, 5, 6, 0x200, 0x101 | 0x200, 2 | grk.COLOUR_FORCE_RGB, 5 | grk.COLOUR_FORCE_RGB):
        for entry in ("grkgpu_decompress_convert", "grkgpu_decompress_mct"):
            rc, msg = _convert_rc(grk, cs, colour, entry=entry)
            assert rc == EINVAL and b"unknown colour" in msg, (colour, entry)
    for colour in (grk.COLOUR_EYCC, grk.COLOUR_CMYK, grk.COLOUR_FORCE_RGB):
        rc, msg = _convert_rc(grk, cs, colour, reserved=1)
        assert rc == EINVAL and b"reserved" in msg


def test_convert_to_refusals():
    grk = _grk()
    L = grk.lib()
    U32, I32 = ctypes.c_uint32, ctypes.c_int32

    def call(n, colour, dx=None, prec=None, sgnd=None, fmt=grk.SAMPLE_I32, src_fmt=grk.SAMPLE_I32, dstride=64,
             layout=grk.LAYOUT_INTERLEAVED, sstride=None):
        op = grk.OutPlanes(sample_fmt=fmt, layout=layout)
        for k in range(16):
            op.planes[k] = 64
        dx = dx or [1] * n
        o = grk.OutOps(colour=colour)
        rc = L.grkgpu_convert_to((ctypes.c_void_p * n)(*[64] * n), (U32 * n)(*(sstride or [8] * n)), src_fmt, n,
                                 (U32 * n)(*dx), (U32 * n)(*dx), (U32 * n)(*(prec or [8] * n)),
                                 (I32 * n)(*(sgnd or [0] * n)), 0, 0, 8, 4, ctypes.byref(op), dstride, ctypes.byref(o),
                                 None)
        return rc, L.grkgpu_last_error()

    E, C, F = grk.COLOUR_EYCC, grk.COLOUR_CMYK, grk.COLOUR_FORCE_RGB
    for args, what in ((dict(n=2, colour=E), b"exactly 3"), (dict(n=3, colour=E, dx=[1, 2, 2]), b"one grid"),
                       (dict(n=3, colour=E, prec=[17] * 3), b"one precision"),
                       (dict(n=3, colour=E, sgnd=[1, 0, 0]), b"unsigned component 0"),
                       (dict(n=3, colour=C), b"at least 4"), (dict(n=5, colour=C, dx=[1, 1, 1, 1, 2]), b"one grid"),
                       (dict(n=4, colour=C, prec=[8, 8, 17, 8]), b"precision 1 .. 16"),
                       (dict(n=4, colour=C, sgnd=[0, 1, 0, 0]), b"unsigned inks"),
                       (dict(n=4, colour=C, dstride=8 * 3 - 1), b"strides must hold a row"),
                       (dict(n=4, colour=C, prec=[12] * 4, fmt=grk.SAMPLE_I16), b"does not hold the output"),
                       (dict(n=3, colour=F), b"don't know how to convert"),
                       (dict(n=1, colour=F, dstride=8 * 3 - 1), b"strides must hold a row"),
                       (dict(n=2, colour=F | E), b"exactly 3"), (dict(n=3, colour=2), b"unknown colour"),
                       (dict(n=3, colour=5), b"unknown colour")):
        rc, msg = call(**args)
        assert rc == EINVAL and what in msg, (args, rc, msg)
    for args in (dict(n=1, colour=F, dx=[2]), dict(n=2, colour=F, src_fmt=grk.SAMPLE_U8, fmt=grk.SAMPLE_U8),
                 dict(n=2, colour=F, sstride=[8, 9])):
        rc, msg = call(**args)
        assert rc == EUNSUPPORTED and b"force-RGB needs int32 sources" in msg, (args, rc, msg)


def _box(typ, payload=b""):
    return struct.pack(">I", 8 + len(payload)) + typ + payload


def jp2_file(cs, h, w, nc, enumcs=None, icc=None, extra=(), bpc=7):
    colr = _box(b"colr", bytes([2, 0, 0]) + icc) if icc else _box(b"colr", bytes([1, 0, 0]) + struct.pack(">I", enumcs))
    head = [_box(b"ihdr", struct.pack(">IIHBBBB", h, w, nc, bpc, 7, 0, 0)), colr] + list(extra)
    return (_box(b"jP  ", b"\x0d\x0a\x87\x0a") + _box(b"ftyp", b"jp2 " + b"\0\0\0\0" + b"jp2 ") +
            _box(b"jp2h", b"".join(head)) + _box(b"jp2c", cs))


def cdef(triples):
    return _box(b"cdef", struct.pack(">H", len(triples)) + b"".join(struct.pack(">HHH", *t) for t in triples))


def test_jp2_refusals(oracle):
    grk = _grk()
    L = grk.lib()
    ctx = ctypes.c_void_p(1)
    op = grk.OutPlanes(sample_fmt=grk.SAMPLE_I32)
    for k in range(16):
        op.planes[k] = 64

    def rc_of(data, colour):
        o = grk.OutOps(colour=colour)
        rc = L.grkgpu_jp2_decompress(ctx, data, len(data), None, 0, 0xFFFFFFFF, None, ctypes.byref(op), ctypes.byref(o),
                                     None)
        return rc, L.grkgpu_last_error()

    A, F = grk.COLOUR_AUTO_RGB, grk.COLOUR_FORCE_RGB
    bgr = cdef([(0, 0, 3), (1, 0, 2), (2, 0, 1)])
    swap4 = cdef([(0, 0, 2), (1, 0, 1), (2, 0, 3), (3, 0, 4)])
    cs3, cs4 = _stream(oracle, 3), _stream(oracle, 4)
    # eYCC / CMYK behind a channel swap
    for data in (jp2_file(cs3, 9, 11, 3, 24, extra=[bgr]), jp2_file(cs4, 9, 11, 4, 12, extra=[swap4])):
        for colour in (A, A | F):
            rc, msg = rc_of(data, colour)
            assert rc == EUNSUPPORTED and b"behind a JP2 palette or channel swap" in msg, (rc, msg)
    # the file says eYCC / CMYK of a shape the conversion does not take
    rc, msg = rc_of(jp2_file(cs4, 9, 11, 4, 24), A)
    assert rc == EINVAL and b"exactly 3" in msg
    rc, msg = rc_of(jp2_file(cs3, 9, 11, 3, 12), A)
    assert rc == EINVAL and b"at least 4" in msg
    # force-RGB: an ICC profile is the colour management library's; unknown spaces of 3+ channels are refused
    rc, msg = rc_of(jp2_file(cs3, 9, 11, 3, icc=bytes(range(64))), F)
    assert rc == EUNSUPPORTED and b"ICC" in msg
    rc, msg = rc_of(jp2_file(_stream(oracle, 1), 9, 11, 1, icc=bytes(range(64))), grk.COLOUR_AUTO | F)
    assert rc == EUNSUPPORTED and b"ICC" in msg
    for enumcs, colour in ((24, grk.COLOUR_AUTO | F), (12, F), (17, A | F)):
        rc, msg = rc_of(jp2_file(cs4 if enumcs == 12 else cs3, 9, 11, 4 if enumcs == 12 else 3, enumcs), colour)
        assert rc == EINVAL and b"don't know how to convert" in msg, (enumcs, rc, msg)
    # AUTO_RGB belongs to the JP2 entry point; unknown values stay refused here too
    rc, msg = rc_of(jp2_file(cs3, 9, 11, 3, 16), 6)
    assert rc == EINVAL and b"unknown colour" in msg


# ---------------------------------------------------------------------------
# Python
# ---------------------------------------------------------------------------
def test_python_arguments_shapes_and_dtypes(oracle):
    grk = _grk()
    codec = object.__new__(grk.Codec)
    codec.device = 0
    codec._ctx = None  # the library's first complaint once Python lets a call through
    through = "grkgpu error -1: null argument"
    cs4 = _stream(oracle, 4, prec=12)
    cs5 = _stream(oracle, 5, prec=[8, 8, 8, 8, 12], sgnd=[False] * 4 + [True])
    cs3s = _stream(oracle, 3, prec=12, sgnd=[False, True, True])
    cs1, cs2 = _stream(oracle, 1, prec=12), _stream(oracle, 2)
    for cs, kw in ((cs4, dict(colour="cmyk", dtype=np.uint8)),
                   (cs4, dict(colour="cmyk", out=np.empty((9, 11, 3), np.uint8), layout="hwc")),
                   (cs4, dict(colour="cmyk", out=np.empty((3, 9, 11), np.uint16))),
                   (cs5, dict(colour="cmyk", out=np.empty((4, 9, 11), np.int32))),
                   (cs3s, dict(colour="eycc", dtype=np.uint16)),
                   (cs3s, dict(colour="eycc", out_prec=8, dtype=np.uint8)),
                   (cs1, dict(force_rgb=True, out=np.empty((3, 9, 11), np.uint16))),
                   (cs1, dict(force_rgb=True, out_prec=8, prec_mode="scale", out=np.empty((9, 11, 3), np.uint8),
                              layout="hwc")),
                   (cs2, dict(force_rgb=True, out=np.empty((4, 9, 11), np.uint8))),
                   (cs4, dict(colour="cmyk", force_rgb=True, out=np.empty((3, 9, 11), np.uint8)))):
        with pytest.raises(grk.GrkGpuError, match=through):
            codec.decompress(cs, **kw)
    for cs, kw, what in ((cs4, dict(colour="cmyk", out=np.empty((4, 9, 11), np.uint8)), "out must be"),
                         (cs5, dict(colour="cmyk", dtype=np.uint8), "do not hold the output precision"),
                         (cs3s, dict(colour="eycc", dtype=np.int16), "do not hold the output precision"),
                         (cs3s, dict(colour="eycc", dtype=np.uint8), "do not hold the output precision"),
                         (cs1, dict(force_rgb=True, out=np.empty((1, 9, 11), np.uint16)), "out must be"),
                         (cs1, dict(force_rgb=True, dtype=np.uint8), "do not hold the output precision"),
                         (cs2, dict(force_rgb=True, out=np.empty((3, 9, 11), np.uint8)), "out must be"),
                         (cs4, dict(colour="ycck"), "colour must be"), (cs4, dict(colour="auto_rgb"), "colour must be")):
        with pytest.raises(grk.GrkGpuError, match=what):
            codec.decompress(cs, **kw)
    # without the new arguments nothing changes: four components come back as four
    with pytest.raises(grk.GrkGpuError, match=through):
        codec.decompress(cs4, out=np.empty((4, 9, 11), np.uint16), dtype=np.uint16)
    # the JP2 entry point: auto_rgb follows the file, auto does not
    f12, f24, f17 = jp2_file(cs4, 9, 11, 4, 12, bpc=11), jp2_file(cs3s, 9, 11, 3, 24, bpc=11), jp2_file(cs1, 9, 11, 1, 17, bpc=11)
    for data, kw in ((f12, dict(colour="auto_rgb", dtype=np.uint8)), (f12, dict(colour="auto", dtype=np.uint16)),
                     (f24, dict(colour="auto_rgb", dtype=np.uint16)), (f17, dict(force_rgb=True, dtype=np.uint16))):
        with pytest.raises(grk.GrkGpuError, match=through):
            codec.decompress_jp2(data, **kw)
    for data, kw, what in ((f12, dict(colour="auto", dtype=np.uint8), "do not hold the output precision"),
                           (f24, dict(colour="auto", dtype=np.uint16), "do not hold the output precision"),
                           (f12, dict(colour="cmyk"), "colour must be")):
        with pytest.raises(grk.GrkGpuError, match=what):
            codec.decompress_jp2(data, **kw)
