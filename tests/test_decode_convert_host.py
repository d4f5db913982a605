"""Host side of the converting decode output (no GPU): the exports, the struct
layouts, the argument checks that come before any device call, the Python
validation of dtype / out= against the output precision, and the numpy closed
forms the GPU tests compare against, checked on values worked by hand from the
reference's loops (color.cpp:136-382, convert.cpp:82-161)."""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLD
from test_gpu_decode_convert import S420, S422, convert, sycc_to_rgb, to_prec


def _grk():
    import grokimagecompression_amd as grk
    if not os.path.exists(grk.LIB_PATH):
        grk.build()
    return grk


def test_library_exports_the_converting_entry_points():
    grk = _grk()
    assert hasattr(grk.lib(), "grkgpu_decompress_convert") and hasattr(grk.lib(), "grkgpu_convert_to")
    assert callable(grk.convert_to)
    assert (grk.COLOUR_NONE, grk.COLOUR_SYCC, grk.PREC_CLIP, grk.PREC_SCALE) == (0, 1, 0, 1)


def test_struct_layouts():
    grk = _grk()
    assert ctypes.sizeof(grk.OutOps) == 16
    assert [getattr(grk.OutOps, f).offset for f in ("colour", "prec", "prec_mode", "reserved")] == [0, 4, 8, 12]
    vp = ctypes.sizeof(ctypes.c_void_p)
    assert ctypes.sizeof(grk.OutPlanes) == 16 * vp + 16  # unchanged


BAD_OPS = [dict(colour=2), dict(prec=8, prec_mode=2), dict(prec=17), dict(reserved=1), dict(colour=1, reserved=7)]


def test_decompress_convert_refuses_bad_ops_without_a_device():
    grk = _grk()
    L = grk.lib()
    cs = b"\xff\x4f\xff\x51"
    ctx = ctypes.c_void_p(1)  # never dereferenced: the output description and the ops are checked first
    op = grk.OutPlanes(sample_fmt=grk.SAMPLE_U16, layout=grk.LAYOUT_PLANAR)
    for kw in BAD_OPS:
        ops = grk.OutOps(**kw)
        assert L.grkgpu_decompress_convert(ctx, cs, len(cs), None, 0, 0xFFFFFFFF, None, ctypes.byref(op),
                                           ctypes.byref(ops)) == -1, kw
    # a format that does not hold the output precision
    for fmt, prec in ((grk.SAMPLE_U8, 9), (grk.SAMPLE_I8, 16)):
        op8 = grk.OutPlanes(sample_fmt=fmt, layout=grk.LAYOUT_PLANAR)
        ops = grk.OutOps(prec=prec)
        assert L.grkgpu_decompress_convert(ctx, cs, len(cs), None, 0, 0xFFFFFFFF, None, ctypes.byref(op8),
                                           ctypes.byref(ops)) == -1
        assert b"output precision" in L.grkgpu_last_error()
    # the layout word keeps its refusals on the new entry point
    for layout in (0x200, 0x300):
        bad = grk.OutPlanes(sample_fmt=grk.SAMPLE_U8, layout=layout)
        assert L.grkgpu_decompress_convert(ctx, cs, len(cs), None, 0, 0xFFFFFFFF, None, ctypes.byref(bad), None) == -1
        assert b"layout" in L.grkgpu_last_error()


def test_convert_to_refuses_bad_arguments_without_a_device():
    grk = _grk()
    L = grk.lib()
    U32, I32 = ctypes.c_uint32, ctypes.c_int32
    SY = dict(colour=grk.COLOUR_SYCC)

    def call(n=3, layout=grk.LAYOUT_INTERLEAVED, fmt=grk.SAMPLE_U8, src_fmt=grk.SAMPLE_U8, src=(64, 64, 64, 64),
             sstride=(8, 4, 4, 4), dx=(1, 2, 2, 2), dy=(1, 2, 2, 2), prec=(8, 8, 8, 8), sgnd=(0, 0, 0, 0),
             rect=(0, 0, 8, 4), dst=64, dstride=32, out=True, ops=None):
        op = grk.OutPlanes(sample_fmt=fmt, layout=layout)
        for k in range(4):
            op.planes[k] = dst
        o = grk.OutOps(**ops) if ops is not None else None
        return L.grkgpu_convert_to((ctypes.c_void_p * n)(*src[:n]), (U32 * n)(*sstride[:n]), src_fmt, n,
                                   (U32 * n)(*dx[:n]), (U32 * n)(*dy[:n]), (U32 * n)(*prec[:n]),
                                   (I32 * n)(*sgnd[:n]), *rect, ctypes.byref(op) if out else None, dstride,
                                   ctypes.byref(o) if o is not None else None, None)

    # (pointers are never dereferenced: every refusal comes before the first device call)
    bad = [dict(ops=kw) for kw in BAD_OPS]
    bad += [dict(ops=dict(prec=9)),                                          # U8 does not hold 9 bits
            dict(n=2, ops=SY), dict(n=4, ops=SY),                            # sYCC: exactly 3 components
            dict(sgnd=(0, 1, 0, 0), ops=SY),                                 # (I8 / U8 cannot hold both either)
            dict(src_fmt=grk.SAMPLE_I8, fmt=grk.SAMPLE_I8, sgnd=(1, 1, 1, 1), ops=SY),
            dict(src_fmt=grk.SAMPLE_U16, fmt=grk.SAMPLE_U16, prec=(8, 8, 10, 8), ops=SY),
            dict(dx=(1, 3, 3, 1), sstride=(8, 3, 3, 3), ops=SY),             # chroma at (3,2)
            dict(dy=(1, 1, 2, 1), ops=SY),                                   # chroma (2,1) + (2,2)
            dict(dx=(2, 2, 2, 2), dy=(2, 2, 2, 2), ops=SY),                  # luma subsampled
            dict(prec=(12, 12, 12, 12), fmt=grk.SAMPLE_U16),                 # src_fmt U8 for a 12-bit source
            dict(prec=(12, 12, 12, 12), src_fmt=grk.SAMPLE_U16),             # ... and U8 for a 12-bit output
            dict(src_fmt=5), dict(prec=(8, 0, 8, 8)),
            # grkgpu_upsample_to's geometry refusals
            dict(layout=0x200), dict(layout=0x102), dict(layout=2), dict(fmt=5), dict(out=False),
            dict(dx=(1, 0, 2, 2)), dict(dy=(1, 2, 0, 2)), dict(dx=(1, 256, 2, 2)),
            dict(src=(64, None, 64, 64)), dict(dst=None), dict(dstride=23),
            dict(layout=grk.LAYOUT_PLANAR, dstride=7), dict(sstride=(8, 3, 4, 4)), dict(sstride=(7, 4, 4, 4)),
            dict(rect=(4, 0, 4, 4)),
            dict(src_fmt=grk.SAMPLE_U16, src=(64, 65, 64, 64)), dict(fmt=grk.SAMPLE_U16, dst=65)]
    for kw in bad:
        assert call(**kw) == -1, kw  # GRKGPU_EINVAL


def test_python_validation_against_the_output_precision():
    """dtype / out= are checked against the output precision before anything
    crosses the C ABI; without the new arguments nothing changes."""
    grk = _grk()
    codec = object.__new__(grk.Codec)
    codec.device = 0
    cs12 = open(f"{GOLD}/rgb12_96x80.j2k", "rb").read()
    # without out_prec: today's refusal, by the library, with its message (the
    # context is never dereferenced: the format is checked from the header)
    codec._ctx = ctypes.c_void_p(1)
    with pytest.raises(grk.GrkGpuError, match="grkgpu error -1: sample format does not hold the component's precision"):
        codec.decompress(cs12, dtype=np.uint8)
    # with out_prec=8: accepted as far as the ABI -- the library's first complaint is the missing context
    codec._ctx = None
    for kw in (dict(dtype=np.uint8), dict(out=np.empty((80, 96, 3), np.uint8), layout="hwc")):
        with pytest.raises(grk.GrkGpuError, match="grkgpu error -1: null argument"):
            codec.decompress(cs12, out_prec=8, prec_mode="scale", **kw)
    for kw in (dict(dtype=np.uint8, out_prec=9), dict(dtype=np.int16, out_prec=8),
               dict(out=np.empty((3, 80, 96), np.uint8), out_prec=12)):
        with pytest.raises(grk.GrkGpuError, match="do not hold the output precision"):
            codec.decompress(cs12, **kw)
    for kw in (dict(colour="rgb"), dict(colour=1), dict(out_prec=8, prec_mode="round"), dict(out_prec=0),
               dict(out_prec=17), dict(prec_mode=None)):
        with pytest.raises(grk.GrkGpuError, match="colour must be|prec_mode must be|out_prec must be"):
            codec.decompress(cs12, **kw)
    # colour="sycc" implies upsample=True: out= has the image's shape
    cs = open(f"{GOLD}/sub_420_rgb8.j2k", "rb").read()  # 97 x 75, 4:2:0
    for kw in (dict(out=np.empty((3, 75, 97), np.uint8)), dict(out=np.empty((75, 97, 3), np.uint8), layout="hwc"),
               dict(out=np.empty((54, 61, 3), np.uint8), layout="hwc", window=(10, 7, 71, 61))):
        with pytest.raises(grk.GrkGpuError, match="grkgpu error -1: null argument"):
            codec.decompress(cs, colour="sycc", **kw)
    for kw in (dict(out=np.empty((3, 75, 96), np.uint8)), dict(out=np.empty((3, 38, 49), np.uint8)),
               dict(out=np.empty((3, 75, 97), np.uint8), layout="hwc"),
               dict(out=[np.empty((75, 97), np.uint8)] * 3), dict(out=np.empty((3, 75, 97), np.float32))):
        with pytest.raises(grk.GrkGpuError, match="out must be"):
            codec.decompress(cs, colour="sycc", **kw)
    with pytest.raises(grk.GrkGpuError, match="subsampled components decode to host planes only"):
        codec.decompress(cs, out=np.empty((3, 75, 97), np.uint8))


def test_sycc_closed_form_is_the_reference_loop():
    """sycc422_to_rgb / sycc420_to_rgb by hand.  Pixel (y, cb, cr) = (100, 148,
    98): cb - 128 = 20, cr - 128 = -30, R = 100 + (int)(-42.06) = 58, G = 100 -
    (int)(6.88 - 21.42) = 114, B = 100 + (int)(35.44) = 135."""
    y = np.array([[100, 110, 120, 130, 140]])
    # origin 0: the pairs (y0 y1 | cb0 cr0), (y2 y3 | cb1 cr1), the tail (y4 | cb2 cr2)
    got = convert([y, np.array([[148, 90, 200]]), np.array([[98, 128, 30]])], (0, 0, 5, 1), S422, 8, colour="sycc")
    assert np.stack(got)[:, 0].T.tolist() == [[58, 114, 135], [68, 124, 145], [120, 133, 53], [130, 143, 63],
                                             [3, 185, 255]]
    # origin 1: the first pixel's chroma is raw 0 (cb - 128 = cr - 128 = -128: R = 100 - 179 -> 0,
    # G = 100 - (int)(-44.032 - 91.392) = 235, B = 100 - 226 -> 0), then the pairs
    got = convert([y, np.array([[90, 200]]), np.array([[128, 30]])], (1, 0, 6, 1), S422, 8, colour="sycc")
    assert np.stack(got)[:, 0].T.tolist() == [[0, 235, 0], [110, 123, 43], [120, 133, 53], [0, 175, 255],
                                             [3, 185, 255]]
    # 4:2:0, a 3 x 3 block at origin (0, 1): the first line takes chroma 0, the
    # row pair below it chroma row 0 -- columns 0, 1 its first sample, column 2 the second
    yy = np.array([[10, 20, 30], [40, 50, 60], [70, 80, 90]])
    got = np.stack(convert([yy, np.array([[148, 90]]), np.array([[98, 200]])], (0, 1, 3, 4), S420, 8, colour="sycc"))
    assert got.transpose(1, 2, 0).tolist() == [[[0, 145, 0], [0, 155, 0], [0, 165, 0]],
                                               [[0, 54, 75], [8, 64, 85], [160, 22, 0]],
                                               [[28, 84, 105], [38, 94, 115], [190, 52, 23]]]


def test_sycc_closed_form_rounds_every_product():
    """Pairs where contracting the G term to an FMA, or float32, would differ:
    cb - 128 = -110, cr - 128 = 60: 0.344 * cb = -37.839999999999996, 0.714 * cr
      = 42.839999999999996, their double sum is exactly 5.0 -> 5; fma(0.344, cb,
      42.839999999999996) = 4.99999999999999... -> 4;
    cb - 128 = -128, cr - 128 = -112: -44.032 + -79.96799999999999 =
      -123.99999999999999 -> -123; in float32 the sum is -124.0 -> -124."""
    g = lambda cb, cr: int(sycc_to_rgb(np.array([[[128]], [[cb + 128]], [[cr + 128]]]), 8)[1, 0, 0])  # noqa: E731
    assert g(-110, 60) == 128 - 5 and g(-128, -112) == 128 + 123
    assert g(-103, -12) == 128 + 43 and g(-127, 92) == 128 - 22
    # every pair at once against the scalar C expression in Python floats (IEEE doubles, no FMA)
    cb, cr = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    got = sycc_to_rgb(np.stack([np.full_like(cb, 128), cb, cr]), 8)
    clamp = lambda v: max(0, min(255, v))  # noqa: E731
    for b, r in ((0, 0), (255, 255), (18, 188), (0, 16), (1, 220), (77, 3), (128, 128), (255, 0)):
        want = [clamp(128 + int(1.402 * (r - 128))), clamp(128 - int(0.344 * (b - 128) + 0.714 * (r - 128))),
                clamp(128 + int(1.772 * (b - 128)))]
        assert got[:, b, r].tolist() == want


def test_precision_closed_forms():
    """clip_component / scale_component on 0, 1, max, min."""
    u = lambda q: [0, 1, (1 << q) - 1]                                   # noqa: E731
    s = lambda q: [0, 1, (1 << (q - 1)) - 1, -(1 << (q - 1)), -1]         # noqa: E731
    f = lambda v, q, sg, p, mode: to_prec(np.array(v), q, sg, p, mode).tolist()  # noqa: E731
    assert f(u(12), 12, False, 8, "clip") == [0, 1, 255]
    assert f(u(12), 12, False, 8, "scale") == [0, 0, 255]                # >> 4
    assert f(u(8), 8, False, 12, "clip") == [0, 1, 255]
    assert f(u(8), 8, False, 12, "scale") == [0, 16, 4095]               # v * 4095 / 255, integer division
    assert f([128], 8, False, 12, "scale") == [2055]                     # 128 * 4095 / 255 = 2055.5...
    assert f(u(16), 16, False, 1, "clip") == [0, 1, 1]
    assert f(u(16) + [32768, 32767], 16, False, 1, "scale") == [0, 0, 1, 1, 0]   # >> 15
    assert f(s(12), 12, True, 8, "clip") == [0, 1, 127, -128, -1]         # max = 255 / 2, min = -max - 1
    assert f(s(12), 12, True, 8, "scale") == [0, 0, 127, -128, -1]        # arithmetic >> 4
    assert f(s(8), 8, True, 12, "clip") == [0, 1, 127, -128, -1]
    assert f(s(8), 8, True, 12, "scale") == [0, 16, 2032, -2048, -16]     # v * 2048 / 128, exact
    assert f(s(8), 8, True, 1, "clip") == [0, 0, 0, -1, -1]               # max = 1 / 2 = 0, min = -1
    assert f(u(8), 8, False, 8, "scale") == u(8)
