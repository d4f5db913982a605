"""Host side of the pixel-interleaved / big-endian encode input (no GPU): the
exports, the grkgpu_planes layout callers were built against, the sample_fmt
checks that come before the context or any device is touched, and the Python
layout / shape / dtype validation."""
import ctypes
import os

import numpy as np
import pytest

EINVAL = -1


def _grk():
    import grokimagecompression_amd as grk
    if not os.path.exists(grk.LIB_PATH):
        grk.build()
    return grk


def test_library_exports_encode_layouts():
    L = _grk().lib()
    assert hasattr(L, "grkgpu_encode_blocks_ex") and hasattr(L, "grkgpu_dcshift_mct_fwd_from")


def test_planes_keeps_its_layout():
    grk = _grk()
    vp = ctypes.sizeof(ctypes.c_void_p)
    # const void *planes[16]; uint32_t sample_fmt; int32_t on_device; uint32_t row0, nrows, col0, ncols
    assert ctypes.sizeof(grk.Planes) == 16 * vp + 24
    want = {"planes": 0, "sample_fmt": 16 * vp, "on_device": 16 * vp + 4, "row0": 16 * vp + 8, "nrows": 16 * vp + 12,
            "col0": 16 * vp + 16, "ncols": 16 * vp + 20}
    assert {f: getattr(grk.Planes, f).offset for f, _ in grk.Planes._fields_} == want
    assert (grk.SAMPLE_INTERLEAVED, grk.SAMPLE_BIG_ENDIAN) == (0x100, 0x200)
    assert (grk.SAMPLE_I32, grk.SAMPLE_U8, grk.SAMPLE_I8, grk.SAMPLE_U16, grk.SAMPLE_I16) == (0, 1, 2, 3, 4)


def _desc(grk, prec, sgnd=0, c=3):
    d = grk.ImageDesc()
    d.x1, d.y1, d.numcomps = 8, 8, c
    for k in range(c):
        d.prec[k], d.sgnd[k], d.dx[k], d.dy[k] = prec, sgnd, 1, 1
    return d


def _bad_formats(grk):
    """(sample_fmt, prec, sgnd) the library refuses: unknown flag bits, a
    big-endian flag on a width that is not 16 bits, a format too narrow for
    the precision (or of the wrong signedness)."""
    IL, BE = grk.SAMPLE_INTERLEAVED, grk.SAMPLE_BIG_ENDIAN
    return [(grk.SAMPLE_U8 | 0x400, 8, 0), (grk.SAMPLE_U16 | 0x80000000, 12, 0), (grk.SAMPLE_I32 | IL | 0x1000, 8, 0),
            (5, 8, 0), (IL | 0x7F, 8, 0),
            (grk.SAMPLE_U8 | BE, 8, 0), (grk.SAMPLE_I8 | BE, 8, 1), (grk.SAMPLE_I32 | BE, 8, 0),
            (grk.SAMPLE_U8 | BE | IL, 8, 0), (grk.SAMPLE_I32 | BE | IL, 12, 0),
            (grk.SAMPLE_U8, 12, 0), (grk.SAMPLE_U8 | IL, 12, 0), (grk.SAMPLE_U16 | BE, 12, 1),
            (grk.SAMPLE_I16 | BE | IL, 12, 0), (grk.SAMPLE_I8 | IL, 12, 1)]


def test_compress_refuses_bad_sample_fmt_without_a_device():
    grk = _grk()
    L = grk.lib()
    ctx = ctypes.c_void_p(1)  # never dereferenced: the format is checked first
    p = grk.CParams.make()
    out, n = ctypes.POINTER(ctypes.c_uint8)(), ctypes.c_size_t()
    blocks, nb = ctypes.c_void_p(), ctypes.c_uint32()
    ds = grk.DeviceSet(n=1)
    for fmt, prec, sgnd in _bad_formats(grk):
        d = _desc(grk, prec, sgnd)
        pl = grk.Planes(sample_fmt=fmt)
        for k in range(3):
            pl.planes[k] = 64  # never dereferenced
        assert L.grkgpu_compress_ex(ctx, ctypes.byref(d), ctypes.byref(p), ctypes.byref(pl), 0, 0xFFFFFFFF, 3,
                                    ctypes.byref(out), ctypes.byref(n)) == EINVAL, hex(fmt)
        assert L.grkgpu_encode_blocks_ex(ctx, ctypes.byref(d), ctypes.byref(p), ctypes.byref(pl), 0,
                                         ctypes.byref(blocks), ctypes.byref(nb)) == EINVAL, hex(fmt)
    assert b"sample format" in L.grkgpu_last_error()


def test_stage_entry_refuses_bad_sample_fmt_without_a_device():
    grk = _grk()
    L = grk.lib()
    dst = (ctypes.c_void_p * 3)(64, 64, 64)  # never dereferenced
    sh = (ctypes.c_int32 * 3)(128, 128, 128)
    for fmt, _, _ in _bad_formats(grk)[:10]:  # flag bits and big-endian widths (the stage takes no precision)
        pl = grk.Planes(sample_fmt=fmt, on_device=1)
        for k in range(3):
            pl.planes[k] = 64
        assert L.grkgpu_dcshift_mct_fwd_from(ctypes.byref(pl), 3, 4, 4, 12, sh, 1, 0, dst, 4, None) == EINVAL, hex(fmt)
    # strides shorter than a row of pixels / of results
    pl = grk.Planes(sample_fmt=grk.SAMPLE_U8 | grk.SAMPLE_INTERLEAVED, on_device=1)
    pl.planes[0] = 64
    assert L.grkgpu_dcshift_mct_fwd_from(ctypes.byref(pl), 3, 4, 4, 11, sh, 1, 0, dst, 4, None) == EINVAL
    assert L.grkgpu_dcshift_mct_fwd_from(ctypes.byref(pl), 3, 4, 4, 12, sh, 1, 0, dst, 3, None) == EINVAL


def test_python_input_formats():
    grk = _grk()
    IL, BE = grk.SAMPLE_INTERLEAVED, grk.SAMPLE_BIG_ENDIAN
    a = np.zeros((5, 7, 3), np.uint16)
    img, shape, fmt, is_tensor = grk._in_samples(a, 12, False, "hwc")
    assert img is a and shape == (3, 5, 7) and fmt == grk.SAMPLE_U16 | IL and not is_tensor
    pl = grk._in_planes(img, shape, fmt, False)
    assert pl.planes[0] == a.ctypes.data and pl.planes[1] is None and pl.sample_fmt == fmt
    # big-endian arrays are passed as they are, planar or interleaved
    b = a.astype(">u2")
    img, shape, fmt, _ = grk._in_samples(b, 12, False, "hwc")
    assert img is b and fmt == grk.SAMPLE_U16 | IL | BE
    img, shape, fmt, _ = grk._in_samples(np.zeros((3, 5, 7), ">i2"), 12, True)
    assert img.dtype == np.dtype(">i2") and shape == (3, 5, 7) and fmt == grk.SAMPLE_I16 | BE
    # a dtype that does not hold the precision (or its signedness) falls back to int32
    for arr, prec, sgnd in ((np.zeros((5, 7, 3), np.uint8), 12, False), (b, 12, True),
                            (np.zeros((5, 7, 3), np.int16), 12, False), (np.zeros((5, 7, 3), ">i4"), 12, False),
                            (np.zeros((5, 7, 3), np.int64), 12, False)):
        img, shape, fmt, _ = grk._in_samples(arr, prec, sgnd, "hwc")
        assert img.dtype == np.int32 and img.dtype.isnative and fmt == grk.SAMPLE_I32 | IL and shape == (3, 5, 7)
    # the default layout is planar: the (c,h,w) call is what it always was
    img, shape, fmt, _ = grk._in_samples(np.zeros((3, 5, 7), np.uint8), 8, False)
    assert shape == (3, 5, 7) and fmt == grk.SAMPLE_U8


def test_python_refuses_bad_input():
    grk = _grk()
    bad = [(np.zeros((5, 7), np.uint8), "hwc"),                       # rank
           (np.zeros((1, 3, 5, 7), np.uint8), "hwc"),
           (np.zeros((5, 7), np.uint8), "chw"),
           (np.zeros((3, 40, 50), np.uint8), "hwc"),                  # a (c,h,w) image read as 50 components
           (np.zeros((3, 5, 7), np.uint8).transpose(1, 2, 0), "hwc"),  # a permuted view: not contiguous
           (np.zeros((5, 14, 3), np.uint8)[:, ::2], "hwc"),
           (np.zeros((5, 7, 3), np.uint8), "cwh"),                    # no such layout
           (np.zeros((5, 7, 3), np.uint8), "HWC")]
    for img, layout in bad:
        with pytest.raises(grk.GrkGpuError):
            grk._in_samples(img, 8, False, layout)
    with pytest.raises(grk.GrkGpuError):
        grk.compress_multi(np.zeros((5, 7, 3), np.uint8), 8, layout="whc")
