"""Host side of the narrow / interleaved decode output (no GPU): the exports,
the argument checks that come before any device call, and the Python
dtype / layout / shape validation."""
import ctypes
import os

import numpy as np
import pytest


def _grk():
    import grokimagecompression_amd as grk
    if not os.path.exists(grk.LIB_PATH):
        grk.build()
    return grk


def test_library_exports_decode_to():
    L = _grk().lib()
    assert hasattr(L, "grkgpu_decompress_to") and hasattr(L, "grkgpu_mct_inv_dcshift_to")


def _bad_outs(grk):
    return [None, ctypes.byref(grk.OutPlanes(sample_fmt=5)), ctypes.byref(grk.OutPlanes(sample_fmt=1, layout=2))]


def test_decompress_to_refuses_bad_out_without_a_device():
    grk = _grk()
    L = grk.lib()
    cs = b"\xff\x4f\xff\x51"
    ctx = ctypes.c_void_p(1)  # never dereferenced: the output description is checked first
    for out in _bad_outs(grk):
        assert L.grkgpu_decompress_to(ctx, cs, len(cs), None, 0, 0xFFFFFFFF, None, out) == -1  # GRKGPU_EINVAL
    assert b"layout" in L.grkgpu_last_error()


def test_mct_inv_dcshift_to_refuses_bad_out_without_a_device():
    grk = _grk()
    L = grk.lib()
    src = (ctypes.c_void_p * 3)(64, 64, 64)  # never dereferenced
    prec = (ctypes.c_uint32 * 3)(8, 8, 8)
    sgnd = (ctypes.c_int32 * 3)(0, 0, 0)
    for out in _bad_outs(grk):
        assert L.grkgpu_mct_inv_dcshift_to(src, 3, 4, 4, 4, prec, sgnd, 1, 0, out, 4, None) == -1
    # a format that does not hold the precision, and a stride shorter than a row of pixels
    op = grk.OutPlanes(sample_fmt=grk.SAMPLE_U8, layout=grk.LAYOUT_INTERLEAVED)
    op.planes[0] = 64
    prec12 = (ctypes.c_uint32 * 3)(12, 12, 12)
    assert L.grkgpu_mct_inv_dcshift_to(src, 3, 4, 4, 4, prec12, sgnd, 1, 0, ctypes.byref(op), 12, None) == -1
    assert L.grkgpu_mct_inv_dcshift_to(src, 3, 4, 4, 4, prec, sgnd, 1, 0, ctypes.byref(op), 11, None) == -1


def test_out_planes_matches_header_layout():
    grk = _grk()
    # void *planes[16]; uint32_t sample_fmt, layout; int32_t on_device; uint32_t pad_
    assert ctypes.sizeof(grk.OutPlanes) == 16 * ctypes.sizeof(ctypes.c_void_p) + 16
    assert grk.OutPlanes.sample_fmt.offset == 16 * ctypes.sizeof(ctypes.c_void_p)
    assert grk.OutPlanes.on_device.offset == grk.OutPlanes.sample_fmt.offset + 8


def test_dtype_to_format_mapping():
    grk = _grk()
    want = {np.int32: grk.SAMPLE_I32, np.uint8: grk.SAMPLE_U8, np.int8: grk.SAMPLE_I8, np.uint16: grk.SAMPLE_U16,
            np.int16: grk.SAMPLE_I16}
    for dt, fmt in want.items():
        assert grk._out_format(dt) == (np.dtype(dt), fmt)
    assert grk._out_format(None) == (np.dtype(np.int32), grk.SAMPLE_I32)
    assert grk._out_format("uint16") == (np.dtype(np.uint16), grk.SAMPLE_U16)
    for bad in (np.float32, np.int64, np.uint32, "pixels"):
        with pytest.raises(grk.GrkGpuError):
            grk._out_format(bad)


def test_check_out_dtype_and_layout():
    grk = _grk()
    shape = (3, 5, 7)
    assert grk._check_out(np.empty(shape, np.int32), shape, 0) is False
    assert grk._check_out(np.empty(shape, np.uint8), shape, 0, np.uint8) is False
    assert grk._check_out(np.empty((5, 7, 3), np.uint16), shape, 0, np.uint16, "hwc") is False
    bad = [(np.empty(shape, np.uint8), np.int32, "chw"),          # dtype
           (np.empty(shape, np.int32), np.uint8, "chw"),
           (np.empty(shape, np.uint16), np.uint16, "hwc"),        # planar shape, interleaved layout
           (np.empty((5, 7, 3), np.uint16), np.uint16, "chw"),
           (np.empty((3, 5, 8), np.uint8), np.uint8, "chw"),      # shape
           (np.empty((3, 7, 5), np.uint8).transpose(0, 2, 1), np.uint8, "chw"),  # not contiguous
           (np.empty(shape, np.float32), np.float32, "chw"),      # no such format
           (np.empty(shape, np.uint8), np.uint8, "cwh")]          # no such layout
    for out, dt, layout in bad:
        with pytest.raises(grk.GrkGpuError):
            grk._check_out(out, shape, 0, dt, layout)
    # the int32 message is the one callers have always seen
    with pytest.raises(grk.GrkGpuError, match="out must be a C-contiguous int32 array of shape"):
        grk._check_out(np.empty(shape, np.int16), shape, 0)
