"""Host side of the upsampled decode output (no GPU): the export, the argument
checks that come before any device call, the Python validation of out= with
upsample=True, and the closed form the GPU tests compare against."""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLD
from test_gpu_decode_upsample import expected, upsample


def _grk():
    import grokimagecompression_amd as grk
    if not os.path.exists(grk.LIB_PATH):
        grk.build()
    return grk


def test_library_exports_upsample_to():
    grk = _grk()
    assert hasattr(grk.lib(), "grkgpu_upsample_to")
    assert grk.LAYOUT_UPSAMPLE == 0x100 and callable(grk.upsample_to)


def test_out_planes_keeps_its_layout():
    grk = _grk()
    # void *planes[16]; uint32_t sample_fmt, layout; int32_t on_device; uint32_t pad_
    vp = ctypes.sizeof(ctypes.c_void_p)
    assert ctypes.sizeof(grk.OutPlanes) == 16 * vp + 16
    assert [getattr(grk.OutPlanes, f).offset - 16 * vp for f in ("sample_fmt", "layout", "on_device", "pad_")] == \
        [0, 4, 8, 12]


def test_decompress_to_refuses_bad_layouts_without_a_device():
    grk = _grk()
    L = grk.lib()
    cs = b"\xff\x4f\xff\x51"
    ctx = ctypes.c_void_p(1)  # never dereferenced: the output description is checked first
    for layout in (0x200, 0x102, 0x300, 2):
        op = grk.OutPlanes(sample_fmt=grk.SAMPLE_U8, layout=layout)
        assert L.grkgpu_decompress_to(ctx, cs, len(cs), None, 0, 0xFFFFFFFF, None, ctypes.byref(op)) == -1
        assert b"layout" in L.grkgpu_last_error()
    # the stage call that does not upsample takes the flag for an unknown bit
    src = (ctypes.c_void_p * 3)(64, 64, 64)
    prec = (ctypes.c_uint32 * 3)(8, 8, 8)
    sgnd = (ctypes.c_int32 * 3)(0, 0, 0)
    op = grk.OutPlanes(sample_fmt=grk.SAMPLE_U8, layout=grk.LAYOUT_UPSAMPLE)
    op.planes[0] = op.planes[1] = op.planes[2] = 64
    assert L.grkgpu_mct_inv_dcshift_to(src, 3, 4, 4, 4, prec, sgnd, 1, 0, ctypes.byref(op), 4, None) == -1


def test_upsample_to_refuses_bad_arguments_without_a_device():
    grk = _grk()
    L = grk.lib()
    U32 = ctypes.c_uint32

    def call(layout=grk.LAYOUT_INTERLEAVED | grk.LAYOUT_UPSAMPLE, fmt=grk.SAMPLE_U8, src=(64, 64, 64),
             sstride=(8, 4, 4), dx=(1, 2, 2), dy=(1, 2, 2), rect=(0, 0, 8, 4), dst=64, dstride=24, out=True):
        op = grk.OutPlanes(sample_fmt=fmt, layout=layout)
        op.planes[0] = op.planes[1] = op.planes[2] = dst
        return L.grkgpu_upsample_to((ctypes.c_void_p * 3)(*src), (U32 * 3)(*sstride), 3, (U32 * 3)(*dx),
                                    (U32 * 3)(*dy), *rect, ctypes.byref(op) if out else None, dstride, None)

    # (pointers are never dereferenced: every refusal comes before the first device call)
    for kw in (dict(layout=0x200), dict(layout=0x102), dict(layout=2), dict(fmt=5), dict(out=False),
               dict(dx=(1, 0, 2)), dict(dy=(1, 2, 0)), dict(dx=(1, 256, 2)),
               dict(src=(64, None, 64)), dict(dst=None),
               dict(dstride=23),                                  # a row of 8 pixels holds 24 samples
               dict(layout=grk.LAYOUT_PLANAR, dstride=7),
               dict(sstride=(8, 3, 4)), dict(sstride=(7, 4, 4)),  # source rows: 8, 4, 4 samples
               dict(rect=(1, 0, 9, 4), sstride=(8, 3, 4)),        # X = 1 .. 8 at dx = 2: chroma columns 1 .. 4
               dict(rect=(4, 0, 4, 4)),
               dict(fmt=grk.SAMPLE_U16, src=(64, 65, 64)), dict(fmt=grk.SAMPLE_U16, dst=65)):
        assert call(**kw) == -1, kw  # GRKGPU_EINVAL


def test_python_validation_of_out_with_upsample():
    """The out= of an upsampled decode is checked like any other decode's,
    before anything crosses the C ABI (no context needed to get that far)."""
    grk = _grk()
    codec = object.__new__(grk.Codec)
    codec.device, codec._ctx = 0, None
    cs = open(f"{GOLD}/sub_420_rgb8.j2k", "rb").read()  # 97 x 75, 4:2:0
    bad = [dict(out=np.empty((3, 75, 96), np.uint8)),                      # shape
           dict(out=np.empty((3, 38, 49), np.uint8)),                      # a chroma plane's size
           dict(out=np.empty((3, 75, 97), np.uint8), layout="hwc"),        # planar shape, interleaved layout
           dict(out=np.empty((75, 97, 3), np.uint8)),
           dict(out=np.empty((3, 75, 97), np.uint8), dtype=np.uint16),     # out against dtype
           dict(out=np.empty((3, 75, 97), np.float32)),                    # no such format
           dict(out=np.empty((3, 97, 75), np.uint8).transpose(0, 2, 1)),   # not contiguous
           dict(out=np.empty((3, 53, 61), np.uint8), window=(10, 7, 71, 61)),  # the window is 61 x 54
           dict(out=[np.empty((75, 97), np.uint8)] * 3),                   # one array, not a list of planes
           dict(dtype=np.float32), dict(layout="cwh")]
    for kw in bad:
        with pytest.raises(grk.GrkGpuError):
            codec.decompress(cs, upsample=True, **kw)
    # without upsample the stream keeps its refusal and its message
    with pytest.raises(grk.GrkGpuError, match="subsampled components decode to host planes only"):
        codec.decompress(cs, out=np.empty((3, 75, 97), np.uint8))


def test_closed_form_is_the_reference_loop():
    """upsample_image_components: dx * ceil(x0 / dx) - x0 zero columns, then
    every source sample dx times, the last one cut at the image's edge."""
    one = lambda row, rect, dx: upsample([np.array([row])], rect, [(dx, 1)])[0, 0].tolist()  # noqa: E731
    assert one([7, 8, 9, 4], (0, 0, 7, 1), 2) == [7, 7, 8, 8, 9, 9, 4]          # origin 0: no lead-in, cut tail
    assert one([7, 8, 9], (1, 0, 8, 1), 2) == [0, 7, 7, 8, 8, 9, 9]             # origin 1: one zero column
    assert one([7, 8], (5, 0, 12, 1), 3) == [0, 7, 7, 7, 8, 8, 8]               # origin 5, dx 3: 3 * 2 - 5 = 1
    # the same down the rows, and both at once
    rows = upsample([np.array([[7], [8]])], (0, 5, 1, 12), [(1, 3)])[0, :, 0].tolist()
    assert rows == [0, 7, 7, 7, 8, 8, 8]
    both = upsample([np.array([[1]])], (1, 1, 4, 4), [(2, 2)])[0].tolist()
    assert both == [[0, 0, 0], [0, 1, 1], [0, 1, 1]]


def test_reference_fixture_has_the_zero_lead_in():
    """sub_422_I_tiles starts at X = 3 with dx = 2: the first chroma column of
    the expected image is zero, the second the reference's first chroma sample."""
    ref, _ = expected("sub_422_I_tiles")
    z = np.load(f"{GOLD}/sub_422_I_tiles.dec.npz")
    assert not ref[1:, :, 0].any() and ref[1, :, 1].any() and np.array_equal(ref[1, :, 1], z["c1"][:, 0])
    assert np.array_equal(ref[0], z["c0"])
