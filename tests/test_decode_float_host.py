"""Float decode output, host half (no GPU): the C ABI of the three entry points,
the refusals that come before any device call, grkgpu_batch_float_plan over the
committed goldens, the Python validation of out= / scale / dtype, the
norm_scale_bias helper and the numpy restatement the GPU tests compare with."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import GOLD, ROOT, load_manifest
from float_fixtures import FLOATS, bits, normalise, same_bits

MAN = load_manifest()
NAMES = sorted(MAN)
OK, EINVAL, EUNSUPPORTED = 0, -1, -4


def _grk():
    import grokimagecompression_amd as grk
    if not os.path.exists(grk.LIB_PATH):
        grk.build()
    return grk


def _cs(name):
    return open(os.path.join(GOLD, name + ".j2k"), "rb").read()


def test_abi():
    grk = _grk()
    L = grk.lib()
    for sym in ("grkgpu_decompress_float", "grkgpu_decompress_batch_float", "grkgpu_batch_float_plan"):
        assert hasattr(L, sym)
    assert (grk.SAMPLE_F32, grk.SAMPLE_F16, grk.SAMPLE_BF16) == (16, 17, 18)
    hdr = open(os.path.join(ROOT, "include", "grk_mi355x.h")).read()
    assert "enum { GRKGPU_SAMPLE_F32 = 16, GRKGPU_SAMPLE_F16 = 17, GRKGPU_SAMPLE_BF16 = 18 };" in hdr
    assert "typedef struct { float scale[GRKGPU_MAX_COMPS], bias[GRKGPU_MAX_COMPS]; } grkgpu_out_norm;" in hdr
    for name in ("JP2 files", "custom-MCT", "force-RGB", "grk_* API", "float input to the encoder"):
        assert name in hdr, name  # the out-of-scope list


def test_struct_sizes(tmp_path):
    """the new struct and the ones that must not have moved, against the header compiled as C"""
    grk = _grk()
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no C compiler"
    src = tmp_path / "abi.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "grk_mi355x.h"\n'
                   "int main(void) { printf(\"%zu %zu %zu %zu %zu %zu\\n\", sizeof(grkgpu_out_norm),\n"
                   "offsetof(grkgpu_out_norm, bias), sizeof(grkgpu_out_ops), sizeof(grkgpu_out_planes),\n"
                   "sizeof(grkgpu_store_job), sizeof(grkgpu_batch_item)); return 0; }\n")
    exe = tmp_path / "abi"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(grk.OutNorm), grk.OutNorm.bias.offset, ctypes.sizeof(grk.OutOps),
                   ctypes.sizeof(grk.OutPlanes), ctypes.sizeof(grk.StoreJob), ctypes.sizeof(grk.BatchItem)]
    vp = ctypes.sizeof(ctypes.c_void_p)
    assert got[:5] == [128, 64, 16, 16 * vp + 16, 144]


def _call(grk, cs, fmt=None, layout=0, ops=None, norm=None, out=True, planes=(64, 64, 64), ctx=1):
    """grkgpu_decompress_float with a context that is never dereferenced"""
    op = grk.OutPlanes(sample_fmt=grk.SAMPLE_F16 if fmt is None else fmt, layout=layout, on_device=1)
    for k, p in enumerate(planes):
        op.planes[k] = p
    L = grk.lib()
    rc = L.grkgpu_decompress_float(ctypes.c_void_p(ctx) if ctx else None, cs, len(cs), None, 0, 0xFFFFFFFF, None,
                                   ctypes.byref(op) if out else None, None if ops is None else ctypes.byref(ops),
                                   None if norm is None else ctypes.byref(norm))
    return rc, L.grkgpu_last_error().decode()


def test_refusals_come_before_any_device_call():
    grk = _grk()
    cs = _cs("rgb8_128x96")
    # an integer format in this call, every one of them
    for fmt in (grk.SAMPLE_I32, grk.SAMPLE_U8, grk.SAMPLE_I8, grk.SAMPLE_U16, grk.SAMPLE_I16, 5, 15, 19):
        rc, msg = _call(grk, cs, fmt=fmt)
        assert rc == EINVAL and "float" in msg, (fmt, msg)
    # a non-finite scale or bias on a used channel (three of them here)
    for field in ("scale", "bias"):
        for bad in (float("nan"), float("inf"), -float("inf")):
            for ch in range(3):
                norm = grk._out_norm(1.0, 0.0)
                getattr(norm, field)[ch] = bad
                rc, msg = _call(grk, cs, norm=norm)
                assert rc == EINVAL and "finite" in msg, (field, bad, ch, msg)
    # what grkgpu_decompress_convert refuses stays refused, alike
    for layout in (0x200, 0x102, 2):
        rc, msg = _call(grk, cs, layout=layout)
        assert rc == EINVAL and "layout" in msg
    O = grk.OutOps
    for ops in (O(prec=17), O(colour=7), O(colour=grk.COLOUR_AUTO), O(prec=8, prec_mode=2), O(reserved=1)):
        assert _call(grk, cs, ops=ops)[0] == EINVAL
    assert _call(grk, cs, out=False)[0] == EINVAL
    assert _call(grk, cs, ctx=0)[0] == EINVAL
    assert _call(grk, cs, planes=(64, 0, 64))[0] == EINVAL            # a null plane
    assert _call(grk, cs, planes=(64, 65, 64))[0] == EINVAL           # float16 at an odd address
    assert _call(grk, cs, fmt=grk.SAMPLE_F32, planes=(64, 66, 64))[0] == EINVAL
    assert _call(grk, _cs("g8_64"), ops=O(colour=grk.COLOUR_SYCC))[0] == EINVAL  # one component
    # ... and what it cannot store through these kernels is unsupported
    rc, msg = _call(grk, _cs("g8_64"), ops=O(colour=grk.COLOUR_FORCE_RGB))
    assert rc == EUNSUPPORTED and "force-RGB" in msg
    import json
    mct = _cs(sorted(json.load(open(os.path.join(GOLD, "manifest_mct.json"))))[0])
    rc, msg = _call(grk, mct)
    assert rc == EUNSUPPORTED and "MCT" in msg
    # a 16-bit precision op is fine in any float format: the format holds every precision
    r = grk.plan_batch_float([_cs("rgb8_128x96")], dtype="float16", out_prec=16, prec_mode="scale")
    assert r["status"] == [OK] and r["img"][0].prec[0] == 16


def test_the_old_entry_points_still_refuse_float_formats():
    grk = _grk()
    L = grk.lib()
    cs = _cs("rgb8_128x96")
    ctx = ctypes.c_void_p(1)
    for fmt in (grk.SAMPLE_F32, grk.SAMPLE_F16, grk.SAMPLE_BF16):
        op = grk.OutPlanes(sample_fmt=fmt, on_device=1)
        op.planes[0] = op.planes[1] = op.planes[2] = 64
        assert L.grkgpu_decompress_to(ctx, cs, len(cs), None, 0, 0xFFFFFFFF, None, ctypes.byref(op)) == EINVAL
        assert L.grkgpu_decompress_convert(ctx, cs, len(cs), None, 0, 0xFFFFFFFF, None, ctypes.byref(op), None) == EINVAL
        assert L.grkgpu_decompress_mct(ctx, cs, len(cs), None, 0, 0xFFFFFFFF, None, ctypes.byref(op), None) == EINVAL
        items, keep = grk._batch_items([cs])
        items[0].out.sample_fmt = fmt
        assert L.grkgpu_batch_plan(items, 1, None, None) == EINVAL
        assert L.grkgpu_batch_convert_plan(items, None, 1, None, None) == EINVAL
    for dt in (np.float32, np.float16, "float32"):
        with pytest.raises(grk.GrkGpuError):
            grk._out_format(dt)
    with pytest.raises(grk.GrkGpuError):
        grk.plan_batch_convert([cs], dtype=np.float32)


def _img(d):
    return [(d.x0, d.y0, d.x1, d.y1, d.numcomps)] + [(d.prec[k], d.sgnd[k], d.dx[k], d.dy[k]) for k in range(d.numcomps)]


def test_plan_over_the_goldens():
    grk = _grk()
    bufs = [_cs(n) for n in NAMES]
    assert len(bufs) == 88
    want = grk.plan_batch_convert(bufs)
    assert want["status"] == [OK] * 88
    for name in FLOATS:
        for layout in ("chw", "hwc"):
            got = grk.plan_batch_float(bufs, dtype=name, layout=layout, scale=1 / 255, bias=-0.5)
            ref = want if layout == "chw" else grk.plan_batch_convert(bufs, layout=layout)
            assert got["rc"] == ref["rc"] and got["status"] == ref["status"] and got["n_launches"] == 0
            assert (got["n_ok"], got["n_blocks"], got["n_store_jobs"]) == (ref["n_ok"], ref["n_blocks"], ref["n_store_jobs"])
            for a, b in zip(got["img"], ref["img"]):
                assert bytes(a) == bytes(b)
    # the descriptor is grkgpu_decompress_convert's: output precision, channels after CMYK, dx = dy = 1 upsampled
    subs = [_cs("sub_420_rgb8"), _cs("sub_422_I_tiles"), _cs("rgb12_96x80")]
    for kw in (dict(upsample=True), dict(colour=["sycc", "sycc", None], out_prec=8, prec_mode="scale"), dict()):
        got = grk.plan_batch_float(subs, dtype="bfloat16", **kw)
        ref = grk.plan_batch_convert(subs, **kw)
        assert got["status"] == ref["status"] == [OK] * 3
        assert [_img(d) for d in got["img"]] == [_img(d) for d in ref["img"]]
        assert (got["n_ok"], got["n_blocks"], got["n_store_jobs"]) == (ref["n_ok"], ref["n_blocks"], ref["n_store_jobs"])


def test_plan_per_item_refusals():
    grk = _grk()
    good, gray = _cs("rgb8_128x96"), _cs("g8_64")
    # an integer-format item fails on its own
    for fmt in (grk.SAMPLE_I32, grk.SAMPLE_U8, grk.SAMPLE_I16):
        r = grk.plan_batch_float([good, good, gray], sample_fmt=[None, fmt, None])
        assert r["status"] == [OK, EINVAL, OK] and r["n_ok"] == 2 and r["rc"] == EINVAL
        assert r["error"].startswith("item 1: ") and "float" in r["error"]
    # a NaN on a used channel is that item's EINVAL; on an unused one it is not read
    nan = np.array([1.0, 1.0, 1.0, np.nan])
    r = grk.plan_batch_float([good, gray], scale=[nan, 1.0], bias=[0.0, nan])
    assert r["status"] == [OK, OK]
    r = grk.plan_batch_float([good, gray], scale=[nan[1:], 1.0])
    assert r["status"] == [EINVAL, OK] and "finite" in r["error"]
    r = grk.plan_batch_float([good, gray], bias=[0.0, np.array([np.inf])])
    assert r["status"] == [OK, EINVAL]
    # CMYK leaves one channel fewer: the fourth entry of a four-ink stream is not read
    r = grk.plan_batch_float([good, gray], ops=[grk.OutOps(colour=grk.COLOUR_FORCE_RGB), None])
    assert r["status"] == [EUNSUPPORTED, OK] and "force-RGB" in r["error"]
    # the call-level rules
    L = grk.lib()
    assert grk.plan_batch_float([])["rc"] == OK
    assert L.grkgpu_batch_float_plan(None, None, None, 1, None, None) == EINVAL
    assert L.grkgpu_decompress_batch_float(None, None, None, None, 0, None, None) == EINVAL  # no context
    # norms = NULL: scale 1, bias 0
    items, keep = grk._batch_items([good])
    items[0].out.sample_fmt = grk.SAMPLE_F32
    assert L.grkgpu_batch_float_plan(items, None, None, 1, None, None) == OK and items[0].status == OK


def test_python_validation():
    """out=, scale and dtype are checked before anything crosses the C ABI (no
    context needed to get that far)."""
    import torch
    grk = _grk()
    codec = object.__new__(grk.Codec)
    codec.device, codec._ctx = 0, None
    cs = open(f"{GOLD}/sub_420_rgb8.j2k", "rb").read()  # 97 x 75, 4:2:0
    bad = [dict(out=np.empty((3, 75, 97), np.float32), dtype="float16"),         # dtype
           dict(out=np.empty((3, 75, 97), np.uint8), dtype="float32"),
           dict(out=np.empty((3, 75, 97), np.float64), dtype="float32"),
           dict(out=np.empty((3, 75, 96), np.float32)),                          # shape
           dict(out=np.empty((3, 38, 49), np.float32)),                          # a chroma plane's size
           dict(out=np.empty((3, 75, 97), np.float32), layout="hwc"),            # planar shape, interleaved layout
           dict(out=np.empty((75, 97, 3), np.float32)),
           dict(out=np.empty((3, 97, 75), np.float32).transpose(0, 2, 1)),       # not contiguous
           dict(out=np.empty((3, 75, 97), np.uint16), dtype="bfloat16"),         # numpy has no bfloat16
           dict(out=torch.empty((3, 75, 97), dtype=torch.float16), dtype="float16"),  # a host tensor of a numpy dtype
           dict(out=torch.empty((3, 75, 97), dtype=torch.float32), dtype="bfloat16"),
           dict(out=torch.empty((3, 75, 98), dtype=torch.bfloat16)[:, :, :97], dtype="bfloat16"),
           dict(out=[np.empty((75, 97), np.float32)] * 3),
           dict(scale=(1.0, 2.0)), dict(bias=np.zeros(4)), dict(scale=[]),       # one value, or one per channel
           dict(dtype=np.uint8), dict(dtype=np.float64), dict(dtype="half"), dict(dtype=torch.int32),
           dict(layout="cwh"), dict(layers=-1)]
    for kw in bad:
        with pytest.raises(grk.GrkGpuError):
            codec.decompress_float(cs, upsample=True, **kw)
    with pytest.raises(grk.GrkGpuError, match="subsampled components decode to host planes only"):
        codec.decompress_float(cs, out=np.empty((3, 75, 97), np.float32))
    # the batch front end: the same checks per item, and the per-item rule for scale / bias
    with pytest.raises(grk.GrkGpuError):
        codec.decompress_batch_float([cs, cs], upsample=True, out=[np.empty((3, 75, 97), np.float16), None])
    with pytest.raises(grk.GrkGpuError):
        codec.decompress_batch_float([cs, cs], upsample=True, scale=[1.0])
    with pytest.raises(grk.GrkGpuError):
        codec.decompress_batch_float([cs, cs], upsample=True, scale=[1.0, (1.0, 2.0)])
    with pytest.raises(grk.GrkGpuError):
        codec.decompress_batch_float([cs, cs], upsample=True, dtype=["float16", np.uint8])
    # the integer calls keep refusing float dtypes
    for call in (codec.decompress, ):
        with pytest.raises(grk.GrkGpuError):
            call(cs, upsample=True, dtype=np.float32)
    with pytest.raises(grk.GrkGpuError):
        grk._check_out(np.empty((3, 4, 4), np.float32), (3, 4, 4), 0, np.float32)
    assert grk._out_dtype(np.empty(3, np.float32)) is None and grk._out_dtype(torch.empty(3, dtype=torch.bfloat16)) is None
    # every spelling of the three dtypes
    for name, spell in (("float32", (np.float32, "float32", torch.float32, np.dtype("float32"))),
                        ("float16", (np.float16, "float16", torch.float16)),
                        ("bfloat16", ("bfloat16", torch.bfloat16))):
        for sp in spell:
            assert grk._float_format(sp) == (name, grk._FLOAT_FMT[name])


def test_norm_scale_bias():
    grk = _grk()
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    for prec in (1, 8, 12, 16):
        s, b = grk.norm_scale_bias(prec, mean, std)
        assert s.dtype == b.dtype == np.float32 and s.shape == b.shape == (3,)
        for k in range(3):
            assert s[k] == np.float32(1.0 / (float(2 ** prec - 1) * std[k]))
            assert b[k] == np.float32(-mean[k] / std[k])
    s, b = grk.norm_scale_bias(8, 0.5, 0.25)
    assert s.tolist() == [np.float32(4.0 / 255.0)] and b.tolist() == [-2.0]
    s, b = grk.norm_scale_bias(12, 0.0, 1.0, sgnd=True)
    assert s[0] == np.float32(1.0 / 4095.0) and b[0] == 0.0
    for kw in (dict(prec=0, mean=0, std=1), dict(prec=8, mean=0, std=0), dict(prec=8, mean=np.nan, std=1)):
        with pytest.raises(grk.GrkGpuError):
            grk.norm_scale_bias(**kw)
    # ToTensor + Normalize on every 8-bit value, in float64
    s, b = grk.norm_scale_bias(8, mean, std)
    x = np.arange(256, dtype=np.float64)
    for k in range(3):
        want = (x / 255.0 - mean[k]) / std[k]
        assert np.allclose(x * np.float64(s[k]) + np.float64(b[k]), want, rtol=0, atol=1e-6)


def _fma(v, s, b):
    """float32(v) * s + b with ONE rounding (what a contracted kernel computes): formed in float64, where the
    product of two float32 values is exact and the sum is too while it spans under 53 bits (asserted)"""
    from fractions import Fraction
    d = np.float64(np.float32(v)) * np.float64(s) + np.float64(b)
    assert Fraction(float(d)) == Fraction(int(v)) * Fraction(float(s)) + Fraction(float(b))
    return np.float32(d)


def test_restatement_tells_the_wrong_kernels_apart():
    s, b = np.float32(1.0 / 65535.0), np.float32(-0.485 / 0.229)
    # 1. two roundings against a fused multiply-add: how often they differ over every 16-bit sample, and one fixed
    # sample where they do
    v = np.arange(65536, dtype=np.int32)
    two = normalise(v[None, None], s, b, "float32")[0, 0]
    one = (v.astype(np.float64) * np.float64(s) + np.float64(b)).astype(np.float32)
    differ = np.flatnonzero(bits(two) != bits(one))
    assert differ.size > 5000
    k = int(differ[0])
    assert bits(normalise(np.array([[[k]]]), s, b, "float32"))[0, 0, 0] != bits(np.array([_fma(k, s, b)]))[0]
    assert two[k] == np.float32(np.float32(np.float32(k) * s) + b)
    # 2. bfloat16: nearest even against truncation
    bf = bits(normalise(v[None, None], s, b, "bfloat16"))[0, 0]
    trunc = (bits(two) >> 16).astype(np.uint16)
    assert np.count_nonzero(bf != trunc) > 20000
    # ... a tie goes to even: 1 + 2^-8 is halfway between 1.0 and the next bfloat16
    tie = normalise(np.array([[[257]]]), np.float32(2.0 ** -8), 0.0, "bfloat16")
    assert bits(tie)[0, 0, 0] == 0x3F80
    tie = normalise(np.array([[[259]]]), np.float32(2.0 ** -8), 0.0, "bfloat16")  # 1 + 3 * 2^-8: up to the even 1 + 2^-6
    assert bits(tie)[0, 0, 0] == 0x3F82
    # 3. float16 subnormals are kept, not flushed: 3 * 2^-24
    sub = normalise(np.array([[[3]]]), np.float32(2.0 ** -24), 0.0, "float16")
    assert bits(sub)[0, 0, 0] == 0x0003 and sub[0, 0, 0] != 0
    # ... and rounded to nearest even like every other value: 2.5 * 2^-24 -> 2 * 2^-24
    sub = normalise(np.array([[[5]]]), np.float32(2.0 ** -25), 0.0, "float16")
    assert bits(sub)[0, 0, 0] == 0x0002
    # 4. overflow is inf: 65520 is the first value that rounds up to it
    big = normalise(np.array([[[65519, 65520, -65520]]]), 1.0, 0.0, "float16")
    assert bits(big)[0, 0].tolist() == [0x7BFF, 0x7C00, 0xFC00]
    # 5. samples nothing decoded: bias as it is, a negative scale gives -0.0 + bias
    z = normalise(np.zeros((2, 1, 1), np.int32), (-1.0, 1.0), (0.0, -0.0), "float32")
    assert bits(z)[:, 0, 0].tolist() == [0x00000000, 0x00000000]  # (-0.0) + (+0.0) and (+0.0) + (-0.0) are +0.0
    z = normalise(np.zeros((1, 1, 1), np.int32), -1.0, -0.0, "float32")
    assert bits(z)[0, 0, 0] == 0x80000000
    # layouts and lists take the channel from the right axis
    v = np.arange(24, dtype=np.int32).reshape(2, 3, 4)
    a = normalise(v, (2.0, 3.0), (1.0, -1.0), "float32")
    h = normalise(np.ascontiguousarray(v.transpose(1, 2, 0)), (2.0, 3.0), (1.0, -1.0), "float32", "hwc")
    assert np.array_equal(a, h.transpose(2, 0, 1)) and a[1, 2, 3] == 23 * 3.0 - 1.0
    assert same_bits(normalise([v[0], v[1]], (2.0, 3.0), (1.0, -1.0), "float32"), [a[0], a[1]])
