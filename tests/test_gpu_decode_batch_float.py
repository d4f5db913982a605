"""A batch of codestreams straight to normalised float tensors in one launch set
(grkgpu_decompress_batch_float, Codec.decompress_batch_float): every item is
its single decompress_float bit for bit, failing items fail on their own, and
the launch count does not grow with the number of items."""
import numpy as np
import pytest

from float_fixtures import bits, same_bits
from test_gpu_decode_float import encode, gold, image, norm_for

pytestmark = pytest.mark.gpu


def _grk():
    import grokimagecompression_amd as grk
    return grk


def _specs(codec):
    """eight items of mixed geometry, component count, float type, layout, ops and norm; two are 4:2:0"""
    s3, b3 = norm_for(3, 1)
    return [
        (gold("sub_420_rgb8"), dict(dtype="float16", layout="hwc", colour="sycc", scale=s3, bias=b3)),
        (gold("sub_420_rgb8"), dict(dtype="bfloat16", layout="chw", upsample=True, scale=2.0, bias=-1.0)),
        (gold("rgb12_96x80"), dict(dtype="float32", layout="hwc", out_prec=8, prec_mode="scale", scale=1 / 255, bias=0.25)),
        (encode(codec, image(1, 3, 17, 8), 8), dict(dtype="float16", layout="chw", scale=0.5, bias=3.0)),
        (encode(codec, image(4, 9, 37, 8), 8), dict(dtype="bfloat16", layout="hwc", colour="cmyk", scale=s3, bias=b3)),
        (encode(codec, image(5, 5, 33, 8), 8, irreversible=True),
         dict(dtype="float32", layout="chw", scale=norm_for(5)[0], bias=norm_for(5)[1])),
        (encode(codec, image(3, 8, 37, 12, sgnd=True), 12, sgnd=True, mct=1, tiles=(32, 8)),
         dict(dtype="float16", layout="hwc", scale=1 / 2048, bias=0.5)),
        (encode(codec, image(2, 7, 9, 8), 8), dict(dtype="float32", layout="hwc", scale=(3.0, 5.0), bias=(0.5, -0.5))),
    ]


KEYS = ("dtype", "layout", "upsample", "colour", "out_prec", "prec_mode", "scale", "bias")
DFLT = dict(dtype="float32", layout="chw", upsample=False, colour=None, out_prec=None, prec_mode="clip", scale=1.0,
            bias=0.0)


def _batch(codec, specs, **kw):
    args = {k: [s[1].get(k, DFLT[k]) for s in specs] for k in KEYS}
    return codec.decompress_batch_float([s[0] for s in specs], **args, **kw)


@pytest.fixture(scope="module")
def workload(codec):
    specs = _specs(codec)
    refs = [codec.decompress_float(cs, **kw) for cs, kw in specs]
    return specs, refs


@pytest.mark.parametrize("device", [True, False])
def test_every_item_is_its_single_decode(codec, workload, device):
    specs, refs = workload
    got = _batch(codec, specs, device_out=device)
    assert codec.batch_info["n_ok"] == len(specs) == 8
    for i, (g, r) in enumerate(zip(got, refs)):
        assert bool(getattr(g, "is_cuda", False)) == device, i
        assert same_bits(g, r), (i, specs[i][1])


def test_failing_items_fail_on_their_own(codec, workload):
    import torch
    grk = _grk()
    specs, refs = workload
    good = [specs[0], specs[3], specs[6]]
    want = [refs[0], refs[3], refs[6]]
    corrupt = (specs[2][0][:200], dict(dtype="float32", layout="hwc"))
    order = [good[0], corrupt, good[1], good[2]]
    outs = []
    for (cs, kw), r in zip(order, [want[0], None, want[1], want[2]]):
        name = kw["dtype"]
        shape = tuple(r.shape) if r is not None else (80, 96, 3)
        outs.append(torch.full(shape, 7.0, dtype=getattr(torch, name), device="cuda:0"))
    got = _batch(codec, order, out=outs, errors="return")
    assert isinstance(got[1], grk.GrkGpuError) and codec.batch_info["n_ok"] == 3
    assert (outs[1] == 7.0).all()  # untouched
    for g, r in zip((got[0], got[2], got[3]), want):
        assert same_bits(g, r)
    with pytest.raises(grk.GrkGpuError, match="item 1"):
        _batch(codec, order, out=outs)
    # an integer-format item through the C ABI: its own EINVAL, its destination untouched, the others decode
    import ctypes
    cs = [specs[3][0], specs[3][0], specs[3][0]]
    items, keep = grk._batch_items(cs)
    dst = [torch.full((1, 3, 17), 7.0, dtype=torch.float16, device="cuda:0") for _ in cs]
    for i in range(3):
        items[i].out = codec._out_planes(dst[i], 1, grk.SAMPLE_F16 if i != 1 else grk.SAMPLE_U16, "chw", True)
    norms = (grk.OutNorm * 3)()
    for i in range(3):
        grk._out_norm(0.5, 3.0, 1, norms[i])
    grk.lib().grkgpu_set_stream(codec._ctx, grk._stream_handle(0))
    info = grk.BatchInfo()
    rc = grk.lib().grkgpu_decompress_batch_float(codec._ctx, items, None, norms, 3, None, ctypes.byref(info))
    assert rc == -1 and [items[i].status for i in range(3)] == [0, -1, 0] and info.n_ok == 2
    assert (bits(dst[1]) == bits(torch.full((1,), 7.0, dtype=torch.float16))[0]).all()
    assert same_bits(dst[0], refs[3]) and same_bits(dst[2], refs[3])


def test_copies_take_the_launches_of_one(codec, workload):
    specs, refs = workload
    for i in (0, 1, 2, 6):
        one = _batch(codec, [specs[i]], device_out=True)
        n1 = codec.batch_info["n_launches"]
        four = _batch(codec, [specs[i]] * 4, device_out=True)
        assert codec.batch_info["n_launches"] == n1 and codec.batch_info["n_ok"] == 4, i
        for g in four:
            assert same_bits(g, refs[i]) and same_bits(one[0], refs[i])


def test_stack(codec, workload):
    import torch
    specs, refs = workload
    cs, kw = specs[0]
    got = codec.decompress_batch_float([cs] * 3, stack=True, device_out=True, **kw)
    assert isinstance(got, torch.Tensor) and tuple(got.shape) == (3, 75, 97, 3) and got.dtype == torch.float16
    for i in range(3):
        assert same_bits(got[i], refs[0])
    # per-item norms under the list rule, on the host: bfloat16 stacks as one torch CPU tensor
    cs, kw = specs[1]
    kw = dict(kw, scale=[1.0, 2.0], bias=[0.0, -1.0])
    got = codec.decompress_batch_float([cs] * 2, stack=True, **kw)
    assert isinstance(got, torch.Tensor) and not got.is_cuda and got.dtype == torch.bfloat16
    assert same_bits(got[1], refs[1])
    assert same_bits(got[0], codec.decompress_float(cs, dtype="bfloat16", upsample=True))
