"""Encode straight from pixel-interleaved and big-endian samples: the
codestream does not depend on the layout or width the samples arrive in, so
the bar is byte equality everywhere -- with the reference's golden codestreams
(tests/golden/<case>.j2k), with the planar encode of the same samples, and for
the loader kernel alone with the planar stage entry point
(test_mct_stage_vs_oracle pins that one)."""
import ctypes
import os

import numpy as np
import pytest

import synth
from conftest import GOLD, load_manifest
from grokimagecompression_amd import shard

pytestmark = pytest.mark.gpu
MAN = load_manifest()

GOLDENS = ["g8_3x5", "g8_1x37", "g8_45x1", "g8_100x77", "g8_off35", "g8_off_tiles",
           "rgb8_128x96", "rgb8_I", "rgb8_nomct", "rgb8_r10_tiles", "rgb8_uniform_64",
           "rgb12_I", "rgb12_96x80", "rgb12_tiles_I",
           "rgb16_64", "g16_I"]


def _img(m):
    h, w, c, bits = m["shape"]
    img = synth.synth_image(h, w, c, bits, m["seed"], m["kind"])
    assert synth.image_sha256(img) == m["image_sha256"]
    return img, bits


def _gold(name):
    return open(os.path.join(GOLD, name + ".j2k"), "rb").read()


def _hwc(img):
    return np.ascontiguousarray(img.transpose(1, 2, 0))


def _dtypes(bits, sgnd=False):
    """Every dtype that holds `bits`-bit samples: int32, the native 8 / 16-bit
    type, and 16-bit big-endian."""
    dts = [np.dtype(np.int32)]
    if bits <= 8:
        dts.append(np.dtype(np.int8 if sgnd else np.uint8))
    dts.append(np.dtype(np.int16 if sgnd else np.uint16))
    dts.append(np.dtype(">i2" if sgnd else ">u2"))
    return dts


def _to_device(a):
    """The device tensor of a native-order array (None where this torch has no
    such dtype: uint16 on older builds)."""
    import torch
    if not isinstance(getattr(torch, a.dtype.name, None), torch.dtype):
        return None
    return torch.from_numpy(a).to("cuda:0")


@pytest.mark.parametrize("name", GOLDENS)
def test_golden_from_interleaved_in_every_dtype(codec, name):
    import grokimagecompression_amd as grk
    img, bits = _img(MAN[name])
    p, off = grk.CParams.from_cli(MAN[name]["args"])
    gold = _gold(name)
    px = _hwc(img)
    ran = 0
    for dt in _dtypes(bits):
        a = px.astype(dt)
        assert codec.compress(a, bits, p, offset=off, layout="hwc") == gold, "host %s" % dt
        if dt.isnative:
            t = _to_device(a)
            if t is not None:
                assert codec.compress(t, bits, p, offset=off, layout="hwc") == gold, "device %s" % dt
                ran += 1
    assert ran >= 1  # int32 always has a device leg


LOADER_CASES = ["rgb8_128x96", "rgb8_uniform_64", "rgb8_r10_tiles", "rgb12_96x80", "rgb16_64",  # RGB 5/3
                "rgb12_I",                                                                       # 9/7
                "g8_100x77"]                                                                     # gray


@pytest.mark.parametrize("fuse", [0, 1, None])
@pytest.mark.parametrize("name", LOADER_CASES)
def test_every_loader(codec, name, fuse):
    """fuse_level0 = 0: the separate pass (k_dcshift_mct_fwd_pixels); default:
    the fused MCT triple from pixels (k_dwt_fwd_mct3, 5/3 RGB); 1: that for
    9/7 too, and the single-component fused loads."""
    import grokimagecompression_amd as grk
    img, bits = _img(MAN[name])
    p, off = grk.CParams.from_cli(MAN[name]["args"])
    gold = _gold(name)
    px = _hwc(img)
    opts = {} if fuse is None else dict(fuse_level0=fuse)
    with grk.dwt_options(**opts):
        for dt in _dtypes(bits):
            a = px.astype(dt)
            assert codec.compress(a, bits, p, offset=off, layout="hwc") == gold, "host %s" % dt
            t = _to_device(a) if dt.isnative else None
            if t is not None:
                assert codec.compress(t, bits, p, offset=off, layout="hwc") == gold, "device %s" % dt
                # a device tensor one pixel into a larger one: the fused loads' unaligned (per-sample) side
                big = t.new_zeros(t.numel() + t.shape[2])
                big[t.shape[2]:] = t.flatten()
                assert codec.compress(big[t.shape[2]:].view(t.shape), bits, p, offset=off, layout="hwc") == gold


# ---- the loader kernel alone, at every alignment ----

SWEEP_W = list(range(1, 41)) + [63, 64, 65, 66]
SWEEP_H = [1, 2, 3]
MAXH, MAXW = 3, 66
SENTINEL = 0x5A5A5A5A
# (name, GRKGPU_SAMPLE_*, big-endian, numpy dtype the samples are drawn in)
SWEEP_TYPES = [("u8", 1, False, np.uint8), ("u16", 3, False, np.uint16), ("u16be", 3, True, np.uint16),
               ("i16", 4, False, np.int16), ("i32", 0, False, np.int32)]
MCT_MODES = [(0, False), (1, False), (1, True)]  # none, RCT, ICT
SHIFTS = [128, 7, 2048, 0, 1]


def _sweep_samples(dt, c):
    """(MAXH, MAXW, c) samples of dtype dt over its whole range (int32: the
    16-bit range the ICT's 32-bit products are exact for, grk_device.h)."""
    rng = np.random.default_rng(1234 + c)
    lo, hi = (-32768, 32767) if dt == np.int32 else (np.iinfo(dt).min, np.iinfo(dt).max)
    s = rng.integers(lo, hi + 1, size=(MAXH, MAXW, c), dtype=np.int64)
    s[0, 0, :] = hi
    s[-1, -1, :] = lo
    return s.astype(dt)


@pytest.mark.parametrize("c", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("tname,fmt,be,dt", SWEEP_TYPES, ids=[t[0] for t in SWEEP_TYPES])
def test_stage_alignment_sweep(tname, fmt, be, dt, c):
    """grkgpu_dcshift_mct_fwd_from on interleaved pixels: every width 1..40 and
    63..66, height 1..3, source byte offset 0..15, tight and odd row strides,
    no MCT / RCT / ICT -- the results of the planar grkgpu_dcshift_mct_fwd on
    the same samples, and nothing written outside them."""
    import torch
    import grokimagecompression_amd as grk
    dev = torch.device("cuda:0")
    samples = _sweep_samples(dt, c)
    sb = samples.dtype.itemsize
    raw = samples.astype(samples.dtype.newbyteorder(">")) if be else samples
    raw = torch.from_numpy(np.ascontiguousarray(raw).view(np.uint8).reshape(MAXH, MAXW * c * sb).copy()).to(dev)
    planar = torch.from_numpy(np.ascontiguousarray(samples.transpose(2, 0, 1)).astype(np.int32)).to(dev)
    refs = [grk.dcshift_mct_fwd(planar.clone(), SHIFTS[:c], mct, irrev) for mct, irrev in MCT_MODES]
    torch.cuda.synchronize()
    flags = fmt | grk.SAMPLE_INTERLEAVED | (grk.SAMPLE_BIG_ENDIAN if be else 0)
    dstride = MAXW + 3
    buf = torch.zeros(16 + MAXH * (MAXW * c + 4) * sb, dtype=torch.uint8, device=dev)
    out = torch.full((c, MAXH + 2, dstride), SENTINEL, dtype=torch.int32, device=dev)
    want = torch.empty_like(out)
    bad = torch.zeros((), dtype=torch.bool, device=dev)
    n = 0
    for w in SWEEP_W:
        row = w * c
        for stride in (row, (row + 1) | 1):
            for h in SWEEP_H:
                rows = torch.zeros((h, stride * sb), dtype=torch.uint8, device=dev)
                rows[:, :row * sb] = raw[:h, :row * sb]
                rows = rows.flatten()
                for off in range(16):
                    buf[off:off + rows.numel()] = rows
                    for (mct, irrev), ref in zip(MCT_MODES, refs):
                        out.fill_(SENTINEL)
                        grk.dcshift_mct_fwd_from(buf, flags, off, out[:, 1:1 + h], w, h, SHIFTS[:c], mct, irrev,
                                                 src_stride=stride)
                        want.fill_(SENTINEL)
                        want[:, 1:1 + h, :w] = ref[:, :h, :w]
                        bad |= (out != want).any()
                        n += 1
    assert n == len(SWEEP_W) * 2 * len(SWEEP_H) * 16 * len(MCT_MODES)
    assert not bool(bad)


@pytest.mark.parametrize("tname,fmt,be,dt", SWEEP_TYPES, ids=[t[0] for t in SWEEP_TYPES])
def test_stage_planar_sources(tname, fmt, be, dt):
    """The planar side of the stage entry point (big-endian planes included),
    from any byte and with a row stride beyond the row."""
    import torch
    import grokimagecompression_amd as grk
    dev = torch.device("cuda:0")
    c, h, w = 3, 3, 37
    samples = _sweep_samples(dt, c)[:h, :w]
    sb = samples.dtype.itemsize
    planar = np.ascontiguousarray(samples.transpose(2, 0, 1))
    ref_in = torch.from_numpy(planar.astype(np.int32)).to(dev)
    stride = w + 5
    strided = np.zeros((c, h, stride), planar.dtype)
    strided[:, :, :w] = planar
    raw = strided.astype(strided.dtype.newbyteorder(">")) if be else strided
    raw = torch.from_numpy(np.ascontiguousarray(raw).view(np.uint8).reshape(-1).copy()).to(dev)
    for off in (0, 1, 2, 4, 7, 8):
        buf = torch.zeros(off + raw.numel(), dtype=torch.uint8, device=dev)
        buf[off:] = raw
        for mct, irrev in MCT_MODES:
            ref = grk.dcshift_mct_fwd(ref_in.clone(), SHIFTS[:c], mct, irrev)
            out = torch.full((c, h + 2, w + 2), SENTINEL, dtype=torch.int32, device=dev)
            grk.dcshift_mct_fwd_from(buf, fmt | (grk.SAMPLE_BIG_ENDIAN if be else 0), off, out[:, 1:1 + h], w, h,
                                     SHIFTS[:c], mct, irrev, src_stride=stride)
            want = torch.full_like(out, SENTINEL)
            want[:, 1:1 + h, :w] = ref
            assert torch.equal(out, want), (off, mct, irrev)


# ---- windows and shards ----

def _compress_ex(grk, codec, d, p, pl, b, e, parts):
    out, n = ctypes.POINTER(ctypes.c_uint8)(), ctypes.c_size_t()
    rc = grk.lib().grkgpu_compress_ex(codec._ctx, ctypes.byref(d), ctypes.byref(p), ctypes.byref(pl), b, e, parts,
                                      ctypes.byref(out), ctypes.byref(n))
    return rc, (ctypes.string_at(out, n.value) if rc == 0 else None)


@pytest.fixture(scope="module")
def tiled_rgb(codec):
    """A 100 x 77 RGB image in 37 x 29 tiles (3 x 3, the last of each row and
    column cut) and its whole-image codestream from the planar call."""
    import grokimagecompression_amd as grk
    img = synth.synth_image(77, 100, 3, 8, 91, "smooth")
    p = grk.CParams.make(tiles=(37, 29))
    return img, p, codec.compress(img, 8, p)


@pytest.mark.parametrize("dt", [np.uint8, np.uint16, ">u2", np.int32])
def test_single_tiles_from_interleaved_windows(codec, tiled_rgb, dt):
    import grokimagecompression_amd as grk
    img, p, whole = tiled_rgb
    px = _hwc(img).astype(dt)
    c, h, w = img.shape
    assert grk.num_tiles(img.shape, 8, p) == 9
    chunks = []
    for t in range(9):
        ty, tx = divmod(t, 3)
        y0, x0 = ty * 29, tx * 37
        y1, x1 = min(h, y0 + 29), min(w, x0 + 37)
        win = np.ascontiguousarray(px[y0:y1, x0:x1])
        _, shape, fmt, _ = grk._in_samples(win, 8, False, "hwc")
        d, _, _ = codec._image(px, 8, (0, 0), False, "hwc")
        pl = grk._in_planes(win, shape, fmt, False)
        pl.row0, pl.nrows, pl.col0, pl.ncols = y0, y1 - y0, x0, x1 - x0
        parts = grk.PART_TILES | (grk.PART_HEADER if t == 0 else 0) | (grk.PART_EOC if t == 8 else 0)
        rc, cs = _compress_ex(grk, codec, d, p, pl, t, t + 1, parts)
        assert rc == 0, grk.lib().grkgpu_last_error()
        chunks.append(cs)
    assert shard.assemble(chunks) == whole


@pytest.mark.parametrize("dt,on_device", [(np.uint8, False), (">u2", False), (np.int32, False),
                                          (np.uint8, True), (np.int32, True)])  # (torch has no big-endian tensors)
def test_tile_row_shards_from_interleaved_rows(codec, tiled_rgb, dt, on_device):
    import torch
    import grokimagecompression_amd as grk
    img, p, whole = tiled_rgb
    px = _hwc(img).astype(dt)
    chunks = []
    for r in range(3):
        r0, r1 = r * 29, min(77, r * 29 + 29)
        rows = np.ascontiguousarray(px[r0:r1])
        if on_device:
            rows = torch.from_numpy(rows).to("cuda:0")
        parts = grk.PART_TILES | (grk.PART_HEADER if r == 0 else 0) | (grk.PART_EOC if r == 2 else 0)
        chunks.append(codec.compress_tiles(rows, 8, p, 3 * r, 3 * r + 3, parts, row0=r0, height=77, layout="hwc"))
    assert shard.assemble(chunks) == whole
    with pytest.raises(grk.GrkGpuError):  # rows that miss a tile of the range
        codec.compress_tiles(np.ascontiguousarray(px[1:3]), 8, p, 0, 1, grk.PART_ALL, row0=1, height=77, layout="hwc")


# ---- signed and multi-component input ----

def _signed(h, w, c, bits, seed):
    img = synth.synth_image(h, w, c, bits, seed, "smooth")
    return img - (1 << (bits - 1))


@pytest.mark.parametrize("irrev", [False, True])
@pytest.mark.parametrize("bits,dts", [(8, [np.int8, np.int16, ">i2", np.int32]), (12, [np.int16, ">i2", np.int32])])
def test_signed_samples(codec, bits, dts, irrev):
    import grokimagecompression_amd as grk
    img = _signed(45, 70, 3, bits, 5)
    p = grk.CParams.make(irreversible=irrev)
    ref = codec.compress(img, bits, p, sgnd=True)
    for fuse in (None, 1):
        with grk.dwt_options(**({} if fuse is None else dict(fuse_level0=fuse))):
            for dt in dts:
                a = _hwc(img).astype(dt)
                assert codec.compress(a, bits, p, sgnd=True, layout="hwc") == ref, dt
                assert codec.compress(np.ascontiguousarray(img.astype(dt)), bits, p, sgnd=True) == ref, dt


@pytest.mark.parametrize("irrev", [False, True])
@pytest.mark.parametrize("c,mct", [(4, 1), (5, 1), (5, 0), (2, 0)])
def test_more_components(codec, c, mct, irrev):
    """4 components with the MCT over the first three (the 16 * 4-byte runs),
    5 and 2 components (the per-sample loader)."""
    import grokimagecompression_amd as grk
    img = synth.synth_image(50, 61, c, 12, 17, "smooth")
    p = grk.CParams.make(irreversible=irrev, mct=mct)
    ref = codec.compress(img, 12, p)
    for fuse in (None, 0, 1):
        with grk.dwt_options(**({} if fuse is None else dict(fuse_level0=fuse))):
            for dt in (np.uint16, ">u2", np.int32):
                assert codec.compress(_hwc(img).astype(dt), 12, p, layout="hwc") == ref, (fuse, dt)
            t = _to_device(_hwc(img).astype(np.int32))
            assert codec.compress(t, 12, p, layout="hwc") == ref, fuse


def test_custom_mct_from_interleaved(codec):
    """The array-based MCT pass reads the same layouts."""
    import grokimagecompression_amd as grk
    img = synth.synth_image(40, 53, 3, 12, 3, "smooth")
    p = grk.CParams.make(irreversible=True)
    p.set_mct([0.299, 0.587, 0.114, -0.16875, -0.33126, 0.5, 0.5, -0.41869, -0.08131], [2048, 2048, 2048])
    ref = codec.compress(img, 12, p)
    for dt in (np.uint16, ">u2", np.int32):
        assert codec.compress(_hwc(img).astype(dt), 12, p, layout="hwc") == ref, dt
        assert codec.compress(np.ascontiguousarray(img.astype(dt)), 12, p) == ref, dt


def test_encode_blocks_ex_from_the_raster(codec):
    """grkgpu_encode_blocks_ex on a big-endian interleaved raster (what the
    plugin hands over): the code-blocks of grkgpu_encode_blocks on int32 planes."""
    import grokimagecompression_amd as grk
    L = grk.lib()
    img = synth.synth_image(60, 75, 3, 12, 8, "smooth")
    p = grk.CParams.make(irreversible=True)

    def blocks_of(call):
        blocks, n = ctypes.c_void_p(), ctypes.c_uint32()
        assert call(ctypes.byref(blocks), ctypes.byref(n)) == 0, L.grkgpu_last_error()

        class Info(ctypes.Structure):
            _fields_ = [("pos", ctypes.c_uint32 * 6), ("rect", ctypes.c_uint32 * 4), ("numbps", ctypes.c_uint32),
                        ("numpasses", ctypes.c_uint32), ("len", ctypes.c_uint32), ("stepsize", ctypes.c_float),
                        ("data", ctypes.c_void_p), ("rate", ctypes.c_void_p), ("distortion", ctypes.c_void_p)]
        arr = ctypes.cast(blocks, ctypes.POINTER(Info))
        return [(tuple(b.pos), tuple(b.rect), b.numbps, b.numpasses, ctypes.string_at(b.data, b.len))
                for b in (arr[i] for i in range(n.value))]

    d, pl, keep = codec._image(img, 12, (0, 0), False)
    ptrs = (ctypes.c_void_p * 3)(*[keep[k].ctypes.data for k in range(3)])
    L.grkgpu_encode_blocks.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                       ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    want = blocks_of(lambda b, n: L.grkgpu_encode_blocks(codec._ctx, ctypes.byref(d), ctypes.byref(p), ptrs, 0, 0, b, n))
    assert len(want) > 10
    d2, pl2, keep2 = codec._image(_hwc(img).astype(">u2"), 12, (0, 0), False, "hwc")
    assert pl2.sample_fmt == grk.SAMPLE_U16 | grk.SAMPLE_INTERLEAVED | grk.SAMPLE_BIG_ENDIAN
    got = blocks_of(lambda b, n: L.grkgpu_encode_blocks_ex(codec._ctx, ctypes.byref(d2), ctypes.byref(p),
                                                          ctypes.byref(pl2), 0, b, n))
    assert got == want


# ---- multi-device, refusals, the default path ----

def test_compress_multi_from_interleaved():
    import grokimagecompression_amd as grk
    name = "rgb12_tiles_I"
    img, bits = _img(MAN[name])
    p, off = grk.CParams.from_cli(MAN[name]["args"])
    try:
        for dt in (np.uint16, ">u2"):
            assert grk.compress_multi(_hwc(img).astype(dt), bits, p, devices=[0, 0], offset=off,
                                      layout="hwc") == _gold(name), dt
    finally:
        grk.multi_release() if hasattr(grk, "multi_release") else grk.lib().grkgpu_multi_release()


def test_interleaved_refuses_mixed_grids(codec):
    """Components on different grids have no pixels: GRKGPU_EUNSUPPORTED, and
    the context encodes a golden correctly afterwards."""
    import grokimagecompression_amd as grk
    px = np.zeros((16, 16, 3), np.uint8)
    d, pl, keep = codec._image(px, 8, (0, 0), False, "hwc")
    d.dx[1] = d.dx[2] = 2
    d.dy[1] = d.dy[2] = 2
    p = grk.CParams.make()
    rc, _ = _compress_ex(grk, codec, d, p, pl, 0, 0xFFFFFFFF, grk.PART_ALL)
    assert rc == -4  # GRKGPU_EUNSUPPORTED
    assert b"grid" in grk.lib().grkgpu_last_error()
    name = "rgb8_128x96"
    img, bits = _img(MAN[name])
    assert codec.compress(_hwc(img).astype(np.uint8), bits, layout="hwc") == _gold(name)


@pytest.mark.parametrize("name", ["rgb8_128x96", "rgb12_tiles_I", "g16_I"])
def test_default_path_unchanged(codec, name):
    """The planar call, untouched: it carries no layout flag, and gives the
    golden from int32 and from the file's width."""
    import grokimagecompression_amd as grk
    img, bits = _img(MAN[name])
    p, off = grk.CParams.from_cli(MAN[name]["args"])
    _, pl, _ = codec._image(img, bits, off, False)
    assert pl.sample_fmt == grk.SAMPLE_I32 and not pl.sample_fmt & (grk.SAMPLE_INTERLEAVED | grk.SAMPLE_BIG_ENDIAN)
    assert codec.compress(img, bits, p, offset=off) == _gold(name)
    assert codec.compress(img.astype(np.uint8 if bits <= 8 else np.uint16), bits, p, offset=off) == _gold(name)
