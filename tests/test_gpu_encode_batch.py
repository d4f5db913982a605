"""Batch encode on the MI355X (grkgpu_compress_batch): every item of a batch is
the single call's codestream byte for byte -- and so the reference's wherever
the single call is pinned to it -- whatever the items differ in, in one launch
set; the job-table load kernel on its own against the per-tile stage call.
All tolerances are 0."""
import numpy as np
import pytest

import synth
from conftest import GOLD, load_manifest
from test_encode_batch_host import EINVAL, EUNSUPPORTED, mixed_descs

pytestmark = pytest.mark.gpu
MAN = load_manifest()
NAMES = sorted(MAN)


def _grk():
    import grokimagecompression_amd as grk
    return grk


def _img(name):
    m = MAN[name]
    h, w, c, bits = m["shape"]
    img = synth.synth_image(h, w, c, bits, m["seed"], m["kind"])
    assert synth.image_sha256(img) == m["image_sha256"]
    return img, bits


def _gold(name):
    return open(f"{GOLD}/{name}.j2k", "rb").read()


def _batch_args(names):
    """imgs, precs, params, offsets of a list of goldens"""
    grk = _grk()
    imgs, precs, pars, offs = [], [], [], []
    for n in names:
        img, bits = _img(n)
        p, off = grk.CParams.from_cli(MAN[n]["args"])
        imgs.append(img)
        precs.append(bits)
        pars.append(p)
        offs.append(off)
    return imgs, precs, pars, offs


@pytest.fixture(scope="module")
def all_goldens(codec):
    """the 88 goldens as one batch: (imgs, precs, params, offsets, codestreams, info, stats)"""
    imgs, precs, pars, offs = _batch_args(NAMES)
    out = codec.compress_batch(imgs, precs, pars, offs)
    return imgs, precs, pars, offs, out, dict(codec.cbatch_info), codec.stats()


def test_all_goldens_one_call(codec, all_goldens):
    imgs, precs, pars, offs, out, info, stats = all_goldens
    assert len(NAMES) == 88
    golds = [_gold(n) for n in NAMES]
    for n, b, g in zip(NAMES, out, golds):
        assert b == g, n
    assert info["n_ok"] == 88
    assert info["n_blocks"] == stats["num_cblks"] > 0
    assert stats["cs_bytes"] == sum(len(g) for g in golds)
    assert info["n_launches"] > 0
    # the same items in reverse order: another merged table, the same bytes
    rev = codec.compress_batch(imgs[::-1], precs[::-1], pars[::-1], offs[::-1])
    for n, b, g in zip(NAMES[::-1], rev, golds[::-1]):
        assert b == g, n
    assert codec.cbatch_info["n_ok"] == 88 and codec.cbatch_info["n_blocks"] == info["n_blocks"]


STYLES = ["g8_M4_termall", "g16_M5_lazy_termall", "g12_M63", "g8_64", "rgb8_M62_I_r", "g8_M1_lazy"]


@pytest.mark.parametrize("opts", [{}, dict(t1_enc_sort=0), dict(t1_enc_sort=1, t1_enc_bpw=16)])
def test_style_groups(codec, opts):
    """every style twice, interleaved so that no two neighbours share one: each
    style group's blocks come from items that are apart in the call"""
    grk = _grk()
    names = STYLES + STYLES
    assert all(MAN[a]["args"] != MAN[b]["args"] for a, b in zip(names, names[1:]))
    imgs, precs, pars, offs = _batch_args(names)
    with grk.dwt_options(**opts):
        out = codec.compress_batch(imgs, precs, pars, offs)
    for n, b in zip(names, out):
        assert b == _gold(n), (n, opts)


def test_mixed_sources(codec):
    """one batch whose images arrive in eight formats / layouts / places"""
    import torch
    grk = _grk()
    dev = "cuda:%d" % codec.device

    def g(name):
        img, bits = _img(name)
        p, off = grk.CParams.from_cli(MAN[name]["args"])
        return img, bits, p, off, _gold(name)

    hwc = lambda a: np.ascontiguousarray(np.transpose(a, (1, 2, 0)))  # noqa: E731
    items = []  # (image as it arrives, prec, params, offset, sgnd, layout, golden or None)
    img, bits, p, off, gold = g("rgb8_128x96")
    items.append((img.astype(np.int32), bits, p, off, False, "chw", gold))
    img, bits, p, off, gold = g("rgb8_I")
    items.append((hwc(img).astype(np.uint8), bits, p, off, False, "hwc", gold))
    img, bits, p, off, gold = g("rgb12_I")
    if hasattr(torch, "uint16"):
        t = torch.from_numpy(img.astype(np.uint16)).to(dev)
    else:
        t = torch.from_numpy(img.astype(np.int32)).to(dev)
    items.append((t, bits, p, off, False, "chw", gold))
    img, bits, p, off, gold = g("rgb12_96x80")
    items.append((hwc(img).astype(">u2"), bits, p, off, False, "hwc", gold))
    sg = synth.synth_image(45, 70, 2, 12, 5, "smooth", signed=True)
    items.append((sg.astype(np.int16), 12, grk.CParams.make(numresolution=4), (0, 0), True, "chw", None))
    img, bits, p, off, gold = g("g8_100x77")
    items.append((torch.from_numpy(img.astype(np.uint8)).to(dev), bits, p, off, False, "chw", gold))
    img, bits, p, off, gold = g("rgb8_nomct")
    items.append((hwc(img).astype(np.int32), bits, p, off, False, "hwc", gold))
    four = synth.synth_image(50, 61, 4, 12, 9)
    items.append((hwc(four).astype(np.uint16), 12, grk.CParams.make(irreversible=True, tiles=(32, 32)), (0, 0), False,
                  "hwc", None))
    out = codec.compress_batch([q[0] for q in items], [q[1] for q in items], [q[2] for q in items],
                               [q[3] for q in items], [q[4] for q in items], [q[5] for q in items])
    assert codec.cbatch_info["n_ok"] == len(items)
    for i, (q, b) in enumerate(zip(items, out)):
        assert b == codec.compress(q[0], q[1], q[2], offset=q[3], sgnd=q[4], layout=q[5]), i
        if q[6] is not None:
            assert b == q[6], i


def test_many_copies_one_launch_set(codec):
    img, bits, = _img("rgb8_I")
    grk = _grk()
    p, off = grk.CParams.from_cli(MAN["rgb8_I"]["args"])
    gold = _gold("rgb8_I")
    assert codec.compress_batch([img], bits, p, off) == [gold]
    one = dict(codec.cbatch_info)
    assert codec.compress_batch([img] * 64, bits, p, off) == [gold] * 64
    many = codec.cbatch_info
    assert many["n_launches"] == one["n_launches"] > 0
    assert many["n_blocks"] == 64 * one["n_blocks"] and many["n_load_jobs"] == 64 * one["n_load_jobs"]
    assert codec.stats()["cs_bytes"] == 64 * len(gold)


def _mixed_items(codec):
    """the host test's mixed list with real planes: compress_batch's images, precs and params"""
    grk = _grk()
    descs = mixed_descs()
    g0, b0 = _img("g8_256")
    g6, b6 = _img("rgb8_128x96")
    rng = np.random.default_rng(3)
    small = rng.integers(0, 256, (3, 32, 32)).astype(np.uint8)
    # a uint8 image whose descriptor asks for 12 bits: prepared, as Codec._image returns it
    d, pl, keep = codec._image(small[:1], 8, (0, 0), False)
    d.prec[0] = 12
    sub = codec._image_subsampled([small[0], small[1, :16, :16], small[2, :16, :16]], 8, (32, 32),
                                  [(1, 1), (2, 2), (2, 2)], (0, 0), False)
    imgs = [g0, small[:1], (d, pl, keep), sub, small, rng.integers(0, 256, (3, 64, 64)).astype(np.uint8), g6]
    precs = [b0, 0, 12, 8, 8, 8, b6]
    pars = [q.get("params") for q in descs]
    return imgs, precs, pars


def test_bad_items_do_not_stop_the_others(codec):
    grk = _grk()
    imgs, precs, pars = _mixed_items(codec)
    out = codec.compress_batch(imgs, precs, pars, errors="return")
    assert out[0] == _gold("g8_256") and out[6] == _gold("rgb8_128x96")
    assert codec.cbatch_info["n_ok"] == 2
    codes = [EUNSUPPORTED, EINVAL, EUNSUPPORTED, EUNSUPPORTED, EUNSUPPORTED]
    for i, code in zip(range(1, 6), codes):
        assert isinstance(out[i], grk.GrkGpuError) and ("error %d:" % code) in str(out[i]), (i, out[i])
    assert "precision" in str(out[1])
    with pytest.raises(grk.GrkGpuError, match="item 1: "):
        codec.compress_batch(imgs, precs, pars)
    # the context is as usable as before
    assert codec.compress_batch([imgs[0]], precs[0], pars[0]) == [_gold("g8_256")]


# ---- the job-table load kernel on its own ----

WIDTHS = [1, 3, 4, 5, 257, 63, 64, 65]  # the 257-wide job (several workgroups) between one-workgroup jobs
HEIGHTS = [1, 2, 5]
SHIFTS = [128, 7, 300, -5]
SENTINEL = -0x5A5A5A5B
LOAD_CASES = [("u8", np.uint8, 0, 0), ("i8", np.int8, 0, 0), ("u16", np.uint16, 0, 0), ("i16", np.int16, 0, 0),
              ("i32", np.int32, 0, 0), ("u16be", np.dtype(">u2"), 0, 0),
              ("u8x2", np.uint8, 2, 0), ("u8x3", np.uint8, 3, 0), ("u16x4", np.uint16, 4, 0),
              ("u16bex3", np.dtype(">u2"), 3, 0), ("i32x3", np.int32, 3, 0), ("i16x4", np.int16, 4, 0),
              ("i8x3", np.int8, 3, 0), ("u16bex2", np.dtype(">u2"), 2, 0)]


@pytest.mark.parametrize("case", LOAD_CASES, ids=[c[0] for c in LOAD_CASES])
def test_load_jobs_stage(codec, case):
    """One launch over jobs of every width and height, sources with row stride
    w + 3 (interleaved: w * c + 3) starting at an odd sample offset, destination
    rows w + 5 apart in a sentinel-filled buffer; mct 0 / RCT / ICT, 1 .. 4
    components, a DC shift per component.  Expected: the per-tile stage call
    (grkgpu_dcshift_mct_fwd) job by job, and for RCT / plain shifts numpy."""
    import torch
    grk = _grk()
    _, dt, il_c, _ = case
    dt = np.dtype(dt)
    dev = "cuda:%d" % codec.device
    native = dt.newbyteorder("=")
    fmt = grk._NP_FMT[native] | (grk.SAMPLE_BIG_ENDIAN if dt.byteorder == ">" else 0) | \
        (grk.SAMPLE_INTERLEAVED if il_c else 0)
    sb = dt.itemsize
    lo, hi = (-30000, 30000) if native == np.int32 else (np.iinfo(native).min, np.iinfo(native).max)
    rng = np.random.default_rng(17 + il_c)
    ODD = 1  # first sample of every source, in samples
    jobs, want, raw = [], [], []
    modes = [(0, False), (1, False), (1, True), (0, True)]
    for q, w in enumerate(WIDTHS):
        h = HEIGHTS[q % 3]
        c = il_c if il_c else 1 + q % 4
        mct, irrev = modes[q % 4]
        vals = rng.integers(lo, hi, (c, h, w), endpoint=True).astype(np.int64)
        if il_c:
            stride = w * c + 3
            a = np.zeros((h, stride), dtype=dt)
            a[:, :w * c] = np.transpose(vals, (1, 2, 0)).reshape(h, w * c)
        else:
            stride = w + 3
            a = np.zeros((c, h, stride), dtype=dt)
            a[:, :, :w] = vals
        bytes_ = np.concatenate([np.zeros(ODD * sb, np.uint8), np.frombuffer(a.tobytes(), np.uint8),
                                 np.zeros(16, np.uint8)])
        src = torch.from_numpy(bytes_.copy()).to(dev)
        dst = torch.full((c, h + 2, w + 5), SENTINEL, dtype=torch.int32, device=dev)
        jobs.append(dict(src=src, byte_offset=ODD * sb, dst=dst[:, 1:1 + h], w=w, h=h, shifts=SHIFTS[:c], mct=mct,
                         irreversible=irrev, src_stride=stride))
        raw.append((dst, vals, c, h, w, mct, irrev))
    codec.dcshift_mct_fwd_jobs(jobs, fmt)
    torch.cuda.synchronize()
    for i, (dst, vals, c, h, w, mct, irrev) in enumerate(raw):
        ref = grk.dcshift_mct_fwd(torch.from_numpy(vals.astype(np.int32)).to(dev), SHIFTS[:c], mct, irrev)
        torch.cuda.synchronize()
        exp = torch.full_like(dst, SENTINEL)
        exp[:, 1:1 + h, :w] = ref
        assert torch.equal(dst, exp), (case[0], i, w, h, c, mct, irrev)  # values and the sentinels around them
        if mct and c >= 3 and irrev:
            continue  # ICT: the per-tile kernel is the reference
        v = vals - np.array(SHIFTS[:c], dtype=np.int64)[:, None, None]
        if mct and c >= 3:
            r, g, b = v[0].copy(), v[1].copy(), v[2].copy()
            v[0], v[1], v[2] = (r + 2 * g + b) >> 2, b - g, r - g
        elif irrev:
            v = v << 11
        assert np.array_equal(dst[:, 1:1 + h, :w].cpu().numpy().astype(np.int64), v), (case[0], i)


def test_load_jobs_arguments(codec):
    grk = _grk()
    L = grk.lib()
    assert L.grkgpu_dcshift_mct_fwd_jobs(codec._ctx, None, 0, grk.SAMPLE_U8) == 0
    assert L.grkgpu_dcshift_mct_fwd_jobs(codec._ctx, None, 1, grk.SAMPLE_U8) == EINVAL
    assert L.grkgpu_dcshift_mct_fwd_jobs(None, None, 0, grk.SAMPLE_U8) == EINVAL
    assert L.grkgpu_dcshift_mct_fwd_jobs(codec._ctx, None, 0, grk.SAMPLE_U8 | grk.SAMPLE_BIG_ENDIAN) == EINVAL
    j = (grk.LoadJob * 1)()
    j[0].numcomps = 5
    assert L.grkgpu_dcshift_mct_fwd_jobs(codec._ctx, j, 1, grk.SAMPLE_U8) == EINVAL


# ---- dirty buffers, neighbours, round trip ----

SMALL = ["g8_64", "g8_3x5", "g8_1x37", "g8_45x1", "rgb8_I", "g8_M4_termall", "rgb8_M62_I_r", "g12_M63", "rgb12_96x80",
         "g8_off35"]


def test_dirty_scratch_and_neighbours():
    grk = _grk()
    codec = grk.Codec(0)
    try:
        big, bits = _img("rgb12_cinema4k")
        p, off = grk.CParams.from_cli(MAN["rgb12_cinema4k"]["args"])
        assert codec.compress(big, bits, p, offset=off) == _gold("rgb12_cinema4k")
        codec.debug_fill(0xA5)
        imgs, precs, pars, offs = _batch_args(SMALL)
        first = codec.compress_batch(imgs, precs, pars, offs)
        for n, b in zip(SMALL, first):
            assert b == _gold(n), n
        codec.debug_fill(0xA5)
        for n in ("rgb12_96x80", "g12_M63"):  # lossless: the decode is the image
            i = SMALL.index(n)
            assert codec.compress(imgs[i], precs[i], pars[i], offset=offs[i]) == _gold(n)
            assert np.array_equal(codec.decompress(_gold(n)), imgs[i])
        assert codec.compress_batch(imgs, precs, pars, offs) == first
    finally:
        codec.close()


def test_roundtrip_through_batch_decode(codec, all_goldens):
    imgs, precs, pars, offs, out, info, stats = all_goldens
    lossless = [i for i, n in enumerate(NAMES) if MAN[n].get("dec_vs_src_maxabs") == 0 and "-I" not in MAN[n]["args"]]
    assert len(lossless) > 20
    dec = codec.decompress_batch([out[i] for i in lossless])
    for i, d in zip(lossless, dec):
        assert np.array_equal(d, imgs[i]), NAMES[i]
