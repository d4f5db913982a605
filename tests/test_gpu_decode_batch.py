"""Batch decode (Codec.decompress_batch / grkgpu_decompress_batch): a list of
codestreams through one launch set -- merged DecBlock / DecSeg tables, one
DwtPlan per wavelet, the last store from a job table (k_store_jobs).

Oracles: the reference's committed decodes (tests/golden/<case>.dec.npy and
their .r<N> / .l<N> variants), the manifests' decode hashes, or the
single-image call on the same stream, which the rest of the suite pins to the
reference.  Tolerance 0 everywhere.
"""
import functools
import hashlib
import json
import os

import numpy as np
import pytest

import synth
from conftest import GOLD, load_manifest
from test_decode_batch_host import mixed_list

pytestmark = pytest.mark.gpu
MAN = load_manifest()
NAMES = sorted(MAN)


def _grk():
    import grokimagecompression_amd as grk
    return grk


@functools.lru_cache(maxsize=None)
def gold(name):
    return open(f"{GOLD}/{name}.j2k", "rb").read()


@functools.lru_cache(maxsize=None)
def ref(name, tag=""):
    a = np.load(f"{GOLD}/{name}{'.' + tag if tag else ''}.dec.npy")
    a.setflags(write=False)
    return a


def to_numpy(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy()


def as_layout(a, layout):
    return a if layout == "chw" else np.transpose(a, (1, 2, 0))


def check_all(outs, names, tag=""):
    for n, o in zip(names, outs):
        r = ref(n, tag)
        o = to_numpy(o)
        assert o.shape == r.shape and o.dtype == np.int32, (n, o.shape, r.shape)
        if not np.array_equal(o, r):
            bad = np.argwhere(o != r)
            pytest.fail("item %d (%s): %d samples differ, first at (c, y, x) = %s"
                        % (names.index(n), n, len(bad), tuple(bad[0])))


def test_all_goldens_one_call(codec):
    """The 88 streams of the manifest as one batch, and reversed: the merged
    tables (data_off and arena offsets rebased per item) over every geometry,
    code-block size, wavelet, component count, precision and marker the
    fixtures hold."""
    assert len(NAMES) == 88
    outs = codec.decompress_batch([gold(n) for n in NAMES])
    info = dict(codec.batch_info)
    assert info["n_ok"] == 88 and info["n_blocks"] == codec.stats()["num_cblks"]
    assert codec.stats()["cs_bytes"] == sum(len(gold(n)) for n in NAMES)
    check_all(outs, NAMES)
    rev = NAMES[::-1]
    outs2 = codec.decompress_batch([gold(n) for n in rev])
    check_all(outs2, rev)
    assert codec.batch_info["n_blocks"] == info["n_blocks"]
    assert codec.batch_info["n_store_jobs"] == info["n_store_jobs"]


@pytest.mark.parametrize("layout", ["chw", "hwc"])
@pytest.mark.parametrize("dev", [False, True])
def test_formats(codec, layout, dev):
    """uint8 over the streams of <= 8 bits and uint16 over all of them: the int32 result, cast."""
    for dt, names in ((np.uint8, [n for n in NAMES if MAN[n]["shape"][3] <= 8]), (np.uint16, NAMES)):
        outs = codec.decompress_batch([gold(n) for n in names], dtype=dt, layout=layout, device_out=dev)
        for n, o in zip(names, outs):
            assert (not isinstance(o, np.ndarray)) == dev
            o = to_numpy(o)
            assert o.dtype == dt
            assert np.array_equal(o, as_layout(ref(n), layout).astype(dt)), (n, dt, layout, dev)


def test_mixed_formats_in_one_batch(codec):
    """Items asking for different formats, layouts and destinations: each its single call's result."""
    names = ["g8_100x77", "rgb8_128x96", "rgb12_I", "g8_off_tiles", "rgb8_I", "g16_I", "g8_1x37", "rgb12_96x80"]
    dts = [None, np.uint8, np.uint16, np.int32, np.uint8, np.uint16, np.uint8, np.int32]
    lays = ["chw", "hwc", "chw", "hwc", "chw", "hwc", "hwc", "hwc"]
    devs = [False, True, True, False, False, False, True, True]
    outs = codec.decompress_batch([gold(n) for n in names], dtype=dts, layout=lays, device_out=devs)
    assert codec.batch_info["n_ok"] == len(names)
    for n, dt, lay, dev, o in zip(names, dts, lays, devs, outs):
        single = codec.decompress(gold(n), dtype=dt, layout=lay, device_out=dev)
        assert type(o) is type(single) and o.dtype == single.dtype
        assert np.array_equal(to_numpy(o), to_numpy(single)), (n, dt, lay, dev)
        assert np.array_equal(to_numpy(o), as_layout(ref(n), lay)), n


def _store_jobs(rng, T, layout, ncomp, mct, irrev, widths, heights, odd):
    """Jobs over random planes, one per (w, h): (job dict, guard-extended destination)."""
    import torch
    prec, sgnd, tdt = {np.uint8: (8, False, torch.uint8), np.int8: (8, True, torch.int8),
                       np.uint16: (12, False, torch.uint16), np.int16: (12, True, torch.int16),
                       np.int32: (16, True, torch.int32)}[T]
    jobs = []
    for w in widths:
        for h in heights:
            stride = w + 3
            lim = 3 << (prec - 1)  # past the component's range on both sides: the clamp works
            a = rng.integers(-lim, lim, size=(ncomp, h, stride))
            src = (a.astype(np.float32) * 0.75).view(np.int32) if irrev else a.astype(np.int32)
            src = torch.from_numpy(np.ascontiguousarray(src)).cuda()
            il = layout == "hwc"
            row = w * ncomp if il else w
            dstride = row + (3 if odd else 0)  # rows that start at odd byte / sample offsets
            need = (h - 1) * dstride + row if il else (ncomp * h - 1) * dstride + row
            off = 1 if odd else 0
            jobs.append(dict(src=src, w=w, prec=prec, sgnd=sgnd, mct=mct, irreversible=irrev, dst_stride=dstride,
                             need=need, off=off, tdt=tdt))
    return jobs


def _run_store_jobs(jobs, layout):
    """The table call against mct_inv_dcshift_to per job, guards around every destination."""
    import torch
    grk = _grk()
    a, b = [], []
    for q in jobs:
        for lst in (a, b):
            buf = torch.full((q["need"] + q["off"] + 7,), 0x5A, dtype=q["tdt"], device="cuda")
            lst.append(buf)
    keys = ("src", "w", "prec", "sgnd", "mct", "irreversible", "dst_stride")
    table = [dict({k: q[k] for k in keys}, dst=buf[q["off"]:q["off"] + q["need"]]) for q, buf in zip(jobs, a)]
    grk.mct_inv_dcshift_jobs_to(table, layout=layout)
    for q, buf in zip(jobs, b):
        grk.mct_inv_dcshift_to(q["src"], buf[q["off"]:q["off"] + q["need"]], q["w"], q["prec"], q["sgnd"], q["mct"],
                               q["irreversible"], layout=layout, dst_stride=q["dst_stride"])
    torch.cuda.synchronize()
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), ("job %d of %d" % (i, len(jobs)), jobs[i]["w"], jobs[i]["src"].shape)


@pytest.mark.parametrize("T", [np.uint8, np.int8, np.uint16, np.int16, np.int32])
@pytest.mark.parametrize("layout", ["chw", "hwc"])
def test_store_jobs_edges(T, layout):
    """k_store_jobs through the stage call: widths around the type's run
    length N = 16 / sizeof(T) and around a workgroup's 256 threads, heights 1
    and 5, odd destination offsets, 1 / 3 (with and without MCT, 5/3 and 9/7)
    / 4 components (and 2, the thread-per-pixel path); the first and last job
    of a table are jobs like the others, checked with their guards."""
    rng = np.random.default_rng(5)
    N = 16 // np.dtype(T).itemsize
    widths = sorted({1, 2, N - 1, N, N + 1, 255, 256, 257})
    for ncomp, mct, irrev in ((1, 0, False), (1, 0, True), (3, 0, False), (3, 1, False), (3, 0, True), (3, 1, True),
                              (4, 1, False), (4, 0, True), (2, 0, False)):
        jobs = _store_jobs(rng, T, layout, ncomp, mct, irrev, widths, (1, 5), odd=True)
        _run_store_jobs(jobs, layout)


def test_store_jobs_table_shapes():
    """A table of one job; 300 jobs of 1x1 (more jobs than a workgroup has
    threads, a workgroup each); jobs of different component counts in one
    table; an empty job between two others."""
    rng = np.random.default_rng(6)
    for layout in ("chw", "hwc"):
        _run_store_jobs(_store_jobs(rng, np.uint8, layout, 3, 1, False, (37,), (3,), odd=True), layout)
        _run_store_jobs(_store_jobs(rng, np.uint16, layout, 3, 1, True, (1,) * 300, (1,), odd=False), layout)
        mixed = (_store_jobs(rng, np.uint8, layout, 1, 0, False, (300,), (2,), odd=True) +
                 _store_jobs(rng, np.uint8, layout, 4, 1, False, (17,), (4,), odd=True) +
                 _store_jobs(rng, np.uint8, layout, 3, 0, True, (16,), (1,), odd=False))
        _run_store_jobs(mixed, layout)
    import torch
    grk = _grk()
    jobs = _store_jobs(rng, np.uint8, "chw", 1, 0, False, (9, 9, 9), (2,), odd=False)
    dsts = [torch.full((q["need"],), 0x5A, dtype=q["tdt"], device="cuda") for q in jobs]
    arr = (grk.StoreJob * 3)()
    for j, q, d in zip(arr, jobs, dsts):
        j.src[0], j.dst[0] = q["src"][0].data_ptr(), d.data_ptr()
        j.src_stride, j.dst_stride, j.w, j.h, j.numcomps = q["src"].shape[2], q["dst_stride"], q["w"], 2, 1
        j.shift[0], j.min[0], j.max[0] = 128, 0, 255
    arr[1].w = 0
    grk._check(grk.lib().grkgpu_mct_inv_dcshift_jobs_to(arr, 3, grk.SAMPLE_U8, 0, None))
    torch.cuda.synchronize()
    assert bool((dsts[1] == 0x5A).all()) and not bool((dsts[0] == 0x5A).all()) and not bool((dsts[2] == 0x5A).all())


TINY = json.load(open(f"{GOLD}/manifest_tiny.json"))
TINY_SMALL = ["t_g16_65_n1_M4", "t_g16u_65_n1_M36", "t_g16_65_n1_M5", "t_rgb16_129_n1_M12", "t_g16_98_b16_n2_M4"]
STYLE_GOLDENS = ["g8_M1_lazy", "g8_M2_reset", "g8_M4_termall", "g8_M8_vsc", "g8_M16_pterm", "g8_M32_segsym",
                 "g8_M20_termall_pterm", "g12_M63"]


def test_code_block_styles_across_items(codec):
    """One Tier-1 launch per style over blocks of different items: the small
    TERMALL / SEGSYM / BYPASS / VSC cases of manifest_tiny.json (streams
    encoded here and pinned by their hash; the reference's decode by its
    hash), the single-style goldens (BYPASS, RESET, TERMALL, VSC, PTERM,
    SEGSYM, two combinations) and mk_mixed_cblksty, interleaved."""
    grk = _grk()
    streams, want = [], []
    for n in TINY_SMALL:
        m = TINY[n]
        h, w, c, bits = m["shape"]
        p, off = grk.CParams.from_cli(m["args"])
        b = codec.compress(synth.synth_image(h, w, c, bits, m["seed"], m["kind"]), bits, p, offset=off)
        assert hashlib.sha256(b).hexdigest() == m["j2k_sha256"], n
        streams.append(b)
        want.append(m["dec_sha256"])
    for n in STYLE_GOLDENS + ["mk_mixed_cblksty"]:
        streams.append(gold(n))
        want.append(synth.image_sha256(ref(n)))
    order = np.random.default_rng(3).permutation(len(streams))
    outs = codec.decompress_batch([streams[i] for i in order])
    for i, o in zip(order, outs):
        assert synth.image_sha256(o) == want[i], "stream %d" % i
    styles = {int(TINY[n]["args"][TINY[n]["args"].index("-M") + 1]) for n in TINY_SMALL}
    assert len(styles) >= 4  # the merged table holds more than one launch range


def _variants(kind):
    """{N: [names]} of the goldens with a .<kind><N>.dec.npy fixture"""
    res = {}
    for f in sorted(os.listdir(GOLD)):
        parts = f.split(".")
        if f.endswith(".dec.npy") and len(parts) == 4 and parts[1][0] == kind and parts[1][1:].isdigit() and \
                os.path.exists(f"{GOLD}/{parts[0]}.j2k"):
            res.setdefault(int(parts[1][1:]), []).append(parts[0])
    return res


def test_reduce(codec):
    """reduce = N over every golden with an .r<N> fixture, g8_off35 and g8_off_tiles at reduce = 1 among
    them (against the single call: the zero margin of a reduced decode at an odd origin)."""
    var = _variants("r")
    assert {1, 2, 3} <= set(var)
    for N, names in var.items():
        outs = codec.decompress_batch([gold(n) for n in names], reduce=N)
        check_all(outs, names, "r%d" % N)
    names = ["g8_off35", "g8_off_tiles", "rgb8_128x96"]
    outs = codec.decompress_batch([gold(n) for n in names], reduce=1, dtype=np.uint8)
    for n, o in zip(names, outs):
        single = codec.decompress(gold(n), reduce=1)
        assert np.array_equal(o, single.astype(np.uint8)) and o.shape == single.shape, n
    assert not outs[0][:, -1, :].any() and not outs[0][:, :, -1].any()  # the margin
    assert hashlib.sha256(np.ascontiguousarray(outs[2], dtype=np.int32).tobytes()).hexdigest() == \
        MAN["rgb8_128x96"]["variants"]["r1"]["dec_sha256"]


def test_layers(codec):
    var = _variants("l")
    assert {1, 2} <= set(var)
    for N, names in var.items():
        outs = codec.decompress_batch([gold(n) for n in names], layers=N)
        check_all(outs, names, "l%d" % N)


def test_failing_items_among_good_ones(codec):
    grk = _grk()
    bufs = mixed_list()
    plan = grk.plan_batch(bufs)
    outs_in = []
    for b, st, d in zip(bufs, plan["status"], plan["img"]):
        ok_hdr = st == 0 or (d.numcomps and all(d.dx[k] == 1 and d.dy[k] == 1 for k in range(d.numcomps)))
        shape = (d.numcomps, d.y1 - d.y0, d.x1 - d.x0) if ok_hdr and d.numcomps else (1, 8, 8)
        outs_in.append(np.full(shape, 0x5A5A5A5A, dtype=np.int32))
    with pytest.raises(grk.GrkGpuError, match="item 1: "):
        codec.decompress_batch(bufs, out=[o.copy() for o in outs_in])
    outs = codec.decompress_batch(bufs, out=outs_in, errors="return")
    assert codec.batch_info["n_ok"] == 2
    assert outs[0] is outs_in[0] and np.array_equal(outs[0], ref("g8_256"))
    assert outs[6] is outs_in[6] and np.array_equal(outs[6], ref("rgb8_128x96"))
    for i in range(1, 6):
        assert isinstance(outs[i], grk.GrkGpuError) and ("%d" % plan["status"][i]) in str(outs[i]), i
        assert (outs_in[i] == 0x5A5A5A5A).all(), i
    # device destinations are left alone too
    import torch
    dev = [torch.from_numpy(o.copy()).cuda() if i in (0, 3) else None for i, o in enumerate(outs_in)]
    dev[0].fill_(0x5A5A5A5A)
    outs = codec.decompress_batch(bufs, out=dev, errors="return")
    assert np.array_equal(outs[0].cpu().numpy(), ref("g8_256")) and bool((dev[3] == 0x5A5A5A5A).all())
    assert np.array_equal(outs[6], ref("rgb8_128x96"))
    # the codec keeps working
    assert np.array_equal(codec.decompress(gold("g8_64")), ref("g8_64"))


def test_cut_stream_as_an_item(codec):
    """A multi-tile prefix the reference decodes with tiles missing, between two whole streams."""
    cuts = json.load(open(f"{GOLD}/manifest_cut.json"))["g8_tiles64"]["cuts"]
    n = min(int(k) for k, v in cuts.items() if v != "error" and len(v["tiles"]) == 2)
    cs = gold("g8_tiles64")[:n]
    single = codec.decompress(cs)
    assert single.any() and not single[:, -8:, -8:].any()
    for dt in (None, np.uint8):
        outs = codec.decompress_batch([gold("rgb8_128x96"), cs, gold("g8_256")], dtype=dt)
        assert np.array_equal(outs[1], single)
        assert synth.image_sha256(outs[1]) == cuts[str(n)]["sha"]
        assert np.array_equal(outs[0], ref("rgb8_128x96")) and np.array_equal(outs[2], ref("g8_256"))


def test_one_launch_set(codec):
    one = codec.decompress_batch([gold("g8_256")])
    i1 = dict(codec.batch_info)
    many = codec.decompress_batch([gold("g8_256")] * 64)
    i64 = dict(codec.batch_info)
    assert i1["n_launches"] > 0 and i64["n_launches"] == i1["n_launches"], (i1, i64)
    assert i64["n_blocks"] == 64 * i1["n_blocks"] and i64["n_store_jobs"] == 64 * i1["n_store_jobs"]
    assert i64["n_ok"] == 64
    for o in many + one:
        assert np.array_equal(o, ref("g8_256"))


def test_stack(codec):
    r = np.transpose(ref("rgb8_128x96"), (1, 2, 0)).astype(np.uint8)
    for dev in (False, True):
        out = codec.decompress_batch([gold("rgb8_128x96")] * 32, dtype=np.uint8, layout="hwc", stack=True,
                                     device_out=dev)
        out = to_numpy(out)
        assert out.shape == (32, 96, 128, 3) and out.dtype == np.uint8
        for i in range(32):
            assert np.array_equal(out[i], r), i
    with pytest.raises(_grk().GrkGpuError, match="one shape"):
        codec.decompress_batch([gold("rgb8_128x96"), gold("g8_64")], stack=True)


def test_dirty_state():
    """On a context whose every buffer holds 0xA5, and after an unrelated
    encode on it, the batch gives the goldens; a single decode right after a
    batch gives its golden."""
    grk = _grk()
    c = grk.Codec(0)
    try:
        bufs = [gold(n) for n in NAMES]
        check_all(c.decompress_batch(bufs), NAMES)
        assert c.debug_fill(0xA5) > 0
        check_all(c.decompress_batch(bufs), NAMES)
        img = synth.synth_image(200, 300, 3, 12, 7)
        c.compress(img, 12, grk.CParams.make(irreversible=True))
        check_all(c.decompress_batch(bufs, dtype=np.int32), NAMES)
        assert np.array_equal(c.decompress(gold("rgb12_I")), ref("rgb12_I"))
        c.debug_fill(0xA5)
        outs = c.decompress_batch([gold("g8_off35"), gold("g8_off_tiles")], reduce=1, dtype=np.uint8, layout="hwc")
        for n, o in zip(("g8_off35", "g8_off_tiles"), outs):
            assert np.array_equal(o, np.transpose(c.decompress(gold(n), reduce=1), (1, 2, 0)).astype(np.uint8))
    finally:
        c.close()
