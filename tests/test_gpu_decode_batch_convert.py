"""Batch decode with the converting / upsampling last store
(grkgpu_decompress_batch_convert, Codec.decompress_batch_convert,
grk.convert_jobs_to).

The table kernels through the stage call: every job against the numpy closed
forms of tests/test_gpu_decode_convert.py / colour_fixtures.py (upsample,
sycc_to_rgb, eycc_to_rgb, cmyk_to_rgb, to_prec), the inverse MCT taken from
grk.mct_inv_dcshift_to, and -- where a job fits its model -- against
grk.convert_to, with sentinel guard bands around every destination.  End to
end: every item of a batch equals the single Codec.decompress call with the
same arguments, bit for bit."""
import json

import numpy as np
import pytest

from colour_fixtures import cmyk_to_rgb, eycc_to_rgb
from conftest import GOLD
from test_gpu_decode_convert import _seam_stream, convert, narrowest, sycc_to_rgb, to_prec
from test_gpu_decode_upsample import SUB, gold, to_numpy

pytestmark = pytest.mark.gpu

S420, S422 = [(1, 1), (2, 2), (2, 2)], [(1, 1), (2, 1), (2, 1)]
S124, S32, S111, S1111 = [(1, 1), (2, 2), (4, 4)], [(3, 2)], [(1, 1)] * 3, [(1, 1)] * 4
cd = lambda a, b: -(-a // b)  # noqa: E731


def _grk_torch():
    import torch
    import grokimagecompression_amd as grk
    return grk, torch


# ---------------------------------------------------------------------------
# the stage call
# ---------------------------------------------------------------------------
def _comp(rng, torch, dx, dy, rect, prec, raw, irrev=False, extra=0, null=False):
    """One component of a job and its finished samples (None: a null source).
    The lead-in starts at ceil(origin / d); `extra` columns / rows of real
    samples lie before it in the source (they must not be read as such)."""
    x0, y0, x1, y1 = rect
    zx0, zy0 = cd(x0, dx), cd(y0, dy)
    gx0, gy0 = max(zx0 - extra, 0), max(zy0 - extra, 0)
    cols, rows = max((x1 - 1) // dx - gx0 + 1, 1), max((y1 - 1) // dy - gy0 + 1, 1)
    stride, half, top = cols + 3, 1 << (prec - 1), (1 << prec) - 1
    if raw and irrev:
        a = rng.uniform(-half - 20, half + 20, (rows, stride)).astype(np.float32)
        fin = np.clip(np.rint(a).astype(np.int64) + half, 0, top)
        a = a.view(np.int32)
    elif raw:
        a = rng.integers(-half - 20, half + 20, (rows, stride)).astype(np.int32)
        fin = np.clip(a.astype(np.int64) + half, 0, top)
    else:
        a = rng.integers(0, top + 1, (rows, stride)).astype(narrowest(prec))
        fin = a.astype(np.int64)
    spec = dict(src=None if null else torch.from_numpy(a).cuda(), prec=prec, sgnd=False, dx=dx, dy=dy,
                origin=(gx0, gy0), lead=(zx0, zy0), raw=raw, irreversible=irrev, dtype=a.dtype)
    return spec, (None if null else fin)


def _ref_planes(rect, comps):
    """the rectangle's pixels from each component's finished samples, zero in the lead-in"""
    x0, y0, x1, y1 = rect
    X, Y = np.arange(x0, x1), np.arange(y0, y1)
    out = []
    for spec, fin in comps:
        col, row = X // spec["dx"], Y // spec["dy"]
        if fin is None:
            out.append(np.zeros((len(Y), len(X)), np.int64))
            continue
        (gx0, gy0), (zx0, zy0) = spec["origin"], spec["lead"]
        v = fin[np.clip(row - gy0, 0, None)[:, None], np.clip(col - gx0, 0, None)[None, :]]
        out.append(np.where((row >= zy0)[:, None] & (col >= zx0)[None, :], v, 0))
    return out


def _ops_ref(planes, precs, colour, out_prec, prec_mode):
    """precision(colour(planes)): the output channels"""
    q = list(precs)
    if colour in (None, "sycc"):  # (planes already on the pixel grid: no upsampling left to do)
        return convert(planes, None, None, q, False, colour, out_prec, prec_mode, up=False)
    if colour == "eycc":
        planes = [p.astype(np.int64) for p in eycc_to_rgb(planes[0], planes[1], planes[2], q[0])]
    elif colour == "cmyk":
        planes = [p.astype(np.int64) for p in cmyk_to_rgb(planes, q)]
        q = [8, 8, 8] + q[4:]
    return [to_prec(p, q[k], False, out_prec, prec_mode) for k, p in enumerate(planes)]


def _job(rng, torch, T, il, rect, subs, precs, raws, colour=None, out_prec=None, prec_mode="clip", mct=0, irrev=False,
         extra=0, null=(), off=0, pad=0):
    """A job of grk.convert_jobs_to with its expected samples and its guarded destination."""
    grk, _ = _grk_torch()
    x0, y0, x1, y1 = rect
    w, h = max(x1 - x0, 0), max(y1 - y0, 0)
    precs = [precs] * len(subs) if np.isscalar(precs) else list(precs)
    raws = [raws] * len(subs) if isinstance(raws, bool) else list(raws)
    if mct:  # raw sources on one grid in one buffer, as the tile buffers of a decode lie
        half = 1 << (precs[0] - 1)
        stride = w + 3
        if irrev:
            a = rng.uniform(-half, half, (len(subs), h, stride)).astype(np.float32).view(np.int32)
        else:
            a = rng.integers(-half, half, (len(subs), h, stride)).astype(np.int32)
        src = torch.from_numpy(a).cuda()
        fin = torch.empty(len(subs) * h * w, dtype=torch.int32, device="cuda")
        grk.mct_inv_dcshift_to(src, fin, w, precs[0], False, 1, irrev, layout="chw")
        fin = fin.cpu().numpy().reshape(len(subs), h, w).astype(np.int64)
        comps = [(dict(src=src[k], prec=precs[k], sgnd=False, dx=1, dy=1, origin=(x0, y0), lead=(x0, y0), raw=True,
                       irreversible=irrev), None) for k in range(len(subs))]
        planes = list(fin)
    else:
        comps = [_comp(rng, torch, dx, dy, rect, precs[k], raws[k], irrev and raws[k], extra if (dx, dy) != (1, 1) else 0,
                       k in null) for k, (dx, dy) in enumerate(subs)]
        planes = _ref_planes(rect, comps)
    exp = np.stack(_ops_ref(planes, precs, colour, out_prec, prec_mode)) if w and h else np.zeros((len(subs), 0, 0))
    no = exp.shape[0]
    info = np.iinfo(T)
    assert not exp.size or (info.min <= exp.min() and exp.max() <= info.max)
    exp = exp.astype(T)
    if il:
        exp = exp.transpose(1, 2, 0)
    row = (no * w if il else w) + pad
    rows = h if il else no * h
    base = torch.from_numpy(np.full(off + rows * row + 16, 0x5A, dtype=T)).cuda()
    q = dict(rect=rect, comps=[s for s, _ in comps], dst=base[off:off + max(rows * row, 0)], dst_stride=row, mct=mct,
             colour=colour, out_prec=out_prec, prec_mode=prec_mode)
    # the same job through grk.convert_to, where it fits that call's model:
    # finished sources of one dtype from ceil(origin / d) on, none null
    alt = None
    if w and h and not mct and not any(raws) and not null and not extra and len({s["dtype"] for s, _ in comps}) == 1:
        alt = torch.from_numpy(np.full(off + rows * row + 16, 0x5A, dtype=T)).cuda()
    return dict(q=q, base=base, exp=exp, off=off, row=row, rows=rows, pad=pad, alt=alt, subs=subs, precs=precs,
                what=(rect, subs, colour, out_prec, prec_mode, mct, irrev, raws, null, off, pad))


def _run(jobs, layout):
    grk, torch = _grk_torch()
    grk.convert_jobs_to([j["q"] for j in jobs], layout=layout)
    for j in jobs:
        if j["alt"] is not None:
            q = j["q"]
            x0, y0, x1, y1 = q["rect"]
            grk.convert_to([u["src"][:cd(y1, u["dy"]) - cd(y0, u["dy"]), :cd(x1, u["dx"]) - cd(x0, u["dx"])]
                            for u in q["comps"]], j["alt"][j["off"]:], q["rect"],
                           j["subs"], j["precs"], False, layout=layout, dst_stride=j["row"], colour=q["colour"],
                           out_prec=q["out_prec"], prec_mode=q["prec_mode"])
    torch.cuda.synchronize()
    for i, j in enumerate(jobs):
        got = j["base"].cpu().numpy()
        off, row, rows, pad = j["off"], j["row"], j["rows"], j["pad"]
        body = got[off:off + rows * row].reshape(rows, row)
        where = ("job %d of %d" % (i, len(jobs)),) + j["what"]
        assert np.array_equal(body[:, :row - pad].reshape(j["exp"].shape), j["exp"]), where
        assert (body[:, row - pad:] == 0x5A).all() and (got[:off] == 0x5A).all(), where
        assert (got[off + rows * row:] == 0x5A).all(), where
        if j["alt"] is not None:
            assert torch.equal(j["alt"], j["base"]), where


@pytest.mark.parametrize("T", [np.uint8, np.uint16, np.int32])
@pytest.mark.parametrize("layout", ["chw", "hwc"])
def test_convert_jobs_table(T, layout):
    """One table per sample format and layout that mixes every shape, so the
    workgroup-to-job search sees a first job, a last job and empty ones
    between: widths 1, N - 1, N, N + 1, 2N + 1 around the run length N = 16 /
    sizeof(T), heights 1, 2, 3, 5, odd destination offsets, even and odd x0,
    origins that are no multiple of dx / dy (the zero lead-in, with real
    samples lying before it), w = 0, null sources, jobs of more than 256
    threads, raw and finished sources in one job; 4:2:0 / 4:2:2 in the run
    shape, (1,1)/(2,2)/(4,4) and (3,2) per pixel, one-grid jobs with RCT / ICT
    and the scale-down to 8 bits, sYCC, eYCC and four-component CMYK."""
    grk, torch = _grk_torch()
    rng = np.random.default_rng(11)
    il = layout == "hwc"
    N = 16 // np.dtype(T).itemsize
    P = 8 if T == np.uint8 else 12  # the precision of samples stored as they are
    widths, heights = [1, N - 1, N, N + 1, 2 * N + 1], [1, 2, 3, 5]
    jobs = []

    def add(rect, subs, precs, raws, **kw):
        jobs.append(_job(rng, torch, T, il, rect, subs, precs, raws, off=kw.pop("off", len(jobs) % 4),
                         pad=kw.pop("pad", len(jobs) % 3), **kw))
    n = 0
    for subs in (S420, S422):
        for w in widths:
            for h in heights:
                x0, y0 = 6 + (n & 1), 4 + ((n >> 1) & 1) * 3  # even / odd: chroma parity and the lead-in
                raws = [(True, True, True), (False, False, False), (True, False, False), (False, True, True)][n % 4]
                ops = [dict(), dict(colour="sycc"), dict(out_prec=8, prec_mode="scale", precs=12),
                       dict(colour="sycc", out_prec=8, prec_mode="scale", precs=12)][(n // 4) % 4]
                add((x0, y0, x0 + w, y0 + h), subs, ops.pop("precs", P), raws, irrev=bool(n & 8), extra=(n // 2) % 2,
                    null=(1,) if n % 7 == 3 else (), **ops)
                n += 1
    add((5, 5, 5, 9), S420, P, False)  # w = 0: nothing stored
    for subs in (S124, S32):
        for w in (1, N + 1, 33):
            for h in (1, 5, 9):
                raws = (n % 2 == 0,) + (n % 3 == 0,) * (len(subs) - 1)
                add((7 + (n & 1), 5 + (n & 2), 7 + (n & 1) + w, 5 + (n & 2) + h), subs, P, raws, extra=(n // 2) % 2,
                    **(dict(out_prec=4, prec_mode="scale") if n % 2 else {}))
                n += 1
    add((9, 9, 9 + 33, 9), S124, P, True)  # h = 0
    for w in widths + [40 * N]:
        h = 8 if w == 40 * N else heights[n % 4]
        for irrev in (False, True):  # RCT and ICT on one grid, 12 bits scaled down to 8
            add((3, 2, 3 + w, 2 + h), S111, 12, True, mct=1, irrev=irrev, out_prec=8, prec_mode="scale")
        add((3, 2, 3 + w, 2 + h), S111, P, True, colour="sycc")                      # the store on one grid ...
        add((3, 2, 3 + w, 2 + h), S111, P, True, mct=1, colour="eycc")
        add((3, 2, 3 + w, 2 + h), S1111, 8, True, colour="cmyk")
        add((3, 2, 3 + w, 2 + h), S111, P, False, colour="eycc")                     # ... and the per-pixel one
        add((3, 2, 3 + w, 2 + h), S1111, 8, (True, False, False, True), colour="cmyk")
        add((3, 2, 3 + w, 2 + h), [(1, 1), (1, 1)], P, True, out_prec=4, prec_mode="clip")
        add((3, 2, 3 + w, 2 + h), S111, P, True, null=(0, 1, 2), colour="sycc")       # converted zeros
        n += 1
    add((0, 0, 40 * N, 8), S420, P, (True, False, False), colour="sycc")  # more than 256 threads, in the run shape
    add((1, 1, 34, 10), S124, P, True)                                     # ... and per pixel, the table's last job
    _run(jobs, layout)


@pytest.mark.parametrize("T", [np.int8, np.int16])
@pytest.mark.parametrize("layout", ["chw", "hwc"])
def test_convert_jobs_signed_one_grid(T, layout):
    """Signed raw sources on one grid with a precision op -- the job kernel's
    int8 / int16 stores with ops -- against grk.convert_to on the same int32
    planes (a signed component has no DC shift, so its raw samples are its
    finished ones; both clamp to the component's range first): 1 .. 4
    components of 12 bits, scaled and clipped to the output precision, widths
    1, N - 1, N, N + 1 around the run length N = 16 / sizeof(T), heights 1 and
    3, destinations at odd offsets with padded rows, guards around them."""
    grk, torch = _grk_torch()
    rng = np.random.default_rng(13)
    il = layout == "hwc"
    N = 16 // np.dtype(T).itemsize
    half = 1 << 11
    jobs, alts = [], []
    for nc in (1, 2, 3, 4):
        for w in (1, N - 1, N, N + 1):
            for h in (1, 3):
                n = len(jobs)
                out_prec, mode = (8 if T == np.int8 else (16, 10)[n % 2]), ("scale", "clip")[(n // 2) % 2]
                x0, y0, off, pad = 3 + (n & 1), 2, n % 4, n % 3
                src = torch.from_numpy(rng.integers(-half - 20, half + 20, (nc, h, w + 3)).astype(np.int32)).cuda()
                row = (nc * w if il else w) + pad
                size = off + (h if il else nc * h) * row + 16
                base, alt = (torch.from_numpy(np.full(size, 0x5A, dtype=T)).cuda() for _ in range(2))
                comps = [dict(src=src[k], prec=12, sgnd=True, dx=1, dy=1, origin=(x0, y0), raw=True) for k in range(nc)]
                jobs.append(dict(rect=(x0, y0, x0 + w, y0 + h), comps=comps, dst=base[off:], dst_stride=row,
                                 out_prec=out_prec, prec_mode=mode))
                grk.convert_to([src[k][:, :w] for k in range(nc)], alt[off:], (x0, y0, x0 + w, y0 + h), [(1, 1)] * nc, 12,
                               True, layout=layout, dst_stride=row, out_prec=out_prec, prec_mode=mode)
                alts.append((base, alt, (nc, w, h, out_prec, mode, off, pad)))
    grk.convert_jobs_to(jobs, layout=layout)
    torch.cuda.synchronize()
    for base, alt, what in alts:
        assert not bool((alt == 0x5A).all()), what  # (the reference call stored something)
        assert torch.equal(base, alt), what


def test_convert_jobs_refusals():
    grk, torch = _grk_torch()
    rng = np.random.default_rng(12)
    ok = _job(rng, torch, np.uint8, False, (0, 0, 8, 2), S420, 8, False)["q"]
    assert grk.convert_jobs_to([], layout="chw") == []
    for bad, msg in ((dict(mct=1), "MCT"), (dict(colour="eycc"), "one grid"), (dict(out_prec=9), "does not hold")):
        with pytest.raises(grk.GrkGpuError, match="grkgpu error -1:.*" + msg):
            grk.convert_jobs_to([ok, dict(ok, **bad)])
    j = grk.ConvertJob()
    j.numcomps, j.ops.colour = 1, grk.COLOUR_FORCE_RGB
    assert grk.lib().grkgpu_convert_jobs_to(j, 1, 1, 0, None) == -4


# ---------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------
def _same(got, ref, what):
    if isinstance(ref, list):
        assert isinstance(got, list) and len(got) == len(ref), what
        for g, r in zip(got, ref):
            assert g.dtype == r.dtype and np.array_equal(g, r), what
        return
    g = to_numpy(got)
    assert g.dtype == ref.dtype and g.shape == ref.shape and np.array_equal(g, ref), what


def _cut(cs):
    """cs cut where the walk still reaches some of its tiles, not all"""
    import grokimagecompression_amd as grk
    full = len(grk.walk_tiles(cs))
    for num in (5, 4, 6, 3, 7):
        try:
            if 0 < len(grk.walk_tiles(cs[:len(cs) * num // 10])) < full:
                return cs[:len(cs) * num // 10]
        except grk.GrkGpuError:
            pass
    raise AssertionError("no cut leaves some tiles")


def _specs():
    """(stream, decompress keywords) of everything one call takes: the
    subsampled fixtures on their grids, upsampled, through sYCC where the shape
    allows and to 8 bits; the seam streams (the staged path, 12 bits staged and
    8 stored); the 4:4:4 MCT-plus-ops streams; the precision fixtures to 8
    bits; a cut stream whose missing tiles come out as converted zeros."""
    from prec_fixtures import PREC, REFUSED, sgnds, stream
    out = []
    for tag in ("sub_420_rgb8", "sub_422_I_tiles", "sub_uniform2_rgb8", "sub_mixed_pcrl", "sub_gray_3x2_rpcl",
                "sub_cprl_tiles_layers"):
        bits, cs = SUB[tag]["bits"], gold(tag)
        nt = narrowest(bits)
        out += [(cs, dict(dtype=nt)), (cs, dict()), (cs, dict(upsample=True, dtype=nt, layout="hwc")),
                (cs, dict(upsample=True)),
                (cs, dict(out_prec=8, prec_mode="clip", dtype=np.uint8)),
                (cs, dict(out_prec=8, prec_mode="scale", dtype=np.uint8)), (cs, dict(out_prec=5, prec_mode="scale")),
                (cs, dict(out_prec=8, prec_mode="scale", dtype=np.uint8, upsample=True, layout="hwc")),
                (cs, dict(out_prec=8, prec_mode="scale", upsample=True))]
        if tag in ("sub_420_rgb8", "sub_422_I_tiles"):
            out += [(cs, dict(colour="sycc", dtype=nt)), (cs, dict(colour="sycc", layout="hwc")),
                    (cs, dict(colour="sycc", out_prec=8, prec_mode="scale", dtype=np.uint8, layout="hwc"))]
    cs8, cs12 = _seam_stream(8)[0], _seam_stream(12)[0]
    out += [(cs8, dict(colour="sycc", dtype=np.uint8)), (cs8, dict(upsample=True, dtype=np.uint8, layout="hwc")),
            (cs12, dict(colour="sycc", out_prec=8, prec_mode="scale", dtype=np.uint8, layout="hwc")),
            (cs12, dict(upsample=True, out_prec=8, prec_mode="clip", dtype=np.uint8)),
            (cs12, dict(upsample=True, dtype=np.uint16)), (cs12, dict())]
    for name in ("rgb12_tiles_I", "rgb16_64"):
        for layout in ("chw", "hwc"):
            out.append((gold(name), dict(out_prec=8, prec_mode="scale", dtype=np.uint8, layout=layout)))
    out.append((gold("rgb12_tiles_I"), dict(colour="sycc", dtype=np.uint16, layout="hwc")))
    # every precision fixture to 8 bits, clipped (planar) and scaled (interleaved where it has pixels): 1 .. 5
    # components, RCT / ICT, signed output, components of different precision and sign (int32 holds those)
    for name in sorted(PREC):
        m = PREC[name]
        if name in REFUSED and not name.startswith("p_g"):
            continue
        sg = sgnds(m)
        dt = narrowest(8, sg[0]) if len(set(sg)) == 1 else np.int32
        out.append((stream(name), dict(out_prec=8, prec_mode="clip", dtype=dt)))
        out.append((stream(name), dict(out_prec=8, prec_mode="scale", dtype=dt, layout="hwc" if len(sg) > 1 else "chw")))
    # five components: per-tile launches, not the tables -- precision, and CMYK's four channels
    c5 = stream("p_x_c5_8u_r10")
    out += [(c5, dict(out_prec=4, prec_mode="scale", dtype=np.uint8, layout="hwc")), (c5, dict(out_prec=12, prec_mode="scale")),
            (c5, dict(colour="cmyk", dtype=np.uint8)), (c5, dict(colour="cmyk", out_prec=4, prec_mode="clip", layout="hwc")),
            (c5, dict(dtype=np.uint8, layout="hwc"))]
    cut = gold("rgb12_tiles_I")[:48890]  # tiles never reached: sYCC(0, 0, 0), not zero
    out += [(cut, dict(colour="sycc", dtype=np.uint16)), (cut, dict(colour="sycc", dtype=np.int32, layout="hwc")),
            (cut, dict(colour="sycc", out_prec=8, prec_mode="scale", dtype=np.uint8)),
            (cut, dict(out_prec=8, prec_mode="clip", dtype=np.uint8)), (cut, dict())]
    cutsub = _cut(_seam_stream(8)[0])  # a cut 4:2:0 stream, upsampled: null sources in the upsampling store
    out += [(cutsub, dict(colour="sycc", dtype=np.uint8, layout="hwc")), (cutsub, dict(upsample=True))]
    return out


@pytest.fixture(scope="module")
def workload(codec):
    """the list and each item's single-call decode, computed once"""
    import grokimagecompression_amd as grk
    specs = _specs()
    assert len(grk.walk_tiles(specs[-1][0])) < 9  # (the cut 4:2:0 stream does miss tiles)
    refs = [codec.decompress(cs, **kw) for cs, kw in specs]
    for r in refs:
        for a in (r if isinstance(r, list) else [r]):
            a.setflags(write=False)
    return specs, refs


def _batch(codec, specs, device, **kw):
    keys = ("dtype", "layout", "upsample", "colour", "out_prec", "prec_mode")
    dflt = dict(dtype=None, layout="chw", upsample=False, colour=None, out_prec=None, prec_mode="clip")
    args = {k: [s[1].get(k, dflt[k]) for s in specs] for k in keys}
    return codec.decompress_batch_convert([s[0] for s in specs], device_out=device, **args, **kw)


def _check(codec, specs, refs, device):
    devs = [device and not isinstance(r, list) for r in refs]  # (a list of planes lives on the host)
    got = _batch(codec, specs, devs)
    assert codec.batch_info["n_ok"] == len(specs)
    for i, (g, r) in enumerate(zip(got, refs)):
        assert isinstance(g, (np.ndarray, list)) != devs[i]
        _same(g, r, (i, specs[i][1]))


@pytest.mark.parametrize("device", [False, True])
def test_every_item_is_the_single_call(codec, workload, device):
    specs, refs = workload
    assert len(specs) > 300 and sum(isinstance(r, list) for r in refs) >= 12
    _check(codec, specs, refs, device)
    # zeros nothing decoded are converted: the cut stream's missing tiles under sYCC
    k = [i for i, s in enumerate(specs) if s[1] == dict(colour="sycc", dtype=np.uint16) and len(s[0]) == 48890][0]
    zero = sycc_to_rgb(np.zeros((3, 1, 1), np.int64), 12)[:, 0, 0].tolist()
    assert zero != [0, 0, 0] and refs[k][:, 149, 199].tolist() == zero


def test_reduced_decode_converts_its_zero_margin(codec):
    """101 x 67 at (3, 5), reduce = 1 (test_sycc_converts_the_zero_margin_of_a_
    reduced_decode's stream): the margin is (0, 135, 0) under sYCC.  cp_reduce is the
    call's, so this list has a call of its own; the subsampled item takes the
    reduce on its grids and refuses it with the upsampled output."""
    import grokimagecompression_amd as grk
    import synth
    p, off = grk.CParams.from_cli(["-t", "37,29", "-d", "3,5", "-Y", "0"])
    cs = codec.compress(synth.synth_image(67, 101, 3, 8, 77), 8, p, offset=off)
    specs = [(cs, dict(colour="sycc", dtype=np.uint8)), (cs, dict(colour="sycc", dtype=np.int32, layout="hwc")),
             (cs, dict(colour="sycc", out_prec=12, prec_mode="scale", dtype=np.uint16)),
             (cs, dict(out_prec=4, prec_mode="scale", dtype=np.uint8)), (cs, dict()),
             (gold("sub_420_rgb8"), dict()), (gold("rgb12_tiles_I"), dict(out_prec=8, prec_mode="scale", dtype=np.uint8))]
    refs = [codec.decompress(c, reduce=1, **kw) for c, kw in specs]
    assert refs[0][:, -1, 0].tolist() == [0, 135, 0] and refs[0][:, 0, -1].tolist() == [0, 135, 0]
    for device in (False, True):
        devs = [device and not isinstance(r, list) for r in refs]
        got = _batch(codec, specs, devs, reduce=1)
        for i, (g, r) in enumerate(zip(got, refs)):
            _same(g, r, (i, specs[i][1]))
    got = _batch(codec, [(gold("sub_420_rgb8"), dict(upsample=True)), specs[0]], False, reduce=1, errors="return")
    assert isinstance(got[0], grk.GrkGpuError) and "grkgpu error -1" in str(got[0])
    _same(got[1], refs[0], "behind a refused item")


def test_failing_items_among_the_others(codec, workload):
    """force-RGB, a custom-MCT stream and an empty buffer among good items of
    mixed formats and layouts: the statuses of the host half, the good items
    decoded, the failing items' destinations untouched."""
    import torch
    import grokimagecompression_amd as grk
    specs, refs = workload
    mct = gold(sorted(json.load(open(f"{GOLD}/manifest_mct.json")))[0])
    pick = [i for i in range(0, len(specs), 9) if not isinstance(refs[i], list)][:12]
    bad = [(gold("g8_64"), dict(colour=grk.OutOps(colour=grk.COLOUR_FORCE_RGB))), (mct, dict()), (b"", dict()),
           (gold("rgb12_96x80"), dict(dtype=np.uint8))]
    lst, want = [], []
    for n, i in enumerate(pick):
        lst.append(specs[i])
        want.append(refs[i])
        if n < len(bad):
            lst.append(bad[n])
            want.append(None)
    plan = grk.plan_batch_convert([s[0] for s in lst], dtype=[s[1].get("dtype") for s in lst],
                                  layout=[s[1].get("layout", "chw") for s in lst],
                                  upsample=[s[1].get("upsample", False) for s in lst],
                                  colour=[s[1].get("colour") for s in lst], out_prec=[s[1].get("out_prec") for s in lst],
                                  prec_mode=[s[1].get("prec_mode", "clip") for s in lst])
    assert [st != 0 for st in plan["status"]] == [w is None for w in want]
    assert [plan["status"][k] for k in (1, 3, 7)] == [-4, -4, -1]
    for device in (False, True):
        outs = []
        for (cs, kw), w in zip(lst, want):
            if w is not None:
                outs.append(None)
                continue
            try:
                d = grk.read_header(cs)
            except grk.GrkGpuError:  # (the empty buffer)
                d = None
            shp = (1, 1, 1) if d is None else (d.numcomps, d.y1 - d.y0, d.x1 - d.x0)
            o = np.full(shp, 0x5A, dtype=kw.get("dtype") or np.int32)
            # (a stream whose header does not read gets no destination at all)
            outs.append(None if d is None else (torch.from_numpy(o).cuda() if device else o))
        got = _batch(codec, lst, device, out=outs, errors="return")
        assert codec.batch_info["n_ok"] == len(pick)
        for k, (g, w) in enumerate(zip(got, want)):
            if w is None:
                assert isinstance(g, grk.GrkGpuError) and "grkgpu error %d" % plan["status"][k] in str(g)
                assert outs[k] is None or (to_numpy(outs[k]) == 0x5A).all()
            else:
                _same(g, w, (k, lst[k][1]))
    with pytest.raises(grk.GrkGpuError, match="grkgpu error -4: item 1: .*force-RGB"):
        _batch(codec, lst, False)


def test_64_copies_take_the_launches_of_one(codec):
    cs = gold("sub_420_rgb8")
    kw = dict(dtype=np.uint8, layout="hwc", colour="sycc")
    ref = codec.decompress(cs, **kw)
    one = codec.decompress_batch_convert([cs], **kw)
    n1 = dict(codec.batch_info)
    _same(one[0], ref, "one copy")
    for device in (False, True):
        got = codec.decompress_batch_convert([cs] * 64, stack=True, device_out=device, **kw)
        assert tuple(got.shape) == (64, 75, 97, 3) and isinstance(got, np.ndarray) != device
        assert codec.batch_info["n_launches"] == n1["n_launches"]
        assert codec.batch_info["n_store_jobs"] == 64 * n1["n_store_jobs"]
        g = to_numpy(got)
        assert g.dtype == np.uint8 and all(np.array_equal(g[i], ref) for i in range(64))
    # the staged path and the store on one grid with ops alike
    for c2, k2 in ((_seam_stream(12)[0], dict(dtype=np.uint8, layout="hwc", colour="sycc", out_prec=8, prec_mode="scale")),
                   (gold("rgb12_tiles_I"), dict(dtype=np.uint8, out_prec=8, prec_mode="scale"))):
        codec.decompress_batch_convert([c2], **k2)
        n1 = codec.batch_info["n_launches"]
        codec.decompress_batch_convert([c2] * 16, **k2)
        assert codec.batch_info["n_launches"] == n1


def test_no_ops_is_decompress_batch_launch_for_launch(codec):
    names = ["g8_64", "rgb8_128x96", "rgb12_tiles_I", "rgb16_64", "g16_128"]
    bufs = [gold(n) for n in names]
    for kw in (dict(), dict(dtype=[np.uint8, np.uint8, np.uint16, np.uint16, np.uint16], layout="hwc")):
        a = codec.decompress_batch(bufs, **kw)
        ia = dict(codec.batch_info)
        b = codec.decompress_batch_convert(bufs, **kw)
        assert codec.batch_info == ia
        for x, y in zip(a, b):
            _same(y, x, kw)


def test_dirty_context(codec, workload):
    """the same list on scratch filled with 0xFF, and after a call of another kind"""
    import synth
    specs, refs = workload
    codec.debug_fill(0xFF)
    _check(codec, specs, refs, False)
    codec.compress(synth.synth_image(96, 128, 3, 8, 5), 8)
    _check(codec, specs, refs, True)
    codec.debug_fill(0xFF)
    _check(codec, specs[:40], refs[:40], True)


def test_precision_fixture_variants(codec):
    """the -l 1 / -r 1 decodes of the precision fixtures that have them: cp_layer and cp_reduce are the call's"""
    from prec_fixtures import PREC, sgnds, stream
    for tag, kw in (("l1", dict(layers=1)), ("r1", dict(reduce=1))):
        names = sorted(n for n, m in PREC.items() if tag in m.get("variants", {}))
        assert names
        specs = []
        for n in names:
            sg = sgnds(PREC[n])
            dt = narrowest(8, sg[0]) if len(set(sg)) == 1 else np.int32
            specs += [(stream(n), dict(out_prec=8, prec_mode="scale", dtype=dt, layout="hwc")), (stream(n), dict())]
        refs = [codec.decompress(c, **k, **kw) for c, k in specs]
        for device in (False, True):
            got = _batch(codec, specs, device, **kw)
            for i, (g, r) in enumerate(zip(got, refs)):
                _same(g, r, (tag, i, specs[i][1]))


def test_cut_upsampled_copies_take_the_launches_of_one(codec):
    """a cut 4:2:0 stream with staged chroma: the zero fill of the staging planes is one for the whole list"""
    cs = _cut(_seam_stream(8)[0])
    kw = dict(dtype=np.uint8, layout="hwc", colour="sycc")
    ref = codec.decompress(cs, **kw)
    full = _seam_stream(8)[0]
    codec.decompress_batch_convert([cs, full], **kw)
    n1 = codec.batch_info["n_launches"]
    got = codec.decompress_batch_convert([cs, full] * 8, **kw)
    assert codec.batch_info["n_launches"] == n1
    rfull = codec.decompress(full, **kw)
    for i, g in enumerate(got):
        _same(g, rfull if i % 2 else ref, i)


def test_more_than_four_components_upsampled(codec):
    """Five components take the per-tile launches in both phases: mixed grids
    (chroma read from the tile buffers), all subsampled alike in tiles at an
    odd origin (every component staged, stored there by the per-tile launch),
    each upsampled with and without a precision op, and on their own grids."""
    import grokimagecompression_amd as grk
    import synth
    streams = []
    for subs, args, rect in (([(1, 1), (2, 2), (2, 2), (1, 1), (2, 1)], ["-t", "32,32"], (0, 0, 70, 50)),
                             ([(2, 2)] * 5, ["-t", "37,29", "-d", "3,5"], (3, 5, 73, 55))):
        planes = [synth.synth_image(cd(rect[3], dy) - cd(rect[1], dy), cd(rect[2], dx) - cd(rect[0], dx), 1, 10,
                                    700 + k)[0] for k, (dx, dy) in enumerate(subs)]
        p, off = grk.CParams.from_cli(args)
        streams.append(codec.compress_subsampled(planes, 10, (rect[2] - rect[0], rect[3] - rect[1]), subs, p, offset=off))
    specs = []
    for cs in streams:
        specs += [(cs, dict(upsample=True)), (cs, dict(upsample=True, dtype=np.uint16, layout="hwc")),
                  (cs, dict(upsample=True, out_prec=8, prec_mode="scale", dtype=np.uint8, layout="hwc")),
                  (cs, dict(upsample=True, out_prec=8, prec_mode="clip", dtype=np.uint8)),
                  (cs, dict(out_prec=8, prec_mode="scale", dtype=np.uint8)), (cs, dict())]
    refs = [codec.decompress(c, **k) for c, k in specs]
    for device in (False, True):
        devs = [device and not isinstance(r, list) for r in refs]
        got = _batch(codec, specs, devs)
        for i, (g, r) in enumerate(zip(got, refs)):
            _same(g, r, (i, specs[i][1]))
