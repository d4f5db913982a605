"""The geometry sweep on the GPU (oracle/make_golden_geom.py,
tests/golden/manifest_geom.json): 256 machine-drawn small images -- odd image
and tile origins, one-sample tiles and tile-components, resolutions empty in
one tile and not in its neighbour, precincts smaller than the code-block or
without a code-block, the position progressions over precinct grids with and
without subsampling -- each pinned by the reference's hashes alone.

Encode: the codestream has the recorded length and SHA-256.  Decode of those
bytes: the recorded hash of the reference's decode, and of its -r / -d decode
where the case has one.  Tolerance 0.  No stream is committed, so the decode
tests run on the encoder's bytes once their hash is the reference's.  Where the
restated oracle covers a case (conftest.oracle_supported; the CPU chain pins it
to the same hashes, tests/test_oracle_golden.py), a mismatch is reported by
sample: component, y, x and the tile it lies in.

What the sweep found in the library: geom_000, geom_001 and geom_002 (-r a,1
on tiles 2 or 3 samples wide, a first-layer budget of 30 bytes) came out with
the reference's length and one code-block's bytes a layer too early.  The
reference's packet simulation counts the inclusion bit of a code-block
without samples that it keeps in a band without samples; t2.cpp
packet_header<SIM> now counts it too (tests/test_host_build.py replays the
three tiles on the host).
"""
import hashlib
import random

import numpy as np
import pytest

import geom_fixtures as gf
from conftest import oracle_supported

pytestmark = pytest.mark.gpu
CHUNKS = [gf.CASES[i:i + gf.CHUNK] for i in range(0, len(gf.CASES), gf.CHUNK)]
EINVAL, EUNSUPPORTED = -1, -4
FORCED = [
    dict(pair_kernel=2, pair_min_samples=0, f01_rows=4, f01_min_samples=0, inv01=2, inv01_min_samples=0),
    dict(t1_lone=-1, t1_dec_sort=1, t1_dec_bpw=16, t1_enc_sort=1, t1_enc_bpw=16),
]
_streams = {}


def _grk():
    import grokimagecompression_amd as grk
    return grk


def sha(b):
    return hashlib.sha256(b).hexdigest()


def params(m):
    return _grk().CParams.from_cli(m["args"])


def oracle_covers(m):
    return oracle_supported(m["args"]) and not m["subsampling"]


def compress(codec, m, src=None, layout="chw"):
    p, off = params(m)
    if m["subsampling"]:
        return codec.compress_subsampled(gf.planes(m), m["bits"], tuple(m["size"]), gf.subsampling(m), p, offset=off)
    return codec.compress(gf.image(m) if src is None else src, m["bits"], p, offset=off, layout=layout)


def encode_mismatch(m, b):
    """None, or what differs between b and the recorded codestream."""
    if len(b) == m["j2k_len"] and sha(b) == m["j2k_sha256"]:
        return None
    msg = "%s %s: codestream of %d bytes, the reference's has %d" % (m["name"], m["args"], len(b), m["j2k_len"])
    if len(b) == m["j2k_len"]:
        msg = "%s %s: codestream hash differs at the reference's length %d" % (m["name"], m["args"], len(b))
    if oracle_covers(m):
        import pyoracle
        ref = pyoracle.encode(gf.image(m), m["bits"], pyoracle.params_from_args(m["args"], nthreads=4),
                              pyoracle.image_offset_from_args(m["args"]))
        if sha(ref) == m["j2k_sha256"]:
            n = min(len(b), len(ref))
            diff = np.flatnonzero(np.frombuffer(b[:n], np.uint8) != np.frombuffer(ref[:n], np.uint8))
            msg += "; first differing byte at %s" % (int(diff[0]) if len(diff) else n)
    return msg


def stream(codec, m, errs):
    """The case's codestream: ours, once it is the reference's byte for byte by
    its hash; else None and the finding in errs (no stream is committed)."""
    if m["name"] not in _streams:
        b = compress(codec, m)
        bad = encode_mismatch(m, b)
        if bad:
            errs.append(bad)
            return None
        _streams[m["name"]] = b
    return _streams[m["name"]]


def as_planes(d):
    return list(d)


def valid_part(planes, v):
    """The decoded samples of a whole-image -r decode (the plane is sized
    ceil(size / 2^r); what lies beyond the decoded samples is zero)."""
    out = []
    for p, (h, w) in zip(planes, v["valid"]):
        assert h <= p.shape[0] <= h + 1 and w <= p.shape[1] <= w + 1, (p.shape, h, w)
        assert not p[h:].any() and not p[:, w:].any(), "samples behind the decoded ones are not zero"
        out.append(p[:h, :w])
    return out


def decode_mismatch(m, got, want_sha, what, reduce=0):
    """None, or the finding: by sample where the oracle covers the case."""
    if gf.planes_sha(got) == want_sha:
        return None
    msg = "%s %s: %s differs from the reference's" % (m["name"], m["args"], what)
    if oracle_covers(m) and what != "window":
        import pyoracle
        ref = pyoracle.decode(_streams[m["name"]], nthreads=4, reduce=reduce)
        if gf.planes_sha(list(ref)) == want_sha:
            scale = " (samples of the 1 / %d image)" % (1 << reduce) if reduce else ""
            msg += ": " + gf.first_difference(m, got, list(ref)) + scale
    elif "-I" not in m["args"] and what == "decode":
        msg += ": " + gf.first_difference(m, got, gf.planes(m))  # lossless: the source is the reference
    return msg


def check_decodes(codec, m, b, errs):
    d = as_planes(codec.decompress(b))
    bad = decode_mismatch(m, d, m["dec_sha256"], "decode")
    if bad:
        errs.append(bad)
    for tag, v in m.get("variants", {}).items():
        kw = gf.variant_kw(v)
        x = as_planes(codec.decompress(b, **kw))
        if "reduce" in kw:
            x = valid_part(x, v)
        if [list(p.shape) for p in x] != v["shapes"]:
            errs.append("%s %s: %s decodes to %s, the reference to %s" % (m["name"], m["args"], tag,
                                                                         [p.shape for p in x], v["shapes"]))
            continue
        bad = decode_mismatch(m, x, v["dec_sha256"], "window" if "window" in kw else "-r decode", kw.get("reduce", 0))
        if bad:
            errs.append(bad)
    return d


def replicate(m, planes_):
    """numpy's upsample=True: sample (X, Y) of the image grid is the component's
    sample (floor(X / dx) - ceil(x0 / dx), floor(Y / dy) - ceil(y0 / dy)), zero where that is negative."""
    (x0, y0), (w, h) = gf.offset(m), m["size"]
    out = np.zeros((len(planes_), h, w), np.int32)
    for k, ((dx, dy), p) in enumerate(zip(gf.subsampling(m), planes_)):
        ix = np.arange(x0, x0 + w) // dx - gf.cd(x0, dx)
        iy = np.arange(y0, y0 + h) // dy - gf.cd(y0, dy)
        full = p[np.clip(iy, 0, None)][:, np.clip(ix, 0, None)]
        out[k] = np.where((iy >= 0)[:, None] & (ix >= 0)[None, :], full, 0)
    return out


def refused(m):
    return gf.CODES[m["refuse"]] if "refuse" in m else None


@pytest.mark.parametrize("chunk", range(len(CHUNKS)))
def test_encode_decode_match_reference(codec, chunk):
    """Every case of the chunk: encode from int32 host planes (a seeded quarter
    also from a cuda tensor of the narrowest dtype, pixel-interleaved where
    there are 2 or more components), decode, the -r / -d variants, a seeded
    quarter also straight to the narrowest dtype / interleaved, subsampled
    cases also upsampled by the last kernel."""
    import torch
    errs = []
    for m in CHUNKS[chunk]:
        if refused(m) is not None:
            continue
        b = compress(codec, m)
        bad = encode_mismatch(m, b)
        if bad:
            errs.append(bad)
            continue
        _streams[m["name"]] = b
        c = m["comps"]
        lay = "hwc" if c >= 2 else "chw"
        if "device" in m["flags"] and not m["subsampling"]:
            a = gf.image(m).astype(gf.narrow_dtype(m))
            t = torch.from_numpy(np.ascontiguousarray(np.transpose(a, (1, 2, 0)) if lay == "hwc" else a)).to("cuda:0")
            if compress(codec, m, t, lay) != b:
                errs.append("%s: encode from a %s %s cuda tensor differs from the int32 host encode"
                            % (m["name"], lay, t.dtype))
        d = check_decodes(codec, m, b, errs)
        if m["subsampling"]:
            up = codec.decompress(b, upsample=True)
            if not np.array_equal(up, replicate(m, d)):
                errs.append("%s %s: upsample=True differs from the planar decode replicated" % (m["name"], m["args"]))
        elif "narrow" in m["flags"]:
            dt = gf.narrow_dtype(m)
            x = codec.decompress(b, dtype=dt, layout=lay)
            full = np.stack(d)
            want = (np.transpose(full, (1, 2, 0)) if lay == "hwc" else full).astype(dt)
            if x.dtype != dt or not np.array_equal(x, want):
                errs.append("%s: decode to %s %s differs from the int32 decode cast" % (m["name"], lay, dt.__name__))
    assert not errs, "%d findings:\n" % len(errs) + "\n".join(errs)


@pytest.mark.parametrize("chunk", range(len(CHUNKS)))
def test_batch_matches_reference(codec, chunk):
    """The chunk as one decode batch (manifest order and one seeded
    permutation) and one encode batch, every image with its own params and
    offset: merged DwtJob / Tier-1 / store and load tables over tile-components
    of unequal size and parity.  Subsampled items are refused item by item, as
    are the code-block shapes the library does not take; the others pass."""
    grk = _grk()
    cases = [m for m in CHUNKS[chunk]]
    errs = []
    bufs = {m["name"]: stream(codec, m, errs) for m in cases if refused(m) is None}
    order = [m for m in cases if bufs.get(m["name"]) is not None]
    perm = list(order)
    random.Random(1000 + chunk).shuffle(perm)
    for items in (order, perm):
        outs = codec.decompress_batch([bufs[m["name"]] for m in items], errors="return")
        assert codec.batch_info["n_ok"] == sum(not m["subsampling"] for m in items)
        for i, (m, o) in enumerate(zip(items, outs)):
            if m["subsampling"]:
                if not (isinstance(o, grk.GrkGpuError) and ("error %d:" % EUNSUPPORTED) in str(o)):
                    errs.append("item %d (%s): a subsampled stream was not refused: %r" % (i, m["name"], o))
                continue
            if isinstance(o, grk.GrkGpuError):
                errs.append("item %d (%s): %s" % (i, m["name"], o))
                continue
            bad = decode_mismatch(m, as_planes(o), m["dec_sha256"], "decode")
            if bad:
                errs.append("item %d of the %s batch: %s" % (i, "ordered" if items is order else "permuted", bad))
    imgs, pars, offs = [], [], []
    for m in cases:
        p, off = params(m)
        if m["subsampling"]:
            imgs.append(codec._image_subsampled(gf.planes(m), m["bits"], tuple(m["size"]), gf.subsampling(m), off, False))
        else:
            imgs.append(gf.image(m))
        pars.append(p)
        offs.append(off)
    outs = codec.compress_batch(imgs, [m["bits"] for m in cases], pars, offs, errors="return")
    for i, (m, o) in enumerate(zip(cases, outs)):
        code = EUNSUPPORTED if m["subsampling"] else refused(m)
        if code is not None:
            if not (isinstance(o, grk.GrkGpuError) and ("error %d:" % code) in str(o)):
                errs.append("item %d (%s): expected the refusal %d, got %r" % (i, m["name"], code, o))
        elif isinstance(o, grk.GrkGpuError):
            errs.append("item %d (%s): %s" % (i, m["name"], o))
        else:
            bad = encode_mismatch(m, o)
            if bad:
                errs.append("item %d of the encode batch: %s" % (i, bad))
    assert not errs, "%d findings:\n" % len(errs) + "\n".join(errs)


@pytest.mark.parametrize("opts", FORCED, ids=["fused_level_pairs", "batch_tier1_packing"])
def test_forced_plans_match_reference(codec, opts):
    """A seeded eighth of the sweep under the fused level-pair DWT kernels
    forced onto every size, and under the batch Tier-1 packing (no lone
    kernel, sorted, 16 blocks a workgroup): multi-job tables of unequal
    tile-components through the plans the defaults pick only for large images."""
    picked = [m for m in gf.CASES if "forced" in m["flags"] and refused(m) is None]
    assert len(picked) >= 16
    errs = []
    with _grk().dwt_options(**opts):
        for m in picked:
            b = compress(codec, m)
            bad = encode_mismatch(m, b)
            if bad:
                errs.append(bad)
                continue
            _streams.setdefault(m["name"], b)
            check_decodes(codec, m, b, errs)
    assert not errs, "%d findings:\n" % len(errs) + "\n".join(errs)


def test_refused_shapes_are_refused_on_the_host(codec):
    """What the reference codes and the library does not: the
    recorded GRKGPU_E* code, from the host plan alone (plan_compress_batch makes
    no device call) and from compress; at most 5 % of the sweep."""
    grk = _grk()
    ref = [m for m in gf.CASES if "refuse" in m]
    assert 0 < len(ref) <= 0.05 * len(gf.CASES)
    descs = []
    for m in ref:
        p, off = params(m)
        descs.append({"shape": (m["comps"], m["size"][1], m["size"][0]), "prec": m["bits"], "params": p, "offset": off})
    plan = grk.plan_compress_batch(descs)
    assert plan["status"] == [refused(m) for m in ref] and plan["n_ok"] == 0 and plan["n_launches"] == 0
    for m in ref:
        with pytest.raises(grk.GrkGpuError, match="error %d:" % refused(m)):
            compress(codec, m)
