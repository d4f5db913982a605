"""k_t1_model's column emission (t1_lane.h emit_stripe and the refinement
pass's group loop: bit-sliced sign contexts, 32-bit bit tests, byte-permute
compaction, the all-member refinement path picked by ballot, the LDS ring)
through grkgpu_t1_encode_blocks_sty, block by block: numbps, pass count, every
cumulative rate and the MQ bytes.

References: for style 0 the oracle's t1_encode_cblk; for every style the host
build of the same encoder (tests/cpp/test_t1_model.cpp --encode), whose
modelling is checked against a plain per-sample modeller by
tests/test_t1_model_host.py and whose styled streams are checked against the
oracle's decoder by tests/test_host_build.py -- the oracle's block encoder has
no mode switches.

Cases: 130 blocks (two full 64-block groups and a last group of two lanes)
of mixed edge shapes and contents, so that the lanes of one wavefront sit in
different paths with different numbps, 0 included; 64 blocks of 64x64 with 16
dense planes, the ring's worst case; one block alone.  Each with style 0 and
with VSC|SEGSYM.

test_t1_tiny_deep_blocks_in_packed_slabs: blocks of 1 to 16 (and 1x64, 64x1)
samples, 1 to 26 planes deep, in ten styles, whose size the pass terminations
decide (TERMALL: about two bytes a pass), with the output slabs packed by
grkgpu_t1_enc_out_bytes over a 0xA5 fill -- the bytes, and that no block
wrote outside its own slab."""
import ctypes
import functools

import numpy as np
import pytest

import t1_host

pytestmark = pytest.mark.gpu

ENC_RESULT = np.dtype([("numbps", "<u4"), ("numpasses", "<u4"), ("len", "<u4"), ("pad", "<u4"),
                       ("nsym", "<u4"), ("p1", "<u4"), ("p2", "<u4"), ("p3", "<u4"),
                       ("rate", "<u4", 96), ("nmsedec", "<i4", 96)])
ENC_BLOCK = np.dtype([("coef_off", "<u8"), ("out_off", "<u8"), ("stride", "<u4"), ("w", "<u4"), ("h", "<u4"),
                      ("orient", "<u4"), ("qmfbid", "<i4"), ("inv_step", "<i4")])
MAX_SEG = 64 * 64 * 4 + 64
WIDTHS = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64]
HEIGHTS = [1, 3, 4, 5, 8, 61, 63, 64]
STYLES = [0, 8 | 32]  # VSC | SEGSYM


def _content(rng, kind, h, w, i):
    nb = 1 + i % 16
    top = (1 << nb) - 1
    mag = np.zeros((h, w), np.int64)
    sign = rng.integers(0, 2, (h, w))
    if kind == 0:    # dense noise of nb planes
        mag = rng.integers(0, top + 1, (h, w))
    elif kind == 1:  # sparse: 1 in 8 nonzero
        mag = rng.integers(0, top + 1, (h, w)) * (rng.integers(0, 8, (h, w)) == 0)
    elif kind == 3:  # a single nonzero sample: corners, columns 7/8, 15/16, 31/32, 63
        xs = [0, w - 1, 0, w - 1, 7, 8, 15, 16, 31, 32, 63]
        ys = [0, 0, h - 1, h - 1, 1, 2, 3, 0, 1, 2, 3]
        q = (i // 6) % 11
        mag[min(ys[q], h - 1), min(xs[q], w - 1)] = top
    elif kind == 4:  # full magnitude: every refinement column has all four rows
        mag[:] = top
    elif kind == 5:  # alternating-sign checkerboard
        yy, xx = np.mgrid[0:h, 0:w]
        mag = top - rng.integers(0, 2, (h, w))
        sign = (xx + yy) & 1
    return (mag * (1 - 2 * sign)).astype(np.int32)


def _mixed(n, seed):
    """(h, w, orient, qmfbid, inv_step, block): shapes and contents cycle at
    different periods, so every 64-block group mixes them."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        w, h = WIDTHS[(i * 5 + i // 16) % 16], HEIGHTS[(i * 3 + i // 8) % 8]
        blk = _content(rng, i % 6, h, w, i)
        if i % 7 == 3:  # the 9/7 path's quantiser: fixed-point coefficients
            out.append((h, w, i % 4, 0, 6553, (blk.astype(np.int64) << 12).astype(np.int32)))
        else:
            out.append((h, w, i % 4, 1, 0, blk))
    return out


def _dense64(seed):
    rng = np.random.default_rng(seed)
    return [(64, 64, i % 4, 1, 0, rng.integers(-(1 << 16) + 1, 1 << 16, (64, 64)).astype(np.int32)) for i in range(64)]


CASES = {"mixed130": lambda: _mixed(130, 11), "dense64": lambda: _dense64(12), "lone": lambda: _mixed(130, 13)[37:38]}


@pytest.fixture(scope="module")
def host_encoder(tmp_path_factory):
    return t1_host.build(tmp_path_factory.mktemp("t1model"))


def _gpu_encode(cases, sty):
    import torch
    import grokimagecompression_amd as grk
    L = grk.lib()
    n = len(cases)
    coef = np.concatenate([c[5].ravel() for c in cases]).astype(np.int32)
    eb = np.zeros(n, ENC_BLOCK)
    off = 0
    for i, (h, w, orient, qmfbid, inv, blk) in enumerate(cases):
        eb[i] = (off, 16 + i * (MAX_SEG + 16), w, w, h, orient, qmfbid, inv)
        off += h * w
    dev = torch.device("cuda", 0)
    t_coef = torch.from_numpy(coef).to(dev)
    t_blocks = torch.from_numpy(eb.view(np.uint8)).to(dev)
    t_out = torch.zeros(16 + n * (MAX_SEG + 16), dtype=torch.uint8, device=dev)
    t_res = torch.zeros(n * ENC_RESULT.itemsize, dtype=torch.uint8, device=dev)
    t_scr = torch.empty(L.grkgpu_t1_scratch_bytes_n(n) + 256, dtype=torch.uint8, device=dev)
    s = ctypes.c_void_p(torch.cuda.current_stream(0).cuda_stream)
    grk._check(L.grkgpu_t1_encode_blocks_sty(t_blocks.data_ptr(), n, t_coef.data_ptr(), t_scr.data_ptr(),
                                             t_out.data_ptr(), t_res.data_ptr(), 0, sty, s))
    torch.cuda.synchronize()
    return t_res.cpu().numpy().view(ENC_RESULT), t_out.cpu().numpy(), eb


@pytest.mark.parametrize("sty", STYLES)
@pytest.mark.parametrize("case", sorted(CASES))
def test_t1_model_blocks(oracle, host_encoder, case, sty):
    cases = CASES[case]()
    res, out, eb = _gpu_encode(cases, sty)
    host = host_encoder(cases, sty)
    seen_nb = set()
    for i, (h, w, orient, qmfbid, inv, blk) in enumerate(cases):
        nbps, npass, rates, data = host[i]
        if sty == 0:  # the host build itself against the oracle
            odata, passes, onb = oracle.t1_encode_cblk(blk, orient, qmfbid, inv)
            assert (nbps, npass, rates, data) == (onb, len(passes), [p[0] for p in passes], odata), (case, i)
        r = res[i]
        where = (case, sty, i, w, h, orient)
        assert r["pad"] == 0, where
        assert r["numbps"] == nbps, where
        assert r["numpasses"] == npass, where
        assert r["len"] == len(data), where
        assert list(r["rate"][:npass]) == rates, where
        o = int(eb[i]["out_off"])
        assert bytes(out[o:o + len(data)]) == data, where
        seen_nb.add(nbps)
    if case == "mixed130":
        assert 0 in seen_nb and len(seen_nb) >= 8, seen_nb


# ---- tiny, deep blocks in every kind of style, slabs packed by the library's own rule ----
# (h, w): the shapes of tests/cpp/test_t1_model.cpp --sweep up to 16 samples, and the two thin 64-sample ones
TINY_SHAPES = [(1, 1), (1, 2), (2, 1), (1, 3), (3, 1), (2, 2), (1, 4), (4, 1), (3, 3), (4, 4), (5, 3), (1, 8), (2, 8),
               (1, 16), (16, 1), (1, 64), (64, 1)]
TINY_DEPTHS = [1, 2, 12, 13, 15, 16, 19, 22, 26]
TINY_STYLES = [0, 1, 4, 5, 6, 12, 20, 36, 46, 63]
# (blocks, dwt_options): one block per wavefront; the wide coder k_t1_mq<.., MQ_WAVES, 19> at 64 and at 16 blocks
# per wavefront
TINY_CALLS = {"n204": (204, {}), "n4160": (4160, {}), "n4160_bpw16": (4160, dict(t1_enc_bpw=16))}


@functools.lru_cache(maxsize=2)
def _tiny(n):
    """Block i: shape i mod 17, depth (i // 3) mod 9, content (i // 5) mod 5 (the sweep's five), so the lanes of a
    wavefront differ in all three.  5/3, and 9/7 (inv_step 6553) for every seventh block of at most 19 planes.  A
    26-plane block exists for one magnitude only: 5/3's |v| = 2^25, v << 6 = INT32_MIN; its samples that carry the
    top bit are that value, the others keep their lower bits."""
    rng = np.random.default_rng(26)
    out = []
    for i in range(n):
        (h, w), nb, kind = TINY_SHAPES[i % len(TINY_SHAPES)], TINY_DEPTHS[(i // 3) % 9], (i // 5) % 5
        top, full = 1 << (nb - 1), (1 << nb) - 1
        mag, neg = np.zeros(h * w, np.int64), np.zeros(h * w, np.int64)
        if kind == 0:
            mag[:] = full
        elif kind == 1:
            mag, neg = top | rng.integers(0, full + 1, h * w), rng.integers(0, 2, h * w)
        elif kind == 2:
            mag[:], neg[:] = top | (0x55555555 & full), 1
        elif kind == 3:
            mag[h * w // 2] = full
        else:
            mag = top >> (np.arange(h * w) % nb)
        if nb == 26:
            mag, neg = np.where(mag >= top, top, mag), np.where(mag >= top, 1, neg)
        if i % 7 == 3 and nb <= 19:
            v = np.where(mag > 0, (((mag << 6) | 32) << 18) // 6553, 0)
            out.append((h, w, i % 4, 0, 6553, (v * (1 - 2 * neg)).astype(np.int32).reshape(h, w), nb))
        else:
            out.append((h, w, i % 4, 1, 0, (mag * (1 - 2 * neg)).astype(np.int32).reshape(h, w), nb))
    return out


def _gpu_encode_packed(cases, sty, opts):
    """Slabs packed as codec.cpp packs them, by the exported rule: 16 bytes, then grkgpu_t1_enc_out_bytes rounded up
    to 16 per block; `out` prefilled with 0xA5."""
    import torch
    import grokimagecompression_amd as grk
    L = grk.lib()
    n = len(cases)
    coef = np.concatenate([c[5].ravel() for c in cases]).astype(np.int32)
    eb = np.zeros(n, ENC_BLOCK)
    slab = np.zeros(n, np.int64)
    off = total = 0
    for i, (h, w, orient, qmfbid, inv, blk, _) in enumerate(cases):
        total += 16
        eb[i] = (off, total, w, w, h, orient, qmfbid, inv)
        slab[i] = (L.grkgpu_t1_enc_out_bytes(w, h, sty) + 15) & ~15
        assert slab[i] >= w * h * 4 + 64
        total += int(slab[i])
        off += h * w
    scr_bytes = L.grkgpu_t1_scratch_bytes_n(n)
    assert scr_bytes < 4 << 30
    dev = torch.device("cuda", 0)
    t_coef = torch.from_numpy(coef).to(dev)
    t_blocks = torch.from_numpy(eb.view(np.uint8)).to(dev)
    t_out = torch.full((total + 16,), 0xA5, dtype=torch.uint8, device=dev)
    t_res = torch.zeros(n * ENC_RESULT.itemsize, dtype=torch.uint8, device=dev)
    t_scr = torch.empty(scr_bytes + 256, dtype=torch.uint8, device=dev)
    s = ctypes.c_void_p(torch.cuda.current_stream(0).cuda_stream)
    with grk.dwt_options(**opts):
        grk._check(L.grkgpu_t1_encode_blocks_sty(t_blocks.data_ptr(), n, t_coef.data_ptr(), t_scr.data_ptr(),
                                                 t_out.data_ptr(), t_res.data_ptr(), 0, sty, s))
    torch.cuda.synchronize()
    return t_res.cpu().numpy().view(ENC_RESULT), t_out.cpu().numpy(), eb, slab


@functools.lru_cache(maxsize=None)
def _tiny_reference(run, n, sty):
    return run([c[:6] for c in _tiny(n)], sty)


@pytest.mark.parametrize("sty", TINY_STYLES)
@pytest.mark.parametrize("call", sorted(TINY_CALLS))
def test_t1_tiny_deep_blocks_in_packed_slabs(oracle, host_encoder, call, sty):
    """Every block's numbps, pass count, rates and bytes equal the host build's (style 0: the oracle's too), and the
    block wrote nothing outside its own slab: from len rounded up to 4 to the slab's end the 0xA5 fill is intact, the
    pad dword before the block is zero, the 12 bytes before that are fill."""
    n, opts = TINY_CALLS[call]
    cases = _tiny(n)
    host = _tiny_reference(host_encoder, n, sty)
    res, out, eb, slab = _gpu_encode_packed(cases, sty, opts)
    past = 0
    for i, (h, w, orient, qmfbid, inv, blk, nb) in enumerate(cases):
        nbps, npass, rates, data = host[i]
        where = (call, sty, i, h, w, nb, orient, qmfbid)
        assert nbps == nb, where  # the generator made the depth it names
        if sty == 0:  # the host build itself against the oracle
            odata, passes, onb = oracle.t1_encode_cblk(blk, orient, qmfbid, inv)
            assert (nbps, npass, rates, data) == (onb, len(passes), [p[0] for p in passes], odata), where
        r = res[i]
        assert r["pad"] == 0, where
        assert r["numbps"] == nbps, where
        assert r["numpasses"] == npass, where
        assert r["len"] == len(data), where
        assert list(r["rate"][:npass]) == rates, where
        assert len(data) <= slab[i], where
        o = int(eb[i]["out_off"])
        assert bytes(out[o:o + len(data)]) == data, where
        assert (out[o + ((len(data) + 3) & ~3):o + int(slab[i])] == 0xA5).all(), where
        assert (out[o - 4:o] == 0).all(), where
        assert (out[o - 16:o - 4] == 0xA5).all(), where
        past += len(data) > w * h * 4 + 64
    assert (out[-16:] == 0xA5).all()
    # TERMALL without BYPASS or PTERM: blocks the packing by w*h*4 + 64 could not hold -- a floor on coverage: the shapes of
    # one or two samples (3 of 17) at 15 or more planes (5 of 9) alone are a tenth of the blocks
    if (sty & 0x15) == 4:  # PTERM's short terminations stay inside it
        assert past >= n // 20, (call, sty, past)
