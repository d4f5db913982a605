"""The two bit-transposes around the lane-per-block coders, through the stage
entry points, block by block and bit-exact:

  * k_t1_rebuild (bit-plane rows -> coefficients: a wavefront per octet of
    blocks, wave-uniform row masks) through grkgpu_t1_decode_blocks, against
    the oracle's t1_decode_cblk + the post-decode scaling (5/3: v / 2 towards
    zero, 9/7: float(v) * step).  Blocks the decoder leaves alone (an all-zero
    block: no passes; len == 0) must come out zero.
  * k_t1_prep (coefficients -> sign and bit-plane rows) through
    grkgpu_t1_encode_blocks_sty (style 0), against the oracle's
    t1_encode_cblk: numbps, pass count, every cumulative rate, the bytes.

Cases: the first 1, 7, 8, 9, 63, 64, 65 and 130 blocks of one list (octet and
group remainders, a last group of two lanes) whose widths, heights, depths
(0 to 16 planes, some 26) and contents cycle at different periods, so an octet
mixes shapes, deep blocks, all-zero blocks and len == 0 blocks, 5/3 and 9/7;
every pass count of a 16x16 and a 64x64 block (low > 0, no refinement pass
decoded, refinement ending above the last plane, samples that became
significant under the last refined plane); and 4160 blocks of 4x4, which the
4-wavefront decoder feeds.  Every decode case runs over scratch filled with
0xFF and over scratch left by a decode of other blocks; the encoder's scratch
is filled with 0xFF.
"""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ENC_RESULT = np.dtype([("numbps", "<u4"), ("numpasses", "<u4"), ("len", "<u4"), ("pad", "<u4"),
                       ("nsym", "<u4"), ("p1", "<u4"), ("p2", "<u4"), ("p3", "<u4"),
                       ("rate", "<u4", 96), ("nmsedec", "<i4", 96)])
ENC_BLOCK = np.dtype([("coef_off", "<u8"), ("out_off", "<u8"), ("stride", "<u4"), ("w", "<u4"), ("h", "<u4"),
                      ("orient", "<u4"), ("qmfbid", "<i4"), ("inv_step", "<i4")])
DEC_BLOCK = np.dtype([("data_off", "<u8"), ("dst_off", "<u8"), ("len", "<u4"), ("numpasses", "<u4"),
                      ("numbps", "<u4"), ("w", "<u4"), ("h", "<u4"), ("orient", "<u4"), ("dstride", "<u4"),
                      ("irrev", "<i4"), ("step", "<f4"), ("pad", "<u4")])
MAX_SEG = 64 * 64 * 4 + 64
SIZES = [1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 63, 64]
DEPTHS = list(range(17)) + [26, 11, 16]  # period 20
COUNTS = [1, 7, 8, 9, 63, 64, 65, 130]
INV_STEP = 6553  # 9/7: the quantiser's 1 / step in 13-bit fixed point; the decoder's step below is its inverse / 4


def _content(rng, kind, h, w, nb, i):
    """nb planes of magnitude; kind 0: dense noise with the top plane present, 1: one sample in 8, 2: all negative,
    3: one sample alone, at column 0 / 31 / 32 / 63 of the first or the last row, 4: full magnitude, odd and negative."""
    if nb == 0:
        return np.zeros((h, w), np.int32)
    top, full = 1 << (nb - 1), (1 << nb) - 1
    mag = rng.integers(0, full + 1, (h, w))
    neg = rng.integers(0, 2, (h, w))
    if kind == 1:
        mag = mag * (rng.integers(0, 8, (h, w)) == 0)
    elif kind == 2:
        neg[:] = 1
    elif kind == 3:
        mag[:] = 0
        mag[(0, h - 1)[(i // 5) % 2], min((0, 31, 32, 63)[(i // 10) % 4], w - 1)] = full
    elif kind == 4:
        mag[:], neg[:] = full, 1
    mag[h // 2, w // 2] |= top  # the block has nb planes whatever the draw
    if nb == 26:  # the one 26-plane magnitude the 5/3 quantiser holds: |v| = 2^25, v << 6 = INT32_MIN
        mag, neg = np.where(mag >= top, top, mag), np.where(mag >= top, 1, neg)
    return (mag * (1 - 2 * neg)).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _mixed(n, seed):
    """(h, w, orient, qmfbid, inv_step, block) x n"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        w, h = SIZES[(i * 5 + i // 13 + 4) % 13], SIZES[(i * 3 + i // 8 + 6) % 13]
        nb = DEPTHS[(i * 7 + i // 20 + 9) % 20]
        blk = _content(rng, i % 5, h, w, nb, i)
        if i % 3 == 1 and nb <= 16:  # 9/7: fixed-point coefficients
            out.append((h, w, i % 4, 0, INV_STEP, (blk.astype(np.int64) << 12).astype(np.int32)))
        else:
            out.append((h, w, i % 4, 1, 0, blk))
    return out


@functools.lru_cache(maxsize=None)
def _edge_blocks():
    """64x64 and 33x47 blocks whose only sample sits at column 0 / 31 / 32 / 63 (the last one inside the block) of
    row 0 and of row h - 1, and blocks of negative samples only."""
    out = []
    for (h, w) in ((64, 64), (47, 33)):
        for y in (0, h - 1):
            for x in (0, 31, 32, 63):
                blk = np.zeros((h, w), np.int32)
                blk[y, min(x, w - 1)] = -777 if x & 1 else 1001
                out.append((h, w, len(out) % 4, 1, 0, blk))
    rng = np.random.default_rng(5)
    out.append((64, 64, 1, 1, 0, -rng.integers(1, 1 << 12, (64, 64)).astype(np.int32)))
    out.append((9, 64, 2, 0, INV_STEP, (-rng.integers(1, 1 << 10, (9, 64)) << 12).astype(np.int32)))
    return out


@functools.lru_cache(maxsize=None)
def _tiny(n):
    """n blocks of 4x4 out of 40 different ones, depths 0 to 16"""
    rng = np.random.default_rng(44)
    kinds = []
    for k in range(40):
        blk = _content(rng, k % 5, 4, 4, DEPTHS[(k * 3) % 17], k)
        kinds.append((4, 4, k % 4, 1, 0, blk) if k % 3 else (4, 4, k % 4, 0, INV_STEP, (blk.astype(np.int64) << 12).astype(np.int32)))
    return [kinds[(i * 7 + i // 64) % 40] for i in range(n)]


def _encode_ref(oracle, cases):
    """the oracle's (data, passes, numbps) per case, once per different block"""
    memo, out = {}, []
    for c in cases:
        if id(c) not in memo:
            memo[id(c)] = oracle.t1_encode_cblk(c[5], c[2], c[3], c[4])
        out.append(memo[id(c)])
    return out


def _post(v, irrev, step):
    if not irrev:
        return np.trunc(v / 2).astype(np.int32)  # C integer division
    return (v.astype(np.float32) * np.float32(step)).view(np.int32)


def _item(oracle, case, enc, npass=None, cut=False):
    """the decode item (data, numpasses, numbps, w, h, orient, irrev, step) of an encoded case and its reference;
    cut: len = 0, which the decoder leaves alone"""
    (h, w, orient, qmfbid, inv, _), (data, passes, nbps) = case, enc
    irrev = 1 if qmfbid == 0 else 0
    step = 1.0 / (inv / 8192.0) / 4.0 if irrev else 0.0
    if cut or not passes:
        return (b"", len(passes), nbps, w, h, orient, irrev, step), np.zeros((h, w), np.int32)
    npass = len(passes) if npass is None else npass
    seg = data[:passes[npass - 1][0]]
    assert seg
    ref = oracle.t1_decode_cblk(seg, npass, nbps, w, h, orient)
    return (seg, npass, nbps, w, h, orient, irrev, step), _post(ref, irrev, step)


_DEC = {}


def _decode_case(oracle, name):
    """(items, references) of a decode case, built once"""
    if name in _DEC:
        return _DEC[name]
    memo = {}

    def item(case, enc, npass=None, cut=False):  # one oracle decode per different (block, pass count)
        key = (id(case), npass, cut)
        if key not in memo:
            memo[key] = _item(oracle, case, enc, npass, cut)
        return memo[key]

    if name == "passes":
        # every pass count of a 16x16 5/3 block of 9 planes and of a 64x64 9/7 block, the two interleaved with a
        # full decode of mixed blocks so that an octet holds different (top, low, qlow)
        rng = np.random.default_rng(9)
        a = (16, 16, 1, 1, 0, _content(rng, 0, 16, 16, 9, 0))
        b = (64, 64, 2, 0, INV_STEP, (_content(rng, 1, 64, 64, 7, 0).astype(np.int64) << 12).astype(np.int32))
        pairs = []
        for c in (a, b):
            enc = oracle.t1_encode_cblk(c[5], c[2], c[3], c[4])
            assert len(enc[1]) == 3 * enc[2] - 2 and enc[2] >= 7
            pairs += [item(c, enc, npass) for npass in range(1, len(enc[1]) + 1)]
        mixed = _mixed(130, 21)
        for k, (c, enc) in enumerate(zip(mixed[:24], _encode_ref(oracle, mixed[:24]))):
            pairs.insert(3 * k, item(c, enc))
    elif name == "tiny4160":
        cases = _tiny(4160)
        pairs = [item(c, enc, None, i % 97 == 5) for i, (c, enc) in enumerate(zip(cases, _encode_ref(oracle, cases)))]
    else:
        cases = _mixed(130, 21)[:int(name[1:])]
        # every 11th block arrives with len == 0; half of the others at a truncated pass count
        pairs = []
        for i, (c, enc) in enumerate(zip(cases, _encode_ref(oracle, cases))):
            npass = len(enc[1])
            if i % 2 and npass > 1:
                npass = 1 + (i * 5) % npass
            pairs.append(item(c, enc, npass or None, i % 11 == 6))
    _DEC[name] = ([p[0] for p in pairs], [p[1] for p in pairs])
    return _DEC[name]


def _gpu_decode(items, t_scr):
    import torch
    import grokimagecompression_amd as grk
    L = grk.lib()
    n = len(items)
    blob = bytearray(16)
    db = np.zeros(n, DEC_BLOCK)
    dst_off = 0
    for i, (data, npass, nbps, w, h, orient, irrev, step) in enumerate(items):
        db[i] = (len(blob), dst_off, len(data), npass, nbps, w, h, orient, w, irrev, step, 0)
        blob += data + bytes(16)
        dst_off += w * h
    dev = torch.device("cuda", 0)
    t_data = torch.from_numpy(np.frombuffer(bytes(blob) + bytes(64), np.uint8).copy()).to(dev)
    t_blocks = torch.from_numpy(db.view(np.uint8)).to(dev)
    t_dst = torch.full((dst_off + 16,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    assert t_scr.numel() >= L.grkgpu_t1_scratch_bytes_n(n)
    s = ctypes.c_void_p(torch.cuda.current_stream(0).cuda_stream)
    grk._check(L.grkgpu_t1_decode_blocks(t_blocks.data_ptr(), n, t_data.data_ptr(), t_scr.data_ptr(),
                                         t_dst.data_ptr(), s))
    torch.cuda.synchronize()
    d = t_dst.cpu().numpy()
    assert (d[dst_off:] == 0x5A5A5A5A).all()
    outs, o = [], 0
    for (_, _, _, w, h, _, _, _) in items:
        outs.append(d[o:o + w * h].reshape(h, w))
        o += w * h
    return outs


DEC_CASES = ["n%d" % n for n in COUNTS] + ["passes", "tiny4160"]


@pytest.mark.parametrize("dirty", ["ff", "other"])
@pytest.mark.parametrize("case", DEC_CASES)
def test_t1_rebuild_vs_oracle(oracle, case, dirty):
    import torch
    import grokimagecompression_amd as grk
    items, refs = _decode_case(oracle, case)
    # the same scratch after other blocks: the tiny blocks moved by three places, else another case's list
    other = items[3:] + items[:3] if case == "tiny4160" else _decode_case(oracle, "passes" if case == "n130" else "n130")[0]
    n = max(len(items), len(other))
    t_scr = torch.full((grk.lib().grkgpu_t1_scratch_bytes_n(n) + 256,), 0xFF, dtype=torch.uint8, device="cuda:0")
    if dirty == "other":
        _gpu_decode(other, t_scr)
    outs = _gpu_decode(items, t_scr)
    bad = [(i, items[i][1:7]) for i, (o, r) in enumerate(zip(outs, refs)) if not np.array_equal(o, r)]
    assert not bad, (len(bad), bad[:8])
    if case == "n130":
        kinds = {(it[2] > 16, it[6], len(it[0]) == 0) for it in items}
        assert len(kinds) >= 5 and sum(1 for r in refs if (r & 1).any() and (r < 0).any()) > 10


def _gpu_encode(cases):
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
    t_scr = torch.full((L.grkgpu_t1_scratch_bytes_n(n) + 256,), 0xFF, dtype=torch.uint8, device=dev)
    s = ctypes.c_void_p(torch.cuda.current_stream(0).cuda_stream)
    grk._check(L.grkgpu_t1_encode_blocks_sty(t_blocks.data_ptr(), n, t_coef.data_ptr(), t_scr.data_ptr(),
                                             t_out.data_ptr(), t_res.data_ptr(), 0, 0, s))
    torch.cuda.synchronize()
    return t_res.cpu().numpy().view(ENC_RESULT), t_out.cpu().numpy(), eb


ENC_CASES = ["n%d" % n for n in COUNTS] + ["edges", "tiny4160"]


@pytest.mark.parametrize("case", ENC_CASES)
def test_t1_prep_vs_oracle(oracle, case):
    if case == "edges":  # inside a group of mixed blocks
        cases = _mixed(130, 21)[:30] + _edge_blocks() + _mixed(130, 21)[30:70]
    elif case == "tiny4160":
        cases = _tiny(4160)
    else:
        cases = _mixed(130, 21)[:int(case[1:])]
    res, out, eb = _gpu_encode(cases)
    seen = set()
    for i, (c, (data, passes, nbps)) in enumerate(zip(cases, _encode_ref(oracle, cases))):
        r, where = res[i], (case, i, c[1], c[0], c[3])
        assert r["pad"] == 0, where
        assert r["numbps"] == nbps, where
        assert r["numpasses"] == len(passes), where
        assert list(r["rate"][:len(passes)]) == [p[0] for p in passes], where
        o = int(eb[i]["out_off"])
        assert bytes(out[o:o + len(data)]) == data, where
        seen.add(nbps)
    if case == "n130":
        assert {0, 1, 16, 26} <= seen and len(seen) >= 17, seen
