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
with VSC|SEGSYM."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

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
    exe = tmp_path_factory.mktemp("t1model") / "test_t1_model"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wno-unknown-pragmas", "-o", str(exe),
                    os.path.join(ROOT, "tests/cpp/test_t1_model.cpp")], check=True)

    def run(cases, sty):
        fin, fout = str(exe) + ".in", str(exe) + ".out"
        with open(fin, "wb") as f:
            f.write(np.uint32(len(cases)).tobytes())
            for h, w, orient, qmfbid, inv, blk in cases:
                f.write(np.array([w, h, orient, qmfbid, inv], np.uint32).tobytes())
                f.write(np.ascontiguousarray(blk, np.int32).tobytes())
        subprocess.run([str(exe), "--encode", fin, fout, str(sty)], check=True)
        raw = open(fout, "rb").read()
        res, pos = [], 0
        for _ in cases:
            rec = np.frombuffer(raw, np.uint32, 99, pos)
            pos += 99 * 4
            res.append((int(rec[0]), int(rec[1]), [int(v) for v in rec[3:3 + rec[1]]], raw[pos:pos + int(rec[2])]))
            pos += int(rec[2])
        assert pos == len(raw)
        return res
    return run


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
