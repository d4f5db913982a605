"""The Tier-1 decoder on code-block bytes no Grok encoder writes
(tests/foreign_bytes.py): a marker inside a segment, a segment shorter than
the decoder consumes, a segment ending in 0xFF, FF 80..8F pairs at any
density, segments back to back.  Bit-exact, 5/3 and 9/7.

Stage tests: grkgpu_t1_decode_blocks on device buffers against the oracle's
t1_decode_cblk + the post_decode scaling of tests/test_gpu_stages.py, block by
block, one test per launch plan of kernels.hip launch_t1_decode:
  small    n <= 1,024          k_t1_unstuff_w, one block per wavefront
  middle   1,024 < n <= 4,096  k_t1_unstuff_w, 2-32 blocks per wavefront
  large    n = 4,160           k_t1_unstuff (lane per block) and k_t1_decode_ub
                               in 4-wavefront workgroups; again at 16 blocks
                               per wavefront (t1_dec_bpw=16)
The host build of the same decoder is held to the same oracle on the same
byte families by tests/test_host_build.py, so a difference here lies in a
kernel or a launch.  The segments sit back to back in the data blob: the byte
before the first is 0xFF, the byte after a segment ending in 0xFF is 0x00 or
0x91, so a kernel that takes a neighbour's byte as the previous byte or as
stream data decodes something else.

Whole streams: the fg_* bases of oracle/make_golden_foreign.py with their
packet bodies overwritten, against the reference decoder's image -- the
segment cursor, raw segments, TERMALL, RESET and segments split over layers,
which the block oracle does not have.
"""
import ctypes
import functools
import hashlib
import json

import numpy as np
import pytest

import foreign_bytes as fb
import synth
from conftest import GOLD
from test_gpu_stages import DEC_BLOCK, MAX_SEG, _post
from test_gpu_t1_many import DEC_OPTS

pytestmark = pytest.mark.gpu

FOREIGN = json.load(open(f"{GOLD}/manifest_foreign.json"))
STEP = float(np.float32(1.0 / (6553 / 8192.0) / 4.0))
SENTINEL = 0x5A5A5A5A
SHAPES = [(1, 1), (4, 4), (7, 3), (1, 64), (64, 1), (64, 16), (47, 33), (64, 64)]  # (h, w)
SMALL_SHAPES = [(1, 1), (4, 4), (7, 3), (1, 16), (16, 1), (16, 16), (13, 11), (16, 4)]
NUMBPS = (1, 2, 16, 30)
LENGTHS = fb.LENGTHS


def _carry_positions(seg):
    """stream bit positions of the segment's carry events (t1_flat.h Unstuff)"""
    pos, out = 0, []
    for i, b in enumerate(seg):
        pff = i and seg[i - 1] == 0xFF
        if pff and b > 0x8F:
            break
        if pff and b & 0x80:
            out.append(pos - 1)
        pos += 7 if pff else 8
    return out


def _specs(oracle, plan):
    """[(kind, make(data_off) -> (seg, numpasses, numbps, w, h, orient), byte after or None)]"""
    large = plan == "large"
    shapes = SMALL_SHAPES if large else SHAPES
    nbs = (1, 2, 5, 8) if large else NUMBPS
    lengths = [n for n in LENGTHS if n <= 256] + [200, 256] if large else list(LENGTHS)
    specs = []
    k = [0]

    def fam(kind, length, nb=None, shape=None, which=None):
        i = k[0] = k[0] + 1
        nb_ = nb or nbs[(i // 4) % 4]
        h, w = shape or shapes[(i // 3) % 8]
        np_ = fb.passes_of(nb_, (i // 5) % 3 if which is None else which)
        seg = fb.FAMILIES[kind](7919 * i + len(plan), length)
        specs.append((kind, lambda off, r=(seg, np_, nb_, w, h, i % 4): r, None))

    # the four families at every length; the pass counts, numbps and shapes cycle
    for rnd in range(2):
        for length in lengths:
            for kind in fb.FAMILIES:
                fam(kind, length)
    # carrymax with its last event on the last and the first bit of a 32-bit word (events sit at bits 7 + 15 k)
    for length in (18, 48, 50, 128, 256):
        fam("carrymax", length, which=2)
    # a block whose segment is empty
    specs.append(("empty", lambda off: (b"", 1, 3, 5, 6, 0), None))
    # edits of valid segments
    bh, bw, bnb = (16, 16, 6) if large else (64, 64, 16)
    bases = [fb.valid_segment(oracle, 100 + j, bh, bw, bnb) for j in range(4)]
    bases += [fb.valid_segment(oracle, 200 + j, *(SMALL_SHAPES if large else SHAPES)[j + 2], (2, 5, 8, 3)[j]) for j in range(4)]
    assert all(130 <= len(b[0]) <= (256 if large else MAX_SEG) for b in bases[:4])

    def edit(kind, base, fn, after=None):
        seg0, np_, nb_, orient = base[0]
        h, w = base[1]
        specs.append((kind, lambda off: (fn(seg0, off), np_, nb_, w, h, orient), after))

    shaped = [(b, (bh, bw)) for b in bases[:4]] + [(b, (SMALL_SHAPES if large else SHAPES)[j + 2]) for j, b in enumerate(bases[4:])]
    for j, bs in enumerate(shaped):
        n = len(bs[0][0])
        for t in sorted({1, 2, 3, n // 2, n - 1}):
            if 0 < t < n and (j % 3 == 0 or t in (1, n - 1)):
                edit("trim", bs, lambda s, off, t=t: fb.trim(s, t))
        edit("end_ff", bs, lambda s, off: fb.end_ff(s), after=(0x00, 0x91)[j % 2])
    for j, bs in enumerate(shaped[:4]):
        n = len(bs[0][0])
        # the FF on lane 62, lane 63 (its second byte opens the next 64-byte step) and lane 0, in a later step
        for p in (126, 127, 128) if j % 2 == 0 or n < 330 else (62 + 64 * 4, 63 + 64 * 4, 64 * 5):
            edit("marker_at", bs, lambda s, off, p=p: fb.marker_at(s, p))
        # the FF on the last two bytes and the first byte of a 16-byte chunk of the blob
        for target in (14, 15, 0):
            edit("marker_at", bs, lambda s, off, g=target, j=j: fb.marker_at(s, (g - off) % 16 + 16 * (1 + j)))
    # fill the plan with family items of mixed lengths
    total = {"small": 300, "middle": 1100, "large": 4158}[plan]
    g = fb.Gen(len(plan))
    while len(specs) < total:
        r = g.raw(3)
        top = 256 if large else (16448 if r[2] < 3 else 640)
        fam(list(fb.FAMILIES)[r[0] % 4], 1 + (r[1] | r[2] << 8) % top)
    if large:  # two long blocks among the short ones: the lanes of one wavefront end far apart
        for at, kind in ((5, "ffdense"), (2100, "stuffed")):
            fam(kind, MAX_SEG, nb=30, shape=(64, 64), which=2)
            specs.insert(at, specs.pop())
    return specs


@functools.lru_cache(maxsize=None)
def _plan(oracle, plan):
    """The plan's block table, data blob, per-block references and coverage figures."""
    specs = _specs(oracle, plan)
    n = len(specs)
    blob = bytearray(b"\x00" * 15 + b"\xff")  # the byte before the first segment
    db = np.zeros(n, DEC_BLOCK)
    kinds, refs, segs = [], [], []
    dst_off = 0
    for i, (kind, make, after) in enumerate(specs):
        seg, npass, nbps, w, h, orient = make(len(blob))
        assert len(seg) <= MAX_SEG and 1 <= nbps <= 30 and 1 <= npass <= 3 * nbps - 2  # the entry point's contract
        irrev = i % 2
        db[i] = (len(blob), dst_off, len(seg), npass, nbps, w, h, orient, w, irrev, STEP if irrev else 0.0, 0)
        blob += seg
        if after is not None:
            assert seg[-1] == 0xFF
            blob.append(after)
        dst_off += w * h
        raw = oracle.t1_decode_cblk(seg, npass, nbps, w, h, orient) if seg else np.zeros((h, w), np.int32)
        refs.append(_post(raw, irrev, STEP))
        kinds.append(kind)
        segs.append(seg)
    blob += b"\xff" + bytes(31 - len(blob) % 16)  # whole 16-byte chunks past the last segment
    return dict(n=n, blob=bytes(blob), db=db, kinds=kinds, refs=refs, segs=segs, dst_len=dst_off)


def _coverage(p, plan):
    """What the plan must hold, from the bytes and the oracle alone."""
    segs, kinds, db = p["segs"], p["kinds"], p["db"]
    scans = [fb.scan(s) for s in segs]
    assert any(m is not None and m + 2 < len(s) for (m, _), s in zip(scans, segs)), "a marker before the segment's end"
    assert any(m is not None and m >= 64 and m % 64 == 63 for m, _ in scans), "a marker's FF on lane 63"
    assert {m % 64 for (m, _), k in zip(scans, kinds) if k == "marker_at" and m is not None and m >= 64} >= {62, 63, 0}
    assert {(int(b["data_off"]) + m) % 16 for (m, _), k, b in zip(scans, kinds, db)
            if k == "marker_at" and m is not None} >= {14, 15, 0}
    assert any(len(s) >= 2 and c == len(s) // 2 for (_, c), s in zip(scans, segs)), "len // 2 carry events"
    ends = {q % 32 for s, k in zip(segs, kinds) if k == "carrymax" for q in _carry_positions(s)}
    assert {31, 0} <= ends, "carry events on both sides of a word edge"
    assert kinds.count("trim") >= 5 and kinds.count("empty") == 1
    after = {p["blob"][int(b["data_off"]) + int(b["len"])] for b, k in zip(db, kinds) if k == "end_ff"}
    assert after >= {0x00, 0x91}
    for kind in fb.KINDS:
        assert any(k == kind and np.any(r) for k, r in zip(kinds, p["refs"])), "%s: no non-zero decode" % kind
    fam = [i for i, k in enumerate(kinds) if k in fb.FAMILIES]
    assert {int(db[i]["data_off"]) % 16 for i in fam} == set(range(16))
    assert {int(db[i]["irrev"]) for i in fam} == {0, 1}
    if plan == "large":
        assert p["n"] == 4160
        big = [i for i in range(p["n"]) if db[i]["len"] > 256]
        assert len(big) == 2 and all(db[i]["len"] == MAX_SEG and db[i]["numbps"] == 30 for i in big)
        rest = np.delete(db, big)
        assert rest["w"].max() <= 16 and rest["h"].max() <= 16 and rest["numbps"].max() <= 8
    else:
        assert (p["n"] <= 1024) == (plan == "small") and p["n"] <= 4096
        assert {len(segs[i]) for i in fam} >= set(LENGTHS)
        assert {int(db[i]["numbps"]) for i in fam} == set(NUMBPS)
        assert {(int(db[i]["h"]), int(db[i]["w"])) for i in fam} == set(SHAPES)


def _gpu_decode(p):
    import torch
    import grokimagecompression_amd as grk
    L = grk.lib()
    n = p["n"]
    dev = torch.device("cuda", 0)
    t_data = torch.from_numpy(np.frombuffer(p["blob"], np.uint8).copy()).to(dev)
    t_blocks = torch.from_numpy(p["db"].view(np.uint8)).to(dev)
    t_dst = torch.full((p["dst_len"] + 16,), SENTINEL, dtype=torch.int32, device=dev)
    t_scr = torch.empty(L.grkgpu_t1_scratch_bytes_n(n) + 256, dtype=torch.uint8, device=dev)
    s = ctypes.c_void_p(torch.cuda.current_stream(0).cuda_stream)
    grk._check(L.grkgpu_t1_decode_blocks(t_blocks.data_ptr(), n, t_data.data_ptr(), t_scr.data_ptr(),
                                         t_dst.data_ptr(), s))
    torch.cuda.synchronize()
    return t_dst.cpu().numpy()


def _compare(p, d):
    assert np.all(d[p["dst_len"]:] == SENTINEL)  # nothing past the last block
    bad = []
    for i, ref in enumerate(p["refs"]):  # every item, none skipped
        b = p["db"][i]
        o = int(b["dst_off"])
        got = d[o:o + ref.size].reshape(ref.shape)
        if not np.array_equal(got, ref):
            val = (lambda a: a.view(np.float32).astype(np.float64)) if b["irrev"] else (lambda a: a.astype(np.float64))
            bad.append((i, p["kinds"][i], int(b["len"]), int(b["data_off"]) % 16, int(b["numpasses"]), int(b["numbps"]),
                        int(b["w"]), int(b["h"]), int(b["irrev"]), float(np.abs(val(got) - val(ref)).max())))
    assert not bad, "%d of %d blocks differ (index, kind, len, offset mod 16, passes, numbps, w, h, 9/7, max abs): %s" % (
        len(bad), p["n"], bad[:12])


@pytest.mark.parametrize("plan", ["small", "middle", "large"])
def test_t1_decode_foreign_bytes(oracle, plan):
    """An empty segment (len == 0) leaves its block all zero: the rebuild
    writes every block, and a block with nothing decoded has no significant
    sample."""
    p = _plan(oracle, plan)
    _coverage(p, plan)
    _compare(p, _gpu_decode(p))


def test_t1_decode_foreign_bytes_16_per_wavefront(oracle):
    """The large plan's blocks at 16 per wavefront (grkgpu_dwt_options t1_dec_bpw)."""
    import grokimagecompression_amd as grk
    p = _plan(oracle, "large")
    _coverage(p, "large")
    with grk.dwt_options(t1_dec_bpw=16):
        d = _gpu_decode(p)
    _compare(p, d)


# ---------------------------------------------------------------- whole streams
@functools.lru_cache(maxsize=2)
def _image(shape, kind, seed):
    h, w, c, bits = shape
    img = synth.synth_image(h, w, c, bits, seed, kind)
    img.setflags(write=False)
    return img


def test_foreign_manifest_covers_the_cases():
    small = FOREIGN["small"]
    modes = {n: int(m["args"][m["args"].index("-M") + 1]) for n, m in small.items()}
    assert sorted(modes.values()) == [0, 1, 4, 5, 10, 63]
    for n, m in small.items():
        assert "-S" in m["args"] and "-E" in m["args"] and m["shape"][0] <= 96 and m["shape"][1] <= 128
        assert set(m["patterns"]) == set(fb.PATTERNS) and all(v["differs"] > 0 for v in m["patterns"].values())
    assert len(FOREIGN["many"]) == 2
    for n, m in FOREIGN["many"].items():
        assert set(m["patterns"]) == {"noise", "sparse"}


@pytest.mark.parametrize("name", sorted(FOREIGN["small"]))
def test_foreign_streams_vs_reference(codec, name):
    import grokimagecompression_amd as grk
    m = FOREIGN["small"][name]
    base = open(f"{GOLD}/{name}.j2k", "rb").read()
    assert hashlib.sha256(base).hexdigest() == m["j2k_sha256"]
    img = _image(tuple(m["shape"]), m["kind"], m["seed"])
    assert synth.image_sha256(img) == m["image_sha256"]
    p, off = grk.CParams.from_cli(m["args"])
    assert codec.compress(img, m["shape"][3], p, offset=off) == base  # our encoder writes the base byte for byte
    for pat, v in m["patterns"].items():
        cs = fb.overwrite_bodies(base, pat, v["seed"])
        assert hashlib.sha256(cs).hexdigest() == v["j2k_sha256"], (name, pat)
        ref = np.load(f"{GOLD}/{name}.{pat}.dec.npy")
        assert synth.image_sha256(ref) == v["dec_sha256"]
        for opts in ({}, dict(t1_dec_sort=1), dict(t1_dec_sort=1, t1_dec_bpw=16)):
            with grk.dwt_options(**opts):
                d = codec.decompress(cs)
            if not np.array_equal(d, ref):
                ys = np.argwhere(np.asarray(d) != ref)
                pytest.fail("%s %s %s: %d samples differ from the reference's decode, first at (c, y, x) = %s, max abs %d"
                            % (name, pat, opts, len(ys), tuple(ys[0]),
                               np.abs(np.asarray(d).astype(np.int64) - ref).max()))


@pytest.mark.parametrize("name", sorted(FOREIGN["many"]))
def test_foreign_many_block_streams_vs_reference(codec, name):
    import grokimagecompression_amd as grk
    m = FOREIGN["many"][name]
    img = _image(tuple(m["shape"]), m["kind"], m["seed"])
    assert synth.image_sha256(img) == m["image_sha256"]
    p, off = grk.CParams.from_cli(m["args"])
    base = codec.compress(img, m["shape"][3], p, offset=off)
    assert codec.stats()["num_cblks"] > 4096
    assert len(base) == m["j2k_len"] and hashlib.sha256(base).hexdigest() == m["j2k_sha256"]
    for pat, v in m["patterns"].items():
        cs = fb.overwrite_bodies(base, pat, v["seed"])
        assert hashlib.sha256(cs).hexdigest() == v["j2k_sha256"], (name, pat)
        for k, opts in enumerate(DEC_OPTS):
            with grk.dwt_options(**opts):
                d = codec.decompress(cs)
            if k == 0:
                assert codec.stats()["num_cblks"] > 4096
            assert synth.image_sha256(d) == v["dec_sha256"], (name, pat, opts)
