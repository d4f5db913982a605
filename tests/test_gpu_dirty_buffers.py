"""Buffer state as a test dimension: every entry point on dirty scratch, on a
dirtied context and after a different call.

The context keeps 20 grow-only device buffers, 13 pinned host buffers and the
pass records of the last encode, and clears almost none of them; the stage
entry points take caller scratch whose contents they must not depend on.  A
call is correct only if every word it reads was written earlier in the same
call ("Read-before-write").  The rest of the suite runs every call
after the same predecessor on one session Codec, on fresh scratch, with
zeroed outputs and tight strides, so a violation cannot show there.  Here:

  * stage entry points (T1 encode / decode, DWT both ways) with scratch,
    outputs and results filled with 0x00 / 0xFF / 0x55 (0xFF: every plane word
    "significant, refined, negative", every float NaN, every int -1; 0x55:
    alternating plane bits, a large finite float, a large positive int),
    guard bands around every buffer and row strides wider than the rows;
  * every kind of codec call right after Codec.debug_fill(byte)
    (grkgpu_debug_fill) on buffers a larger call has grown;
  * every kind of codec call after a different call, in four orders on fresh
    contexts, and chains of same-geometry calls (the kept pass records).

Every assertion is exact equality with the references the existing tests use:
oracle.t1_encode_cblk, oracle.t1_decode_cblk + _post, oracle.dwt_fwd / dwt_inv,
the host build of the encoder (tests/cpp/test_t1_model.cpp --encode) for styled
blocks, and the reference's goldens under tests/golden.

grkgpu_mct_inv_dcshift_to, grkgpu_upsample_to and grkgpu_dcshift_mct_fwd_from
have no case here: their existing tests already run them into a pre-filled
destination with a row stride wider than the row and check the samples
between the rows, before the first and after the last one
(test_gpu_decode_formats.py::test_stage_entry_point,
test_gpu_decode_upsample.py::test_stage_sweep, test_gpu_encode_layouts.py::
test_stage_alignment_sweep / test_stage_planar_sources); none of the three
takes scratch.
"""
import ctypes
import functools
import hashlib
import json
import struct

import numpy as np
import pytest

import synth
from conftest import GOLD, load_manifest
from prec_fixtures import PREC, image as prec_image, precs, ref_decode, sgnds, stream as prec_stream
from test_gpu_decode_upsample import assert_is, expected as sub_expected
from test_gpu_stages import DEC_BLOCK, _blocks, _post
from test_gpu_t1_model import ENC_BLOCK, ENC_RESULT, MAX_SEG, _mixed, host_encoder  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

FILLS = [0x00, 0xFF, 0x55]
SENTINEL = 0x5A5A5A5A
GUARD = 256  # sentinel words on each side of a guarded buffer
MAN = load_manifest()
MCT = json.load(open(f"{GOLD}/manifest_mct.json"))
CUT = json.load(open(f"{GOLD}/manifest_cut.json"))


def _filled(nbytes, fill, dev):
    import torch
    return torch.full((nbytes,), fill, dtype=torch.uint8, device=dev)


# ---------------------------------------------------------------------------
# 1. stage entry points
# ---------------------------------------------------------------------------

T1_STYLES = [0, 8 | 32, 1 | 4]  # none, VSC | SEGSYM, BYPASS | TERMALL
TAIL = 64                       # bytes of `out` past the last block's slab


@functools.lru_cache(maxsize=None)
def _enc_cases():
    return _mixed(130, 11)  # two full 64-block groups and a last group of two lanes


@pytest.fixture(scope="module")
def host_streams(host_encoder):  # noqa: F811
    """The host encoder's (numbps, passes, rates, bytes) per block, per style."""
    return {sty: host_encoder(_enc_cases(), sty) for sty in T1_STYLES}


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("sty", T1_STYLES)
def test_t1_encode_blocks_dirty(oracle, host_streams, sty, fill):
    """grkgpu_t1_encode_blocks_sty with scratch, out and results filled: the
    host encoder's streams (style 0: the oracle's too), pad == 0, and nothing
    of `out` written outside the blocks' slabs and their pad dwords."""
    import torch
    import grokimagecompression_amd as grk
    L = grk.lib()
    cases = _enc_cases()
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
    t_out = _filled(16 + n * (MAX_SEG + 16) + TAIL, fill, dev)
    t_res = _filled(n * ENC_RESULT.itemsize, fill, dev)
    t_scr = _filled(L.grkgpu_t1_scratch_bytes_n(n) + 256, fill, dev)
    s = ctypes.c_void_p(torch.cuda.current_stream(0).cuda_stream)
    grk._check(L.grkgpu_t1_encode_blocks_sty(t_blocks.data_ptr(), n, t_coef.data_ptr(), t_scr.data_ptr(),
                                             t_out.data_ptr(), t_res.data_ptr(), 0, sty, s))
    torch.cuda.synchronize()
    res = t_res.cpu().numpy().view(ENC_RESULT)
    out = t_out.cpu().numpy()
    host = host_streams[sty]
    for i, (h, w, orient, qmfbid, inv, blk) in enumerate(cases):
        nbps, npass, rates, data = host[i]
        if sty == 0:
            odata, passes, onb = oracle.t1_encode_cblk(blk, orient, qmfbid, inv)
            assert (nbps, npass, rates, data) == (onb, len(passes), [p[0] for p in passes], odata), i
        r = res[i]
        where = (sty, fill, i, w, h, orient)
        assert r["pad"] == 0, where
        assert r["numbps"] == nbps, where
        assert r["numpasses"] == npass, where
        assert r["len"] == len(data), where
        assert list(r["rate"][:npass]) == rates, where
        o = int(eb[i]["out_off"])
        assert bytes(out[o:o + len(data)]) == data, where
        # the 16 bytes before the slab: 12 untouched, then the block's pad dword
        assert (out[o - 16:o - 4] == fill).all(), where
    last = int(eb[n - 1]["out_off"]) + MAX_SEG
    assert last + 16 + TAIL == out.size and (out[last:] == fill).all()


@functools.lru_cache(maxsize=None)
def _dec_items():
    """test_t1_decode_blocks_vs_oracle's items (all, half and one pass of every
    block: a cut inside a bit-plane leaves a plane row partly decoded), with a
    zero-length block between the first two."""
    import pyoracle
    items, refs = [], []
    for (h, w, orient, qmfbid, inv, blk) in _blocks(4):
        data, passes, nbps = pyoracle.t1_encode_cblk(blk, orient, qmfbid, inv)
        if not passes:
            continue
        irrev = 1 if qmfbid == 0 else 0
        step = 0.0 if not irrev else 1.0 / (inv / 8192.0) / 4.0
        for npass in sorted({len(passes), max(1, len(passes) // 2), 1}):
            seg = data[:passes[npass - 1][0]]
            items.append((seg, npass, nbps, w, h, orient, irrev, step))
            refs.append(_post(pyoracle.t1_decode_cblk(seg, npass, nbps, w, h, orient), irrev, step))
    items.insert(1, (b"", 0, 0, 33, 47, 1, 0, 0.0))
    refs.insert(1, np.zeros((47, 33), np.int32))
    assert len(items) > 64 and len(items) % 64  # more than one group, a partial last one
    return items, refs


@pytest.mark.parametrize("fill", FILLS)
def test_t1_decode_blocks_dirty(oracle, fill):
    """grkgpu_t1_decode_blocks with the scratch filled and dst = a sentinel,
    rows dstride = w + 3 apart, no two blocks sharing a row: the oracle's
    samples inside every block (zeros for the empty one), the sentinel
    everywhere else."""
    import torch
    import grokimagecompression_amd as grk
    L = grk.lib()
    items, refs = _dec_items()
    n = len(items)
    blob = bytearray(16)
    db = np.zeros(n, DEC_BLOCK)
    dst_off = 5
    for i, (data, npass, nbps, w, h, orient, irrev, step) in enumerate(items):
        db[i] = (len(blob), dst_off, len(data), npass, nbps, w, h, orient, w + 3, irrev, step, 0)
        blob += data + bytes(16)
        dst_off += h * (w + 3)
    dev = torch.device("cuda", 0)
    t_data = torch.from_numpy(np.frombuffer(bytes(blob) + bytes(64), np.uint8).copy()).to(dev)
    t_blocks = torch.from_numpy(db.view(np.uint8)).to(dev)
    t_dst = torch.full((dst_off + 16,), SENTINEL, dtype=torch.int32, device=dev)
    t_scr = _filled(L.grkgpu_t1_scratch_bytes_n(n) + 256, fill, dev)
    s = ctypes.c_void_p(torch.cuda.current_stream(0).cuda_stream)
    grk._check(L.grkgpu_t1_decode_blocks(t_blocks.data_ptr(), n, t_data.data_ptr(), t_scr.data_ptr(),
                                         t_dst.data_ptr(), s))
    torch.cuda.synchronize()
    d = t_dst.cpu().numpy()
    outside = np.ones(d.size, bool)
    for i, ref in enumerate(refs):
        w, h, o = int(db[i]["w"]), int(db[i]["h"]), int(db[i]["dst_off"])
        rows = d[o:o + h * (w + 3)].reshape(h, w + 3)
        assert np.array_equal(rows[:, :w], ref), (fill, i, items[i][1:6])
        outside[o:o + h * (w + 3)].reshape(h, w + 3)[:, :w] = False
    assert (d[outside] == SENTINEL).all(), (fill, int(np.argmax(outside & (d != SENTINEL))))


DWT_SHAPES = [((33, 35), (1, 1)), ((77, 100), (3, 5)), ((129, 200), (1, 0)), ((1, 37), (0, 1)), ((45, 1), (1, 0)),
              ((2, 3), (1, 1))]
DWT_NUMRES = [1, 3, 6]
DWT_FAMILIES = {  # forced as tests/test_gpu_parity.py forces each kernel family
    "default": {},
    "fwd01": dict(f01_rows=4, f01_min_samples=0, pair_kernel=0),
    "pair": dict(pair_kernel=2, pair_min_samples=0),
    "inv01": dict(inv01=2, inv01_min_samples=0),
}


@functools.lru_cache(maxsize=None)
def _dwt_ref(shape_off, numres, irrev):
    """(forward input, oracle forward, inverse input, expected inverse)."""
    import pyoracle
    (h, w), (x0, y0) = shape_off
    rng = np.random.default_rng(h * 1000 + w + numres + 17 * irrev)
    mag = (1 << 20) if irrev else 4096
    a = rng.integers(-mag, mag, size=(h, w)).astype(np.int32)
    fwd = pyoracle.dwt_fwd(a, x0, y0, numres, irrev)
    if not irrev:  # 5/3 inverts the forward transform exactly
        return a, fwd, fwd, a
    f = (rng.standard_normal((h, w)) * 100).astype(np.float32).view(np.int32)
    return a, fwd, f, pyoracle.dwt_inv(f, x0, y0, numres, True)


def _guarded(words, fill_word, dev):
    """A tensor of GUARD sentinel words, `words` words of fill_word, GUARD
    sentinel words; returns (whole tensor, the middle slice)."""
    import torch
    whole = torch.full((GUARD + words + GUARD,), SENTINEL, dtype=torch.int32, device=dev)
    whole[GUARD:GUARD + words] = fill_word
    return whole, whole[GUARD:GUARD + words]


def _guards_intact(whole, words):
    g = whole.cpu().numpy()
    return (g[:GUARD] == SENTINEL).all() and (g[GUARD + words:] == SENTINEL).all()


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("family", sorted(DWT_FAMILIES))
@pytest.mark.parametrize("irrev", [False, True])
def test_dwt_stage_dirty(oracle, irrev, family, fill):
    """grkgpu_dwt_fwd / grkgpu_dwt_inv with the scratch filled, the buffer a
    slice of a larger tensor: the oracle's transform, and the 256 words before
    and after the buffer and before and after the scratch untouched."""
    import torch
    import grokimagecompression_amd as grk
    L = grk.lib()
    dev = torch.device("cuda", 0)
    fill_word = int(np.array([fill] * 4, np.uint8).view(np.int32)[0])
    for shape_off in DWT_SHAPES:
        (h, w), (x0, y0) = shape_off
        for numres in DWT_NUMRES:
            a, fwd, inv_in, inv_out = _dwt_ref(shape_off, numres, irrev)
            need = L.grkgpu_dwt_scratch_bytes(x0, y0, x0 + w, y0 + h, numres)
            assert need and need % 4 == 0
            for src, want, call in ((a, fwd, grk.dwt_fwd), (inv_in, inv_out, grk.dwt_inv)):
                buf_all, buf = _guarded(h * w, 0, dev)
                buf.copy_(torch.from_numpy(src.ravel()).to(dev))
                scr_all, scr = _guarded(need // 4, fill_word, dev)
                with grk.dwt_options(**DWT_FAMILIES[family]):
                    call(buf.view(h, w), x0, y0, numres, irrev, scratch=scr)
                    torch.cuda.synchronize()
                where = (irrev, family, fill, shape_off, numres, call.__name__)
                assert np.array_equal(buf.cpu().numpy().reshape(h, w), want), where
                assert _guards_intact(buf_all, h * w), where
                assert _guards_intact(scr_all, need // 4), where


def test_dwt_scratch_argument_checked():
    """scratch=: too small a tensor is refused before any launch."""
    import torch
    import grokimagecompression_amd as grk
    t = torch.zeros((33, 35), dtype=torch.int32, device="cuda:0")
    need = grk.lib().grkgpu_dwt_scratch_bytes(0, 0, 35, 33, 3)
    with pytest.raises(grk.GrkGpuError):
        grk.dwt_fwd(t, 0, 0, 3, False, scratch=torch.zeros(need // 4 - 1, dtype=torch.int32, device="cuda:0"))


# ---------------------------------------------------------------------------
# 4. / 5. whole calls
# ---------------------------------------------------------------------------

def _gold(name):
    with open(f"{GOLD}/{name}.j2k", "rb") as f:
        return f.read()


@functools.lru_cache(maxsize=None)
def _man_image(name):
    m = MAN.get(name) or MCT[name]
    h, w, c, bits = m["shape"]
    img = synth.synth_image(h, w, c, bits, m["seed"], m["kind"])
    assert synth.image_sha256(img) == m["image_sha256"]
    img.setflags(write=False)
    return img, bits, m["args"]


@functools.lru_cache(maxsize=None)
def _dec_gold(name, tag=""):
    d = np.load(f"{GOLD}/{name}{'.' + tag if tag else ''}.dec.npy")
    d.setflags(write=False)
    return d


def _tile_parts(cs, begin, end):
    """The bytes of the tile-parts of tiles [begin, end) of a codestream whose
    tile-parts come in tile order (walk of the SOT markers' Psot)."""
    pos = cs.index(b"\xff\x90")
    assert cs[pos + 2:pos + 4] == b"\x00\x0a"
    out = b""
    while cs[pos:pos + 2] == b"\xff\x90":
        isot, psot = struct.unpack(">HI", cs[pos + 4:pos + 10])
        assert psot
        if begin <= isot < end:
            out += cs[pos:pos + psot]
        pos += psot
    assert cs[pos:pos + 2] == b"\xff\xd9"
    return out


def _enc_plain(name):
    def run(codec):
        import grokimagecompression_amd as grk
        img, bits, args = _man_image(name)
        p, off = grk.CParams.from_cli(args)
        b = codec.compress(img, bits, p, offset=off)
        assert b == _gold(name), name
    return run


def _enc_prec(name):
    def run(codec):
        import grokimagecompression_amd as grk
        m = PREC[name]
        assert all(sgnds(m))
        p, off = grk.CParams.from_cli(m["args"])
        one = lambda v: v[0] if len(set(v)) == 1 else v  # noqa: E731
        b = codec.compress(prec_image(m), one(precs(m)), p, offset=off, sgnd=one(sgnds(m)))
        assert b == prec_stream(name), name
    return run


def _enc_u8_hwc(name):
    def run(codec):
        import grokimagecompression_amd as grk
        img, bits, args = _man_image(name)
        p, off = grk.CParams.from_cli(args)
        px = np.ascontiguousarray(img.astype(np.uint8).transpose(1, 2, 0))
        assert codec.compress(px, bits, p, offset=off, layout="hwc") == _gold(name), name
    return run


def _enc_fuse(name, fuse):
    def run(codec):
        import grokimagecompression_amd as grk
        with grk.dwt_options(fuse_level0=fuse):
            _enc_plain(name)(codec)
    return run


def _enc_tiles(name, begin, end):
    def run(codec):
        import grokimagecompression_amd as grk
        img, bits, args = _man_image(name)
        p, off = grk.CParams.from_cli(args)
        assert 0 < begin < end < grk.num_tiles(img.shape, bits, p, off)
        b = codec.compress_tiles(img, bits, p, begin, end, grk.PART_TILES, offset=off)
        assert b == _tile_parts(_gold(name), begin, end), name
    return run


def _dec_plain(name, tag="", **kw):
    def run(codec):
        ref = _dec_gold(name, tag)
        d = codec.decompress(_gold(name), **kw)
        assert d.dtype == np.int32 and d.shape == ref.shape and np.array_equal(d, ref), (name, tag)
    return run


def _dec_prec(name):
    def run(codec):
        ref = ref_decode(name)
        d = codec.decompress(prec_stream(name))
        assert d.shape == ref.shape and np.array_equal(d, ref), name
    return run


def _dec_reduce_oracle(name, reduce):
    """A -r decode no reference golden exists for: the oracle's reduced decode,
    as tests/test_gpu_parity.py::test_reduced_decode_matches_oracle."""
    def run(codec):
        import pyoracle
        ref = pyoracle.decode(_gold(name), reduce=reduce)
        d = codec.decompress(_gold(name), reduce=reduce)
        assert d.shape == ref.shape and np.array_equal(d, ref), (name, reduce)
    return run


def _dec_cut(name, n, ntiles):
    def run(codec):
        want = CUT[name]["cuts"][str(n)]
        assert 0 < len(want["tiles"]) < ntiles  # only some tiles were reached
        out = codec.decompress(_gold(name)[:n])
        assert hashlib.sha256(np.ascontiguousarray(out, dtype=np.int32).tobytes()).hexdigest() == want["sha"], (name, n)
    return run


def _dec_upsample(tag):
    def run(codec):
        ref, _ = sub_expected(tag)
        got = codec.decompress(_gold(tag), upsample=True, dtype=np.uint16, layout="hwc")
        assert_is(got, ref, np.uint16, "hwc")
    return run


def _dec_u8(name):
    def run(codec):
        ref = _dec_gold(name)
        d = codec.decompress(_gold(name), dtype=np.uint8)
        assert d.dtype == np.uint8 and np.array_equal(d, ref), name
    return run


def _dec_tiles_device(name, begin, end, tile=64):
    def run(codec):
        import torch
        ref = _dec_gold(name)
        out = torch.full(ref.shape, SENTINEL, dtype=torch.int32, device="cuda:%d" % codec.device)
        codec.decompress_tiles(_gold(name), begin, end, out)
        got = out.cpu().numpy()
        tw = -(-ref.shape[2] // tile)
        want = np.full(ref.shape, SENTINEL, np.int32)
        for t in range(begin, end):
            ys, xs = slice(t // tw * tile, (t // tw + 1) * tile), slice(t % tw * tile, (t % tw + 1) * tile)
            want[:, ys, xs] = ref[:, ys, xs]
        assert (want != SENTINEL).any() and (want == SENTINEL).any()
        assert np.array_equal(got, want), name
    return run


BIG = "rgb12_M46_tiles"  # the largest case of either direction: 150 x 200 x 3, 12 tiles
SIGNED = "p_rgb5s_I"
MAN_ENC = ["g8_3x5", "g8_const_64", "g8_off_tiles", "rgb12_tiles_I", "rgb8_r20_I", "rgb12_cinema2k", "g12_M63",
           "g16_M5_lazy_termall", "g8_roi_U5", "rgb8_poc_r15_I", "g12_prec_r12_A1", "rgb8_tp_L"]
CASES = {}
for _n in MAN_ENC:
    CASES["enc-" + _n] = _enc_plain(_n)
CASES["enc-mct_rgba8_m4_tiles"] = _enc_plain("mct_rgba8_m4_tiles")
CASES["enc-" + SIGNED] = _enc_prec(SIGNED)
CASES["enc-rgb8_128x96-u8-hwc"] = _enc_u8_hwc("rgb8_128x96")
CASES["enc-rgb12_I-fuse1"] = _enc_fuse("rgb12_I", 1)
CASES["enc-rgb12_I-fuse0"] = _enc_fuse("rgb12_I", 0)
CASES["enc-g8_tiles64-tiles5_9"] = _enc_tiles("g8_tiles64", 5, 9)
# every encode case with a decode golden (the custom-MCT stream is refused by the reference's decoder)
for _n in MAN_ENC + ["rgb8_128x96", "rgb12_I", "g8_tiles64"]:
    CASES["dec-" + _n] = _dec_plain(_n)
CASES["dec-" + SIGNED] = _dec_prec(SIGNED)
CASES["dec-g12_M4_layers-l1"] = _dec_plain("g12_M4_layers", "l1", layers=1)  # passes cut, blocks with none at all
CASES["dec-g16_128-r2"] = _dec_reduce_oracle("g16_128", 2)
CASES["dec-g16_128-r2-window"] = _dec_plain("g16_128", "r2d33_20_100_99", reduce=2, window=(33, 20, 100, 99))
CASES["dec-rgb12_I-r1-window"] = _dec_plain("rgb12_I", "r1d9_13_70_61", reduce=1, window=(9, 13, 70, 61))
CASES["dec-g16_128.gb3"] = _dec_plain("g16_128.gb3")
CASES["dec-mk_ppt_tparts"] = _dec_plain("mk_ppt_tparts")
CASES["dec-mk_mixed_wavelet"] = _dec_plain("mk_mixed_wavelet")  # both DWT job tables in one call
CASES["dec-mk_mixed_cblksty"] = _dec_plain("mk_mixed_cblksty")
CASES["dec-g8_tiles64-cut11545"] = _dec_cut("g8_tiles64", 11545, 12)      # 6 of 12 tiles reached
CASES["dec-rgb12_M46_tiles-cut81894"] = _dec_cut(BIG, 81894, 12)       # 7 of 12, the last cut inside its data
CASES["dec-sub_422_I_tiles-up-u16-hwc"] = _dec_upsample("sub_422_I_tiles")
CASES["dec-rgb8_128x96-u8"] = _dec_u8("rgb8_128x96")
CASES["dec-g8_tiles64-tiles1_3-device"] = _dec_tiles_device("g8_tiles64", 1, 3)
WARMUP = {"enc": _enc_plain(BIG), "dec": _dec_plain(BIG)}


@pytest.fixture(scope="module")
def own_codec():
    import grokimagecompression_amd as grk
    c = grk.Codec(0)
    yield c
    c.close()


def test_debug_fill_reaches_the_buffers(own_codec):
    """The hook fills at least what one call of each direction has grown, and
    fills nothing on a fresh context."""
    import grokimagecompression_amd as grk
    fresh = grk.Codec(0)
    assert fresh.debug_fill(0xFF) == 0
    fresh.close()
    WARMUP["enc"](own_codec)
    img, _, _ = _man_image(BIG)
    n_enc = own_codec.debug_fill(0x55)
    assert n_enc > 2 * img.size * 4  # at least the two coefficient arenas
    WARMUP["dec"](own_codec)
    assert own_codec.debug_fill(0x55) >= n_enc
    # the pinned output buffer of a compress: still the context's after the
    # call, so the fill lands in the very bytes the call returned
    img, bits, args = _man_image("g8_3x5")
    d, pl, keep = own_codec._image(img, bits, (0, 0), False)
    out, n = ctypes.POINTER(ctypes.c_uint8)(), ctypes.c_size_t()
    grk._check(grk.lib().grkgpu_compress_ex(own_codec._ctx, ctypes.byref(d), ctypes.byref(grk.CParams.from_cli(args)[0]),
                                            ctypes.byref(pl), 0, 0xFFFFFFFF, grk.PART_ALL, ctypes.byref(out),
                                            ctypes.byref(n)))
    assert ctypes.string_at(out, n.value) == _gold("g8_3x5")
    own_codec.debug_fill(0xA5)
    assert ctypes.string_at(out, n.value) == b"\xa5" * n.value


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_call_on_dirty_context(oracle, own_codec, case, fill):
    """One warm-up call of the largest case of the direction (so that every
    buffer is larger than the call needs), debug_fill(fill), then the call:
    the golden, exactly."""
    WARMUP[case[:3]](own_codec)
    assert own_codec.debug_fill(fill) > 0
    CASES[case](own_codec)


@pytest.mark.parametrize("irrev", [False, True])
@pytest.mark.parametrize("fill", FILLS)
def test_single_resolution_tiles_on_dirty_context(oracle, own_codec, fill, irrev):
    """One resolution (-n 1) has no DWT: a copy per tile-component moves the
    samples between the two arenas, and each has to move its own
    tile-component's sample count -- 150 x 200 in tiles of 64 x 64 has edge
    tiles of three other sizes, the last one the smallest.  (Found by the
    read-before-write audit: one count, the last tile-component's, served every
    copy, so the rest of every larger tile was whatever the arena held.)  The
    oracle's codestream and decode; 5/3 restores the image."""
    import grokimagecompression_amd as grk
    img = synth.synth_image(150, 200, 3, 8, 77)
    p = grk.CParams.make(numresolution=1, irreversible=irrev, tiles=(64, 64))
    ref = oracle.encode(img, 8, oracle.params(numres=1, irreversible=irrev, tiles=(64, 64)))
    WARMUP["enc"](own_codec)
    own_codec.debug_fill(fill)
    assert own_codec.compress(img, 8, p) == ref
    WARMUP["dec"](own_codec)
    own_codec.debug_fill(fill)
    d = own_codec.decompress(ref)
    assert np.array_equal(d, oracle.decode(ref))
    if not irrev:
        assert np.array_equal(d, img)


def _interleaved():
    enc = [c for c in CASES if c.startswith("enc-")]
    dec = [c for c in CASES if c.startswith("dec-")]
    out = []
    for i in range(max(len(enc), len(dec))):
        out += enc[i:i + 1] + dec[i:i + 1]
    assert sorted(out) == sorted(CASES)
    return out


ORDER_SEEDS = {"shuffle-a": 20240607, "shuffle-b": 977}


@pytest.mark.parametrize("order", ["listed", "reversed"] + sorted(ORDER_SEEDS))
def test_call_order_does_not_matter(oracle, order):
    """Every case above on one fresh Codec, encodes and decodes interleaved,
    in the listed order, reversed and in two seeded permutations: real
    leftovers, growth from empty and reallocation in the middle of a run."""
    import grokimagecompression_amd as grk
    names = _interleaved()
    if order == "reversed":
        names = names[::-1]
    elif order != "listed":
        names = [names[i] for i in np.random.default_rng(ORDER_SEEDS[order]).permutation(len(names))]
    codec = grk.Codec(0)
    try:
        for prev, name in zip([None] + names, names):
            try:
                CASES[name](codec)
            except AssertionError as e:
                raise AssertionError("%s after %s (%s): %s" % (name, prev, order, e)) from e
    finally:
        codec.close()


# 96 x 128 goldens that share one block table: what the pass records kept
# between encodes (enc_passes), h_results and the symbol slots expose
CHAIN_GRAY = ["g8_M2_reset", "g8_M4_termall", "g8_M1_lazy", "g8_M32_segsym", "g8_r40_20_10", "g8_sop_eph", "g8_q30",
              "g8_roi_U5"]
CHAIN_RGB = ["rgb8_M62_I_r", "rgb8_M1_I_r", "rgb8_r20_I", "rgb8_roi_c1_I_r", "rgb8_poc"]
# the case with the most passes and codeword segments of each family
CHAINS = {"gray": (CHAIN_GRAY, "g8_M4_termall"), "rgb": (CHAIN_RGB, "rgb8_M62_I_r")}


@pytest.mark.parametrize("order", ["listed", "reversed", "after-heaviest"])
@pytest.mark.parametrize("family", sorted(CHAINS))
def test_same_geometry_chain(family, order):
    """Encode and decode the same-geometry goldens back to back on one fresh
    Codec: as listed, reversed, and each one directly after the family's
    heaviest (TERMALL: the most passes and segments per block)."""
    import grokimagecompression_amd as grk
    names, heavy = CHAINS[family]
    assert len({tuple(MAN[n]["shape"]) for n in names}) == 1
    if order == "reversed":
        seq = names[::-1]
    elif order == "after-heaviest":
        seq = [x for n in names if n != heavy for x in (heavy, n)]
    else:
        seq = list(names)
    codec = grk.Codec(0)
    try:
        for prev, name in zip([None] + seq, seq):
            try:
                _enc_plain(name)(codec)
                _dec_plain(name)(codec)
            except AssertionError as e:
                raise AssertionError("%s after %s: %s" % (name, prev, e)) from e
    finally:
        codec.close()


def test_multi_workers_keep_their_contexts():
    """compress_multi / decompress_multi over two workers on device 0: the
    small tiled golden directly after the large one on the contexts the
    workers keep between calls."""
    import grokimagecompression_amd as grk
    for name in (BIG, "g8_tiles64"):
        img, bits, args = _man_image(name)
        p, off = grk.CParams.from_cli(args)
        assert grk.compress_multi(img, bits, p, devices=[0, 0], offset=off) == _gold(name), name
        assert np.array_equal(grk.decompress_multi(_gold(name), devices=[0, 0]), _dec_gold(name)), name
