"""JP2 box layer on the host (csrc/jp2.cpp, grkgpu_jp2_read_info / _read_palette
/ _write_boxes): no GPU.  The fixtures (scripts/make_golden_jp2.py) are pinned
by the reference: files it encodes (A), files assembled around its codestreams
that it decodes (B), files it refuses (C)."""
import ctypes
import hashlib
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
HAVE_REF = os.path.isdir("/root/reference/src/lib/jp2")
MAN = json.load(open(os.path.join(GOLD, "manifest_jp2.json")))
AB = sorted(t for t, r in MAN.items() if r["kind"] in "AB")
A = sorted(t for t, r in MAN.items() if r["kind"] == "A")
C = sorted(t for t, r in MAN.items() if r["kind"] == "C")
FUZZED = ["jp2_b_pal_direct_alpha", "jp2_b_pal8_cdef_swap", "jp2_b_extra_boxes"]
EINVAL, EUNSUPPORTED, ECORRUPT = -1, -4, -5


def _grk():
    import grokimagecompression_amd as grk
    return grk


def load(tag):
    with open(os.path.join(GOLD, tag + ".jp2"), "rb") as f:
        return f.read()


def read_info_rc(data):
    grk = _grk()
    ji, d = grk.Jp2Info(), grk.ImageDesc()
    return grk.lib().grkgpu_jp2_read_info(data, len(data), ctypes.byref(ji), ctypes.byref(d)), ji, d


def test_library_exports_jp2():
    L = _grk().lib()
    for sym in ("grkgpu_jp2_read_info", "grkgpu_jp2_read_palette", "grkgpu_jp2_decompress", "grkgpu_jp2_compress",
                "grkgpu_jp2_write_boxes", "grkgpu_palette_to"):
        assert hasattr(L, sym), sym


@pytest.mark.skipif(not HAVE_REF, reason="reference sources not present (GPU box)")
def test_jp2_fixtures_regenerate():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "make_golden_jp2.py"), "--check"], cwd=ROOT,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "mismatches 0" in r.stdout


def test_fixture_files_are_the_manifests():
    for tag, rec in MAN.items():
        data = load(tag)
        assert hashlib.sha256(data).hexdigest() == rec["sha256"] and len(data) == rec["len"], tag
        assert len(data) < 16384, tag


@pytest.mark.parametrize("tag", AB)
def test_jp2_info_matches_the_reference(tag):
    """payload offset, colour space, channel list, palette and ICC bytes against what the reference's decode reported"""
    grk = _grk()
    rec, data = MAN[tag], load(tag)
    info = grk.jp2_info(data)
    e = rec["expect"]
    off, n = info["codestream"]
    assert off == rec["cs_offset"] and data[off:off + 2] == b"\xff\x4f" and off + n <= len(data)
    assert grk.COLOUR_SPACES[info["colour_space"]] == e["colour_space"]
    got = [(c["prec"], int(c["sgnd"]), c["alpha"]) for c in info["channels"]]
    assert got == [(c["prec"], c["sgnd"], c["alpha"]) for c in e["comps"]]
    icc = info["icc"] or b""
    assert len(icc) == e["icc_len"]
    if e["icc_len"]:
        assert hashlib.sha256(icc).hexdigest() == e["icc_sha256"]
    if rec["palette"]:
        p, want = info["palette"], rec["palette"]
        assert p["entries"].shape == (want["ne"], want["npc"]) and p["prec"] == want["sizes"]
        assert hashlib.sha256(p["entries"].astype("<u2").tobytes()).hexdigest() == want["entries_sha256"]
        assert [list(t) for t in p["cmap"]] == want["cmap"]
        for c in info["channels"]:
            assert c["pcol"] is None or c["pcol"] < want["npc"]
        assert info["mapped"]
    else:
        assert info["palette"] is None
    # the image description holds the output channels
    rc, ji, d = read_info_rc(data)
    assert rc == 0 and d.numcomps == len(e["comps"])
    assert [d.x0, d.y0, d.x1, d.y1] == e["rect"]
    for k, c in enumerate(e["comps"]):
        assert (d.prec[k], d.sgnd[k], d.dx[k], d.dy[k]) == (c["prec"], c["sgnd"], c["dx"], c["dy"])


def test_channel_sources():
    """which component / palette column feeds each channel, after the cdef swaps"""
    grk = _grk()
    src = lambda tag: [(c["comp"], c["pcol"]) for c in grk.jp2_info(load(tag))["channels"]]  # noqa: E731
    assert src("jp2_b_pal8") == [(0, 0), (0, 1), (0, 2)]
    assert src("jp2_b_pal_weird_cmap") == [(0, 0), (0, 1), (0, 2)]
    assert src("jp2_b_pal_direct_alpha") == [(0, 0), (0, 1), (0, 2), (1, None)]
    assert src("jp2_b_cdef_bgr") == [(2, None), (1, None), (0, None)]
    assert src("jp2_b_pal8_cdef_swap") == [(0, 2), (0, 1), (0, 0)]
    assert src("jp2_b_pclr_no_cmap") == [(0, None)]
    assert not grk.jp2_info(load("jp2_b_pclr_no_cmap"))["mapped"]
    assert grk.jp2_info(load("jp2_b_cielab_default"))["cielab"] == [14, 0x44454600]


@pytest.mark.parametrize("tag", C)
def test_refused_where_the_reference_refuses(tag):
    rc, _, _ = read_info_rc(load(tag))
    assert rc == ECORRUPT, _grk().lib().grkgpu_last_error()


def test_raw_codestream_is_corrupt_and_jp2_is_no_codestream():
    grk = _grk()
    data = load("jp2_a_gray8")
    off, n = grk.jp2_info(data)["codestream"]
    rc, _, _ = read_info_rc(data[off:off + n])
    assert rc == ECORRUPT
    d = grk.ImageDesc()
    assert grk.lib().grkgpu_read_header(data, len(data), ctypes.byref(d)) != 0  # as before this file format existed


# ---- deliberate narrowings: files the reference decodes, hand-built around a fixture's codestream ----
def _box(typ, payload=b""):
    return struct.pack(">I", 8 + len(payload)) + typ + payload


def _file(header_boxes, cs, jp2c=None):
    sig = _box(b"jP  ", b"\x0d\x0a\x87\x0a") + _box(b"ftyp", b"jp2 \0\0\0\0jp2 ")
    return sig + _box(b"jp2h", b"".join(header_boxes)) + (jp2c if jp2c is not None else _box(b"jp2c", cs))


def _pclr(ne, sizes_bytes, entry_bytes):
    return _box(b"pclr", struct.pack(">HB", ne, len(sizes_bytes)) + bytes(sizes_bytes) + entry_bytes)


def _cmap(triples):
    return _box(b"cmap", b"".join(struct.pack(">HBB", *t) for t in triples))


def _payload(tag):
    data = load(tag)
    off, n = _grk().jp2_info(data)["codestream"]
    return data[off:off + n]


def test_deliberately_unsupported():
    """Every narrowing but one: the refusal of a jp2c payload of 4 GiB or more
    is not tested -- the payload's length is clamped to the file's, so only a
    real file of that size reaches the branch (jp2_read_boxes, csrc/jp2.cpp)."""
    g8 = _payload("jp2_b_pal8")          # one 8-bit component, 40 x 52
    two = _payload("jp2_b_pal_direct_alpha")  # two 8-bit components
    sub = _payload("jp2_a_sycc420_12")   # components 1, 2 at (2,2)
    ih = lambda nc, bpc=7, h=40, w=52: _box(b"ihdr", struct.pack(">IIHBBBB", h, w, nc, bpc, 7, 0, 0))  # noqa: E731
    colr = _box(b"colr", bytes([1, 0, 0]) + struct.pack(">I", 16))
    cases = {
        "17 columns": _file([ih(1), colr, _pclr(2, [7] * 17, bytes(34)), _cmap([(0, 1, i) for i in range(17)])], g8),
        "17-bit column": _file([ih(1), colr, _pclr(2, [16, 7, 7], bytes(2 * 5)), _cmap([(0, 1, 0), (0, 1, 1), (0, 1, 2)])],
                               g8),
        "signed column": _file([ih(1), colr, _pclr(2, [0x87, 7, 7], bytes(6)), _cmap([(0, 1, 0), (0, 1, 1), (0, 1, 2)])],
                               g8),
        "pcol not own index": _file([ih(2), colr, _pclr(2, [7, 7], bytes(4)), _cmap([(0, 1, 1), (1, 1, 0)])], two),
        "cmap over a subsampled component": _file([ih(3, 11, 48, 64), colr, _pclr(2, [7, 7, 7], bytes(6)),
                                                   _cmap([(1, 1, 0), (1, 1, 1), (1, 1, 2)])], sub),
        "cdef swap on a subsampled image": _file([ih(3, 11, 48, 64), colr,
                                                  _box(b"cdef", struct.pack(">H", 3) + struct.pack(">HHH", 0, 0, 3) +
                                                       struct.pack(">HHH", 1, 0, 2) + struct.pack(">HHH", 2, 0, 1))], sub),
        "65 channel definitions": _file([ih(1), colr, _box(b"cdef", struct.pack(">H", 65) +
                                                           struct.pack(">HHH", 0, 0, 1) * 65)], g8),
    }
    L = _grk().lib()
    for name, data in cases.items():
        rc, _, _ = read_info_rc(data)
        assert rc == EUNSUPPORTED, (name, rc, L.grkgpu_last_error())
        assert L.grkgpu_last_error(), name


def test_argument_checks_come_before_the_device():
    grk = _grk()
    L = grk.lib()
    data = load("jp2_b_pal8")
    ctx = ctypes.c_void_p(1)  # never dereferenced
    ji = grk.Jp2Info()
    assert L.grkgpu_jp2_read_info(None, 0, ctypes.byref(ji), None) == EINVAL
    assert L.grkgpu_jp2_read_info(data, len(data), None, None) == EINVAL
    n = ctypes.c_uint32()
    small = (ctypes.c_uint16 * 4)()
    assert L.grkgpu_jp2_read_palette(data, len(data), small, 4, ctypes.byref(n)) == EINVAL and n.value == 768
    for out in (None, ctypes.byref(grk.OutPlanes(sample_fmt=5)), ctypes.byref(grk.OutPlanes(sample_fmt=1, layout=2))):
        assert L.grkgpu_jp2_decompress(ctx, data, len(data), None, 0, 0xFFFFFFFF, None, out, None, None) == EINVAL
    op = grk.OutPlanes(sample_fmt=1)
    bad = grk.OutOps(colour=3)
    assert L.grkgpu_jp2_decompress(ctx, data, len(data), None, 0, 0xFFFFFFFF, None, ctypes.byref(op), ctypes.byref(bad),
                                   None) == EINVAL
    # AUTO belongs to the JP2 entry point alone
    auto = grk.OutOps(colour=grk.COLOUR_AUTO)
    cs = _payload("jp2_b_pal8")
    assert L.grkgpu_decompress_convert(ctx, cs, len(cs), None, 0, 0xFFFFFFFF, None, ctypes.byref(op),
                                       ctypes.byref(auto)) == EINVAL
    # a damaged file is refused before the context is looked at
    assert L.grkgpu_jp2_decompress(ctx, data[:40], 40, None, 0, 0xFFFFFFFF, None, ctypes.byref(op), None, None) == ECORRUPT
    with pytest.raises(grk.GrkGpuError):
        grk.jp2_boxes((3, 8, 8), 8, 10, "icc")  # the ICC colour space needs its profile
    with pytest.raises(grk.GrkGpuError):
        grk.jp2_boxes((3, 8, 8), 8, 10, "no such space")


@pytest.mark.parametrize("tag", A)
def test_writer_boxes_equal_the_reference_files_prefix(tag):
    """our boxes for the same image = the bytes the reference wrote ahead of its codestream"""
    grk = _grk()
    rec, data = MAN[tag], load(tag)
    h, w, c, bits = rec["spec"]["shape"]
    args = rec["spec"]["args"]
    val = lambda o: [int(v) for v in args[args.index(o) + 1].split(",")] if o in args else None  # noqa: E731
    names = {v: k for k, v in grk.COLOUR_SPACES.items()}
    off = rec["cs_offset"]
    icc = bytes((i * 7 + 3) & 0xFF for i in range(300)) if "-icc" in args else None
    boxes = grk.jp2_boxes((c, h, w), val("-prec") or bits, len(data) - off, names[rec["spec"]["colour_space"]], icc,
                          val("-alpha"), sgnd=bool(rec["spec"]["sgnd"]))
    assert boxes == data[:off]


@pytest.mark.parametrize("tag", FUZZED)
def test_truncations_and_corruptions_return_a_code(tag):
    """every truncation and 5,000 seeded random corruptions of the first 600
    bytes: a return code, no crash; an accepted palette lies inside its table"""
    grk = _grk()
    L = grk.lib()
    data = load(tag)
    codes = set()

    def run(buf):
        ji, d = grk.Jp2Info(), grk.ImageDesc()
        rc = L.grkgpu_jp2_read_info(buf, len(buf), ctypes.byref(ji), ctypes.byref(d))
        assert rc in (0, EUNSUPPORTED, ECORRUPT), rc
        codes.add(rc)
        if rc == 0:
            assert 1 <= ji.numchannels <= 16 and ji.cs_offset + ji.cs_length <= len(buf)
            n = ctypes.c_uint32()
            tab = (ctypes.c_uint16 * (1024 * 16))()
            assert L.grkgpu_jp2_read_palette(buf, len(buf), tab, len(tab), ctypes.byref(n)) == 0
            assert n.value == ji.pal_entries * ji.pal_columns
            for k in range(ji.numchannels):
                assert ji.chan_pcol[k] < int(ji.pal_columns)
        return rc
    assert run(data) == 0
    for n in range(len(data)):
        run(data[:n])
    r = np.random.RandomState(len(data))
    for _ in range(5000):
        b = bytearray(data)
        for _ in range(r.randint(1, 4)):
            b[r.randint(0, min(600, len(b)))] = r.randint(0, 256)
        run(bytes(b))
    assert ECORRUPT in codes


def test_parser_survives_damaged_files_sanitized(tmp_path):
    """tests/cpp/jp2_parse_check.cpp under AddressSanitizer + UBSan: a host
    program of its own over the same truncations and corruptions"""
    exe = tmp_path / "jp2_parse_check"
    c = os.path.join(ROOT, "grokimagecompression_amd", "csrc")
    subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-std=c++17",
                    "-I" + c, "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "jp2_parse_check.cpp"),
                    os.path.join(c, "jp2.cpp"), os.path.join(c, "codestream.cpp")], check=True)
    r = subprocess.run([str(exe)] + [os.path.join(GOLD, n + ".jp2") for n in FUZZED], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("accepted") == len(FUZZED)


def test_python_mirror_keywords():
    import inspect
    grk = _grk()
    sig = inspect.signature(grk.Codec.decompress_jp2).parameters
    for kw in ("dtype", "layout", "colour", "out_prec", "prec_mode", "window", "reduce", "layers", "device_out"):
        assert kw in sig, kw
    assert sig["colour"].default == "auto"
    sig = inspect.signature(grk.Codec.compress_jp2).parameters
    for kw in ("colour_space", "icc", "alpha"):
        assert kw in sig, kw
