"""JP2 files on the GPU: Codec.compress_jp2 / decompress_jp2 against the files
the reference encoded and the reference's decodes (tests/golden/jp2_*,
scripts/make_golden_jp2.py), and the palette store (k_palette_planar /
k_palette_pixels) through every format, layout and destination.  Every
comparison is equality with the reference's bytes or samples."""
import numpy as np
import pytest

import jp2_fixtures as jf

pytestmark = pytest.mark.gpu


def _grk():
    import grokimagecompression_amd as grk
    return grk


def payload(tag):
    data = jf.load(tag)
    off, n = _grk().jp2_info(data)["codestream"]
    return data[off:off + n]


def as_planes(out):
    return [np.asarray(p, dtype=np.int32) for p in out]


@pytest.mark.parametrize("tag", jf.A)
def test_compress_jp2_equals_the_reference_file(codec, tag):
    grk = _grk()
    spec = jf.MAN[tag]["spec"]
    h, w, c, bits = spec["shape"]
    params, _ = grk.CParams.from_cli(jf.codec_args(spec["args"]))
    names = {v: k for k, v in grk.COLOUR_SPACES.items()}
    planes = jf.source_planes(tag)
    kw = dict(colour_space=names[spec["colour_space"]], icc=jf.ICC300 if "-icc" in spec["args"] else None,
              alpha=jf.option(spec["args"], "-alpha"), params=params, sgnd=bool(spec["sgnd"]))
    prec = jf.option(spec["args"], "-prec") or bits
    if spec["subsampling"]:
        got = codec.compress_jp2(planes, prec, subsampling=[tuple(s) for s in spec["subsampling"]], size=(w, h), **kw)
    else:
        got = codec.compress_jp2(np.stack(planes), prec, **kw)
    assert got == jf.load(tag)
    # and it is compress's codestream behind the boxes
    off = jf.MAN[tag]["cs_offset"]
    if not spec["subsampling"]:
        assert got[off:] == codec.compress(np.stack(planes), prec, params, sgnd=bool(spec["sgnd"]))


@pytest.mark.parametrize("tag", jf.A + jf.B)
def test_decompress_jp2_equals_the_reference_decode(codec, tag):
    out, info = codec.decompress_jp2(jf.load(tag), colour=None)
    want = jf.ref_planes(tag)
    got = as_planes(out)
    assert len(got) == len(want) == len(info["channels"])
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and np.array_equal(a, b), (tag, k)
    assert [c["alpha"] for c in info["channels"]] == [c["alpha"] for c in jf.MAN[tag]["expect"]["comps"]]


def _dtypes_holding(tag):
    prec = max(c["prec"] for c in jf.MAN[tag]["expect"]["comps"])
    sgnd = any(c["sgnd"] for c in jf.MAN[tag]["expect"]["comps"])
    if sgnd:
        return [np.int32]
    return [d for d, bits in ((np.uint8, 8), (np.uint16, 16)) if prec <= bits] + [np.int32]


@pytest.mark.parametrize("tag", jf.PALETTE + ["jp2_b_cdef_bgr"])
def test_palette_formats_layouts_destinations(codec, tag):
    """uint8 / uint16 / int32, planar and pixel-interleaved, host and device: each equal to the int32 planar result"""
    data = jf.load(tag)
    want = jf.ref_image(tag)
    for dt in _dtypes_holding(tag):
        for layout in ("chw", "hwc"):
            for dev in (False, True):
                out, _ = codec.decompress_jp2(data, dtype=dt, layout=layout, colour=None, device_out=dev)
                got = out.cpu().numpy() if dev else out
                assert got.dtype == np.dtype(dt)
                exp = want if layout == "chw" else want.transpose(1, 2, 0)
                assert got.shape == exp.shape and np.array_equal(got.astype(np.int32), exp), (tag, dt, layout, dev)


def test_palette_windows_reduce_layers(codec):
    """windows (1-sample corners, one across the tile seam), reduce = 1 and layers = 1, pinned by the reference"""
    tag = "jp2_b_pal8_tiles_I"
    data = jf.load(tag)
    seen = set()
    for vt, v in jf.MAN[tag]["variants"].items():
        args = v["args"]
        kw = {}
        if args[0] == "-r":
            kw["reduce"] = int(args[1])
        elif args[0] == "-l":
            kw["layers"] = int(args[1])
        else:
            kw["window"] = tuple(int(x) for x in args[1].split(","))
        seen.add(args[0])
        want = jf.ref_image(tag, vt)
        for dt, layout in ((np.int32, "chw"), (np.uint8, "hwc")):
            out, _ = codec.decompress_jp2(data, dtype=dt, layout=layout, colour=None, **kw)
            exp = want if layout == "chw" else want.transpose(1, 2, 0)
            assert out.shape == exp.shape and np.array_equal(out.astype(np.int32), exp), (vt, dt, layout)
    assert seen == {"-r", "-l", "-d"}
    assert sum(1 for v in jf.MAN[tag]["variants"].values() if v["args"][0] == "-d") >= 9


def test_cut_stream_gives_entry_zero(codec):
    """a tile the stream never reaches comes out as palette entry 0, as the reference's pass over its zero plane gives"""
    tag = "jp2_b_pal8_tiles_cut"
    out, info = codec.decompress_jp2(jf.load(tag), dtype=np.uint8, layout="hwc", colour=None)
    want = jf.ref_image(tag).transpose(1, 2, 0)
    assert np.array_equal(out.astype(np.int32), want)
    assert (out[:, 64:] == info["palette"]["entries"][0].astype(np.uint8)).all()


def test_tile_range_leaves_the_other_tiles_untouched(codec):
    import ctypes
    grk = _grk()
    tag = "jp2_b_pal8_tiles_I"
    data, want = jf.load(tag), jf.ref_image(tag)
    for layout, dt in (("chw", np.int32), ("hwc", np.uint8)):
        chw = layout == "chw"
        out = np.full((3, 64, 128) if chw else (64, 128, 3), 0x5A, dtype=dt)
        op = codec._out_planes(out, 3, grk._out_format(dt)[1], layout, False)
        rc = grk.lib().grkgpu_jp2_decompress(codec._ctx, data, len(data), None, 1, 2, None, ctypes.byref(op), None, None)
        assert rc == 0, grk.lib().grkgpu_last_error()
        exp = want if chw else want.transpose(1, 2, 0)
        right = (slice(None), slice(None), slice(64, 128)) if chw else (slice(None), slice(64, 128))
        left = (slice(None), slice(None), slice(0, 64)) if chw else (slice(None), slice(0, 64))
        assert np.array_equal(out[right].astype(np.int32), exp[right]), layout
        assert (out[left] == 0x5A).all(), layout


def _prec_op(v, q, p, mode):
    v = v.astype(np.int64)
    if mode == "clip":
        return np.minimum(v, (1 << p) - 1)
    if p < q:
        return v >> (q - p)
    return v * ((1 << p) - 1) // ((1 << q) - 1)


@pytest.mark.parametrize("tag,p", [("jp2_b_pal10_ne700", 8), ("jp2_b_pal4_565", 8), ("jp2_b_pal4_565", 4)])
def test_precision_ops_on_palette_output(codec, tag, p):
    data = jf.load(tag)
    want = jf.ref_image(tag)
    precs = [c["prec"] for c in jf.MAN[tag]["expect"]["comps"]]
    for mode in ("clip", "scale"):
        exp = np.stack([_prec_op(want[k], precs[k], p, mode) for k in range(len(precs))]).astype(np.int32)
        for layout in ("chw", "hwc"):
            out, _ = codec.decompress_jp2(data, dtype=np.uint8, layout=layout, colour=None, out_prec=p, prec_mode=mode)
            e = exp if layout == "chw" else exp.transpose(1, 2, 0)
            assert np.array_equal(out.astype(np.int32), e), (tag, p, mode, layout)


def test_odd_origin_three_byte_pixels(codec):
    """33 x 17 at image origin (5, 3): lead-in, 16-byte grid and cut last run with 3-byte pixels"""
    tag = "jp2_b_pal8_odd_origin"
    assert jf.MAN[tag]["expect"]["rect"] == [5, 3, 38, 20]
    want = jf.ref_image(tag).transpose(1, 2, 0)
    for dev in (False, True):
        out, _ = codec.decompress_jp2(jf.load(tag), dtype=np.uint8, layout="hwc", colour=None, device_out=dev)
        got = out.cpu().numpy() if dev else out
        assert got.shape == (17, 33, 3) and np.array_equal(got.astype(np.int32), want)


def test_colour_auto(codec):
    # the sYCC file: auto = sYCC -> RGB, as decompress(colour="sycc") of its payload
    tag = "jp2_a_sycc420_12"
    for dt, layout in ((np.int32, "chw"), (np.uint16, "hwc")):
        out, info = codec.decompress_jp2(jf.load(tag), dtype=dt, layout=layout)
        assert info["colour_space"] == "sycc"
        assert np.array_equal(out, codec.decompress(payload(tag), dtype=dt, layout=layout, colour="sycc"))
    # the sRGB file: auto = nothing
    tag = "jp2_a_rgb8_I_tiles"
    out, _ = codec.decompress_jp2(jf.load(tag), dtype=np.uint8, layout="hwc")
    assert np.array_equal(out, codec.decompress(payload(tag), dtype=np.uint8, layout="hwc"))
    assert np.array_equal(out.astype(np.int32), jf.ref_image(tag).transpose(1, 2, 0))


def test_stage_palette_to():
    """grkgpu_palette_to against numpy, the destination starting 1 .. 3 samples
    past an aligned base and dirty all around"""
    import torch
    grk = _grk()
    rng = np.random.default_rng(23)
    table = rng.integers(0, 1 << 12, size=(100, 5)).astype(np.uint16)
    ttab = torch.from_numpy(table).cuda()
    for (w, h) in ((1, 1), (5, 3), (67, 19), (130, 9)):
        stride = w + 5
        a = rng.integers(-300, 300, size=(2, h, stride)).astype(np.int32)
        src = torch.from_numpy(a).cuda()
        fin = np.clip(a[:, :, :w] + 128, 0, 255)  # two unsigned 8-bit components: DC shift, clamp
        idx = np.clip(fin[0], 0, 99)
        for chans in ([(0, 0), (0, 1), (0, 2)], [(0, 0), (0, 1), (0, 2), (1, None)], [(0, 4), (1, None)],
                      [(0, 3), (0, 0), (1, None), (0, 1), (0, 2)], [(1, None)]):
            want = np.stack([fin[c] if p is None else table[idx, p].astype(np.int64) for c, p in chans])
            n = len(chans)
            for tdt in (torch.uint16, torch.int32):
                npdt = np.dtype(str(tdt).replace("torch.", ""))
                for layout in ("chw", "hwc"):
                    exp = want.astype(npdt) if layout == "chw" else want.astype(npdt).transpose(1, 2, 0)
                    for off, pad in ((1, 0), (2, 3), (3, 0)):
                        row = (w if layout == "chw" else n * w) + pad
                        rows = n * h if layout == "chw" else h
                        base = torch.from_numpy(np.full(off + rows * row + 16, 0x5A5A, dtype=npdt)).cuda()
                        grk.palette_to(src, base[off:], w, 8, False, [c for c, _ in chans], [p for _, p in chans],
                                       [8 if p is None else 12 for _, p in chans], ttab, layout=layout, dst_stride=row)
                        got = base.cpu().numpy()
                        body = got[off:off + rows * row].reshape(rows, row)
                        used = row - pad
                        assert np.array_equal(body[:, :used].reshape(exp.shape), exp), (w, h, chans, tdt, layout, off)
                        assert (body[:, used:] == 0x5A5A).all() and (got[:off] == 0x5A5A).all()
                        assert (got[off + rows * row:] == 0x5A5A).all()


def test_file_without_palette_issues_its_payloads_launches(codec):
    tag = "jp2_a_rgb8_I_tiles"
    codec.set_launch_timing(True)
    try:
        a = codec.decompress(payload(tag), dtype=np.uint8, layout="hwc")
        names_cs = [t["kernel"] for t in codec.launch_times()]
        b, _ = codec.decompress_jp2(jf.load(tag), dtype=np.uint8, layout="hwc", colour=None)
        names_jp2 = [t["kernel"] for t in codec.launch_times()]
    finally:
        codec.set_launch_timing(False)
    assert names_cs and names_cs == names_jp2
    assert np.array_equal(a, b)


def test_after_debug_fill_and_after_another_call_kind(codec):
    tag = "jp2_b_pal_direct_alpha"
    data = jf.load(tag)
    want = jf.ref_image(tag)
    codec.debug_fill(0xFF)
    out, _ = codec.decompress_jp2(data, colour=None)
    assert np.array_equal(out, want)
    # an encode, a plain decode and a bigger palette in between
    src = np.stack(jf.source_planes("jp2_a_rgba_typ1"))
    assert codec.compress_jp2(src, 8, colour_space="srgb", alpha=[0, 0, 0, 1]) == jf.load("jp2_a_rgba_typ1")
    codec.decompress(payload("jp2_a_rgb8_I_tiles"))
    codec.decompress_jp2(jf.load("jp2_b_pal10_ne700"), colour=None)
    codec.debug_fill(0xFF)
    out, _ = codec.decompress_jp2(data, dtype=np.uint8, layout="hwc", colour=None)
    assert np.array_equal(out.astype(np.int32), want.transpose(1, 2, 0))


def test_refusals(codec):
    grk = _grk()
    for tag in jf.C:
        with pytest.raises(grk.GrkGpuError):
            codec.decompress_jp2(jf.load(tag))
    with pytest.raises(grk.GrkGpuError):  # JP2 bytes handed to the codestream decoder fail as before
        codec.decompress(jf.load("jp2_a_gray8"))
    with pytest.raises(grk.GrkGpuError):  # a raw codestream is no JP2 file
        codec.decompress_jp2(payload("jp2_a_gray8"))
    with pytest.raises(grk.GrkGpuError):  # uint8 does not hold 12-bit palette columns
        codec.decompress_jp2(jf.load("jp2_b_pal10_ne700"), dtype=np.uint8, colour=None)
    # the context is still usable
    out, _ = codec.decompress_jp2(jf.load("jp2_b_pal8"), colour=None)
    assert np.array_equal(out, jf.ref_image("jp2_b_pal8"))


# ---- libgrok.so: the grk_* API on JP2 files, through tests/cpp/jp2_driver.cpp built against include/grk_api.h ----
@pytest.fixture(scope="module")
def grk_driver(tmp_path_factory):
    import os
    import subprocess
    lib = os.path.join(jf.ROOT, "grokimagecompression_amd", "lib")
    exe = str(tmp_path_factory.mktemp("jp2drv") / "jp2_driver")
    subprocess.run(["g++", "-std=c++17", "-O2", "-DJP2_DRIVER_GRK_API_H", "-I" + os.path.join(jf.ROOT, "include"), "-o", exe,
                    os.path.join(jf.ROOT, "tests", "cpp", "jp2_driver.cpp"), "-L" + lib, "-lgrok",
                    "-Wl,-rpath," + lib], check=True)
    return exe


def _driver_decode(exe, data, tmp, extra=()):
    """None when the library refuses; else (first line's fields, per-component fields, planes, ICC bytes)"""
    import os
    import subprocess
    src, out = os.path.join(tmp, "in.jp2"), os.path.join(tmp, "out.i32")
    with open(src, "wb") as f:
        f.write(data)
    r = subprocess.run([exe, "dec", src, out] + list(extra), capture_output=True, text=True)
    if r.returncode == 1 and r.stdout.strip().endswith("error"):
        return None
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith(("image", "comp"))]
    head = [int(v) for v in lines[0][1:]]
    comps = [[int(v) for v in ln[1:]] for ln in lines[1:]]
    raw = np.fromfile(out, dtype="<i4")
    planes, off = [], 0
    for w, h, *_ in comps:
        planes.append(raw[off:off + w * h].reshape(h, w))
        off += w * h
    assert off == raw.size
    with open(out + ".icc", "rb") as f:
        return head, comps, planes, f.read()


@pytest.mark.parametrize("tag", jf.A)
def test_grk_api_encodes_the_reference_file(grk_driver, tmp_path, tag):
    import subprocess
    spec = jf.MAN[tag]["spec"]
    h, w, c, bits = spec["shape"]
    src, out, icc = str(tmp_path / "in.i32"), str(tmp_path / "out.jp2"), str(tmp_path / "p.icc")
    np.concatenate([np.ascontiguousarray(p, dtype="<i4").ravel() for p in jf.source_planes(tag)]).tofile(src)
    with open(icc, "wb") as f:
        f.write(jf.ICC300)
    args = ["-cs", str(spec["colour_space"])] + [icc if a == "@ICC" else a for a in spec["args"]]
    subprocess.run([grk_driver, "enc", src, out, str(w), str(h), str(c), str(bits), str(int(spec["sgnd"]))] + args,
                   check=True, stdout=subprocess.DEVNULL)
    with open(out, "rb") as f:
        assert f.read() == jf.load(tag)


@pytest.mark.parametrize("tag", jf.A + jf.B)
def test_grk_api_decodes_as_the_reference(grk_driver, tmp_path, tag):
    """colour space, alpha flags, ICC bytes, geometry and planes of grk_read_header + grk_decode on the file"""
    import hashlib
    rec = jf.MAN[tag]
    todo = [(None, rec["expect"]["rect"], rec["expect"]["comps"], [])]
    todo += [(vt, v["rect"], v["comps"], v["args"]) for vt, v in rec["variants"].items()]
    for vt, rect, comps, args in todo:
        r = _driver_decode(grk_driver, jf.load(tag), str(tmp_path), args)
        assert r is not None, (tag, vt)
        head, gcomps, planes, icc = r
        e = rec["expect"]
        assert head == rect + [len(comps), e["colour_space"], e["icc_len"]], (tag, vt)
        assert gcomps == [[c["w"], c["h"], c["dx"], c["dy"], c["prec"], c["sgnd"], c["alpha"]] for c in comps], (tag, vt)
        assert len(icc) == e["icc_len"] and (not icc or hashlib.sha256(icc).hexdigest() == e["icc_sha256"])
        for k, (a, b) in enumerate(zip(planes, jf.ref_planes(tag, vt))):
            assert a.shape == b.shape and np.array_equal(a, b), (tag, vt, k)


def test_grk_api_refuses_what_the_reference_refuses(grk_driver, tmp_path):
    for tag in jf.C:
        assert _driver_decode(grk_driver, jf.load(tag), str(tmp_path)) is None, tag
