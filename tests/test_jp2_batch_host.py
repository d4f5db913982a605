"""Batch decode of JP2 files, host half (grkgpu_jp2_batch_plan: no device call):
the C ABI of the three new entry points, the per-item descriptor and info
rules of grkgpu_jp2_decompress, the per-item refusals (every refused fixture
among good files, a raw codestream, force-RGB) and the call-level rules of
grkgpu_decompress_batch."""
import ctypes
import os
import shutil
import subprocess

import jp2_fixtures as jf
from conftest import GOLD, ROOT

OK, EINVAL, EUNSUPPORTED, ECORRUPT = 0, -1, -4, -5


def _grk():
    import grokimagecompression_amd as grk
    return grk


def _img(d):
    return [(d.x0, d.y0, d.x1, d.y1, d.numcomps)] + [(d.prec[k], d.sgnd[k], d.dx[k], d.dy[k]) for k in range(d.numcomps)]


def _read_info(grk, buf):
    """(rc, Jp2Info, ImageDesc) of grkgpu_jp2_read_info on the file alone"""
    ji, d = grk.Jp2Info(), grk.ImageDesc()
    rc = grk.lib().grkgpu_jp2_read_info(buf, len(buf), ctypes.byref(ji), ctypes.byref(d))
    return rc, ji, d


def test_error_codes_are_the_headers():
    hdr = open(os.path.join(ROOT, "include", "grk_mi355x.h")).read()
    for name, v in (("GRKGPU_EINVAL", EINVAL), ("GRKGPU_ECORRUPT", ECORRUPT), ("GRKGPU_EUNSUPPORTED", EUNSUPPORTED)):
        assert "%s = %d" % (name, v) in hdr, name


def test_abi():
    grk = _grk()
    L = grk.lib()
    for sym in ("grkgpu_jp2_decompress_batch", "grkgpu_jp2_batch_plan", "grkgpu_palette_jobs_to"):
        assert hasattr(L, sym), sym
    hdr = open(os.path.join(ROOT, "include", "grk_mi355x.h")).read()
    for decl in ("int grkgpu_jp2_decompress_batch(grkgpu_ctx *ctx, grkgpu_batch_item *items, const grkgpu_out_ops *ops, "
                 "uint32_t n,\n                                const grkgpu_dparams *p, grkgpu_batch_info *info, "
                 "grkgpu_jp2_info *infos);",
                 "int grkgpu_jp2_batch_plan(grkgpu_batch_item *items, const grkgpu_out_ops *ops, uint32_t n, "
                 "const grkgpu_dparams *p,\n                          grkgpu_batch_info *info, grkgpu_jp2_info *infos);",
                 "int grkgpu_palette_jobs_to(const grkgpu_palette_job *jobs, uint32_t n, const uint16_t *table, "
                 "uint32_t table_entries,\n                           uint32_t sample_fmt, uint32_t layout, void *stream);"):
        assert decl in hdr, decl


def test_palette_job_layout(tmp_path):
    """the ctypes mirror against sizeof / offsetof from the header, compiled as C
    (codec.cpp pins the same layout against the device record)"""
    grk = _grk()
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no C compiler"
    fields = [f for f, _ in grk.PaletteJob._fields_]
    src = tmp_path / "abi.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "grk_mi355x.h"\n'
                   "int main(void) { printf(\"%zu\", sizeof(grkgpu_palette_job));\n"
                   + "".join('printf(" %%zu", offsetof(grkgpu_palette_job, %s));\n' % f for f in fields)
                   + "return 0; }\n")
    exe = tmp_path / "abi"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    J = grk.PaletteJob
    assert got == [ctypes.sizeof(J)] + [getattr(J, f).offset for f in fields]
    assert ctypes.sizeof(J) == 200 and J.chan_comp.offset == ctypes.sizeof(grk.StoreJob) and J.table_off.offset == 196
    # the first fields are grkgpu_store_job's
    for f, _ in grk.StoreJob._fields_:
        assert getattr(J, "ops_" if f == "pad_" else f).offset == getattr(grk.StoreJob, f).offset, f


def test_plan_every_good_file():
    grk = _grk()
    tags = jf.A + jf.B
    bufs = [jf.load(t) for t in tags]
    r = grk.plan_jp2_batch(bufs, colour=None)
    assert r["rc"] == OK and r["status"] == [OK] * len(tags) and r["n_ok"] == len(tags) and r["n_launches"] == 0
    for t, b, d, ji in zip(tags, bufs, r["img"], r["infos"]):
        rc, want_ji, want_d = _read_info(grk, b)
        assert rc == OK
        assert _img(d) == _img(want_d), t
        assert bytes(ji) == bytes(want_ji), t
    # colour="auto": the sYCC 4:2:0 file is converted, so it leaves on the image grid
    r = grk.plan_jp2_batch(bufs, colour="auto")
    assert r["status"] == [OK] * len(tags)
    d = r["img"][tags.index("jp2_a_sycc420_12")]
    assert [(d.dx[k], d.dy[k]) for k in range(3)] == [(1, 1)] * 3
    for t, b, d in zip(tags, bufs, r["img"]):
        if t != "jp2_a_sycc420_12":
            assert _img(d) == _img(_read_info(grk, b)[2]), t
    # colour="auto_rgb" with an output precision: _out_channels' precisions
    r = grk.plan_jp2_batch(bufs, colour="auto_rgb", out_prec=8)
    assert r["status"] == [OK] * len(tags)
    for t, b, d in zip(tags, bufs, r["img"]):
        _, ji, dd = _read_info(grk, b)
        space = grk._COLOUR_SPACE_NAMES.get(ji.colour_space, "unknown")
        c = dd.numcomps
        want = grk._out_channels(grk._jp2_conversion("auto_rgb", space), False, [dd.prec[k] for k in range(c)],
                                 [dd.sgnd[k] for k in range(c)], 8)
        assert [(d.prec[k], bool(d.sgnd[k])) for k in range(d.numcomps)] == want, t
        assert all(p == 8 for p, _ in want)


def test_refused_files_among_good_ones():
    grk = _grk()
    good = jf.load("jp2_b_pal8")
    bufs, want = [], []
    for t in jf.C:
        b = jf.load(t)
        rc = _read_info(grk, b)[0]
        assert rc != OK, t
        bufs += [good, b]
        want += [OK, rc]
    bufs.append(jf.load("jp2_a_gray8"))
    want.append(OK)
    r = grk.plan_jp2_batch(bufs, colour=None)
    assert r["status"] == want
    assert r["n_ok"] == len(jf.C) + 1
    assert r["rc"] == want[1] and r["error"].startswith("item 1: ")
    # each refused file alone between two good ones keeps its code and its message
    for t in jf.C:
        b = jf.load(t)
        rc = _read_info(grk, b)[0]
        msg = grk.lib().grkgpu_last_error().decode()
        r = grk.plan_jp2_batch([good, good, b, good], colour=None)
        assert r["status"] == [OK, OK, rc, OK] and r["rc"] == rc and r["error"] == "item 2: " + msg, t


def test_raw_codestream_is_corrupt():
    grk = _grk()
    raw = open(os.path.join(GOLD, "g8_64.j2k"), "rb").read()
    r = grk.plan_jp2_batch([jf.load("jp2_a_gray8"), raw])
    assert r["status"] == [OK, ECORRUPT] and r["rc"] == ECORRUPT and r["error"].startswith("item 1: ")
    # the payload of a file is a raw codestream too
    data = jf.load("jp2_b_pal8")
    off, n = grk.jp2_info(data)["codestream"]
    assert grk.plan_jp2_batch([data[off:off + n]])["status"] == [ECORRUPT]
    assert grk.plan_jp2_batch([b""])["status"][0] != OK


def test_force_rgb():
    grk = _grk()
    tags = ["jp2_a_gray8", "jp2_a_graya", "jp2_b_pal8", "jp2_a_icc", "jp2_a_unknown"]
    r = grk.plan_jp2_batch([jf.load(t) for t in tags], colour=None, force_rgb=True)
    assert r["status"] == [OK, OK, OK, EUNSUPPORTED, EINVAL]
    assert r["rc"] == EUNSUPPORTED and r["error"].startswith("item 3: ") and "ICC" in r["error"]
    assert [d.numcomps for d in r["img"][:3]] == [3, 4, 3]
    g = r["img"][0]
    assert [(g.prec[k], g.sgnd[k]) for k in range(3)] == [(8, 0)] * 3
    # per item: only the second file is forced
    r = grk.plan_jp2_batch([jf.load("jp2_a_gray8")] * 2, colour=None, force_rgb=[False, True])
    assert [d.numcomps for d in r["img"]] == [1, 3]
    # without the flag the ICC file and the unknown-space file decode
    assert grk.plan_jp2_batch([jf.load("jp2_a_icc"), jf.load("jp2_a_unknown")], colour=None)["status"] == [OK, OK]
    # the raw-codestream batch calls keep their refusal
    cs = open(os.path.join(GOLD, "g8_64.j2k"), "rb").read()
    r = grk.plan_batch_convert([cs], ops=[grk.OutOps(colour=grk.COLOUR_FORCE_RGB)])
    assert r["status"] == [EUNSUPPORTED] and "force-RGB" in r["error"]


def test_call_level_rules():
    grk = _grk()
    L = grk.lib()
    good = jf.load("jp2_b_pal8")
    assert grk.plan_jp2_batch([])["rc"] == OK
    assert L.grkgpu_jp2_batch_plan(None, None, 0, None, None, None) == OK
    assert L.grkgpu_jp2_batch_plan(None, None, 1, None, None, None) == EINVAL
    assert L.grkgpu_jp2_decompress_batch(None, None, None, 0, None, None, None) == EINVAL  # no context
    items, keep = grk._batch_items([good])
    dp = grk.DParams(DA_x0=0, DA_y0=0, DA_x1=8, DA_y1=8)
    info = grk.BatchInfo(n_ok=7)
    assert L.grkgpu_jp2_batch_plan(items, None, 1, ctypes.byref(dp), ctypes.byref(info), None) == EINVAL
    assert b"decode area" in L.grkgpu_last_error() and info.n_ok == 0
    # ops = NULL: nothing converted, nothing forced
    items[0].status = 9
    assert L.grkgpu_jp2_batch_plan(items, None, 1, None, ctypes.byref(info), None) == OK
    assert items[0].status == OK and info.n_ok == 1 and items[0].img.numcomps == 3
    # cp_reduce / cp_layer apply to every item
    r = grk.plan_jp2_batch([jf.load("jp2_b_pal8_tiles_I"), good], colour=None, reduce=1, layers=1)
    assert r["status"] == [OK, OK]
    d = r["img"][0]
    assert (d.x1 - d.x0, d.y1 - d.y0) == (64, 32)


def test_store_records():
    grk = _grk()
    one = grk.plan_jp2_batch([jf.load("jp2_b_pal8_tiles_I")], colour=None)
    assert one["n_store_jobs"] == 2  # (two tiles of 64 x 64)
    many = grk.plan_jp2_batch([jf.load("jp2_b_pal8_tiles_I")] * 64, colour=None)
    assert many["status"] == [OK] * 64 and many["n_store_jobs"] == 64 * one["n_store_jobs"]
    assert many["n_blocks"] == 64 * one["n_blocks"]
    # a cut stream: a record per tile reached and a zero record per tile never reached
    assert grk.plan_jp2_batch([jf.load("jp2_b_pal8_tiles_cut")], colour=None)["n_store_jobs"] == 2
    # a file without a palette or swap: the records of grkgpu_batch_convert_plan on its payload
    for tag in ("jp2_a_rgb8_I_tiles", "jp2_a_sycc420_12", "jp2_a_gray_s16"):
        data = jf.load(tag)
        off, n = grk.jp2_info(data)["codestream"]
        for colour, conv in ((None, None), ("auto", "sycc" if tag == "jp2_a_sycc420_12" else None)):
            a = grk.plan_jp2_batch([data], colour=colour)
            b = grk.plan_batch_convert([data[off:off + n]], colour=conv)
            assert a["status"] == b["status"] == [OK]
            assert (a["n_blocks"], a["n_store_jobs"]) == (b["n_blocks"], b["n_store_jobs"]), (tag, colour)
            assert _img(a["img"][0])[1:] == _img(b["img"][0])[1:], (tag, colour)
