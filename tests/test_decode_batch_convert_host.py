"""Batch decode with the converting / upsampling last store, host half
(grkgpu_batch_convert_plan: no device call): which items the new entry points
take that grkgpu_decompress_batch refuses, the img descriptor rules of
grkgpu_decompress_convert per item, the per-item refusals, and that the old
entry points keep theirs.  The C ABI of the three new entry points."""
import ctypes
import json
import os
import shutil
import subprocess

from conftest import GOLD, ROOT, load_manifest

MAN = load_manifest()
NAMES = sorted(MAN)
SUB = json.load(open(os.path.join(GOLD, "manifest_sub.json")))
OK, EINVAL, EUNSUPPORTED = 0, -1, -4


def _grk():
    import grokimagecompression_amd as grk
    return grk


def _cs(name):
    return open(os.path.join(GOLD, name + ".j2k"), "rb").read()


def test_abi():
    grk = _grk()
    L = grk.lib()
    for sym in ("grkgpu_decompress_batch_convert", "grkgpu_batch_convert_plan", "grkgpu_convert_jobs_to"):
        assert hasattr(L, sym)
    hdr = open(os.path.join(ROOT, "include", "grk_mi355x.h")).read()
    for decl in ("int grkgpu_decompress_batch_convert(grkgpu_ctx *ctx, grkgpu_batch_item *items, "
                 "const grkgpu_out_ops *ops,\n                                    uint32_t n, const grkgpu_dparams *p, "
                 "grkgpu_batch_info *info);",
                 "int grkgpu_batch_convert_plan(grkgpu_batch_item *items, const grkgpu_out_ops *ops, uint32_t n,\n"
                 "                              const grkgpu_dparams *p, grkgpu_batch_info *info);",
                 "int grkgpu_convert_jobs_to(const grkgpu_convert_job *jobs, uint32_t n, uint32_t sample_fmt, "
                 "uint32_t layout,"):
        assert decl in hdr, decl


def test_struct_sizes(tmp_path):
    """ctypes mirrors against sizeof / offsetof from the header, compiled as C
    (codec.cpp pins the same layout against the device records)"""
    grk = _grk()
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no C compiler"
    src = tmp_path / "abi.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "grk_mi355x.h"\n'
                   "int main(void) { printf(\"%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n\", sizeof(grkgpu_convert_comp),\n"
                   "sizeof(grkgpu_convert_job), offsetof(grkgpu_convert_comp, stride), offsetof(grkgpu_convert_comp, dx),\n"
                   "offsetof(grkgpu_convert_comp, kind), offsetof(grkgpu_convert_comp, shift),\n"
                   "offsetof(grkgpu_convert_job, dst), offsetof(grkgpu_convert_job, x0),\n"
                   "offsetof(grkgpu_convert_job, mct), offsetof(grkgpu_convert_job, ops)); return 0; }\n")
    exe = tmp_path / "abi"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    C, J = grk.ConvertComp, grk.ConvertJob
    assert got == [ctypes.sizeof(C), ctypes.sizeof(J), C.stride.offset, C.dx.offset, C.kind.offset, C.shift.offset,
                   J.dst.offset, J.x0.offset, J.mct.offset, J.ops.offset]
    assert ctypes.sizeof(C) == 48 and ctypes.sizeof(J) == 272 and J.ops.offset == 256
    assert (grk.SRC_RAW, grk.SRC_SAMPLES) == (1, 2)


def _expect_img(grk, cs, up, colour, out_prec):
    """grkgpu_decompress_convert's descriptor rules on the stream's header"""
    h = grk.read_header(cs)
    c = h.numcomps
    sub = any((h.dx[k], h.dy[k]) != (1, 1) for k in range(c))
    one = (up or colour == "sycc") and sub
    return [(h.x0, h.y0, h.x1, h.y1, c)] + [
        (out_prec or h.prec[k], h.sgnd[k], 1 if one else h.dx[k], 1 if one else h.dy[k]) for k in range(c)]


def _img(d):
    return [(d.x0, d.y0, d.x1, d.y1, d.numcomps)] + [(d.prec[k], d.sgnd[k], d.dx[k], d.dy[k]) for k in range(d.numcomps)]


def test_plan_every_subsampled_golden():
    grk = _grk()
    tags = sorted(SUB)
    assert len(tags) == 6
    bufs = [_cs(t) for t in tags]
    for up in (False, True):
        for out_prec in (None, 8):
            dt = None if out_prec is None else "uint8"
            r = grk.plan_batch_convert(bufs, dtype=dt, upsample=up, out_prec=out_prec, prec_mode="scale")
            assert r["rc"] == OK and r["status"] == [OK] * 6 and r["n_ok"] == 6 and r["n_launches"] == 0, (up, out_prec)
            for b, d in zip(bufs, r["img"]):
                assert _img(d) == _expect_img(grk, b, up, None, out_prec)
            assert r["n_blocks"] == sum(grk.plan_batch_convert([b])["n_blocks"] for b in bufs)
    # sYCC where the shape allows (4:2:0 / 4:2:2, three unsigned components), with and without a precision
    ycc = [_cs("sub_420_rgb8"), _cs("sub_422_I_tiles")]
    for out_prec in (None, 8):
        r = grk.plan_batch_convert(ycc, dtype="uint8" if out_prec else None, colour="sycc", out_prec=out_prec,
                                   prec_mode="scale")
        assert r["status"] == [OK, OK]
        for b, d in zip(ycc, r["img"]):
            assert _img(d) == _expect_img(grk, b, False, "sycc", out_prec)
            assert all(d.dx[k] == 1 and d.dy[k] == 1 for k in range(3))
    # ... and is that item's EINVAL where it does not (the others still plan)
    r = grk.plan_batch_convert(bufs, colour="sycc")
    want = [OK if t in ("sub_420_rgb8", "sub_422_I_tiles") else EINVAL for t in tags]
    assert r["status"] == want and r["n_ok"] == 2 and r["rc"] == EINVAL
    # the job tables: one record per (tile, component) on mixed grids, plus one per tile when upsampled
    a = grk.plan_batch_convert([_cs("sub_420_rgb8")])
    b = grk.plan_batch_convert([_cs("sub_420_rgb8")], upsample=True)
    assert a["n_store_jobs"] == 3 and b["n_store_jobs"] == 1  # (one tile: chroma read from the tile buffers)
    assert grk.plan_batch_convert([_cs("sub_420_rgb8")] * 64, upsample=True)["n_store_jobs"] == 64


def test_per_item_refusals():
    grk = _grk()
    good = _cs("rgb8_128x96")
    mct = _cs(sorted(json.load(open(os.path.join(GOLD, "manifest_mct.json"))))[0])
    O = grk.OutOps

    def plan(cs, ops=None, **kw):
        r = grk.plan_batch_convert([good, cs, good], ops=None if ops is None else [None, ops, None], **kw)
        assert r["status"][0] == OK and r["status"][2] == OK and r["n_ok"] == 2, r
        assert r["rc"] == r["status"][1] and r["error"].startswith("item 1: ")
        return r["status"][1], r["error"]
    st, msg = plan(_cs("g8_64"), O(colour=grk.COLOUR_FORCE_RGB))
    assert st == EUNSUPPORTED and "force-RGB" in msg
    st, msg = plan(mct)
    assert st == EUNSUPPORTED and "MCT" in msg
    assert plan(good, O(prec=17))[0] == EINVAL
    assert plan(good, O(colour=7))[0] == EINVAL
    assert plan(good, O(colour=grk.COLOUR_AUTO))[0] == EINVAL
    assert plan(good, O(colour=grk.COLOUR_AUTO_RGB))[0] == EINVAL
    assert plan(good, O(prec=8, prec_mode=2))[0] == EINVAL
    assert plan(good, O(colour=0, prec=0, prec_mode=0, reserved=1))[0] == EINVAL
    assert plan(_cs("g8_64"), O(colour=grk.COLOUR_SYCC))[0] == EINVAL  # one component
    # uint8 does not hold a 12-bit stream as it is; with out_prec = 8 it does
    r = grk.plan_batch_convert([good, _cs("rgb12_96x80")], dtype="uint8")
    assert r["status"] == [OK, EINVAL] and "does not hold" in r["error"]
    assert grk.plan_batch_convert([good, _cs("rgb12_96x80")], dtype="uint8", out_prec=8)["status"] == [OK, OK]
    # cp_reduce with the upsampled output of a subsampled stream is that item's EINVAL; a plain stream takes it
    r = grk.plan_batch_convert([_cs("sub_420_rgb8"), good], reduce=1, upsample=True)
    assert r["status"] == [EINVAL, OK] and "reduced" in r["error"]
    r = grk.plan_batch_convert([_cs("sub_420_rgb8"), good], reduce=1, colour=["sycc", None])
    assert r["status"] == [EINVAL, OK]
    assert grk.plan_batch_convert([_cs("sub_420_rgb8"), good], reduce=1)["status"] == [OK, OK]
    # the call-level rules of grkgpu_decompress_batch
    L = grk.lib()
    assert grk.plan_batch_convert([])["rc"] == OK
    assert L.grkgpu_batch_convert_plan(None, None, 0, None, None) == OK
    assert L.grkgpu_batch_convert_plan(None, None, 1, None, None) == EINVAL
    assert L.grkgpu_decompress_batch_convert(None, None, None, 0, None, None) == EINVAL  # no context
    items, keep = grk._batch_items([good])
    dp = grk.DParams(DA_x0=0, DA_y0=0, DA_x1=8, DA_y1=8)
    info = grk.BatchInfo(n_ok=7)
    assert L.grkgpu_batch_convert_plan(items, None, 1, ctypes.byref(dp), ctypes.byref(info)) == EINVAL
    assert b"decode area" in L.grkgpu_last_error() and info.n_ok == 0


def test_no_ops_is_the_plain_plan():
    """ops = NULL, nothing subsampled, no flag: grkgpu_batch_plan's tables"""
    grk = _grk()
    bufs = [_cs(n) for n in NAMES]
    assert len(bufs) == 88
    a, b = grk.plan_batch(bufs), grk.plan_batch_convert(bufs)
    assert b["rc"] == OK and b["status"] == [OK] * 88
    assert (a["n_ok"], a["n_blocks"], a["n_store_jobs"]) == (b["n_ok"], b["n_blocks"], b["n_store_jobs"])
    for x, y in zip(a["img"], b["img"]):
        assert bytes(x) == bytes(y)


def test_the_old_entry_points_still_refuse():
    grk = _grk()
    L = grk.lib()
    mct = _cs(sorted(json.load(open(os.path.join(GOLD, "manifest_mct.json"))))[0])
    r = grk.plan_batch([_cs("g8_64"), _cs("sub_420_rgb8"), mct])
    assert r["status"] == [OK, EUNSUPPORTED, EUNSUPPORTED] and r["rc"] == EUNSUPPORTED
    assert r["error"] == "item 1: subsampled components are not supported in a batch"
    items, keep = grk._batch_items([_cs("g8_64"), _cs("g8_64")])
    items[1].out.layout = grk.LAYOUT_UPSAMPLE
    assert L.grkgpu_batch_plan(items, 2, None, None) == EUNSUPPORTED
    assert [items[0].status, items[1].status] == [OK, EUNSUPPORTED]
    assert L.grkgpu_last_error() == b"item 1: upsampled output is not supported in a batch"
    # the same two items through the new entry point
    items[0].status = items[1].status = 9
    assert L.grkgpu_batch_convert_plan(items, None, 2, None, None) == OK
    assert [items[0].status, items[1].status] == [OK, OK]
