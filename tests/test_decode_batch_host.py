"""Batch decode, host half (grkgpu_batch_plan: no device call): every check
that can refuse a stream runs here, an item that fails gets its own status
and never stops the others, and the merged block table is the sum of the
streams' own.  The C ABI of the three new entry points."""
import ctypes
import json
import os
import shutil
import struct
import subprocess

import pytest

from conftest import GOLD, ROOT, load_manifest

MAN = load_manifest()
NAMES = sorted(MAN)
OK, EINVAL, EUNSUPPORTED, ECORRUPT = 0, -1, -4, -5


def _grk():
    import grokimagecompression_amd as grk
    return grk


def _cs(name):
    return open(os.path.join(GOLD, name + ".j2k"), "rb").read()


def _code(fn, *a):
    """the grkgpu code a single-stream call gives (0: none)"""
    grk = _grk()
    try:
        fn(*a)
    except grk.GrkGpuError as e:
        return int(str(e).split()[2].rstrip(":"))
    return 0


def _ht(cs):
    """-M 64 (HT code-block style) in the main COD, as tests/test_errors.py patches it"""
    pos = 2
    while True:
        m, L = struct.unpack(">HH", cs[pos:pos + 4])
        if m == 0xFF52:
            break
        pos += 2 + L
    b = bytearray(cs)
    b[pos + 4 + 8] = 0x40
    return bytes(b)


def mixed_list():
    """good / empty / cut in the main header / HT / subsampled / custom MCT / good"""
    sub = sorted(json.load(open(os.path.join(GOLD, "manifest_sub.json"))))[0]
    mct = sorted(json.load(open(os.path.join(GOLD, "manifest_mct.json"))))[0]
    return [_cs("g8_256"), b"", _cs("rgb8_128x96")[:60], _ht(_cs("g8_256")), _cs(sub), _cs(mct), _cs("rgb8_128x96")]


def test_plan_all_goldens():
    grk = _grk()
    bufs = [_cs(n) for n in NAMES]
    assert len(bufs) == 88
    r = grk.plan_batch(bufs)
    assert r["rc"] == OK and r["status"] == [OK] * len(bufs) and r["n_ok"] == len(bufs)
    assert r["n_launches"] == 0
    for b, d in zip(bufs, r["img"]):
        assert bytes(d) == bytes(grk.read_header(b))
    assert r["n_blocks"] == sum(grk.plan_batch([b])["n_blocks"] for b in bufs)
    assert r["n_store_jobs"] >= len(bufs)


def test_plan_reduced_geometry():
    """img is the decoded geometry: ceil(size / 2^reduce) from ceil(origin / 2^reduce)"""
    grk = _grk()
    r = grk.plan_batch([_cs("g8_off35"), _cs("g8_256")], reduce=1)
    assert r["status"] == [OK, OK]
    for b, d in zip(["g8_off35", "g8_256"], r["img"]):
        h = grk.read_header(_cs(b))
        cd = lambda v: -(-v // 2)  # noqa: E731
        assert (d.x0, d.y0) == (cd(h.x0), cd(h.y0))
        assert (d.x1 - d.x0, d.y1 - d.y0) == (cd(h.x1 - h.x0), cd(h.y1 - h.y0))


def test_plan_failing_items_do_not_stop_the_others():
    grk = _grk()
    bufs = mixed_list()
    r = grk.plan_batch(bufs)
    st = r["status"]
    assert st[0] == OK and st[6] == OK and r["n_ok"] == 2
    assert st[1] == _code(grk.read_header, bufs[1]) != OK
    assert st[2] == _code(grk.walk_tiles, bufs[2]) and st[2] in (ECORRUPT, EUNSUPPORTED)
    assert st[3] == EUNSUPPORTED and st[4] == EUNSUPPORTED and st[5] == EUNSUPPORTED
    assert r["rc"] == st[1] and r["error"].startswith("item 1: ")
    good = grk.plan_batch([bufs[0], bufs[6]])
    assert (r["n_blocks"], r["n_store_jobs"]) == (good["n_blocks"], good["n_store_jobs"])
    # the first failure is the one reported
    r = grk.plan_batch([bufs[0], bufs[4], bufs[1]])
    assert r["rc"] == EUNSUPPORTED and r["error"].startswith("item 1: ") and "subsampled" in r["error"]


def test_plan_arguments():
    grk = _grk()
    L = grk.lib()
    assert grk.plan_batch([])["rc"] == OK
    assert L.grkgpu_batch_plan(None, 0, None, None) == OK
    assert L.grkgpu_batch_plan(None, 1, None, None) == EINVAL
    assert L.grkgpu_decompress_batch(None, None, 0, None, None) == EINVAL  # no context
    items, keep = grk._batch_items([_cs("g8_64")])
    dp = grk.DParams(DA_x0=0, DA_y0=0, DA_x1=8, DA_y1=8)
    info = grk.BatchInfo(n_ok=7)
    assert L.grkgpu_batch_plan(items, 1, ctypes.byref(dp), ctypes.byref(info)) == EINVAL
    assert b"decode area" in L.grkgpu_last_error() and info.n_ok == 0
    # reduce beyond a stream's resolutions is that item's error
    r = grk.plan_batch([_cs("g8_64"), _cs("g8_256")], reduce=30)
    assert r["status"] == [EINVAL, EINVAL]
    # an upsampled layout is refused per item, before anything else of the stream is looked at
    items, keep = grk._batch_items([_cs("g8_64"), _cs("g8_64")])
    items[1].out.layout = grk.LAYOUT_UPSAMPLE
    assert L.grkgpu_batch_plan(items, 2, None, None) == EUNSUPPORTED
    assert [items[0].status, items[1].status] == [OK, EUNSUPPORTED]


def test_abi():
    grk = _grk()
    L = grk.lib()
    for sym in ("grkgpu_decompress_batch", "grkgpu_batch_plan", "grkgpu_mct_inv_dcshift_jobs_to"):
        assert hasattr(L, sym)
    hdr = open(os.path.join(ROOT, "include", "grk_mi355x.h")).read()
    for decl in ("int grkgpu_decompress_batch(grkgpu_ctx *ctx, grkgpu_batch_item *items, uint32_t n,",
                 "int grkgpu_batch_plan(grkgpu_batch_item *items, uint32_t n,",
                 "int grkgpu_mct_inv_dcshift_jobs_to(const grkgpu_store_job *jobs, uint32_t n,"):
        assert decl in hdr


def test_struct_sizes(tmp_path):
    """ctypes mirrors against sizeof / offsetof from the header, compiled as C"""
    grk = _grk()
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no C compiler"
    src = tmp_path / "abi.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "grk_mi355x.h"\n'
                   "int main(void) { printf(\"%zu %zu %zu %zu %zu %zu %zu %zu\\n\", sizeof(grkgpu_batch_item),\n"
                   "sizeof(grkgpu_batch_info), sizeof(grkgpu_store_job), offsetof(grkgpu_batch_item, out),\n"
                   "offsetof(grkgpu_batch_item, img), offsetof(grkgpu_batch_item, status),\n"
                   "offsetof(grkgpu_store_job, src_stride), offsetof(grkgpu_store_job, shift)); return 0; }\n")
    exe = tmp_path / "abi"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(grk.BatchItem), ctypes.sizeof(grk.BatchInfo), ctypes.sizeof(grk.StoreJob),
                   grk.BatchItem.out.offset, grk.BatchItem.img.offset, grk.BatchItem.status.offset,
                   grk.StoreJob.src_stride.offset, grk.StoreJob.shift.offset]
    assert ctypes.sizeof(grk.BatchInfo) == 16 and ctypes.sizeof(grk.StoreJob) == 144
