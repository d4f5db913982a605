"""Batch encode, host half (grkgpu_compress_batch_plan: no device call): every
check that can refuse an image before a device is touched runs here, an item
that fails gets its own status and never stops the others, and the merged
block table is the sum of the images' own.  The C ABI of the three new entry
points."""
import ctypes
import os
import shutil
import subprocess

from conftest import ROOT, load_manifest

MAN = load_manifest()
NAMES = sorted(MAN)
OK, EINVAL, EUNSUPPORTED = 0, -1, -4


def _grk():
    import grokimagecompression_amd as grk
    return grk


def desc(name):
    """plan_compress_batch's descriptor of a golden of tests/golden/manifest.json"""
    grk = _grk()
    h, w, c, bits = MAN[name]["shape"]
    p, off = grk.CParams.from_cli(MAN[name]["args"])
    return dict(shape=(c, h, w), prec=bits, params=p, offset=off)


def mixed_descs():
    """good / precision 0 / sample format that does not hold the precision /
    subsampled / custom MCT / tile grid that gives more than 255 tile-parts /
    good"""
    grk = _grk()
    mct = grk.CParams.make()
    mct.set_mct([1, 0, 0, 0, 1, 0, 0, 0, 1], [0, 0, 0])
    # LRCP tile-parts split down to the resolution: 50 layers x 6 resolutions = 300 in each tile of the grid
    tp, _ = grk.CParams.from_cli(["-t", "32,32", "-r", ",".join(str(200 - 2 * k) for k in range(50)), "-u", "R"])
    return [desc("g8_256"),
            dict(shape=(1, 32, 32), prec=0),
            dict(shape=(1, 32, 32), prec=12, fmt=grk.SAMPLE_U8),
            dict(shape=(3, 32, 32), prec=8, subsampling=[(1, 1), (2, 2), (2, 2)]),
            dict(shape=(3, 32, 32), prec=8, params=mct),
            dict(shape=(3, 64, 64), prec=8, params=tp),
            desc("rgb8_128x96")]


def single_code(d):
    """the grkgpu code the host half gives this image alone"""
    return _grk().plan_compress_batch([d])["status"][0]


def test_plan_all_goldens():
    grk = _grk()
    descs = [desc(n) for n in NAMES]
    assert len(descs) == 88
    r = grk.plan_compress_batch(descs)
    assert r["rc"] == OK and r["status"] == [OK] * len(descs) and r["n_ok"] == len(descs)
    assert r["n_launches"] == 0
    singles = [grk.plan_compress_batch([d]) for d in descs]
    assert all(s["rc"] == OK for s in singles)
    assert r["n_blocks"] == sum(s["n_blocks"] for s in singles) > 0
    assert r["n_load_jobs"] == sum(s["n_load_jobs"] for s in singles) >= len(descs)


def test_plan_failing_items_do_not_stop_the_others():
    grk = _grk()
    descs = mixed_descs()
    r = grk.plan_compress_batch(descs)
    st = r["status"]
    assert st[0] == OK and st[6] == OK and r["n_ok"] == 2
    assert st[1] == EUNSUPPORTED  # setup_params: "precision must be 1..16"
    assert st[2] == EINVAL        # the sample-format rule of grkgpu_compress_ex
    assert st[3] == EUNSUPPORTED and st[4] == EUNSUPPORTED  # not taken by the batch
    assert st[5] == EUNSUPPORTED  # more than 255 tile-parts in a tile
    assert r["rc"] == st[1] and r["error"].startswith("item 1: ")
    good = grk.plan_compress_batch([descs[0], descs[6]])
    assert (r["n_blocks"], r["n_load_jobs"]) == (good["n_blocks"], good["n_load_jobs"])
    # each refusal names its reason
    for i, word in ((1, "precision"), (2, "sample format"), (3, "subsampled"), (4, "custom MCT"), (5, "255 tile-parts")):
        e = grk.plan_compress_batch([descs[0], descs[i]])
        assert e["rc"] == st[i] and e["error"].startswith("item 1: ") and word in e["error"], (i, e["error"])
    # the first failure is the one reported
    e = grk.plan_compress_batch([descs[0], descs[3], descs[1]])
    assert e["rc"] == EUNSUPPORTED and e["error"].startswith("item 1: ") and "subsampled" in e["error"]


def test_plan_arguments():
    grk = _grk()
    L = grk.lib()
    assert grk.plan_compress_batch([])["rc"] == OK
    assert L.grkgpu_compress_batch_plan(None, 0, None) == OK
    assert L.grkgpu_compress_batch_plan(None, 1, None) == EINVAL
    assert L.grkgpu_compress_batch(None, None, 0, None) == EINVAL  # no context
    # info is cleared by a refused call; params NULL = grkgpu_default_cparams
    info = grk.CBatchInfo(n_ok=7)
    assert L.grkgpu_compress_batch_plan(None, 1, ctypes.byref(info)) == EINVAL and info.n_ok == 0
    r = grk.plan_compress_batch([dict(shape=(1, 64, 64), prec=8), dict(shape=(1, 64, 64), prec=8,
                                                                     params=grk.CParams.make())])
    assert r["status"] == [OK, OK] and r["n_blocks"] % 2 == 0
    # unknown sample-format flags, and big-endian on a width other than 16 bits: the item's EINVAL
    r = grk.plan_compress_batch([dict(shape=(1, 8, 8), prec=8, fmt=grk.SAMPLE_U8 | 0x400),
                                 dict(shape=(1, 8, 8), prec=8, fmt=grk.SAMPLE_U8 | grk.SAMPLE_BIG_ENDIAN),
                                 dict(shape=(1, 8, 8), prec=8, fmt=grk.SAMPLE_U8)])
    assert r["status"] == [EINVAL, EINVAL, OK]


def test_abi():
    grk = _grk()
    L = grk.lib()
    for sym in ("grkgpu_compress_batch", "grkgpu_compress_batch_plan", "grkgpu_dcshift_mct_fwd_jobs"):
        assert hasattr(L, sym)
    hdr = open(os.path.join(ROOT, "include", "grk_mi355x.h")).read()
    for decl in ("int grkgpu_compress_batch(grkgpu_ctx *ctx, grkgpu_cbatch_item *items, uint32_t n,",
                 "int grkgpu_compress_batch_plan(grkgpu_cbatch_item *items, uint32_t n,",
                 "int grkgpu_dcshift_mct_fwd_jobs(grkgpu_ctx *ctx, const grkgpu_load_job *jobs, uint32_t n,"):
        assert decl in hdr


def test_struct_sizes(tmp_path):
    """ctypes mirrors against sizeof / offsetof from the header, compiled as C"""
    grk = _grk()
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no C compiler"
    src = tmp_path / "abi.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "grk_mi355x.h"\n'
                   "int main(void) { printf(\"%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n\",\n"
                   "sizeof(grkgpu_cbatch_item), sizeof(grkgpu_cbatch_info), sizeof(grkgpu_load_job),\n"
                   "offsetof(grkgpu_cbatch_item, p), offsetof(grkgpu_cbatch_item, in), offsetof(grkgpu_cbatch_item, cs),\n"
                   "offsetof(grkgpu_cbatch_item, len), offsetof(grkgpu_cbatch_item, status),\n"
                   "offsetof(grkgpu_load_job, dst), offsetof(grkgpu_load_job, src_stride),\n"
                   "offsetof(grkgpu_load_job, shift)); return 0; }\n")
    exe = tmp_path / "abi"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(grk.CBatchItem), ctypes.sizeof(grk.CBatchInfo), ctypes.sizeof(grk.LoadJob),
                   grk.CBatchItem.p.offset, grk.CBatchItem.in_.offset, grk.CBatchItem.cs.offset,
                   grk.CBatchItem.len.offset, grk.CBatchItem.status.offset,
                   grk.LoadJob.dst.offset, grk.LoadJob.src_stride.offset, grk.LoadJob.shift.offset]
    assert ctypes.sizeof(grk.CBatchInfo) == 16 and ctypes.sizeof(grk.LoadJob) == 112
