"""The decoder's host half on damaged streams, no device: the ~2,650 cases of
tests/golden/manifest_damage.json (oracle/make_golden_damage.py: 1 to 3 bytes
of a golden replaced in the SOT fields, the tile-part marker segments, behind
SOD, at SOP / EPH markers, in packed packet headers, in the tile data and at
the tail of a tile-part, each decoded by the reference).

* The host half (main header, tile-part walk, packet headers, table layout:
  grkgpu_dec_tables_of, grkgpu_walk_tiles) refuses exactly the streams the
  reference refuses, as corrupt or unsupported, and decodes the reference's
  tiles.
* The tables it hands the Tier-1, DWT and store kernels for the streams it
  accepts keep every offset inside its buffer (damage_fixtures.plan_problems).
* The same code compiled with AddressSanitizer and UBSan
  (tests/cpp/damage_plan_check.cpp, a stand-alone program) runs every case
  on an exactly sized copy of the stream, alone and in batches, clean."""
import ctypes
import os
import shutil
import struct
import subprocess

import pytest

import damage_fixtures as dmg
from conftest import ROOT

CSRC = os.path.join(ROOT, "grokimagecompression_amd", "csrc")
_RESULT = {}


def _grk():
    import grokimagecompression_amd as grk
    return grk


def _run(name):
    """[(case, damaged stream, tables or None, error code)] of stream `name`, computed once"""
    if name not in _RESULT:
        grk = _grk()
        out = []
        for c, cs in dmg.cases(name):
            try:
                out.append((c, cs, grk.dec_tables(cs), 0))
            except grk.GrkGpuError as e:
                out.append((c, cs, None, dmg.error_code(e)))
        _RESULT[name] = out
    return _RESULT[name]


def test_manifest_shape():
    man = dmg.manifest()
    assert len(man) == 22
    ndev = 0
    for name, rec in man.items():
        kept = len(rec["cases"])
        assert kept >= 115 and sum(rec["left_out"].values()) <= 0.01 * rec["drawn"], name
        assert rec["refused"] >= 0.15 * kept and rec["decoded"] >= 0.30 * kept, name
        assert {"sot", "sod48", "uniform", "tail16"} <= {c["s"] for c in rec["cases"]}, name
        assert all(1 <= len(c["p"]) <= 3 for c in rec["cases"]), name
        ndev += sum("deviation" in c for c in rec["cases"])
    assert ndev <= 8


@pytest.mark.parametrize("name", dmg.STREAMS)
def test_refuses_where_the_reference_refuses(name):
    grk = _grk()
    wrong = []
    for c, cs, tab, code in _run(name):
        if c["r"] == "error":
            if tab is not None:
                wrong.append((c["p"], "accepted; the reference refuses"))
            elif code not in (dmg.ECORRUPT, dmg.EUNSUPPORTED):
                wrong.append((c["p"], "refused with code %d" % code))
            with pytest.raises(grk.GrkGpuError):
                grk.walk_tiles(cs)
            continue
        if tab is None:
            wrong.append((c["p"], "refused (%d); the reference decodes" % code))
        elif "t" in c:
            got = grk.walk_tiles(cs)
            if got != c["t"]:
                wrong.append((c["p"], "tiles %s, the reference's image holds %s" % (got, c["t"])))
    assert not wrong, (name, len(wrong), wrong[:8])


@pytest.mark.parametrize("name", dmg.STREAMS)
def test_plan_stays_inside_its_buffers(name):
    wrong = []
    n = 0
    for c, cs, tab, code in _run(name):
        if tab is None:
            continue
        n += 1
        assert tab["data_bytes"] >= len(cs)
        bad = dmg.plan_problems(tab)
        if bad:
            wrong.append((c["p"], bad))
    assert n >= 30
    assert not wrong, (name, len(wrong), wrong[:4])


@pytest.mark.parametrize("name", dmg.STREAMS)
def test_clean_plan_stays_inside_its_buffers(name):
    grk = _grk()
    cs = dmg.clean(name)
    tab = grk.dec_tables(cs)
    assert dmg.plan_problems(tab) == []
    if name != "sub_422_I_tiles":  # (the plain batch plan refuses a subsampled stream)
        assert len(tab["blocks"]) == grk.plan_batch([cs])["n_blocks"]
    assert len(tab["blocks"]) > 0 and tab["coef_elems"] > 0 and tab["ll_elems"] > 0
    assert len(tab["style"]) == len(tab["blocks"]) and (tab["roi"] is None or len(tab["roi"]) == len(tab["blocks"]))
    assert (tab["roi"] is not None) == (name == "g12_roi_M1_tiles")
    # reduce and layers reach the tables: fewer blocks decoded, fewer passes
    if name == "g8_256":
        assert len(grk.dec_tables(cs, reduce=1)["blocks"]) < len(tab["blocks"])
    if name == "rgb8_rlcp_layers":
        assert grk.dec_tables(cs, layers=1)["blocks"]["len"].sum() < tab["blocks"]["len"].sum()


def test_plan_checks_catch_a_bad_table():
    """the checks themselves: each broken field is reported"""
    grk = _grk()
    good = grk.dec_tables(dmg.clean("g8_tiles64"))
    assert dmg.plan_problems(good) == []

    def broken(field, i, v, table="blocks"):
        t = dict(good)
        t[table] = good[table].copy()
        t[table][field][i] = v
        return dmg.plan_problems(t)

    big = int(good["blocks"]["dst_off"].argmax())
    assert broken("dst_off", big, good["coef_elems"])
    assert broken("dst_off", 1, good["blocks"]["dst_off"][0])        # overlap
    assert broken("w", 0, 65) and broken("h", 0, 0) and broken("orient", 0, 4) and broken("dstride", 0, 1)
    assert broken("numbps", 0, 31) and broken("numpasses", 0, 200) and broken("len", 0, 0)
    assert broken("data_off", 0, good["data_bytes"], "segs") and broken("len", 0, 1 << 30, "segs")
    assert broken("npasses", 0, 0, "segs")
    t = dict(good)
    t["seg_first"] = good["seg_first"][::-1].copy()
    assert dmg.plan_problems(t)


def test_dec_tables_arguments():
    grk = _grk()
    L = grk.lib()
    t = grk.DecTables()
    cs = dmg.clean("g8_256")
    buf = ctypes.create_string_buffer(cs, len(cs))
    assert L.grkgpu_dec_tables_of(None, 0, None, ctypes.byref(t)) == dmg.EINVAL
    assert L.grkgpu_dec_tables_of(buf, len(cs), None, None) == dmg.EINVAL
    assert L.grkgpu_dec_tables_of(buf, len(cs), None, ctypes.byref(t)) == dmg.OK and t.n_blocks > 0 and not t.roi
    L.grkgpu_dec_tables_free(ctypes.byref(t))
    assert t.n_blocks == 0 and not t.blocks and not t.segs
    L.grkgpu_dec_tables_free(ctypes.byref(t))   # twice, and NULL: nothing
    L.grkgpu_dec_tables_free(None)
    assert L.grkgpu_dec_tables_of(buf, 40, None, ctypes.byref(t)) != dmg.OK and not t.blocks
    dp = grk.DParams(cp_reduce=30)
    assert L.grkgpu_dec_tables_of(buf, len(cs), ctypes.byref(dp), ctypes.byref(t)) == dmg.EINVAL


def test_struct_sizes(tmp_path):
    """ctypes mirrors against sizeof / offsetof from the header, compiled as C"""
    grk = _grk()
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no C compiler"
    src = tmp_path / "abi.c"
    fields = [("grkgpu_dec_block", grk.DecBlock, ["data_off", "dst_off", "len", "numpasses", "numbps", "w", "h",
                                                  "orient", "dstride", "irreversible", "stepsize", "pad"]),
              ("grkgpu_dec_seg", grk.DecSeg, ["data_off", "len", "npasses", "pad_"]),
              ("grkgpu_dec_tables", grk.DecTables, ["n_blocks", "n_segs", "data_bytes", "coef_elems", "ll_elems",
                                                    "blocks", "segs", "seg_first", "style", "roi"])]
    exprs, want = [], []
    for cname, py, names in fields:
        assert [f for f, _ in py._fields_] == names
        exprs.append("sizeof(%s)" % cname)
        want.append(ctypes.sizeof(py))
        for f in names:
            exprs.append("offsetof(%s, %s)" % (cname, f))
            want.append(getattr(py, f).offset)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "grk_mi355x.h"\nint main(void) {\n' +
                   "".join('printf("%%zu\\n", (size_t)%s);\n' % e for e in exprs) + "return 0; }\n")
    exe = tmp_path / "abi"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == want
    assert ctypes.sizeof(grk.DecBlock) == 56 and ctypes.sizeof(grk.DecSeg) == 24


def test_sanitized_plan_check(tmp_path):
    """The host half under AddressSanitizer and UBSan: tests/cpp/damage_plan_check.cpp
    (its own main, nothing preloaded) applies every case's patch to an exactly
    sized malloc copy of its stream and runs the batch plan and the table
    export on it, alone and in lists of 16 with clean streams mixed in.  Host
    code only: the five .cpp files are compiled for the host with the
    sanitizers, the kernels' objects are the ones the build made, and the
    program makes no device call."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    objs = [os.path.join(CSRC, "build", o) for o in ("kernels.o", "dwt.o")]
    assert os.path.exists(hipcc) and all(os.path.exists(o) for o in objs), "build() first"
    man = dmg.manifest()
    blob = [struct.pack("<I", len(man))]
    for name in dmg.STREAMS:
        cs = dmg.clean(name)
        cases = man[name]["cases"]
        blob.append(struct.pack("<III", len(cs), int(name.startswith("sub_")), len(cases)) + cs)
        for c in cases:
            blob.append(struct.pack("<I", len(c["p"])) + b"".join(struct.pack("<II", o, v) for o, v in c["p"]))
    data = tmp_path / "cases.bin"
    data.write_bytes(b"".join(blob))
    exe = tmp_path / "damage_plan_check"
    srcs = [os.path.join(CSRC, f) for f in ("codec.cpp", "codestream.cpp", "t2.cpp", "multi.cpp", "jp2.cpp")]
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]
    srcs.append(os.path.join(ROOT, "tests", "cpp", "damage_plan_check.cpp"))
    # (objects first: hipcc reads every input behind a .cpp as HIP source)
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-w", *san,
                    "-I", os.path.join(ROOT, "include"), "-I", CSRC, "-c", *srcs], check=True, timeout=1500, cwd=tmp_path)
    mine = [str(tmp_path / (os.path.splitext(os.path.basename(f))[0] + ".o")) for f in srcs]
    subprocess.run([hipcc, "--offload-arch=gfx950", *san[:2], *mine, *objs, "-o", str(exe)], check=True, timeout=600)
    r = subprocess.run([str(exe), str(data)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    total = sum(len(man[n]["cases"]) for n in man)
    assert "cases %d " % total in r.stdout and " mismatches 0" in r.stdout, r.stdout[-2000:]
