"""tests/cpp/test_t1_fused.cpp: the T1 decoder's column step (one step per
sample: the zero-coding or run decision and the sign decision it leads to)
compiled for the host, against the C oracle's decode -- six block sizes, six
contents, seven styles; plain, and once more under AddressSanitizer + UBSan
(a stand-alone program, no GPU needed)."""
import os
import re
import subprocess

from conftest import ROOT


def _build(exe, flags):
    ob = os.path.join(ROOT, "oracle", "build")
    subprocess.run(["g++", *flags, "-std=c++17", "-Wno-unknown-pragmas", "-o", str(exe),
                    os.path.join(ROOT, "tests/cpp/test_t1_fused.cpp"), "-L" + ob, "-lgrk_oracle", "-Wl,-rpath," + ob],
                   check=True)


def _check(r):
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    m = re.search(r"OK: 0 failures / (\d+) blocks, (\d+) decodes", r.stdout)
    assert m, r.stdout[-2000:]
    # 6 sizes x 6 contents x 4 orientations; all but the empty ones decoded
    # once from the oracle's bytes and once per style from our own
    assert int(m.group(1)) == 144 and int(m.group(2)) == 120 * 8


def test_fused_column_step_host_matches_oracle(oracle, tmp_path):
    exe = tmp_path / "test_t1_fused"
    _build(exe, ["-O2"])
    _check(subprocess.run([str(exe)], capture_output=True, text=True))


def test_fused_column_step_host_sanitized(oracle, tmp_path):
    exe = tmp_path / "test_t1_fused_san"
    # the runtimes linked into the program itself: nothing depends on the order libraries load in
    _build(exe, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                 "-static-libasan", "-static-libubsan"])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    _check(r)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
