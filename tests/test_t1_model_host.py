"""The encoder's context modelling (t1_lane.h t1_model_plane, the code of
k_t1_model) compiled for the host, against the plain per-sample modeller of
tests/cpp/test_t1_model.cpp: symbol bytes and pass counts of every plane of a
few thousand blocks (every edge width and stripe-remainder height, all
orientations, dense / sparse / empty / single-sample / full-magnitude /
checkerboard-sign content, styles 0, VSC, SEGSYM, VSC|SEGSYM, BYPASS).  No
GPU needed."""
import os
import subprocess

from conftest import ROOT

SRC = os.path.join(ROOT, "tests/cpp/test_t1_model.cpp")


def _build(exe, flags):
    subprocess.run(["g++", *flags, "-std=c++17", "-Wno-unknown-pragmas", "-o", str(exe), SRC], check=True)


def test_t1_model_host_matches_plain_modeller(tmp_path):
    exe = tmp_path / "test_t1_model"
    _build(exe, ["-O2"])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "OK: 0 failures / 3072 blocks" in r.stdout


def test_t1_model_host_sanitized(tmp_path):
    """The same stand-alone program under AddressSanitizer and UBSan, every
    plane's symbol slot an allocation of exactly sym_slot_bytes(w, h): no
    report, exit status 0."""
    exe = tmp_path / "test_t1_model_san"
    # the runtimes linked into the program itself: nothing depends on the order libraries load in
    _build(exe, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                 "-static-libasan", "-static-libubsan"])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
    assert "OK: 0 failures / 3072 blocks" in r.stdout
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
