"""The MQ output slab rule (t1_lane.h t1_enc_slab_bytes) against the host
build of the block encoder (tests/cpp/test_t1_model.cpp --sweep): every style
0..63 on the shapes where the pass terminations, not the samples, decide a
block's size -- 1x1 up to 4x4, thin blocks, 64x64 -- at every depth 1..26, 5/3
and 9/7, five contents.  A block whose len exceeds the rule fails the run with
its case named; the largest len / rule per style is printed (DESIGN.md 4
keeps the figures).  Also the exported grkgpu_t1_enc_out_bytes.  No GPU
needed."""
import os
import re
import subprocess

from conftest import ROOT

SRC = os.path.join(ROOT, "tests/cpp/test_t1_model.cpp")
NBLOCKS = 64 * 19 * 5 * (25 + 19 + 1)  # styles x shapes x contents x (5/3 depths 1..25, 9/7 1..19, planes at 26)


def _build(exe, flags):
    subprocess.run(["g++", *flags, "-std=c++17", "-Wno-unknown-pragmas", "-o", str(exe), SRC], check=True)


def _ratios(out):
    got = {int(s): float(q) for s, q in re.findall(r"^MAX sty=(\d+) len/rule=([0-9.]+)", out, re.M)}
    assert sorted(got) == list(range(64)), out[-3000:]
    return got


def test_t1_slab_rule_holds_over_the_sweep(tmp_path):
    """The output buffer is far larger than any block, so the verdict is the
    explicit len <= rule comparison, not where the heap puts things."""
    exe = tmp_path / "test_t1_model"
    _build(exe, ["-O2"])
    r = subprocess.run([str(exe), "--sweep"], capture_output=True, text=True)
    print(r.stdout[-6000:])
    assert r.returncode == 0, r.stdout[:4000] + r.stderr[-2000:]
    assert "OK: 0 over the rule / %d blocks" % NBLOCKS in r.stdout
    ratios = _ratios(r.stdout)
    assert max(ratios.values()) <= 1.0, ratios
    # the sweep reaches the regime it is for: blocks the area term alone does not hold
    assert int(re.search(r"blocks past w\*h\*4\+64: (\d+)", r.stdout).group(1)) > 1000


def test_t1_slab_rule_sanitized(tmp_path):
    """The same stand-alone program under AddressSanitizer and UBSan, every
    block's output an allocation of the 16 bytes of headroom plus exactly the
    rule rounded up to 4: no report, exit status 0."""
    exe = tmp_path / "test_t1_model_san"
    # the runtimes linked into the program itself: nothing depends on the order libraries load in
    _build(exe, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                 "-static-libasan", "-static-libubsan"])
    r = subprocess.run([str(exe), "--sweep", "rule"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[:4000] + r.stderr[-4000:]
    assert "OK: 0 over the rule / %d blocks" % NBLOCKS in r.stdout
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert max(_ratios(r.stdout).values()) <= 1.0


def _rule(w, h, sty, bound):
    """t1_enc_slab_bytes restated: the area term, and per terminated pass but
    the last 3 bytes (MQ) or 1 (raw), less 1 where the next pass is MQ."""
    LAZY, TERMALL = 1, 4

    def info(k):
        return (bound - 1, 2) if k == 0 else (bound - 2 - (k - 1) // 3, (k - 1) % 3)

    def raw(bp, pt):
        return bool(sty & LAZY) and bp < bound - 4 and pt < 2

    def term(bp, pt):
        if (pt == 2 and bp == 0) or sty & TERMALL:
            return True
        return bool(sty & LAZY) and ((bp == bound - 4 and pt == 2) or (bp < bound - 4 and pt > 0))

    t = 0
    for k in range(3 * bound - 3):
        bp, pt = info(k)
        if term(bp, pt):
            nbp, npt = info(k + 1)
            t += (1 if raw(bp, pt) else 3) - (0 if raw(nbp, npt) else 1)
    return w * h * 4 + 64 + t


def test_enc_out_bytes_export():
    """grkgpu_t1_enc_out_bytes: the rule at 26 planes; w*h*4 + 64 exactly where
    no pass but the last is terminated; 2 bytes for each of the 75 other
    passes under TERMALL."""
    import grokimagecompression_amd as grk
    if not os.path.exists(grk.LIB_PATH):
        grk.build()
    L = grk.lib()
    for w, h in ((1, 1), (2, 1), (3, 5), (16, 16), (64, 1), (64, 64)):
        for sty in range(64):
            want = _rule(w, h, sty, 26)
            assert L.grkgpu_t1_enc_out_bytes(w, h, sty) == want, (w, h, sty)
            if not sty & 5:
                assert want == w * h * 4 + 64
            if (sty & 5) == 4:
                assert want == w * h * 4 + 64 + 2 * 75
    assert L.grkgpu_t1_enc_out_bytes(65, 1, 0) == 0 and L.grkgpu_t1_enc_out_bytes(1, 65, 4) == 0
