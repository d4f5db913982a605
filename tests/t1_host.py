"""The host build of the whole block encoder (tests/cpp/test_t1_model.cpp
--encode: prep, t1_model_plane per plane, t1_mq_block) as a reference for the
styled streams of single code-blocks: build(dir) compiles it once and returns
run(cases, sty) -> [(numbps, numpasses, rates, bytes)] for cases of
(h, w, orient, qmfbid, inv_step, int32 block)."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(workdir):
    exe = os.path.join(str(workdir), "test_t1_model")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wno-unknown-pragmas", "-o", exe,
                    os.path.join(ROOT, "tests/cpp/test_t1_model.cpp")], check=True)

    def run(cases, sty):
        fin, fout = exe + ".in", exe + ".out"
        with open(fin, "wb") as f:
            f.write(np.uint32(len(cases)).tobytes())
            for h, w, orient, qmfbid, inv, blk in cases:
                f.write(np.array([w, h, orient, qmfbid, inv], np.uint32).tobytes())
                f.write(np.ascontiguousarray(blk, np.int32).tobytes())
        subprocess.run([exe, "--encode", fin, fout, str(sty)], check=True)
        raw = open(fout, "rb").read()
        res, pos = [], 0
        for _ in cases:
            rec = np.frombuffer(raw, np.uint32, 99, pos)
            pos += 99 * 4
            res.append((int(rec[0]), int(rec[1]), [int(v) for v in rec[3:3 + rec[1]]], raw[pos:pos + int(rec[2])]))
            pos += int(rec[2])
        assert pos == len(raw)
        return res
    return run
