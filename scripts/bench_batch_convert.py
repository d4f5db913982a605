#!/usr/bin/env python3
"""Small frames decoded straight to displayable pixels: N single calls against
one converting batch call.

Frames: yuv420 = 512x512 8-bit 4:2:0, 5/3, decoded to (h,w,3) uint8 RGB with
colour="sycc"; rgb12 = 512x512 12-bit RGB, 9/7 with the ICT, decoded to (h,w,3)
uint8 with out_prec=8, prec_mode="scale".  Each is encoded once; the N streams
are that stream N times, resident on the host.  For N = 1, 16, 64, 256:

  (a) N Codec.decompress calls on one context;
  (b) the same over 16 contexts and threads (how bench.py keeps frames in flight);
  (c) one Codec.decompress_batch_convert call (absent on a library without it: skipped).

Mpixels/s from the median of 10 timed repetitions after 2 warm-ups: host-clock
call times around calls that end in a stream synchronise, uint8 pixels to the
host -- not kernel shares of a peak.  The outputs of (a) and (c) are compared
sample for sample.  (c)'s stage times are those of grkgpu_get_stats for the
last repetition.

Every (frame, N) step runs in a child process under its own time limit; the
first step that fails or runs out of time ends the run.  --parent-lib FILE:
each step is followed by the same step on that build of the library
(GRKGPU_LIB in the child), alternating, its lines kept as parent_lines.  One
JSON line per (frame, N, mode); --out FILE also writes them all, with the
device and commit.

    python scripts/bench_batch_convert.py --out profiles/batch_convert.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

FRAMES = {"yuv420": dict(colour="sycc"), "rgb12": dict(out_prec=8, prec_mode="scale")}
NS = (1, 16, 64, 256)
REPS, WARMUP, THREADS = 10, 2, 16
H = W = 512


def stream(grk, codec, frame):
    import synth
    if frame == "yuv420":
        subs = [(1, 1), (2, 2), (2, 2)]
        planes = [synth.synth_image(H // dy, W // dx, 1, 8, 5 + k)[0] for k, (dx, dy) in enumerate(subs)]
        return codec.compress_subsampled(planes, 8, (W, H), subs, grk.CParams.make(irreversible=False))
    return codec.compress(synth.synth_image(H, W, 3, 12, 5), 12, grk.CParams.make(irreversible=True))


def step(frame, n):
    import numpy as np
    import torch
    from concurrent.futures import ThreadPoolExecutor

    import grokimagecompression_amd as grk
    assert torch.cuda.is_available(), "bench_batch_convert needs cuda:0"
    kw = dict(dtype=np.uint8, layout="hwc", **FRAMES[frame])
    codec = grk.Codec(0)
    cs = stream(grk, codec, frame)
    bufs = [cs] * n
    pix = n * H * W

    def timed(fn):
        for _ in range(WARMUP):
            res = fn()
        ts = []
        for _ in range(REPS):
            t0 = time.perf_counter()
            res = fn()
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts), min(ts), max(ts), res

    def line(mode, t, lo, hi, **extra):
        d = dict(frame=frame, n=n, mode=mode, ms=round(t * 1e3, 3), ms_min=round(lo * 1e3, 3),
                 ms_max=round(hi * 1e3, 3), mpix_s=round(pix / t / 1e6, 1), **extra)
        print(json.dumps(d), flush=True)

    t, lo, hi, ra = timed(lambda: [codec.decompress(b, **kw) for b in bufs])
    assert ra[0].shape == (H, W, 3) and ra[0].dtype == np.uint8
    line("a", t, lo, hi)
    pool_codecs = [grk.Codec(0) for _ in range(THREADS)]
    with ThreadPoolExecutor(THREADS) as pool:
        def many():
            def work(k):
                return [pool_codecs[k].decompress(b, **kw) for b in bufs[k::THREADS]]
            return list(pool.map(work, range(THREADS)))
        t, lo, hi, _ = timed(many)
    line("b", t, lo, hi)
    for pc in pool_codecs:
        pc.close()
    if hasattr(grk.lib(), "grkgpu_decompress_batch_convert"):
        t, lo, hi, rc = timed(lambda: codec.decompress_batch_convert(bufs, stack=True, **kw))
        same = len(ra) == len(rc) and all(np.array_equal(x, y) for x, y in zip(ra, rc))
        st = {k: round(float(v), 3) for k, v in codec.stats().items() if k.endswith("_ms")}
        line("c", t, lo, hi, same_as_a=bool(same), stats=st, info=codec.batch_info)
        assert same, "batch output differs from the single calls'"
    codec.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--step", nargs=2, metavar=("FRAME", "N"), help="run one step in this process")
    ap.add_argument("--out", help="write every line, the device and the commit to this JSON file")
    ap.add_argument("--parent-lib", help="another build of the library, run step by step after this one")
    ap.add_argument("--step-timeout", type=int, default=240)
    args = ap.parse_args()
    if args.step:
        step(args.step[0], int(args.step[1]))
        return 0
    lines, parent_lines = [], []
    for frame in FRAMES:
        for n in NS:
            for lib, into in ((None, lines), (args.parent_lib, parent_lines)):
                if into is parent_lines and not lib:
                    continue
                env = dict(os.environ, GRKGPU_LIB=os.path.abspath(lib)) if lib else None
                try:
                    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", frame, str(n)],
                                       capture_output=True, text=True, timeout=args.step_timeout, env=env)
                except subprocess.TimeoutExpired:
                    print("step %s N=%d ran out of time: stopping" % (frame, n), file=sys.stderr)
                    return 1
                sys.stdout.write(r.stdout if not lib else r.stdout.replace('{"frame"', '{"lib": "parent", "frame"'))
                sys.stdout.flush()
                if r.returncode:
                    sys.stderr.write(r.stderr[-2000:])
                    print("step %s N=%d failed (%d): stopping" % (frame, n, r.returncode), file=sys.stderr)
                    return 1
                into += [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    if args.out:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip()
        import torch
        box = torch.cuda.get_device_name(0) if torch.cuda.is_available() else "no device"
        with open(args.out, "w") as f:
            json.dump(dict(device=box, commit=commit or None, reps=REPS, warmup=WARMUP, threads=THREADS,
                           unit="Mpixels/s over the median repetition; host-clock call times",
                           lines=lines, parent_lines=parent_lines), f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
