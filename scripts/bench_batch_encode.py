#!/usr/bin/env python3
"""Small-image encode throughput: N single calls against one batch call.

Frames: g8 = 512x512 8-bit gray, 5/3 (DESIGN.md 5, configs[0]); rgb8 = 512x512
8-bit RGB, 9/7.  The N images are one synthetic frame N times, int32 planes
resident on the host.  For N = 1, 16, 64, 256:

  (a) N Codec.compress calls on one context;
  (b) the same over 16 contexts and threads (how bench.py keeps frames in flight);
  (c) one Codec.compress_batch call (absent on a library without it: skipped).

Mpixels/s from the median of 10 timed repetitions after 2 warm-ups, host clock
around calls that end in a stream synchronise, codestreams as bytes on the
host.  The outputs of (a), (b) and (c) are compared byte for byte.  Each
mode's stage times are those of grkgpu_get_stats for the last call of its last
repetition: a whole batch for (c) -- its h2d_ms is the one upload of the
staged samples -- and one image for (a).

Every (frame, N) step runs in a child process under its own time limit; the
first step that fails or runs out of time ends the run.  One JSON line per
(frame, N, mode); --out FILE also writes them all, with the device and commit.

    python scripts/bench_batch_encode.py --out profiles/batch_encode.json
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

FRAMES = {"g8": (512, 512, 1, 8, False), "rgb8": (512, 512, 3, 8, True)}
NS = (1, 16, 64, 256)
REPS, WARMUP, THREADS = 10, 2, 16


def step(frame, n):
    import torch
    from concurrent.futures import ThreadPoolExecutor

    import grokimagecompression_amd as grk
    import synth
    assert torch.cuda.is_available(), "bench_batch_encode needs cuda:0"
    h, w, c, bits, irrev = FRAMES[frame]
    img = synth.synth_image(h, w, c, bits, 5)
    p = grk.CParams.make(irreversible=irrev)
    codec = grk.Codec(0)
    imgs = [img] * n
    pix = n * h * w

    def timed(fn):
        for _ in range(WARMUP):
            res = fn()
        ts = []
        for _ in range(REPS):
            t0 = time.perf_counter()
            res = fn()
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts), min(ts), max(ts), res

    def stage_ms(cd):
        return {k: round(float(v), 3) for k, v in cd.stats().items() if k.endswith("_ms")}

    def line(mode, t, lo, hi, **extra):
        d = dict(frame=frame, n=n, mode=mode, ms=round(t * 1e3, 3), ms_min=round(lo * 1e3, 3),
                 ms_max=round(hi * 1e3, 3), mpix_s=round(pix / t / 1e6, 1), **extra)
        print(json.dumps(d), flush=True)

    t, lo, hi, ra = timed(lambda: [codec.compress(a, bits, p) for a in imgs])
    line("a", t, lo, hi, stats=stage_ms(codec))
    pool_codecs = [grk.Codec(0) for _ in range(THREADS)]
    with ThreadPoolExecutor(THREADS) as pool:
        def many():
            def work(k):
                return [pool_codecs[k].compress(a, bits, p) for a in imgs[k::THREADS]]
            return list(pool.map(work, range(THREADS)))
        t, lo, hi, rb = timed(many)
    same_b = all(x == ra[0] for part in rb for x in part) and sum(len(part) for part in rb) == n
    line("b", t, lo, hi, same_as_a=bool(same_b))
    for pc in pool_codecs:
        pc.close()
    assert same_b, "threaded output differs from the single calls'"
    if hasattr(grk.lib(), "grkgpu_compress_batch"):
        t, lo, hi, rc = timed(lambda: codec.compress_batch(imgs, bits, p))
        same = rc == ra
        line("c", t, lo, hi, same_as_a=bool(same), stats=stage_ms(codec), info=codec.cbatch_info)
        assert same, "batch output differs from the single calls'"
    codec.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--step", nargs=2, metavar=("FRAME", "N"), help="run one step in this process")
    ap.add_argument("--out", help="write every line, the device and the commit to this JSON file")
    ap.add_argument("--step-timeout", type=int, default=240)
    args = ap.parse_args()
    if args.step:
        step(args.step[0], int(args.step[1]))
        return 0
    lines = []
    for frame in FRAMES:
        for n in NS:
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", frame, str(n)],
                                   capture_output=True, text=True, timeout=args.step_timeout)
            except subprocess.TimeoutExpired:
                print("step %s N=%d ran out of time: stopping" % (frame, n), file=sys.stderr)
                return 1
            sys.stdout.write(r.stdout)
            if r.returncode:
                sys.stderr.write(r.stderr[-2000:])
                print("step %s N=%d failed (%d): stopping" % (frame, n, r.returncode), file=sys.stderr)
                return 1
            lines += [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    if args.out:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip()
        import torch
        box = torch.cuda.get_device_name(0) if torch.cuda.is_available() else "no device"
        with open(args.out, "w") as f:
            json.dump(dict(device=box, commit=commit or None, reps=REPS, warmup=WARMUP, threads=THREADS,
                           unit="Mpixels/s over the median repetition", lines=lines), f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
