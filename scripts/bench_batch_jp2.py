#!/usr/bin/env python3
"""Small JP2 files decoded straight to displayable pixels: N single
Codec.decompress_jp2 calls against one Codec.decompress_jp2_batch call.

Files: pal = 512x512, one 8-bit index component (5/3) behind a 256 x 3 palette
of 8-bit columns (pclr + cmap, sRGB); srgb = 512x512 8-bit RGB (5/3 with the
RCT), EnumCS 16.  Both decode to (h,w,3) uint8.  Each is encoded once; the N
files are that file N times, resident on the host.  For every N:

  single  N Codec.decompress_jp2 calls on one context;
  batch   one Codec.decompress_jp2_batch call, stack=True (absent on a library
          without it: skipped).

ms and Mpixels/s from the median of 10 timed repetitions after 2 warm-ups:
host-clock call times around calls that end in a stream synchronise, uint8
pixels to the host.  The outputs of both legs are compared sample for sample.
batch's stage times are grkgpu_get_stats' for the last repetition
(dcshift_mct_ms: the last store -- the palette job launch of pal, the
k_store_jobs launch of srgb, the same pixel count).

Every (file, N, leg) step runs in a child process under its own time limit;
the first step that fails or runs out of time ends the run.  --parent-lib
FILE: the single leg runs on that build of the library (GRKGPU_LIB in the
child), the batch leg on this one, alternating, --rounds times.  One JSON line
per step; --out FILE also writes them all as text lines.

    python scripts/bench_batch_jp2.py --n 64 256 --parent-lib build_ab/libgrk_parent.so --out profiles/batch_jp2.txt
"""
import argparse
import json
import os
import statistics
import struct
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

FILES = ("pal", "srgb")
REPS, WARMUP = 10, 2
H = W = 512


def box(typ, payload=b""):
    return struct.pack(">I", 8 + len(payload)) + typ + payload


def make_file(grk, codec, kind):
    import numpy as np
    import synth
    params = grk.CParams.make(irreversible=False)
    if kind == "srgb":
        return codec.compress_jp2(synth.synth_image(H, W, 3, 8, 5), 8, colour_space="srgb", params=params)
    cs = codec.compress(synth.synth_image(H, W, 1, 8, 5), 8, params)
    entries = np.random.default_rng(7).integers(0, 256, size=(256, 3))
    pclr = struct.pack(">HB", 256, 3) + bytes([7, 7, 7]) + bytes(int(v) for v in entries.reshape(-1))
    cmap = b"".join(struct.pack(">HBB", 0, 1, k) for k in range(3))
    jp2h = (box(b"ihdr", struct.pack(">IIHBBBB", H, W, 1, 7, 7, 0, 0)) + box(b"colr", bytes([1, 0, 0]) + struct.pack(">I", 16))
            + box(b"pclr", pclr) + box(b"cmap", cmap))
    return (box(b"jP  ", b"\x0d\x0a\x87\x0a") + box(b"ftyp", b"jp2 " + b"\0\0\0\0" + b"jp2 ") + box(b"jp2h", jp2h)
            + box(b"jp2c", cs))


def step(kind, n, leg):
    import numpy as np
    import torch

    import grokimagecompression_amd as grk
    assert torch.cuda.is_available(), "bench_batch_jp2 needs cuda:0"
    kw = dict(dtype=np.uint8, layout="hwc", colour=None)
    codec = grk.Codec(0)
    data = make_file(grk, codec, kind)
    bufs = [data] * n
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

    def line(t, lo, hi, **extra):
        d = dict(file=kind, n=n, leg=leg, ms=round(t * 1e3, 3), ms_min=round(lo * 1e3, 3), ms_max=round(hi * 1e3, 3),
                 mpix_s=round(pix / t / 1e6, 1), **extra)
        print(json.dumps(d), flush=True)

    ref = codec.decompress_jp2(data, **kw)[0]
    assert ref.shape == (H, W, 3) and ref.dtype == np.uint8
    if leg == "single":
        t, lo, hi, res = timed(lambda: [codec.decompress_jp2(b, **kw)[0] for b in bufs])
        assert all(np.array_equal(r, ref) for r in res)
        line(t, lo, hi)
    elif hasattr(grk.lib(), "grkgpu_jp2_decompress_batch"):
        t, lo, hi, res = timed(lambda: codec.decompress_jp2_batch(bufs, stack=True, **kw)[0])
        same = res.shape == (n, H, W, 3) and all(np.array_equal(r, ref) for r in res)
        st = {k: round(float(v), 3) for k, v in codec.stats().items() if k.endswith("_ms")}
        line(t, lo, hi, same_as_single=bool(same), stats=st, info=codec.batch_info)
        assert same, "batch output differs from the single call's"
    codec.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--step", nargs=3, metavar=("FILE", "N", "LEG"), help="run one step in this process")
    ap.add_argument("--n", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", help="write every line, the device and the commit to this text file")
    ap.add_argument("--parent-lib", help="another build of the library for the single leg")
    ap.add_argument("--step-timeout", type=int, default=240)
    args = ap.parse_args()
    if args.step:
        step(args.step[0], int(args.step[1]), args.step[2])
        return 0
    lines = []
    for rnd in range(args.rounds):
        for kind in FILES:
            for n in args.n:
                for leg in ("single", "batch"):
                    lib = args.parent_lib if leg == "single" else None
                    env = dict(os.environ, GRKGPU_LIB=os.path.abspath(lib)) if lib else None
                    try:
                        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", kind, str(n), leg],
                                           capture_output=True, text=True, timeout=args.step_timeout, env=env)
                    except subprocess.TimeoutExpired:
                        print("step %s N=%d %s ran out of time: stopping" % (kind, n, leg), file=sys.stderr)
                        return 1
                    tag = '{"round": %d, "lib": "%s", ' % (rnd, "parent" if lib else "this")
                    out = [tag + x[1:] for x in r.stdout.splitlines() if x.startswith("{")]
                    print("\n".join(out), flush=True)
                    lines += out
                    if r.returncode:
                        sys.stderr.write(r.stderr[-2000:])
                        print("step %s N=%d %s failed (%d): stopping" % (kind, n, leg, r.returncode), file=sys.stderr)
                        return 1
    if args.out:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip()
        import torch
        box_ = torch.cuda.get_device_name(0) if torch.cuda.is_available() else "no device"
        with open(args.out, "w") as f:
            f.write("# scripts/bench_batch_jp2.py: %s, parent commit %s, %d reps after %d warm-ups, %d alternating rounds\n"
                    % (box_, commit or "?", REPS, WARMUP, args.rounds))
            f.write("# single: N decompress_jp2 calls (lib parent = the parent commit's build); batch: one decompress_jp2_batch\n")
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
