#!/usr/bin/env python3
"""What the fused float store saves: a decode to a device (h,w,3) float16
tensor normalised with the ImageNet mean and std, three ways.

Workloads: 8k = one 7680x4320 8-bit RGB frame, 9/7 with the ICT; batch = 64
frames of 512x512 8-bit RGB, 9/7, in one batch call.  Routes:

  (a) Codec.decompress_float / decompress_batch_float(dtype="float16",
      layout="hwc", device_out=True): the normalisation in the last store;
  (b) what a build without it offers: decompress / decompress_batch_convert(
      dtype=np.uint8, layout="hwc", device_out=True), then the torch ops that
      give the same bits, x.to(torch.float32) * s + b, then .to(torch.float16);
  (c) (b) with that expression under torch.compile, where it compiles here
      (otherwise the line says why not).

Each repetition runs (a), (b), (c) one after the other, so the routes alternate
and share whatever else the machine is doing.  ms per frame from a host clock
around work that ends in a device synchronise; median, min and max of REPS
repetitions after WARMUP.  store_ms is the last-store stage's own device time
(the event interval grkgpu_get_stats reports as dcshift_mct_ms: the fills and
store launches of the decode; Codec.launch_times() lists the DWT launches
only) for the float16 store of (a) and the uint8 store of (b).  The outputs of
(a) and (b) are compared bit for bit.  One JSON line per (workload, route);
--out FILE also writes them all with the device.

    python scripts/bench_float.py --out profiles/float_store.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

REPS, WARMUP = 10, 3
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
WORKLOADS = {"8k": (4320, 7680, 1), "batch": (512, 512, 64)}


def run(name, reps, warmup):
    import numpy as np
    import synth
    import torch

    import grokimagecompression_amd as grk
    assert torch.cuda.is_available(), "bench_float needs cuda:0"
    h, w, n = WORKLOADS[name]
    codec = grk.Codec(0)
    cs = codec.compress(synth.synth_image(h, w, 3, 8, 5), 8, grk.CParams.make(irreversible=True))
    bufs = [cs] * n
    scale, bias = grk.norm_scale_bias(8, MEAN, STD)
    s, b = torch.from_numpy(scale).cuda(), torch.from_numpy(bias).cuda()

    def follow(x):
        return (x.to(torch.float32) * s + b).to(torch.float16)

    def dec_float():
        if n == 1:
            return codec.decompress_float(cs, dtype="float16", scale=scale, bias=bias, layout="hwc", device_out=True)
        return codec.decompress_batch_float(bufs, dtype="float16", scale=scale, bias=bias, layout="hwc", device_out=True,
                                            stack=True)

    def dec_u8():
        if n == 1:
            return codec.decompress(cs, dtype=np.uint8, layout="hwc", device_out=True)
        return codec.decompress_batch_convert(bufs, dtype=np.uint8, layout="hwc", device_out=True, stack=True)

    routes = {"a": lambda: dec_float(), "b": lambda: follow(dec_u8())}
    why_not = None
    try:
        compiled = torch.compile(follow)
        compiled(dec_u8())
        torch.cuda.synchronize()
        routes["c"] = lambda: compiled(dec_u8())
    except Exception as e:  # noqa: BLE001  (whatever keeps inductor from building here)
        why_not = "%s: %s" % (type(e).__name__, str(e).splitlines()[0][:200] if str(e) else "")
    times = {r: [] for r in routes}
    store = {r: [] for r in routes}
    last = {}
    for rep in range(warmup + reps):
        for r, fn in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[r] = fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if rep >= warmup:
                times[r].append(dt * 1e3 / n)
                store[r].append(float(codec.stats()["dcshift_mct_ms"]) / n)
    same = bool(torch.equal(last["a"].view(torch.int16), last["b"].view(torch.int16)))
    lines = []
    for r in routes:
        t = times[r]
        lines.append(dict(workload=name, route=r, frames=n, ms_per_frame=round(statistics.median(t), 4),
                          ms_min=round(min(t), 4), ms_max=round(max(t), 4),
                          store_ms_per_frame=round(statistics.median(store[r]), 4),
                          store_ms_min=round(min(store[r]), 4), store_ms_max=round(max(store[r]), 4),
                          store_format="float16" if r == "a" else "uint8", same_bits_a_b=same))
    if why_not is not None:
        lines.append(dict(workload=name, route="c", not_run=why_not))
    for d in lines:
        print(json.dumps(d), flush=True)
    assert same, "the fused store and the torch follow-up disagree"
    codec.close()
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", nargs="+", default=list(WORKLOADS), choices=list(WORKLOADS))
    ap.add_argument("--reps", type=int, default=REPS)
    ap.add_argument("--warmup", type=int, default=WARMUP)
    ap.add_argument("--out", help="write every line and the device to this JSON file")
    args = ap.parse_args()
    lines = []
    for name in args.workloads:
        lines += run(name, args.reps, args.warmup)
    if args.out:
        import torch
        with open(args.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), reps=args.reps, warmup=args.warmup,
                           unit="ms per frame, host clock around calls that end in a device synchronise", lines=lines),
                      f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
