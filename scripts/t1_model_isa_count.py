"""Instruction counts of the emission loops of k_t1_model<true> (t1_lane.h
t1_model_plane: the loops of the significance, refinement and cleanup passes
that form a stripe's symbol bytes and store them to the LDS ring), from the
gfx950 assembly.  An emission loop is a loop with a ring store
(ds_write_b32) in its own blocks; the pass is the stripe loop (depth 1) it sits in, in code
order SPP, MRP, CUP.  Per iteration: VALU / SALU / LDS / VMEM with every
exec-masked region entered (all regions), and without the blocks in which a
64-byte run leaves the ring (less run16: they hold the 16-byte global
stores), and how many of the VALU are variable 64-bit shifts, 24-bit
multiplies and byte permutes.  A loop nested in an emission loop (the skip
of empty column groups) is not counted with it.  --cols N: columns per iteration (1: a loop over set columns; 4:
a loop over 4-column groups), for the per-column figures.
  python scripts/t1_model_isa_count.py [kernels.hip] [--cols N]"""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
args = sys.argv[1:]
cols = 1
if "--cols" in args:
    i = args.index("--cols")
    cols = int(args[i + 1])
    del args[i:i + 2]
src = os.path.abspath(args[0]) if args else os.path.join(ROOT, "grokimagecompression_amd", "csrc", "kernels.hip")
out = "/tmp/t1_model_isa_%d.s" % os.getpid()
subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
                "--cuda-device-only", "-S", src, "-o", out], check=True, cwd=os.path.dirname(src),
               stderr=subprocess.DEVNULL)
s = open(out).read()
os.unlink(out)
name = re.search(r"^(_ZN6grkgpu10k_t1_modelILb1E\S*):", s, re.M).group(1)
body = s[s.index(name + ":"):]
body = body[:body.index(".Lfunc_end")]

# blocks in code order; for each its innermost loop (header label) and, for a
# header, its depth and whether it is an innermost loop
blocks, order, loopof, depth, inner = {}, [], {}, {}, set()
cur = None
for ln in body.split("\n"):
    m = re.match(r"^(\.LBB\d+_\d+|; %bb\.\d+):\s*(.*)$", ln)
    if m:
        cur = m.group(1).replace("; ", "")
        blocks[cur] = []
        order.append(cur)
        loopof[cur] = None
        ln = m.group(2)
    if cur is None:
        continue
    if not blocks[cur]:
        h = re.search(r"in Loop: Header=BB(\d+_\d+) Depth=(\d+)", ln)
        if h:
            loopof[cur] = ".LBB" + h.group(1)
        h = re.search(r"This (Inner )?Loop Header: Depth=(\d+)", ln)
        if h:
            loopof[cur] = cur
            depth[cur] = int(h.group(2))
            if h.group(1):
                inner.add(cur)
    if ln.startswith("\t") and not ln.startswith("\t;") and not ln.startswith("\t."):
        blocks[cur].append(ln.strip())


def kind(x):
    op = x.split()[0]
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "buffer_", "flat_")):
        return "vmem"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("s_"):
        return "salu"
    return "other"


def count(bs):
    t = {"valu": 0, "salu": 0, "lds": 0, "vmem": 0, "other": 0, "sh64": 0, "mul24": 0, "perm": 0}
    for b in bs:
        for x in blocks[b]:
            t[kind(x)] += 1
            op = x.split()[0]
            t["sh64"] += op.startswith(("v_lshrrev_b64", "v_lshlrev_b64", "v_ashrrev_i64"))
            t["mul24"] += op.startswith("v_mul_u32_u24")
            t["perm"] += op.startswith("v_perm_b32")
    return t


stripe_loops = [b for b in order if depth.get(b) == 1 and b not in inner]
PASS = ["SPP", "MRP", "CUP"]
print("%s: %d instructions" % (name[:40], sum(len(v) for v in blocks.values())))
fmt = "VALU %4d (64-bit shifts %3d, mul24 %3d, perm %3d)  SALU %3d  LDS %3d  VMEM %2d"
for hb in order:
    if hb not in depth or depth[hb] < 2:
        continue
    lb = [b for b in order if loopof.get(b) == hb]  # its own blocks: nested loops (the skip of empty groups) apart
    if not any(x.startswith("ds_write_b32") for b in lb for x in blocks[b]):
        continue
    before = [q for q in stripe_loops if order.index(q) < order.index(hb)]
    if not before or len(before) > 3:
        continue
    run16 = [b for b in lb if any(x.startswith("global_store_dwordx4") for x in blocks[b])]
    allc, com = count(lb), count([b for b in lb if b not in run16])
    print("%s emission loop %s (depth %d, %d blocks), per iteration of %d column%s:" % (
        PASS[len(before) - 1], hb, depth[hb], len(lb), cols, "" if cols == 1 else "s"))
    for label, t in (("all regions", allc), ("less run16", com)):
        print(("  %-12s " + fmt) % (label, t["valu"], t["sh64"], t["mul24"], t["perm"], t["salu"], t["lds"], t["vmem"]))
        if cols > 1:
            print("  %-12s VALU %.1f per column" % ("", t["valu"] / cols))
