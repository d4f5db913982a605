"""Colour-step fixtures: tests/golden/manifest_colour.json.

The REFERENCE's own bin/common/color.cpp, compiled as it stands into
oracle/_ref/ (nothing compiled is committed) with a grk_apps_config.h made
from the reference's template with no optional library, and linked with
tests/cpp/colour_driver.cpp and oracle/_ref/libgrok.so, converts the seeded
inputs of tests/colour_fixtures.py; the manifest keeps, per case, the input
recipe's digest, the sha256 of the reference's output planes and the
precision / sign the reference leaves on each output component.  The numpy
closed forms of colour_fixtures.py -- what the GPU tests compare with -- have
to reproduce every digest (tests/test_decode_colour_host.py).

  python scripts/make_golden_colour.py [--check]"""
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

import colour_fixtures as cf  # noqa: E402
import make_golden as mg  # noqa: E402

REF = "/root/reference/src"
OUT = os.path.join(ROOT, "oracle", "_ref")
DRIVER = os.path.join(OUT, "colour_driver")
GEN = os.path.join(OUT, "gen_apps")


def build_driver():
    mg.build_ref()
    src = os.path.join(ROOT, "tests", "cpp", "colour_driver.cpp")
    if os.path.exists(DRIVER) and os.path.getmtime(DRIVER) >= os.path.getmtime(src):
        return
    os.makedirs(GEN, exist_ok=True)
    with open(os.path.join(REF, "bin", "common", "grk_apps_config.h.cmake.in")) as f:
        tmpl = f.read()
    # no optional library: every #cmakedefine left undefined, as CMake does for a library it did not find
    with open(os.path.join(GEN, "grk_apps_config.h"), "w") as f:
        f.write(re.sub(r"^#cmakedefine\s+(\w+).*$", r"/* #undef \1 */", tmpl, flags=re.M))
    inc = ["-I" + GEN, "-I" + os.path.join(OUT, "gen"), "-I" + os.path.join(REF, "lib", "jp2"),
           "-I" + os.path.join(REF, "include"), "-I" + os.path.join(REF, "bin", "common")]
    obj = os.path.join(OUT, "obj", "bin_common_color.o")
    os.makedirs(os.path.dirname(obj), exist_ok=True)
    # x86-64 without -march: no FMA instruction exists to contract into
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-w"] + inc +
                   ["-c", os.path.join(REF, "bin", "common", "color.cpp"), "-o", obj], check=True)
    subprocess.run(["g++", "-std=c++17", "-O2"] + inc + ["-o", DRIVER, src, obj, "-L" + OUT, "-lgrok",
                                                         "-Wl,-rpath,$ORIGIN", "-lpthread"], check=True)


def ref_convert(kind, precs, sgnds, planes, tmp):
    src, out = os.path.join(tmp, "in.i32"), os.path.join(tmp, "out.i32")
    n = planes[0].size
    np.concatenate([np.ascontiguousarray(p, dtype="<i4").ravel() for p in planes]).tofile(src)
    r = subprocess.run([DRIVER, kind, src, out, str(n), ",".join(str(p) for p in precs),
                        ",".join(str(s) for s in sgnds)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    comps = [[int(v) for v in ln.split()[1:]] for ln in r.stdout.splitlines() if ln.startswith("comp")]
    raw = np.fromfile(out, dtype="<i4")
    assert raw.size == n * len(comps)
    return [raw[k * n:(k + 1) * n] for k in range(len(comps))], comps


def main():
    check = "--check" in sys.argv
    build_driver()
    man = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, (kind, precs, sgnds, planes) in cf.cases().items():
            outp, comps = ref_convert(kind, precs, sgnds, planes, tmp)
            man[name] = dict(kind=kind, prec=precs, sgnd=sgnds, n=int(planes[0].size), in_sha256=cf.digest(planes),
                             ref_sha256=cf.digest(outp), ref_comps=comps,
                             ref_min=[int(p.min()) for p in outp], ref_max=[int(p.max()) for p in outp])
            print(name, kind, len(outp), "planes", flush=True)
    if check:
        old = cf.manifest()
        bad = [k for k in sorted(set(old) | set(man)) if old.get(k) != json.loads(json.dumps(man.get(k)))]
        print("mismatches", len(bad), bad)
        sys.exit(1 if bad else 0)
    with open(cf.MANIFEST, "w") as f:
        json.dump(man, f, indent=1)


if __name__ == "__main__":
    main()
