#!/usr/bin/env python3
"""Builds oracle/_ref/: the reference's OWN vote kernels (ppf_voting, backvote, rot_voting), executed text, as

    libref_vote_host.so          host C++ (g++ -O2 -ffp-contract=off, glibc trig), serial over the launch indices
    ref_vote_gfx950.hsaco        gfx950 code object, hipcc defaults: what a straight HIP port of the reference would run
    ref_vote_gfx950_nofma.hsaco  the same with -ffp-contract=off
    ref_vote_runner              plain C over libamdhip64: loads a code object, runs one kernel, files in / file out

TEST INFRASTRUCTURE ONLY.  Nothing of the reference is stored in this repository: the kernel text is read at build time
from <reference>/models/voting.py (the cupy.RawKernel strings, found by pattern) and models/include/helper_math.cuh
(its one CUDA-toolkit include line, found by pattern, redirected to oracle/ref_shim.h) and written to oracle/_ref/, which
git ignores.  `findpeak` is left out (never launched by the reference).

    python oracle/ref_build.py [<reference root>]        (default: $CPPF_REFERENCE or /root/reference)

build(): returns the directory when it was built, None when the reference is absent (an existing oracle/_ref/ is left
alone); raises when the reference is present and any step fails.
"""
import os
import re
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "_ref")
KERNELS = ("ppf_voting", "backvote", "rot_voting")
HOST_SO, RUNNER = "libref_vote_host.so", "ref_vote_runner"
CODE_OBJECTS = {"default": "ref_vote_gfx950.hsaco", "nofma": "ref_vote_gfx950_nofma.hsaco"}

_RAW_KERNEL = re.compile(r"RawKernel\(\s*r'''(.*?)'''\s*,\s*'(\w+)'", re.S)
_TOOLKIT_INCLUDE = re.compile(r'^[ \t]*#[ \t]*include[ \t]*"[^"\n]*cuda_runtime\.h"[ \t]*$', re.M)


def reference_root(arg=None):
    return arg or os.environ.get("CPPF_REFERENCE") or "/root/reference"


def _rocm():
    return os.environ.get("ROCM_PATH", "/opt/rocm")


def extract(ref, out=OUT):
    """the three kernel strings -> out/<name>.cu.inc, helper_math.cuh -> out/helper_math.cuh (include redirected)"""
    with open(os.path.join(ref, "models", "voting.py")) as f:
        found = {name: text for text, name in _RAW_KERNEL.findall(f.read())}
    missing = [k for k in KERNELS if k not in found]
    if missing:
        raise RuntimeError(f"kernel strings not found in the reference's models/voting.py: {missing}")
    with open(os.path.join(ref, "models", "include", "helper_math.cuh")) as f:
        header, n = _TOOLKIT_INCLUDE.subn('#include "ref_shim.h"', f.read())
    if n != 1:
        raise RuntimeError(f"expected one CUDA-toolkit include line in helper_math.cuh, found {n}")
    os.makedirs(out, exist_ok=True)
    for name in KERNELS:
        with open(os.path.join(out, name + ".cu.inc"), "w") as f:
            f.write(found[name])
    with open(os.path.join(out, "helper_math.cuh"), "w") as f:
        f.write(header)


def _run(cmd):
    p = subprocess.run(cmd, capture_output=True, text=True)
    if p.returncode != 0:
        raise RuntimeError("oracle/_ref: " + " ".join(cmd) + "\n" + p.stdout + p.stderr)


def compile_all(out=OUT):
    rocm = _rocm()
    hipcc = shutil.which("hipcc") or os.path.join(rocm, "bin", "hipcc")
    inc = ["-I" + out, "-I" + HERE]
    entry = os.path.join(HERE, "ref_host_entry.cpp")
    _run([os.environ.get("CXX", "g++"), "-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-w", *inc, entry,
          "-o", os.path.join(out, HOST_SO), "-lm"])
    for tag, name in CODE_OBJECTS.items():
        extra = ["-ffp-contract=off"] if tag == "nofma" else []
        _run([hipcc, "-x", "hip", "--offload-arch=gfx950", "--genco", "-DREF_DEVICE_ONLY", "-w", *extra, *inc, entry,
              "-o", os.path.join(out, name)])
    lib = os.path.join(rocm, "lib")
    _run([os.environ.get("CC", "gcc"), "-std=c99", "-O1", "-Wall", "-I" + os.path.join(rocm, "include"),
          os.path.join(HERE, "ref_runner.c"), "-o", os.path.join(out, RUNNER), "-L" + lib, "-lamdhip64", "-Wl,-rpath," + lib])


def build(ref=None):
    ref = reference_root(ref)
    if not os.path.isfile(os.path.join(ref, "models", "voting.py")):
        return None
    extract(ref)
    compile_all()
    return OUT


def artefacts(out=OUT):
    """paths of what build() makes, or None when any is missing"""
    names = [HOST_SO, RUNNER, *CODE_OBJECTS.values()]
    paths = {n: os.path.join(out, n) for n in names}
    return paths if all(os.path.isfile(p) for p in paths.values()) else None


if __name__ == "__main__":
    r = build(sys.argv[1] if len(sys.argv) > 1 else None)
    print("built " + r if r else "reference not found: oracle/_ref left as it is")
