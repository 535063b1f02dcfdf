"""Builds the host-sanitizer programs (san_ingest, san_index, san_input) into a directory outside the tree.

TEST INFRASTRUCTURE ONLY.  The host layer of the product (ks_ingest.cpp, ks_host.cpp, ks_input.cpp, ks_hostfn.cpp) is
compiled host-only against the HIP headers and linked with the CPU stand-in of this directory (hip_stub.cpp, ks_stub.cpp)
and the oracle — no libamdhip64, no GPU.  By hand:

    python tests/hostsan/build.py /tmp/hostsan            # both sanitizer sets -> /tmp/hostsan/{asan,tsan}/san_*
    TSAN_OPTIONS=halt_on_error=1 /tmp/hostsan/tsan/san_ingest sketch tests/golden/ced9.fasta 16 5 hp 0 100 1 /tmp/out.bin 8 200
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CSRC = os.path.join(ROOT, "kmerseek_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")

SANITIZERS = {
    "asan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"],
    "tsan": ["-fsanitize=thread"],
}
# gcc links the sanitizer runtimes dynamically unless told otherwise; linked statically (clang's default) a program does not
# depend on where the runtime comes in the list of loaded libraries
STATIC_RUNTIME = {"asan": ["-static-libasan", "-static-libubsan"], "tsan": ["-static-libtsan"]}
PRODUCT = ["ks_ingest.cpp", "ks_host.cpp", "ks_input.cpp", "ks_hostfn.cpp"]  # the code under test, as it stands
STUBS = ["hip_stub.cpp", "ks_stub.cpp"]
PROGRAMS = ["san_ingest", "san_index", "san_input"]
MAX_JOBS = 16


def compilers():
    """(C++ compiler, C compiler): $CXX / $CC, else g++ / gcc, else ROCm's clang."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or os.path.join(ROCM, "lib", "llvm", "bin", "clang++")
    cc = os.environ.get("CC") or shutil.which("gcc") or os.path.join(ROCM, "lib", "llvm", "bin", "clang")
    return cxx, cc


def build(out_dir: str, which=("asan", "tsan"), verbose: bool = False) -> dict:
    """Returns {sanitizer: {program: path}}.  Objects and programs go to out_dir/<sanitizer>/ only."""
    cxx, cc = compilers()
    common = ["-O1", "-g", "-fno-omit-frame-pointer", "-pthread"]
    cxxflags = common + ["-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include")]
    jobs, links, result = [], [], {}
    for san in which:
        d = os.path.join(out_dir, san)
        os.makedirs(d, exist_ok=True)
        flags = SANITIZERS[san]
        objs = []
        for src in [os.path.join(CSRC, f) for f in PRODUCT] + [os.path.join(HERE, f) for f in STUBS]:
            o = os.path.join(d, os.path.basename(src) + ".o")
            jobs.append([cxx] + cxxflags + flags + ["-c", src, "-o", o])
            objs.append(o)
        o = os.path.join(d, "ks_oracle.c.o")
        jobs.append([cc] + common + ["-std=c11"] + flags + ["-c", os.path.join(ROOT, "oracle", "ks_oracle.c"), "-o", o])
        objs.append(o)
        result[san] = {}
        for prog in PROGRAMS:
            po = os.path.join(d, prog + ".cpp.o")
            jobs.append([cxx] + cxxflags + flags + ["-c", os.path.join(HERE, prog + ".cpp"), "-o", po])
            exe = os.path.join(d, prog)
            static = [] if "clang" in os.path.basename(cxx) else STATIC_RUNTIME[san]
            links.append([cxx] + common + flags + static + ["-o", exe, po] + objs + ["-lz", "-ldl"])
            result[san][prog] = exe

    def run(cmd):
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if p.returncode != 0:
            raise RuntimeError("command failed: " + " ".join(cmd) + "\n" + p.stdout)

    with ThreadPoolExecutor(max_workers=MAX_JOBS) as ex:
        list(ex.map(run, jobs))
        list(ex.map(run, links))
    return result


def build_alone(out_dir: str, prog: str, san: str = "asan") -> str:
    """A program of this directory that needs neither the product's objects nor the stand-in (san_slices: a header's host
    half), with the same compiler, flags and runtime linkage as the others.  Returns its path, out_dir/<sanitizer>/<prog>."""
    cxx, _ = compilers()
    d = os.path.join(out_dir, san)
    os.makedirs(d, exist_ok=True)
    exe = os.path.join(d, prog)
    static = [] if "clang" in os.path.basename(cxx) else STATIC_RUNTIME[san]
    cmd = [cxx, "-O1", "-g", "-fno-omit-frame-pointer", "-std=c++17"] + SANITIZERS[san] + static + ["-o", exe, os.path.join(HERE, prog + ".cpp")]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0:
        raise RuntimeError("command failed: " + " ".join(cmd) + "\n" + p.stdout)
    return exe


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit("usage: build.py OUT_DIR [asan|tsan ...]")
    for san, progs in build(sys.argv[1], tuple(sys.argv[2:]) or ("asan", "tsan"), verbose=True).items():
        for exe in progs.values():
            print(san, exe)
