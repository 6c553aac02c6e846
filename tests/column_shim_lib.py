"""Building and loading the host shims of the column calls (tests/*_shim.cpp) — TEST INFRASTRUCTURE.  A shim is rebuilt when it is
older than its sources: the .cpp file, tests/column_shim.hpp and the headers whose per-thread bodies it runs.  load() gives the
shared library for ctypes; sanitized() builds the same file with its own main under -fsanitize=address,undefined and runs it: a
process of its own, on the CPU — a sanitized build is never loaded into an interpreter."""
import ctypes
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "trre_amd", "csrc")
OUT = os.path.join(HERE, "_shim")


def _build(target, name, flags):
    src = os.path.join(HERE, name + "_shim.cpp")
    deps = [src, os.path.join(HERE, "column_shim.hpp"), os.path.join(CSRC, "records_block.hpp"), os.path.join(CSRC, "scan_block.hpp")]
    if not (os.path.exists(target) and all(os.path.getmtime(target) >= os.path.getmtime(d) for d in deps)):
        os.makedirs(OUT, exist_ok=True)
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas"] + flags + [src, "-o", target], check=True)
    return target


def load(name):
    """tests/<name>_shim.cpp as a shared library"""
    return ctypes.CDLL(_build(os.path.join(OUT, "lib%s_shim.so" % name), name, ["-O2", "-fPIC", "-shared"]))


def sanitized(name):
    """tests/<name>_shim.cpp with its own main (-D<NAME>_SHIM_MAIN), run under the sanitizers: the finished process"""
    exe = _build(os.path.join(OUT, name + "_shim_san"), name,
                 ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-D%s_SHIM_MAIN" % name.upper()])
    return subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
