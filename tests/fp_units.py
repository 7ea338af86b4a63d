"""Build and load the Fp unit libraries of tests/test_gpu_fp_sqr.py (test-only, beside tests/hostlib.py):

* tests/native/libfp_units.so       gfx950: fp_sqr, fp_sqr_n, fp_mul(a, a) and fp_pow on raw limbs, one lane each
* tests/native/libfp_units_host.so  g++: the host build of fp_pow on the same limbs
"""
import ctypes
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "charon_amd", "csrc")
GPU_SRC = os.path.join(HERE, "native", "fp_units.hip")
GPU_LIB = os.path.join(HERE, "native", "libfp_units.so")
HOST_SRC = os.path.join(HERE, "native", "fp_units_host.cpp")
HOST_LIB = os.path.join(HERE, "native", "libfp_units_host.so")


def _stale(lib, src):
    deps = [src] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    return not os.path.exists(lib) or any(os.path.getmtime(d) > os.path.getmtime(lib) for d in deps)


def build():
    """Called from __graft_entry__.build(); the GPU tests only load what it left."""
    if _stale(GPU_LIB, GPU_SRC):
        subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-I" + CSRC,
                               "-o", GPU_LIB + ".tmp", GPU_SRC])
        os.replace(GPU_LIB + ".tmp", GPU_LIB)
    if _stale(HOST_LIB, HOST_SRC):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-o", HOST_LIB + ".tmp", HOST_SRC])
        os.replace(HOST_LIB + ".tmp", HOST_LIB)


def _load(path):
    if not os.path.exists(path):
        raise RuntimeError("%s not built (run __graft_entry__.build())" % os.path.relpath(path, os.path.dirname(HERE)))
    return ctypes.CDLL(path)


def gpu_lib():
    return _load(GPU_LIB)


def host_lib():
    return _load(HOST_LIB)
