"""The keyed Verify latency route, what can be checked without a GPU: the built library's kernel
table and the two new kernels' resources, the unchanged ABI version, the binding's lone call, and the H(m) cache's
host bookkeeping (charon_amd/csrc/hcache_assign.h) as a stand-alone program under the address and undefined-behaviour
sanitizers.
"""
import ctypes
import os
import subprocess

from charon_amd import codeobj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "charon_amd", "libhipbls.so")
PREP, GATHER = "k_verify_prep8_keys", "k_verify_gather_keys"


def _need_lib():
    assert os.path.exists(LIB), "libhipbls.so not built (run __graft_entry__.build())"


def test_kernel_table_lists_both_new_kernels():
    _need_lib()
    lib = ctypes.CDLL(LIB)
    lib.hipbls_kernel_names.restype = ctypes.c_char_p
    table = lib.hipbls_kernel_names().decode().split()
    assert PREP in table and GATHER in table


def test_new_kernels_resources():
    _need_lib()
    rows = {r[0]: r for r in codeobj.resource_table(LIB)}
    assert PREP in rows and GATHER in rows
    # the octet roles carry curve arithmetic: they spill like the kernel whose roles they take, and no deeper
    assert 0 < rows[PREP][1] <= codeobj.PRIVATE_SEGMENT_BUDGET, rows[PREP]
    assert rows[PREP][1] <= rows["k_verify_prep8"][1], (rows[PREP], rows["k_verify_prep8"])
    # the gather is index arithmetic and copies
    assert rows[GATHER][1] == 0, rows[GATHER]


def test_abi_version_still_12_and_binding_has_the_lone_call():
    _need_lib()
    lib = ctypes.CDLL(LIB)
    assert lib.hipbls_abi_version() == 12
    from charon_amd.tbls import HipBLS
    assert callable(HipBLS.verify_keys)


def test_hcache_assign_host_program_under_sanitizers(tmp_path):
    """Cold and warm calls, the bypass, FIFO wrap with hit demotion at capacity 4 (map and key_of agree after every
    call, no two live keys share a slot) and the error-path erase: tests/native/hcache_assign_main.cpp."""
    exe = tmp_path / "hcache_assign_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "charon_amd", "csrc"), "-o", str(exe),
                           os.path.join(ROOT, "tests", "native", "hcache_assign_main.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.strip() == "ok"
