"""The H(m) prefetch (hipbls_hcache_prefetch), what can be checked without a GPU: the fill kernel in
the built library's kernel table and its resources, the unchanged ABI version, the binding's call, the argument checks
that return before the device is initialised, and the prefetch's host bookkeeping (charon_amd/csrc/hcache_assign.h) as
a stand-alone program under the address and undefined-behaviour sanitizers.
"""
import ctypes
import os
import subprocess

from charon_amd import codeobj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "charon_amd", "libhipbls.so")
FILL, PREP = "k_hcache_fill8", "k_verify_prep8_keys"
OK, ERR_ARG = 0, 16


def _lib():
    assert os.path.exists(LIB), "libhipbls.so not built (run __graft_entry__.build())"
    lib = ctypes.CDLL(LIB)
    lib.hipbls_kernel_names.restype = ctypes.c_char_p
    u64p = ctypes.POINTER(ctypes.c_uint64)
    lib.hipbls_hcache_prefetch.argtypes = [ctypes.c_char_p, u64p, ctypes.c_uint64, u64p, u64p]
    lib.hipbls_hcache_prefetch.restype = ctypes.c_int
    return lib


def test_kernel_table_lists_the_fill_kernel():
    assert FILL in _lib().hipbls_kernel_names().decode().split()


def test_fill_kernel_resources():
    _lib()
    rows = {r[0]: r for r in codeobj.resource_table(LIB)}
    assert FILL in rows and PREP in rows
    # the hash role of the keyed prep alone: it spills like that kernel, and no deeper
    assert 0 < rows[FILL][1] <= rows[PREP][1], (rows[FILL], rows[PREP])
    assert rows[FILL][1] <= codeobj.PRIVATE_SEGMENT_BUDGET, rows[FILL]


def test_abi_version_still_12_and_binding_has_the_call():
    assert _lib().hipbls_abi_version() == 12
    from charon_amd.tbls import HipBLS, exported_symbols
    assert callable(HipBLS.hcache_prefetch)
    assert "hipbls_hcache_prefetch" in exported_symbols()


def test_argument_checks_return_before_device_init():
    """None of these reaches ENSURE_INIT (there is no device here): an empty call is OK with zeroed outputs, null or
    decreasing offsets and null messages with a non-zero total are HIPBLS_ERR_ARG."""
    lib = _lib()
    h, p = ctypes.c_uint64(7), ctypes.c_uint64(9)
    assert lib.hipbls_hcache_prefetch(None, None, 0, ctypes.byref(h), ctypes.byref(p)) == OK
    assert (h.value, p.value) == (0, 0)
    assert lib.hipbls_hcache_prefetch(None, None, 0, None, None) == OK  # both outputs may be null
    h.value, p.value = 7, 9
    assert lib.hipbls_hcache_prefetch(b"abc", None, 3, ctypes.byref(h), ctypes.byref(p)) == ERR_ARG
    assert (h.value, p.value) == (0, 0)
    down = (ctypes.c_uint64 * 4)(0, 2, 1, 3)
    assert lib.hipbls_hcache_prefetch(b"abc", down, 3, ctypes.byref(h), ctypes.byref(p)) == ERR_ARG
    nonzero_start = (ctypes.c_uint64 * 2)(1, 3)
    assert lib.hipbls_hcache_prefetch(b"abc", nonzero_start, 1, None, None) == ERR_ARG
    up = (ctypes.c_uint64 * 3)(0, 1, 3)
    assert lib.hipbls_hcache_prefetch(None, up, 2, None, None) == ERR_ARG  # null messages, three bytes of them


def test_hcache_prefetch_host_program_under_sanitizers(tmp_path):
    """The non-counting assign leaves hits / misses alone, present / hashed with duplicates folded, wrap and hit
    demotion at capacity 4 (map, key_of and live agree after every call), the bypass, and the erase after a failed
    prefetch: tests/native/hcache_prefetch_main.cpp."""
    exe = tmp_path / "hcache_prefetch_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "charon_amd", "csrc"), "-o", str(exe),
                           os.path.join(ROOT, "tests", "native", "hcache_prefetch_main.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.strip() == "ok"
