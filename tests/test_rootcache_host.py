"""The root cache (charon_amd/csrc/rootcache.h), what can be checked without a GPU: the entry's
pack/check functions and the probe/insert rules in a host program (tests/native/rootcache_host.cpp, also under
AddressSanitizer + UBSan), the built library's symbols, and the resources of the two kernels that use the cache.
"""
import ctypes
import os
import subprocess

from charon_amd import codeobj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "charon_amd", "libhipbls.so")
SRC = os.path.join(ROOT, "tests", "native", "rootcache_host.cpp")
SYMBOLS = ("hipbls_rootcache_config", "hipbls_rootcache_stats")


def _build_and_run(tmp_path, extra, name):
    exe = tmp_path / name
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-o", str(exe), SRC] + extra)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "rootcache_host ok: 13 roots" in r.stdout
    return r


def test_entry_pack_check_and_table_rules(tmp_path):
    """Pack/get round-trip; any zeroed non-zero word (one, or a seeded sample of subsets) fails the check; a tag off by
    one bit is rejected; an all-zero slot matches no message, the all-zero one included; the serial probe and insert
    publish a root once and, with a full window, nothing."""
    _build_and_run(tmp_path, [], "rootcache_host")


def test_entry_pack_check_under_asan_ubsan(tmp_path):
    # a stand-alone program with the sanitizers' runtimes linked into it
    r = _build_and_run(tmp_path, ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                  "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan"],
                       "rootcache_host_san")
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr


def _need_lib():
    assert os.path.exists(LIB), "libhipbls.so not built (run __graft_entry__.build())"


def test_rootcache_symbols_exported():
    _need_lib()
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for s in SYMBOLS:
        assert s in names, s
    from charon_amd.tbls import HipBLS, exported_symbols
    assert set(SYMBOLS) <= set(exported_symbols())
    assert callable(HipBLS.rootcache_config) and callable(HipBLS.rootcache_stats)
    # adding functions leaves the ABI version where it was
    assert ctypes.CDLL(LIB).hipbls_abi_version() == 12


def test_fused_keeps_its_resources_and_lookup_is_small():
    _need_lib()
    rows = {r[0]: r for r in codeobj.resource_table(LIB)}
    fused, lookup = rows["k_verify_fused"], rows["k_root_lookup"]
    # k_verify_fused: its 36 KiB of LDS, the one-wave register class, scratch within the budget
    assert fused[3] == 36 * 1024, fused
    assert fused[2] > 256, fused
    assert fused[1] <= codeobj.PRIVATE_SEGMENT_BUDGET, fused
    # k_root_lookup: scratch within the budget, no LDS, and two waves per SIMD (at most 256 registers)
    assert lookup[1] <= codeobj.PRIVATE_SEGMENT_BUDGET, lookup
    assert lookup[2] <= 256, lookup
    assert lookup[3] == 0, lookup
