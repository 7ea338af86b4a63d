"""The key cache (charon_amd/csrc/keycache.h), what can be checked without a GPU: the entry's
pack/check functions and the probe/insert rules in a host program (tests/native/keycache_host.cpp, also under
AddressSanitizer + UBSan), the built library's symbols, and the resources of the four kernels that use the cache.
"""
import ctypes
import os
import subprocess

import pytest

from charon_amd import codeobj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "charon_amd", "libhipbls.so")
SRC = os.path.join(ROOT, "tests", "native", "keycache_host.cpp")
R_ORDER = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
SYMBOLS = ("hipbls_keycache_config", "hipbls_keycache_stats")
KERNELS = ("k_verify_fused", "k_verify_prep", "k_rlc_items", "k_rlcb_items")


def _keys(n=12):
    from oracle import bls12381 as bls
    return [bls.secret_to_public_key(((0xC0FFEE + 7919 * i) % R_ORDER).to_bytes(32, "big")).hex() for i in range(n)]


def _build_and_run(tmp_path, extra, name):
    exe = tmp_path / name
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-o", str(exe), SRC] + extra)
    r = subprocess.run([str(exe)] + _keys(), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "keycache_host ok: 12 keys" in r.stdout
    return r


def test_entry_pack_check_and_table_rules(tmp_path):
    _build_and_run(tmp_path, [], "keycache_host")


def test_entry_pack_check_under_asan_ubsan(tmp_path):
    # a stand-alone program with the sanitizers' runtimes linked into it
    r = _build_and_run(tmp_path, ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                  "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan"],
                       "keycache_host_san")
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr


def _need_lib():
    assert os.path.exists(LIB), "libhipbls.so not built (run __graft_entry__.build())"


def test_keycache_symbols_exported():
    _need_lib()
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for s in SYMBOLS:
        assert s in names, s
    from charon_amd.tbls import HipBLS, exported_symbols
    assert set(SYMBOLS) <= set(exported_symbols())
    assert callable(HipBLS.keycache_config) and callable(HipBLS.keycache_stats)
    # adding functions leaves the ABI version where it was
    assert ctypes.CDLL(LIB).hipbls_abi_version() == 12


def test_cache_kernels_within_scratch_budget_and_fused_keeps_four_workgroups_per_cu():
    _need_lib()
    rows = {r[0]: r for r in codeobj.resource_table(LIB)}
    for k in KERNELS:
        assert k in rows, k
        assert rows[k][1] <= codeobj.PRIVATE_SEGMENT_BUDGET, rows[k]
    # k_verify_fused: one wave per SIMD (more than 256 registers) and four one-wave workgroups' LDS in a CU's 160 KiB
    assert 4 * rows["k_verify_fused"][3] <= 160 * 1024, rows["k_verify_fused"]
    assert rows["k_verify_fused"][3] == 36 * 1024, rows["k_verify_fused"]
    assert rows["k_verify_fused"][2] > 256, rows["k_verify_fused"]
    # the RLC item stages stay at two waves per SIMD
    for k in ("k_rlc_items", "k_rlcb_items"):
        assert rows[k][2] <= 256, rows[k]
