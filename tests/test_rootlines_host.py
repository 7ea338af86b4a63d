"""The root cache's line blocks (charon_amd/csrc/rootcache.h), what can be checked without a GPU:
the block format and its check, the recording and the replaying Miller loops against miller_loop_2 word for word, the
statuses of the chain k_verify_fused runs and the plan / publish rules on a serial table, all in a host program
(tests/native/rootlines_host.cpp, also under AddressSanitizer + UBSan); the built library's symbols; and the resources
of the kernels that take the root cache.
"""
import ctypes
import os
import subprocess

from charon_amd import codeobj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "charon_amd", "libhipbls.so")
SRC = os.path.join(ROOT, "tests", "native", "rootlines_host.cpp")
SYMBOLS = ("hipbls_rootcache_lines_config", "hipbls_rootcache_lines_stats")


def _build_and_run(tmp_path, extra, name):
    exe = tmp_path / name
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-o", str(exe), SRC] + extra)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "rootlines_host ok: 12 items" in r.stdout
    return r


def test_record_replay_block_check_and_pool_rules(tmp_path):
    """Record then replay gives miller_loop_2's f and T1 word for word for a dozen seeded items; statuses equal
    pairing_check_verify_sig's for a valid item, a wrong root, a swapped key, a flipped signature bit and a signature
    outside G2, recording, replaying and after a corrupt block's fallback; any word of a block zeroed or flipped, an
    all-zero block and another root's block fail the check; a full pool publishes H alone, an entry's index is written
    once, an index outside the pool is never followed and the counter starts over at a rollover."""
    _build_and_run(tmp_path, [], "rootlines_host")


def test_record_replay_under_asan_ubsan(tmp_path):
    # a stand-alone program with the sanitizers' runtimes linked into it
    r = _build_and_run(tmp_path, ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                  "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan"],
                       "rootlines_host_san")
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr


def _need_lib():
    assert os.path.exists(LIB), "libhipbls.so not built (run __graft_entry__.build())"


def test_lines_symbols_exported_and_abi_version_kept():
    _need_lib()
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for s in SYMBOLS:
        assert s in names, s
    from charon_amd.tbls import HipBLS, exported_symbols
    assert set(SYMBOLS) <= set(exported_symbols())
    assert callable(HipBLS.rootcache_lines_config) and callable(HipBLS.rootcache_lines_stats)
    assert ctypes.CDLL(LIB).hipbls_abi_version() == 12


def test_fused_and_lookup_resources():
    _need_lib()
    rows = {r[0]: r for r in codeobj.resource_table(LIB)}
    lookup = rows["k_root_lookup"]
    # k_verify_fused (lines off) and k_verify_fused_lines (the replaying and the recording loop beside the plain one):
    # 36 KiB of LDS, the one-wave register class and scratch within the budget
    for name in ("k_verify_fused", "k_verify_fused_lines"):
        fused = rows[name]
        print(name, fused)
        assert fused[3] == 36 * 1024, fused
        assert fused[2] > 256, fused
        assert fused[1] <= codeobj.PRIVATE_SEGMENT_BUDGET, fused
    print("k_root_lookup", lookup)
    # k_root_lookup: two waves per SIMD (at most 256 registers), no LDS
    assert lookup[2] <= 256, lookup
    assert lookup[3] == 0, lookup
    assert lookup[1] <= codeobj.PRIVATE_SEGMENT_BUDGET, lookup
