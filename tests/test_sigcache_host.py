"""The signature cache (charon_amd/csrc/sigcache.h), what can be checked without a GPU: the entry's
pack/check functions, the probe/insert rules, the generation threshold and sigagg's scaling lane on its hit path
against its miss path in a host program (tests/native/sigcache_host.cpp, also under AddressSanitizer + UBSan) on
partials signed by the oracle; the built library's symbols; and the kernels' resources -- the new ones within the
scratch budget, the ones the cache's routes replace exactly as they were before the cache.
"""
import ctypes
import os
import subprocess

import pytest

from charon_amd import codeobj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "charon_amd", "libhipbls.so")
SRC = os.path.join(ROOT, "tests", "native", "sigcache_host.cpp")
SYMBOLS = ("hipbls_sigcache_config", "hipbls_sigcache_stats")
NEW_KERNELS = ("k_sigcache_insert", "k_verify_prep_keys_sc", "k_rlc_items_sc", "k_rlcb_items_sc", "k_tagg_scale_sc",
               "k_tv_phase_a_sc", "k_tv_phase_a_keys_sc")
# (scratch B/lane, VGPRs incl. AGPRs, LDS B) of the kernels whose routes gained a cache-taking twin, recorded from a
# build of the commit before the signature cache: with the cache off a call runs these very kernels.
PARENT_ROWS = {
    "k_tagg_scale": (7016, 308, 0),
    "k_tv_phase_a": (7016, 309, 0),
    "k_tv_phase_a_keys": (7016, 310, 0),
    "k_verify_prep": (7128, 306, 0),
    "k_verify_pair_lg2": (10984, 510, 0),
    "k_verify_pair_lq4": (10072, 512, 0),
    "k_rlc_items": (5048, 256, 0),
    "k_rlcb_items": (3816, 256, 0),
}
# (threshold ids, message): 4-of-6 and 7-of-10 over ids 1..n, where some c_k are negative, and one group whose ids
# leave the small-integer path
GROUPS = (
    ((1, 3, 4, 6), b"sigcache host 4-of-6"),
    ((1, 2, 4, 5, 7, 9, 10), b"sigcache host 7-of-10"),
    ((2, 3, 5, 6), b"sigcache host 4-of-6 b"),
    (tuple(2 ** 40 + k for k in (1, 2, 4, 7)), b"sigcache host field path"),
)


@pytest.fixture(scope="module")
def groups_file(tmp_path_factory):
    from oracle import bls12381 as bls
    lines = []
    for g, (ids, msg) in enumerate(GROUPS):
        poly = [(0x5157CAC4E + 104729 * g) % bls.R] + [(0xA11CE + 7919 * (g + 1) * (j + 1)) % bls.R
                                                       for j in range(len(ids) - 1)]
        parts = {}
        for i in ids:
            acc = 0
            for c in reversed(poly):
                acc = (acc * i + c) % bls.R
            parts[i] = bls.sign(bls.sk_serialize(acc), msg)
        agg = bls.threshold_aggregate(parts)
        # the aggregate is the group secret's signature: the oracle's Lagrange sum and its Sign agree
        assert agg == bls.sign(bls.sk_serialize(poly[0]), msg)
        lines.append("G %d" % len(ids))
        lines += ["P %d %s" % (i, parts[i].hex()) for i in ids]
        lines.append("A " + agg.hex())
    path = tmp_path_factory.mktemp("sigcache") / "groups.txt"
    path.write_text("\n".join(lines) + "\n")
    return str(path)


def _build_and_run(tmp_path, groups_file, extra, name):
    exe = tmp_path / name
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-o", str(exe), SRC] + extra)
    r = subprocess.run([str(exe), groups_file], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "sigcache_host ok: %d groups, %d partials" % (len(GROUPS), sum(len(g[0]) for g in GROUPS)) in r.stdout
    return r


def test_entry_table_and_hit_path_against_miss_path(tmp_path, groups_file):
    r = _build_and_run(tmp_path, groups_file, [], "sigcache_host")
    ops = {}
    for ln in r.stdout.splitlines():
        if ln.startswith("ops "):
            w = ln.split()
            ops[(w[1], w[2].rstrip(":"))] = float(w[3]) + float(w[5])
    print(r.stdout)
    # a hit skips the square root and the subgroup test: less field work on both paths
    assert ops[("small", "hit")] < ops[("small", "miss")]
    assert ops[("field", "hit")] < ops[("field", "miss")]


def test_host_program_under_asan_ubsan(tmp_path, groups_file):
    # a stand-alone program with the sanitizers' runtimes linked into it
    r = _build_and_run(tmp_path, groups_file, ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                               "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan"],
                       "sigcache_host_san")
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr


def _need_lib():
    assert os.path.exists(LIB), "libhipbls.so not built (run __graft_entry__.build())"


def test_sigcache_symbols_exported():
    _need_lib()
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for s in SYMBOLS:
        assert s in names, s
    from charon_amd.tbls import HipBLS, exported_symbols
    assert set(SYMBOLS) <= set(exported_symbols())
    assert callable(HipBLS.sigcache_config) and callable(HipBLS.sigcache_stats)
    # adding functions leaves the ABI version where it was
    assert ctypes.CDLL(LIB).hipbls_abi_version() == 12


def test_new_kernels_within_scratch_budget():
    _need_lib()
    rows = {r[0]: r for r in codeobj.resource_table(LIB)}
    for k in NEW_KERNELS:
        assert k in rows, k
        assert rows[k][1] <= codeobj.PRIVATE_SEGMENT_BUDGET, rows[k]
    # the RLC item stages' twins stay at two waves per SIMD, as the stages themselves
    for k in ("k_rlc_items_sc", "k_rlcb_items_sc"):
        assert rows[k][2] <= 256, rows[k]
    # the producer behind prep + pair is a small kernel: no square root, no pairing
    assert rows["k_sigcache_insert"][1] <= 1024, rows["k_sigcache_insert"]


def test_replaced_kernels_keep_the_parents_rows():
    _need_lib()
    rows = {r[0]: r for r in codeobj.resource_table(LIB)}
    for k, want in PARENT_ROWS.items():
        assert rows[k][1:] == want, (k, rows[k], want)
