"""sigagg by resident key index (hipbls_threshold_aggregate_verify_batch_keys), what can be checked
without a GPU: the built library's symbols and kernels, a host build of the key role's lane body against the
wire-format lane, and the Go binding's text.
"""
import ctypes
import os
import re
import subprocess

import pytest

from charon_amd import codeobj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "charon_amd", "libhipbls.so")
R_ORDER = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
ERR_PUBKEY, ERR_VERIFY, ERR_ARG, PENDING = 1, 3, 16, -1

SYMBOLS = ("hipbls_threshold_aggregate_verify_batch_keys", "hipbls_threshold_aggregate_verify_batch_keys_device")
HEAVY = ("k_tv_phase_a_keys", "k_tv_prep8_keys")  # the roles with curve arithmetic: they spill, like their parents
COPY = ("k_tv_join_keys", "k_tv_gather_keys")     # the gathers: index arithmetic and copies only


def _need_lib():
    assert os.path.exists(LIB), "libhipbls.so not built (run __graft_entry__.build())"


# ------------------------------------------------------------------------------------------------ library
def test_both_symbols_exported_and_abi_still_12():
    _need_lib()
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for s in SYMBOLS:
        assert s in names, s
    lib = ctypes.CDLL(LIB)
    assert lib.hipbls_abi_version() == 12
    from charon_amd.tbls import HipBLS, exported_symbols
    assert set(SYMBOLS) <= set(exported_symbols())
    assert callable(HipBLS.batch_threshold_aggregate_verify_keys)


def test_new_kernels_in_the_kernel_table_and_within_the_scratch_budget():
    _need_lib()
    lib = ctypes.CDLL(LIB)
    lib.hipbls_kernel_names.restype = ctypes.c_char_p
    table = lib.hipbls_kernel_names().decode().split()
    rows = {r[0]: r for r in codeobj.resource_table(LIB)}
    for k in HEAVY + COPY:
        assert k in table, k
        assert k in rows, k
        assert rows[k][1] <= codeobj.PRIVATE_SEGMENT_BUDGET, rows[k]
    for k in HEAVY:
        assert rows[k][1] > 0, rows[k]
    # no deeper than the kernels whose roles they take over
    assert rows["k_tv_phase_a_keys"][1] <= rows["k_tv_phase_a"][1]
    assert rows["k_tv_prep8_keys"][1] <= rows["k_tv_prep8"][1]


# ------------------------------------------------------------------------------------------------ host lane body
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = tmp_path_factory.mktemp("sigagg_keys") / "libsigagg_keys_host.so"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-o", str(so),
                           os.path.join(ROOT, "tests", "native", "sigagg_keys_host.cpp")])
    return ctypes.CDLL(str(so))


def _keys():
    """(name, 48 key bytes, table load status, lane status)."""
    import json
    from oracle import bls12381 as bls
    with open(os.path.join(ROOT, "tests", "golden", "fixtures.json")) as f:
        small_pk = bytes.fromhex(json.load(f)["small_order"]["verify"][16]["pk"])
    valid = bls.secret_to_public_key((0x1234567 % R_ORDER).to_bytes(32, "big"))
    # an x with no point on the curve: count up from the valid key's x until decompression fails on the curve test
    off_curve = None
    x = int.from_bytes(bytes([valid[0] & 0x1F]) + valid[1:], "big")
    for d in range(1, 64):
        cand = (x + d).to_bytes(48, "big")
        cand = bytes([cand[0] | 0x80]) + cand[1:]
        try:
            bls.g1_decompress(cand)
        except bls.BLSError:
            off_curve = cand
            break
    assert off_curve is not None
    return [("valid", valid, 0, PENDING), ("infinity", b"\xc0" + bytes(47), 0, ERR_VERIFY),
            ("off_curve", off_curve, ERR_PUBKEY, ERR_PUBKEY), ("off_subgroup", small_pk, ERR_PUBKEY, ERR_PUBKEY)]


ID_SETS = [[1, 2], [2, 5, 9, 10], [1, -5, 3], [1, 2 ** 32, 7], [3, 2 ** 40 + 1]]


def test_keyed_lane_equals_wire_lane(host):
    keys = _keys()
    tab = b"".join(k[1] for k in keys)
    T = len(keys)
    for k, (name, pk, want_load, want_st) in enumerate(keys):
        for ids in ID_SETS:
            arr = (ctypes.c_int64 * len(ids))(*ids)
            out_k, out_w = (ctypes.c_uint32 * 24)(), (ctypes.c_uint32 * 24)()
            load = (ctypes.c_int32 * T)()
            st_k = host.sk_keyed_lane(tab, ctypes.c_uint64(T), ctypes.c_uint64(k), arr, len(ids), out_k, load)
            st_w = host.sk_wire_lane(pk, arr, len(ids), out_w)
            assert list(load) == [x[2] for x in keys]
            assert st_k == st_w == want_st, (name, ids)
            assert list(out_k) == list(out_w), (name, ids)
            if want_st == PENDING:
                assert any(out_k), (name, ids)
    # an index outside the table
    arr = (ctypes.c_int64 * 2)(1, 2)
    out_k, load = (ctypes.c_uint32 * 24)(), (ctypes.c_int32 * T)()
    assert host.sk_keyed_lane(tab, ctypes.c_uint64(T), ctypes.c_uint64(T), arr, 2, out_k, load) == ERR_ARG
    assert host.sk_keyed_lane(b"", ctypes.c_uint64(0), ctypes.c_uint64(0), arr, 2, out_k, load) == ERR_ARG


def test_keyed_lane_scales_by_the_groups_L(host):
    """[L] pk for ids {1, 2}: L = lcm-style denominator of the Lagrange coefficients; whatever tagg_group_L gives, the
    point must be on the curve's affine form of a multiple of pk, i.e. differ from pk unless L == 1, and two id sets
    with different L give different points."""
    name, pk, _, _ = _keys()[0]
    outs = []
    for ids in ([1, 2], [2, 5, 9, 10]):
        arr = (ctypes.c_int64 * len(ids))(*ids)
        out, load = (ctypes.c_uint32 * 24)(), (ctypes.c_int32 * 1)()
        assert host.sk_keyed_lane(pk, ctypes.c_uint64(1), ctypes.c_uint64(0), arr, len(ids), out, load) == PENDING
        outs.append(list(out))
    assert outs[0] != outs[1]


# ------------------------------------------------------------------------------------------------ Go text
def _read(*rel):
    with open(os.path.join(ROOT, *rel)) as f:
        return f.read()


def test_go_binding_takes_the_keyed_call_under_the_table_lock():
    src = _read("integration", "charon", "tbls", "hipbls", "batch.go")
    fn = src[src.index("func (HipBLS) BatchThresholdAggregateVerify("):]
    fn = fn[:fn.index("\n}\n")]
    assert "C.hipbls_threshold_aggregate_verify_batch_keys(" in fn
    assert "C.hipbls_threshold_aggregate_verify_batch(" in fn  # the wire-format call stays for keys outside the table
    assert "lockTable(dvPks)" in fn
    assert fn.index("lockTable(dvPks)") < fn.index("C.hipbls_threshold_aggregate_verify_batch_keys(") < \
        fn.index("release()")
    assert '"batch_threshold_aggregate_verify_keys"' in fn
    assert "distinctRoots(msgs)" in fn and "func distinctRoots(" in src


def test_go_app_configures_the_cache_and_loads_root_keys():
    app = _read("integration", "charon", "app", "gpubls_hipbls.go")
    assert "hipbls.ConfigHCache(hipbls.DefaultHCacheCapacity)" in app
    pkg = _read("integration", "charon", "tbls", "hipbls", "hipbls.go")
    assert "C.hipbls_hcache_config(" in pkg
    assert re.search(r"const DefaultHCacheCapacity = 65536\b", pkg)
    patch = _read("integration", "patches", "0004-app-gpu-bls-feature.patch")
    added = "\n".join(ln[1:] for ln in patch.splitlines() if ln.startswith("+") and not ln.startswith("+++"))
    loop = added[added.index("var pubShareTable"):added.index("tbls.LoadPubShares(pubShareTable)")]
    assert re.search(r"for _, k := range eth2Pubkeys \{\s*pubShareTable = append\(pubShareTable, tbls\.PublicKey\(k\)\)",
                     loop)
    # the package patch carries the same files as the integration tree
    p2 = _read("integration", "patches", "0002-tbls-hipbls-package.patch")
    assert "hipbls_threshold_aggregate_verify_batch_keys(" in p2 and "func ConfigHCache(" in p2
