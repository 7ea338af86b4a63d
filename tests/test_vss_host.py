"""Batched PublicKeyShare / PublicKeyRecover (charon_amd/csrc/vss.h, vss.hip), what can be checked
without a GPU:

  * the lane functions in a host program (tests/native/vss_host.cpp, also a stand-alone executable under
    AddressSanitizer + UBSan): bytes and statuses against the Python oracle over tests/vss_vectors.py;
  * the built library's symbols and Python methods;
  * the new kernels in the runtime kernel table and within the scratch budget.
"""
import ctypes
import os
import re
import subprocess

from charon_amd import codeobj
from tests import vss_vectors as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "charon_amd", "libhipbls.so")
SRC = os.path.join(ROOT, "tests", "native", "vss_host.cpp")
SYMBOLS = ("hipbls_public_key_share_batch", "hipbls_public_key_recover_batch",
           "hipbls_public_key_share_batch_device", "hipbls_public_key_recover_batch_device")
KERNELS = ("k_vss_dealer_sum", "k_vss_eval", "k_vss_scale", "k_vss_sum")


def _build_and_run(tmp_path, extra, name):
    exe = tmp_path / name
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-o", str(exe), SRC] + extra)
    f = tmp_path / "vectors.txt"
    want = V.write_host_file(str(f))
    r = subprocess.run([str(exe), str(f)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"vss_host ok: (\d+) share calls \((\d+) lanes\), (\d+) groups", r.stdout)
    assert m, r.stdout
    assert tuple(map(int, m.groups())) == want, r.stdout
    return r


def test_vectors_cover_the_list():
    calls, gs = V.share_calls(), V.groups()
    assert {(c.threshold, len(c.ids), c.n_dealers) for c in calls} >= {(t, i, d) for t, i in V.SHAPES
                                                                      for d in V.DEALERS}
    ids = {i for c in calls for i in c.ids}
    assert {0, 1, 2, -1, V.INT64_MIN} <= ids and any(i > 1 << 40 for i in ids)
    assert any(len(set(c.ids)) < len(c.ids) for c in calls)  # a repeated id
    assert any(V.INF48 in row for c in calls for row in c.pubs)  # an identity output, status OK
    assert len(V.bad_encodings()) == 5
    for c in calls:  # a bad validator has good neighbours
        for v, st in enumerate(c.status):
            if st != V.OK:
                assert c.status[v - 1] == V.OK and c.status[v + 1] == V.OK, c.name
    assert {len(g.pairs) for g in gs} >= {0, 1, 3, 7, 17}
    assert {g.status for g in gs} == {V.OK, V.ERR_PUBKEY, V.ERR_COMBINE}
    flat = [i for g in gs for i, _ in g.pairs]
    assert {1 << 20, -(1 << 20), (1 << 20) + 1, 0} <= set(flat) and any(i < 0 for i in flat)
    by = {g.name: g for g in gs}
    assert by["bad_and_duplicate"].status == V.ERR_COMBINE and by["identity_share"].status == V.OK


def test_lane_functions_match_the_oracle(tmp_path):
    r = _build_and_run(tmp_path, [], "vss_host")
    m = re.search(r"decode (\d+) per commitment, dealer sum (\d+) per coefficient .*evaluation (\d+) per lane .*"
                  r"recovered share (\d+) small path / (\d+) field path", r.stdout)
    assert m, r.stdout
    decode, dsum, ev, small, field = map(int, m.groups())
    # the decode (a square root and the subgroup test) is the expensive part; a Horner lane over ids 0..10 is not;
    # the small-integer path saves most of the 255-bit multiplication
    assert decode > 1000 and ev < decode and dsum < decode and decode < small < field, r.stdout


def test_host_program_under_asan_ubsan(tmp_path):
    # a stand-alone program with the sanitizers' runtimes linked into it
    r = _build_and_run(tmp_path, ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                  "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan"], "vss_host_san")
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr


def _need_lib():
    assert os.path.exists(LIB), "libhipbls.so not built (run __graft_entry__.build())"


def test_symbols_exported():
    _need_lib()
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for s in SYMBOLS:
        assert s in names, s
    from charon_amd.tbls import HipBLS, exported_symbols
    assert set(SYMBOLS) <= set(exported_symbols())
    for m in ("public_key_share_batch", "public_key_recover_batch", "verify_secret_shares", "verify_pubshares"):
        assert callable(getattr(HipBLS, m)), m
    assert ctypes.CDLL(LIB).hipbls_abi_version() == 12  # functions were only added


def test_kernels_registered_and_within_budget():
    _need_lib()
    rows = {r[0]: r for r in codeobj.resource_table(LIB)}
    for k in KERNELS:
        assert k in rows, k
        assert rows[k][1] <= codeobj.PRIVATE_SEGMENT_BUDGET, rows[k]
        assert rows[k][3] == 0, rows[k]  # no LDS
    lib = ctypes.CDLL(LIB)
    lib.hipbls_kernel_names.restype = ctypes.c_char_p
    table = lib.hipbls_kernel_names().decode().split()
    for k in KERNELS + ("k_g1_decode",):
        assert k in table, k
