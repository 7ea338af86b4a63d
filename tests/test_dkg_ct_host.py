"""A joint-Feldman dealing round in batches (charon_amd/csrc/dkg_ct.h, dkg_ct.hip), what can be checked
without a GPU:

  * the vectors themselves (tests/dkg_vectors.py): they cover the list, the oracle compresses the identity to 0xc0 then
    47 zero bytes, and the identities a joint dealing rests on hold on the oracle alone;
  * the lane functions in a host program (tests/native/dkg_ct_host.cpp, also under AddressSanitizer + UBSan): bytes and
    statuses against the Python oracle and op_sk_to_pk, and ONE operation trace (field.h BLS_CT_TRACE) for every
    secret at a fixed public shape, for each of the three lane functions;
  * the built library's symbols and Python methods, the ABI still 12;
  * the gfx950 code of k_commit_ct, k_share_check_ct and k_share_sum_ct: no branch on a vector condition at all, no
    flat load, no private-memory load addressed from a vector register, the comb table read by scalar loads only (a
    whole row through one base register), every global vector load enumerated, resources within budget;
  * the resource rows of every kernel the library had before, against the table recorded from the parent
    (tests/golden/kernel_resources_r21.json).
"""
import ctypes
import json
import os
import re
import subprocess

from charon_amd import codeobj
from oracle import bls12381 as O
from tests import dkg_vectors as V
from tests import vss_vectors as VS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "charon_amd", "libhipbls.so")
SRC = os.path.join(ROOT, "tests", "native", "dkg_ct_host.cpp")
PARENT_TABLE = os.path.join(ROOT, "tests", "golden", "kernel_resources_r21.json")
SYMBOLS = ("hipbls_deal_commit_batch_ct", "hipbls_verify_secret_shares_batch_ct", "hipbls_combine_shares_batch_ct",
           "hipbls_deal_commit_batch_ct_device", "hipbls_verify_secret_shares_batch_ct_device",
           "hipbls_combine_shares_batch_ct_device")
KERNELS = ("k_commit_ct", "k_share_check_ct", "k_share_sum_ct")

# Every global (vector) load of each kernel, by mnemonic and count, with the public address it reads.  The comb table
# is NOT among them: it is read by scalar loads (s_load_dword*), whose address is the wave's.
GLOBAL_LOADS = {
    "k_commit_ct": {
        # tails + 32 ((threshold-1) v + j'-1) in the validity scan, secrets + 32 v after it, and the lane's own
        # coefficient (secrets + 32 v or tails + 32 ((threshold-1) v + j-1), selected on j): two 16-byte halves each
        "global_load_dwordx4": 6,
    },
    "k_share_check_ct": {
        # shares + 32 l: two 16-byte halves; expected + 48 l: 16 + 16 + 12 + 4 bytes; decode_status + 4 l: one word
        "global_load_dwordx4": 4,
        "global_load_dwordx3": 1,
        "global_load_dword": 2,
    },
    "k_share_sum_ct": {
        "global_load_ubyte": 1,    # include + (v n_dealers + d) stride, in the loop over the dealers
        "global_load_dwordx4": 2,  # shares + 32 (v n_dealers + d) in the same loop: two 16-byte halves
    },
}
COMB_ROW_WORDS = 15 * 24


def test_vectors_cover_the_list():
    ds, cs, us = V.dealings(), V.checks(), V.combines()
    assert [(d.threshold, d.total) for d in ds] == list(V.SHAPES)
    for d in ds:
        assert {p[0] for p in d.polys} >= set(V.COEFFS)  # 0, 1, r-1, r, 2^256-1 as the secret
        if d.threshold > 1:
            assert {p[-1] for p in d.polys} >= set(V.COEFFS)  # and as the top coefficient: a zero one among them
        bad = [v for v, s in enumerate(d.status) if s != V.OK]
        assert any(0 < v < d.n_val - 1 and d.status[v - 1] == V.OK == d.status[v + 1] for v in bad)
        for v in range(d.n_val):
            assert (d.com_status[v] == [V.OK] * d.threshold) == (d.status[v] == V.OK)
    assert {c.my_id for c in cs} >= {1, 10, -1, V.INT64_MIN, 0}
    flat = [(int.from_bytes(c.shares[v][d], "big"), c.status[v][d]) for c in cs for v in range(c.n_val)
            for d in range(c.n_dealers)]
    assert (0, V.OK) in flat and (0, V.ERR_VERIFY) in flat and (V.R, V.ERR_SECRET) in flat
    assert (2**256 - 1, V.ERR_SECRET) in flat and (V.R, V.ERR_PUBKEY) in flat
    assert {s for _, s in flat} == {V.OK, V.ERR_PUBKEY, V.ERR_SECRET, V.ERR_VERIFY}
    bad_enc = set(VS.bad_encodings().values())
    assert {x for c in cs for val in c.commitments for poly in val for x in poly} >= bad_enc
    masks = [tuple(bool(f) for f in row) for c in us if c.include is not None for row in c.include]
    assert any(all(m) for m in masks) and any(not any(m) for m in masks) and any(sum(m) == 1 for m in masks)
    assert any(c.include is None for c in us)
    assert {s for c in us for s in c.status} == {V.OK, V.ERR_SECRET, V.ERR_COMBINE}
    # a mask that excludes the dealer whose share is >= r gives OK; a sum that is 0 mod r is OK without a pubshare
    assert any(c.include is not None and c.status[v] == V.OK and
               any(int.from_bytes(s, "big") >= V.R and not f for s, f in zip(c.shares[v], c.include[v]))
               for c in us for v in range(c.n_val))
    assert any(c.status[v] == V.OK and c.out[v] == V.ZERO32 and c.pub_status[v] == V.ERR_SECRET
               for c in us for v in range(c.n_val))
    secrets = V.trace_secrets()
    assert sum(1 for s in secrets if s >= V.R) >= 3 and 0 in secrets and 1 in secrets and V.R - 1 in secrets


def test_oracle_identity_encoding_and_joint_dealing_identities():
    assert O.g1_compress(None) == V.INF48 == bytes([0xC0]) + bytes(47)
    assert O.g1_decompress(V.INF48) is None and O.g1_mul(O.G1_GEN, 0) is None
    assert V.enc(0) == V.INF48 and V.enc(V.R) == V.INF48
    polys, final, sums = V.joint_dealing()
    total = [sum(p[j] for p in polys) % V.R for j in range(2)]
    for i, x in final.items():
        # the sum of the dealers' shares is the share of the summed polynomial ...
        assert x == V.poly_at(total, i)
        # ... each dealer's share passes its own Feldman check ...
        for p in polys:
            want = O.g1_add(VS.point(p[0]), O.g1_mul(VS.point(p[1]), i))
            assert O.g1_compress(want) == V.enc(V.poly_at(p, i))
        # ... and the final pubshare is the summed commitments evaluated at the id
        assert O.g1_compress(O.g1_add(sums[0], O.g1_mul(sums[1], i))) == V.enc(x)
    # any 2 final shares recover the sum of the dealers' secrets, whose key is the summed constant commitment
    for ids in ((1, 2), (1, 3), (2, 3)):
        got = O.recover_secret({i: V.b32(final[i]) for i in ids})
        assert got == V.b32(total[0])
    assert O.g1_compress(sums[0]) == V.enc(total[0])


def _build_and_run(tmp_path, extra, name):
    exe = tmp_path / name
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-o", str(exe), SRC] + extra)
    f = tmp_path / "vectors.txt"
    n_com, n_chk, n_sum, ns = V.write_host_file(str(f))
    r = subprocess.run([str(exe), str(f)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"dkg_ct_host ok: (\d+) validators \((\d+) commitment lanes\), (\d+) check lanes, (\d+) sums, "
                  r"(\d+) trace", r.stdout)
    assert m, r.stdout
    assert tuple(map(int, m.groups())) == (sum(d.n_val for d in V.dealings()), n_com, n_chk, n_sum, ns), r.stdout
    return r


def test_bytes_and_uniform_trace(tmp_path):
    r = _build_and_run(tmp_path, [], "dkg_ct_host")
    for what in ("commit", "check", "sum"):
        m = re.search(what + r" trace [0-9a-f]+, (\d+) mul \+ (\d+) sqr", r.stdout)
        assert m, r.stdout
        # one comb multiplication of 64 mixed additions (7 products + 4 squarings) and one compression: no doubling
        mul, sqr = map(int, m.groups())
        assert 64 * 7 <= mul < 64 * 7 + 16 and 64 * 4 <= sqr < 64 * 4 + 8, r.stdout


def test_host_program_under_asan_ubsan(tmp_path):
    # a stand-alone program with the sanitizers' runtimes linked into it
    r = _build_and_run(tmp_path, ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                  "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan"],
                       "dkg_ct_host_san")
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
    for m in ("deal_commit_batch_ct", "verify_secret_shares_batch_ct", "combine_shares_batch_ct", "verify_secret_shares"):
        assert callable(getattr(HipBLS, m)), m
    assert ctypes.CDLL(LIB).hipbls_abi_version() == 12  # functions were only added


def _objdump():
    for p in ("/opt/rocm/lib/llvm/bin/llvm-objdump", "/opt/rocm/llvm/bin/llvm-objdump"):
        if os.path.exists(p):
            return p
    raise AssertionError("ROCm's llvm-objdump not found")


def _kernel_code(tmp_path):
    """{kernel: [instruction lines]} for the three kernels, from the library's gfx950 code objects."""
    funcs = {}
    for i, co in enumerate(codeobj.code_objects(LIB)):
        f = tmp_path / ("co%d.elf" % i)
        f.write_bytes(co)
        dis = subprocess.run([_objdump(), "-d", "--no-show-raw-insn", str(f)], check=True, capture_output=True,
                             text=True).stdout
        name = None
        for ln in dis.splitlines():
            m = re.match(r"^[0-9a-f]+ <(.+)>:", ln)
            if m:
                name = m.group(1) if m.group(1) in KERNELS else None
                if name:
                    assert name not in funcs, name
                    funcs[name] = []
            elif name and ln.startswith("\t"):
                funcs[name].append(ln.strip())
    return funcs


def test_secret_kernels_code_is_uniform(tmp_path):
    _need_lib()
    funcs = _kernel_code(tmp_path)
    for k in KERNELS:
        assert k in funcs and len(funcs[k]) > 1000, (k, sorted(funcs))
        ins = funcs[k]
        # private-memory loads: the frame plus a constant, never a vector register
        for i in [i for i in ins if re.match(r"(scratch_load|buffer_load)", i)]:
            ops = [o.strip() for o in i.split(None, 1)[1].split(",")]
            assert ops[1] == "off" and "offen" not in i and "idxen" not in i, (k, i)
        assert not [i for i in ins if i.startswith("flat_load")], k
        # no branch on a vector condition at all: the stores are steered, the loops count in scalar registers
        branches = [i for i in ins if re.match(r"s_cbranch_(vccz|vccnz|execz|execnz)\b", i)]
        assert not branches, (k, branches)
        # the comb: one step reads a row of 15 entries x 24 words by scalar loads through ONE base register pair (the
        # row pointer), every word of the row exactly once; all other scalar loads (the kernel arguments) go through
        # other bases and are a few words
        by_base = {}
        for i in ins:
            m = re.match(r"s_load_dword(?:x(\d+))?\s+\S+, (s\[\d+:\d+\]), (\S+)", i)
            if m:
                by_base.setdefault(m.group(2), []).append((int(m.group(3), 0), int(m.group(1) or 1)))
        rows = [v for v in by_base.values() if sum(w for _, w in v) >= COMB_ROW_WORDS]
        assert len(rows) == 1, (k, {b: sum(w for _, w in v) for b, v in by_base.items()})
        covered = sorted(o // 4 + j for o, w in rows[0] for j in range(w))
        assert covered == list(range(COMB_ROW_WORDS)), k
        assert sum(w for v in by_base.values() for _, w in v) - COMB_ROW_WORDS <= 32, k
        # what is left for vector loads is the lane's own input at its public position: exactly the listed loads
        gl = {}
        for i in ins:
            if i.startswith("global_load"):
                gl[i.split()[0]] = gl.get(i.split()[0], 0) + 1
        assert gl == GLOBAL_LOADS[k], (k, gl)


def test_kernels_registered_and_within_budget():
    _need_lib()
    rows = {r[0]: r for r in codeobj.check_budget(LIB)}
    for k in KERNELS:
        assert k in rows, k
        assert rows[k][1] <= codeobj.PRIVATE_SEGMENT_BUDGET, rows[k]
        assert rows[k][3] == 0, rows[k]  # no LDS
    lib = ctypes.CDLL(LIB)
    lib.hipbls_kernel_names.restype = ctypes.c_char_p
    table = lib.hipbls_kernel_names().decode().split()
    for k in KERNELS:
        assert k in table, k


def test_every_earlier_kernel_keeps_its_resource_row():
    """The new kernels live in a translation unit and a namespace of their own: every code object the library had
    before is what it was.  The recorded table is codeobj.resource_table of the parent's build."""
    _need_lib()
    with open(PARENT_TABLE) as f:
        parent = sorted(tuple(r) for r in json.load(f))
    now = sorted(tuple(r) for r in codeobj.resource_table(LIB))
    added = [r for r in now if r[0] in KERNELS]
    assert len(added) == len(KERNELS)
    assert [r for r in now if r[0] not in KERNELS] == parent
