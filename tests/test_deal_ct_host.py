"""Batched, secret-independent ThresholdSplit / RecoverSecret (charon_amd/csrc/deal_ct.h, deal_ct.hip),
what can be checked without a GPU:

  * the lane functions in a host program (tests/native/deal_ct_host.cpp, also under AddressSanitizer + UBSan): bytes and
    statuses against the variable-time forms and the Python oracle over tests/deal_ct_vectors.py, the fixed-base comb
    over every table entry, ONE operation trace (field.h BLS_CT_TRACE) for every secret at a fixed public shape, and
    the same trace telling jac_mul_limbs' secrets apart;
  * the built library's symbols and Python methods;
  * the gfx950 code of k_deal_ct and k_recover_ct: no private-memory load addressed from a vector register, no flat
    load, no branch on a vector condition at all, the comb table read by scalar loads only (a whole row through one
    base register, every vector load enumerated), resources within budget.
"""
import ctypes
import os
import re
import subprocess

from charon_amd import codeobj
from tests import deal_ct_vectors as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "charon_amd", "libhipbls.so")
SRC = os.path.join(ROOT, "tests", "native", "deal_ct_host.cpp")
SYMBOLS = ("hipbls_threshold_split_batch_ct", "hipbls_recover_secret_batch_ct",
           "hipbls_threshold_split_batch_ct_device", "hipbls_recover_secret_batch_ct_device")
CT_KERNELS = ("k_deal_ct", "k_recover_ct")
ALL_KERNELS = CT_KERNELS + ("k_g1_comb_build", "k_recover_plan")

# Vector-condition branches (s_cbranch_vccz / vccnz / execz / execnz) each kernel may hold, one per PUBLIC condition.
# None: the stores of lanes that must not store (i >= n, k = 0 for the share bytes, k != 0 for the status) are steered
# to a sink by address arithmetic, "public keys wanted" is a kernel argument (a scalar branch), the Horner and comb
# loops count in scalar registers, and k_recover_ct loops over the launch's largest group, read into a scalar.
PUBLIC_VECTOR_BRANCHES = {"k_deal_ct": [], "k_recover_ct": []}

# Every global (vector) load of each kernel, by mnemonic and count, with the public address it reads.  The comb table
# is NOT among them: it is read by scalar loads (s_load_dword*), whose address is the wave's.
GLOBAL_LOADS = {
    "k_deal_ct": {
        # tails + 32 ((threshold-1) v + j-1) in the Horner loop and secrets + 32 v after it: two 16-byte halves each
        "global_load_dwordx4": 4,
    },
    "k_recover_ct": {
        "global_load_dword": 2,    # group_offsets[g] and group_offsets[g+1] (their low words)
        "global_load_dwordx4": 2,  # shares + 32 (group_offsets[g] + k) in the recovery loop: two 16-byte halves
    },
}
COMB_ROW_WORDS = 15 * 24


def _build_and_run(tmp_path, extra, name):
    exe = tmp_path / name
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-o", str(exe), SRC] + extra)
    f = tmp_path / "vectors.txt"
    nv, ng, ns = V.write_host_file(str(f))
    r = subprocess.run([str(exe), str(f)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"deal_ct_host ok: (\d+) validators \((\d+) lanes\), (\d+) groups, (\d+) comb scalars, (\d+) trace",
                  r.stdout)
    assert m, r.stdout
    assert tuple(map(int, m.groups())) == (nv, sum(v.total + 1 for v in V.validators()), ng, 64 * 16, ns), r.stdout
    return r


def test_vectors_cover_the_list():
    vs, gs = V.validators(), V.groups()
    assert {(v.total, v.threshold) for v in vs} >= set(V.SHAPES)
    for shape in V.SHAPES:
        assert {v.secret for v in vs if (v.total, v.threshold) == shape} >= set(V.ROOTS)
    assert any(v.secret < V.R and any(c >= V.R for c in v.tail) for v in vs)
    assert any(v.status == V.OK and 0 in v.scalars[1:] for v in vs)
    assert {len(g.pairs) for g in gs} >= {0, 1, 3, 7}
    assert any(i < 0 for g in gs for i, _ in g.pairs)
    assert {g.status for g in gs} == {V.OK, V.ERR_SECRET, V.ERR_COMBINE}
    secrets = V.trace_secrets()
    assert sum(1 for s in secrets if s >= V.R) >= 3 and 0 in secrets and 1 in secrets and V.R - 1 in secrets


def test_bytes_uniform_trace_and_instrument(tmp_path):
    r = _build_and_run(tmp_path, [], "deal_ct_host")
    m = re.search(r"variable-time products sk=1 / sk=r-1: (\d+) / (\d+)", r.stdout)
    assert m, r.stdout
    a, b = map(int, m.groups())
    assert a != b  # the instrument resolves what the variable-time form does with the secret
    m = re.search(r"comb \+ key trace [0-9a-f]+, (\d+) mul \+ (\d+) sqr", r.stdout)
    # two comb multiplications of 64 mixed additions (7 products + 4 squarings) and one compression: no doubling
    mul, sqr = map(int, m.groups())
    assert 2 * 64 * 7 <= mul < 2 * 64 * 7 + 16 and 2 * 64 * 4 <= sqr < 2 * 64 * 4 + 8, r.stdout


def test_host_program_under_asan_ubsan(tmp_path):
    # a stand-alone program with the sanitizers' runtimes linked into it
    r = _build_and_run(tmp_path, ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                  "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan"],
                       "deal_ct_host_san")
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr


def _need_lib():
    assert os.path.exists(LIB), "libhipbls.so not built (run __graft_entry__.build())"


def test_symbols_exported():
    _need_lib()
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for s in SYMBOLS + ("hipbls_threshold_split", "hipbls_recover_secret"):
        assert s in names, s
    from charon_amd.tbls import HipBLS, exported_symbols
    assert set(SYMBOLS) <= set(exported_symbols())
    assert callable(HipBLS.threshold_split_batch_ct) and callable(HipBLS.recover_secret_batch_ct)
    assert ctypes.CDLL(LIB).hipbls_abi_version() == 12  # functions were only added


def _objdump():
    for p in ("/opt/rocm/lib/llvm/bin/llvm-objdump", "/opt/rocm/llvm/bin/llvm-objdump"):
        if os.path.exists(p):
            return p
    raise AssertionError("ROCm's llvm-objdump not found")


def _kernel_code(tmp_path):
    """{kernel: [instruction lines]} for the deal kernels, from the library's gfx950 code objects."""
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
                name = m.group(1) if m.group(1) in ALL_KERNELS else None
                if name:
                    assert name not in funcs, name
                    funcs[name] = []
            elif name and ln.startswith("\t"):
                funcs[name].append(ln.strip())
    return funcs


def test_secret_kernels_code_is_uniform(tmp_path):
    _need_lib()
    funcs = _kernel_code(tmp_path)
    for k in CT_KERNELS:
        assert k in funcs and len(funcs[k]) > 1000, (k, sorted(funcs))
        ins = funcs[k]
        # private-memory loads: the frame plus a constant, never a vector register
        for i in [i for i in ins if re.match(r"(scratch_load|buffer_load)", i)]:
            ops = [o.strip() for o in i.split(None, 1)[1].split(",")]
            assert ops[1] == "off" and "offen" not in i and "idxen" not in i, (k, i)
        assert not [i for i in ins if i.startswith("flat_load")], k
        branches = [i for i in ins if re.match(r"s_cbranch_(vccz|vccnz|execz|execnz)\b", i)]
        assert len(branches) <= len(PUBLIC_VECTOR_BRANCHES[k]), (k, branches)
        # the comb: one step reads a row of 15 entries x 24 words by scalar loads through ONE base register pair (the
        # row pointer), every word of the row exactly once; all other scalar loads (the kernel arguments, the plan
        # word) go through other bases and are a few words
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
        assert sum(1 for i in ins if i.startswith("v_bfi_b32")) >= 14 * 24, k
        # what is left for vector loads is the lane's own input at its public position: exactly the listed loads
        gl = {}
        for i in ins:
            if i.startswith("global_load"):
                gl[i.split()[0]] = gl.get(i.split()[0], 0) + 1
        assert gl == GLOBAL_LOADS[k], (k, gl)


def test_kernels_registered_and_within_budget():
    _need_lib()
    rows = {r[0]: r for r in codeobj.check_budget(LIB)}
    for k in ALL_KERNELS:
        assert k in rows, k
        assert rows[k][1] <= codeobj.PRIVATE_SEGMENT_BUDGET, rows[k]
        assert rows[k][3] == 0, rows[k]  # no LDS
    assert "k_threshold_split" not in rows and "k_recover_secret" not in rows  # replaced, not kept beside
    lib = ctypes.CDLL(LIB)
    lib.hipbls_kernel_names.restype = ctypes.c_char_p
    table = lib.hipbls_kernel_names().decode().split()
    for k in ALL_KERNELS:
        assert k in table, k
    assert "k_threshold_split" not in table and "k_recover_secret" not in table
