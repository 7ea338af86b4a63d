"""Secret-independent Sign / SecretToPublicKey (charon_amd/csrc/sign_ct.h, sign_ct.hip), what can be
checked without a GPU:

  * the lane functions in a host program (tests/native/sign_ct_host.cpp, also under AddressSanitizer + UBSan): the
    bytes and statuses of op_sign / op_sk_to_pk over the edge scalars and seeded random ones, ONE operation trace
    (field.h BLS_CT_TRACE) for every secret, and the same trace telling the variable-time forms' secrets apart;
  * the built library's symbols and Python methods;
  * the gfx950 code of the kernels that see a secret: no private-memory load addressed from a vector register, no
    vector-condition branch beyond the listed public ones, resources within the budget.
"""
import ctypes
import os
import re
import subprocess

from charon_amd import codeobj
from tests import sign_ct_vectors as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "charon_amd", "libhipbls.so")
SRC = os.path.join(ROOT, "tests", "native", "sign_ct_host.cpp")
SYMBOLS = ("hipbls_sign_batch_ct", "hipbls_secret_to_public_key_batch_ct", "hipbls_sign_batch_ct_device",
           "hipbls_secret_to_public_key_batch_ct_device")
CT_KERNELS = ("k_sign_ct_mul", "k_sk_to_pk_ct")

# Vector-condition branches (s_cbranch_vccz / vccnz / execz / execnz) each kernel may hold, one per PUBLIC condition.
# Both kernels: the `i < n` guard of the final stores.  The status zero-fill and sk = 0 are masks in this
# implementation, so they add none; every loop counter is a scalar count (s_cbranch_scc*, not listed here).
PUBLIC_VECTOR_BRANCHES = {"k_sign_ct_mul": ["i < n store guard"], "k_sk_to_pk_ct": ["i < n store guard"]}


def _secrets_file(tmp_path):
    secrets = V.edge_secrets() + V.random_secrets(128)
    # every entry is classified against r here, not assumed
    assert sum(1 for s in secrets if s >= V.R) == 3 and secrets.count(0) == 1
    assert all(0 <= s < 2**256 for s in secrets)
    f = tmp_path / "secrets.txt"
    f.write_text("".join("%s %d\n" % (V.sk_bytes(s).hex(), V.expected_status(s)) for s in secrets))
    return f, len(secrets)


def _build_and_run(tmp_path, extra, name):
    exe = tmp_path / name
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-o", str(exe), SRC] + extra)
    f, n = _secrets_file(tmp_path)
    r = subprocess.run([str(exe), str(f)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "sign_ct_host ok: %d secrets x 3 messages" % n in r.stdout, r.stdout
    return r


def test_bytes_uniform_trace_and_instrument(tmp_path):
    """op_sign_ct == op_sign and op_sk_to_pk_ct == op_sk_to_pk (status, bytes; zero-filled output on ERR_SECRET) over
    the edge list + 128 random secrets x three messages; after the hash, the trace digest and both product counts are
    identical for every secret; g2_mul_glv4 and jac_mul_limbs give different digests for sk = 1 and sk = r - 1."""
    r = _build_and_run(tmp_path, [], "sign_ct_host")
    m = re.search(r"variable-time products sk=1 / sk=r-1: sign (\d+) / (\d+), sk_to_pk (\d+) / (\d+)", r.stdout)
    assert m, r.stdout
    a, b, c, d = map(int, m.groups())
    assert a != b and c != d  # the old forms' work depends on the secret; the instrument resolves it


def test_host_program_under_asan_ubsan(tmp_path):
    # a stand-alone program with the sanitizers' runtimes linked into it
    r = _build_and_run(tmp_path, ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                  "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan"],
                       "sign_ct_host_san")
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
    assert callable(HipBLS.sign_batch_ct) and callable(HipBLS.secret_to_public_key_batch_ct)
    # adding functions leaves the ABI version where it was
    assert ctypes.CDLL(LIB).hipbls_abi_version() == 12


def _objdump():
    for p in ("/opt/rocm/lib/llvm/bin/llvm-objdump", "/opt/rocm/llvm/bin/llvm-objdump"):
        if os.path.exists(p):
            return p
    raise AssertionError("ROCm's llvm-objdump not found")


def _ct_functions(tmp_path):
    """{symbol: [instruction lines]} of every function of the library's gfx950 code objects whose name holds `_ct`
    (the namespace prefix bls_ct does not count): the kernels that see a secret and whatever of their lane functions
    the compiler kept out of line."""
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
                name = m.group(1)
                if "_ct" in name.replace("bls_ct", ""):
                    assert name not in funcs, name
                    funcs[name] = []
                else:
                    name = None
            elif name and ln.startswith("\t"):
                funcs[name].append(ln.strip())
    return funcs


def test_secret_kernels_code_is_uniform(tmp_path):
    _need_lib()
    funcs = _ct_functions(tmp_path)
    for k in CT_KERNELS:
        assert k in funcs and len(funcs[k]) > 1000, (k, sorted(funcs))
    for name, ins in funcs.items():
        if name == "k_sign_ct_hash":  # sees the public message only
            continue
        # private-memory loads: the address is the frame (`off` / an SGPR) plus a constant, never a vector register --
        # the form a lane-dependent table index would produce
        loads = [i for i in ins if re.match(r"(scratch_load|buffer_load)", i)]
        for i in loads:
            ops = [o.strip() for o in i.split(None, 1)[1].split(",")]
            assert ops[1] == "off" and "offen" not in i and "idxen" not in i, (name, i)
        # a generic (flat) load could reach private memory through a pointer: none either
        assert not [i for i in ins if i.startswith("flat_load")], name
        branches = [i for i in ins if re.match(r"s_cbranch_(vccz|vccnz|execz|execnz)\b", i)]
        assert len(branches) <= len(PUBLIC_VECTOR_BRANCHES.get(name, [])), (name, branches)
    # the table scans are there: at least 15 entries x 72 (G2) / 36 (G1) words of bitwise selects and loads
    sel = {k: sum(1 for i in funcs[k] if i.startswith("v_bfi_b32")) for k in CT_KERNELS}
    assert sel["k_sign_ct_mul"] >= 15 * 72 and sel["k_sk_to_pk_ct"] >= 15 * 36, sel


def test_kernels_registered_and_within_budget():
    _need_lib()
    rows = {r[0]: r for r in codeobj.check_budget(LIB)}
    for k in ("k_sign_ct_hash",) + CT_KERNELS:
        assert k in rows, k
        assert rows[k][1] <= codeobj.PRIVATE_SEGMENT_BUDGET, rows[k]
        assert rows[k][3] == 0, rows[k]  # no LDS
    lib = ctypes.CDLL(LIB)
    lib.hipbls_kernel_names.restype = ctypes.c_char_p
    table = lib.hipbls_kernel_names().decode().split()
    for k in ("k_sign_ct_hash",) + CT_KERNELS:
        assert k in table, k
