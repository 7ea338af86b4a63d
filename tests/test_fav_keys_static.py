"""FastAggregateVerify by resident key index (hipbls_verify_aggregate_batch_keys), what can be checked
without a GPU: the header and the ctypes mirror, the built library's symbols and kernels, the resources of the kernels
that now share a body with their `_keys` twins, the host program for the slice planner and the message fold, and the
Go binding's text.
"""
import ctypes
import os
import re
import subprocess

from charon_amd import codeobj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "charon_amd", "libhipbls.so")
ERR_ARG = 16

SYMBOLS = ("hipbls_verify_aggregate_batch_keys", "hipbls_verify_aggregate_batch_keys_device")
KERNELS = ("k_fav_pair_lq16_keys", "k_fav_batch_keys", "k_fav_sum_keys")


def _need_lib():
    assert os.path.exists(LIB), "libhipbls.so not built (run __graft_entry__.build())"


def _read(*rel):
    with open(os.path.join(ROOT, *rel)) as f:
        return f.read()


def _decl(text, name):
    """The parameter list of `name`'s declaration, whitespace folded."""
    m = re.search(r"\bint %s\(([^)]*)\)" % name, text)
    assert m, name
    return " ".join(m.group(1).split())


# ------------------------------------------------------------------------------------------------ header and mirror
def test_header_declares_both_calls_as_the_issue_states_them_and_abi_stays_12():
    hdr = re.sub(r"/\*.*?\*/", "", _read("include", "hipbls.h"), flags=re.S)
    assert _decl(hdr, "hipbls_verify_aggregate_batch_keys") == (
        "const uint32_t* key_idx, const uint64_t* key_offsets, uint64_t n_groups, const uint8_t* sigs, "
        "const uint8_t* msgs, const uint64_t* msg_offsets, int32_t* status")
    assert _decl(hdr, "hipbls_verify_aggregate_batch_keys_device") == (
        "const uint32_t* d_key_idx, uint64_t nkeys, const uint64_t* d_key_offsets, uint64_t n_groups, "
        "const uint8_t* d_sigs, const uint8_t* d_msgs, const uint64_t* d_msg_offsets, int32_t* d_status, void* stream")
    assert re.search(r"#define HIPBLS_ABI_VERSION 12\b", hdr)


def test_symbols_exported_and_mirrored():
    _need_lib()
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for s in SYMBOLS:
        assert s in names, s
    from charon_amd.tbls import HipBLS, exported_symbols, load_library
    assert set(SYMBOLS) <= set(exported_symbols())
    lib = load_library()
    assert lib.hipbls_abi_version() == 12
    u32p, u64p, i32p = (ctypes.POINTER(t) for t in (ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int32))
    host = lib.hipbls_verify_aggregate_batch_keys.argtypes
    assert len(host) == 7 and host[0] == u32p and host[1] == u64p and host[2] == ctypes.c_uint64
    assert host[5] == u64p and host[6] == i32p
    dev = lib.hipbls_verify_aggregate_batch_keys_device.argtypes
    assert len(dev) == 9 and dev[1] == ctypes.c_uint64 and dev[3] == ctypes.c_uint64 and dev[8] == ctypes.c_void_p
    assert callable(HipBLS.batch_verify_aggregate_keys_status) and callable(HipBLS.verify_aggregate_keys)


def test_argument_errors_need_no_device():
    """Null pointers and bad offsets are refused before the library binds a device."""
    _need_lib()
    from charon_amd.tbls import load_library
    lib = load_library()
    st = (ctypes.c_int32 * 2)(7, 7)
    koff = (ctypes.c_uint64 * 3)(0, 1, 2)
    idx = (ctypes.c_uint32 * 2)(0, 0)
    sig = bytes(192)
    assert lib.hipbls_verify_aggregate_batch_keys(idx, koff, 0, sig, b"", koff, st) == 0  # no groups: nothing to do
    assert lib.hipbls_verify_aggregate_batch_keys(idx, None, 2, sig, b"ab", koff, st) == ERR_ARG
    assert lib.hipbls_verify_aggregate_batch_keys(idx, koff, 2, None, b"ab", koff, st) == ERR_ARG
    assert lib.hipbls_verify_aggregate_batch_keys(idx, koff, 2, sig, b"ab", koff, None) == ERR_ARG
    assert lib.hipbls_verify_aggregate_batch_keys(None, koff, 2, sig, b"ab", koff, st) == ERR_ARG  # two keys, no indices
    assert lib.hipbls_verify_aggregate_batch_keys(idx, koff, 2, sig, None, koff, st) == ERR_ARG    # two bytes, no messages
    down = (ctypes.c_uint64 * 3)(0, 2, 1)
    assert lib.hipbls_verify_aggregate_batch_keys(idx, down, 2, sig, b"ab", koff, st) == ERR_ARG
    assert lib.hipbls_verify_aggregate_batch_keys(idx, koff, 2, sig, b"ab", down, st) == ERR_ARG
    nonzero = (ctypes.c_uint64 * 3)(1, 1, 2)
    assert lib.hipbls_verify_aggregate_batch_keys(idx, nonzero, 2, sig, b"ab", koff, st) == ERR_ARG
    assert list(st) == [7, 7]


# ------------------------------------------------------------------------------------------------ kernels
def test_new_kernels_in_the_kernel_table_and_within_the_scratch_budget():
    _need_lib()
    lib = ctypes.CDLL(LIB)
    lib.hipbls_kernel_names.restype = ctypes.c_char_p
    table = lib.hipbls_kernel_names().decode().split()
    rows = {r[0]: r for r in codeobj.resource_table(LIB)}
    for k in KERNELS:
        assert k in table, k
        assert k in rows, k
        assert rows[k][1] <= codeobj.PRIVATE_SEGMENT_BUDGET, rows[k]
    # the check at two waves per SIMD: 256 registers, like the wire-format kernel it shares its body with
    assert rows["k_fav_pair_lq16_keys"][2] <= 256 and rows["k_fav_pair_lq16"][2] <= 256
    # the twins are no deeper and hold no more LDS than the wire-format kernels
    for keyed, wire in (("k_fav_pair_lq16_keys", "k_fav_pair_lq16"), ("k_fav_batch_keys", "k_fav_batch")):
        assert rows[keyed][1] <= rows[wire][1], (rows[keyed], rows[wire])
        assert rows[keyed][3] <= rows[wire][3], (rows[keyed], rows[wire])
    # the slice sum is curve additions only: far from the pairing kernels' frames
    assert rows["k_fav_sum_keys"][1] < rows["k_fav_batch_keys"][1] // 4


def test_wire_format_kernels_keep_their_lds_and_occupancy():
    """The shared body declares no LDS of its own: k_fav_batch and k_fav_pair_lq16 hold what their arrays declare (36
    words x 64 lanes, the signature and H(m) staging, the flags), the twins the same, and the check stays at two waves
    per SIMD.  DESIGN.md 4.7.1 states the full before / after table."""
    _need_lib()
    rows = {r[0]: r[1:] for r in codeobj.resource_table(LIB)}
    assert rows["k_fav_batch"][2] == rows["k_fav_batch_keys"][2] == 4 * (64 * 36 + 48 + 48 + 3)
    assert rows["k_fav_pair_lq16"][2] == rows["k_fav_pair_lq16_keys"][2]
    assert 4 * (64 * 36 + 2) <= rows["k_fav_pair_lq16"][2] <= 4 * (64 * 36 + 2) + 64  # + bls_race's words
    assert rows["k_fav_prep8"][2] <= 64


def test_one_body_per_kernel_pair():
    """The wire-format kernels and their twins instantiate one body each; the key loop exists once."""
    hexs = _read("charon_amd", "csrc", "verify_hex.hip")
    kern = _read("charon_amd", "csrc", "kernels.h")
    keys = _read("charon_amd", "csrc", "fav_keys.h")
    assert hexs.count("fav_pair_lq16_body(") == 3 and kern.count("fav_batch_body(") == 3  # the body and two uses
    assert "jac_add_aff" not in hexs[hexs.index("fav_pair_lq16_body"):]
    assert keys.count("jac_add_aff(acc, acc, a)") == 1
    body = kern[kern.index("void fav_batch_body("):kern.index("__global__ void __launch_bounds__(kFavBlock) k_fav_batch(")]
    assert "jac_add_aff" not in body and "fav_fold_group(" in body
    assert "fav_fold(" in kern[kern.index("k_fav_sum_keys("):]


# ------------------------------------------------------------------------------------------------ host program
def test_slice_planner_and_message_fold_host_program_under_sanitizers(tmp_path):
    """tests/native/fav_split_main.cpp: no keys at all, groups of 0 and 1 keys, a group at the threshold, an exact
    multiple of the slice, mixed groups above and below -- the slices tile each cut group exactly, none empty; the
    groups' messages folded and read from the cache without an insert."""
    exe = tmp_path / "fav_split_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "charon_amd", "csrc"), "-o", str(exe),
                           os.path.join(ROOT, "tests", "native", "fav_split_main.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.strip() == "ok"


def test_split_threshold_is_read_from_the_environment_at_init():
    src = _read("charon_amd", "csrc", "hipbls.hip")
    assert re.search(r'getenv\("HIPBLS_FAV_SUM_SPLIT"\)', src)
    assert re.search(r"constexpr uint64_t kFavSumSplit = \d+;", src)
    assert "fav_split_plan(koffs, n_groups, g_fav_sum_split, plan)" in src
    for name in ('"fav_prep8_keys"', '"fav_lq16_keys"', '"fav_keys"', '"fav_sum_keys"'):
        assert name in src, name


# ------------------------------------------------------------------------------------------------ Go text
def test_go_binding_takes_the_keyed_call_under_the_table_lock():
    for rel, head, wire, keys in (
            ("hipbls.go", "func (HipBLS) VerifyAggregate(", "C.hipbls_verify_aggregate(", "lockTable(shares)"),
            ("batch.go", "func (h HipBLS) BatchVerifyAggregate(", "C.hipbls_verify_aggregate_batch(",
             "lockTable(allKeys)")):
        src = _read("integration", "charon", "tbls", "hipbls", rel)
        fn = src[src.index(head):]
        fn = fn[:fn.index("\n}\n")]
        assert "C.hipbls_verify_aggregate_batch_keys(" in fn
        assert wire in fn  # the wire-format call stays for keys outside the table
        # the read lock is taken before the keyed call and released after it
        assert fn.index(keys) < fn.index("C.hipbls_verify_aggregate_batch_keys(") < fn.index("release()")
        assert fn.index(wire) < fn.index("release()")
    p2 = _read("integration", "patches", "0002-tbls-hipbls-package.patch")
    assert "hipbls_verify_aggregate_batch_keys(" in p2 and '"batch_verify_aggregate_keys"' in p2
