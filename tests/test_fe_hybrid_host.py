"""The fused Verify's shortened final exponentiation (charon_amd/csrc/pairing_lds.h), what can be
checked without a GPU: the hybrid a^|x| (compressed squarings to bit 57, Granger-Scott squarings for bits 60, 62 and
63) against the Granger-Scott exponentiation word for word, and the comparison that can stand in for the last product
(final_exp_is_one_l; Verify's check takes it with -DBLS_FE_CMP=1) against fp12_is_one(final_exponentiation(f)), in a
host program (tests/native/fe_hybrid_host.cpp, also under AddressSanitizer + UBSan); and the resources of the two
fused kernels.
"""
import os
import subprocess

from charon_amd import codeobj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "charon_amd", "libhipbls.so")
SRC = os.path.join(ROOT, "tests", "native", "fe_hybrid_host.cpp")


def _build_and_run(tmp_path, extra, name):
    exe = tmp_path / name
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-o", str(exe), SRC] + extra)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "fe_hybrid_host ok: 200 powers" in r.stdout
    return r


def test_hybrid_power_and_is_one_form(tmp_path):
    """The _l power equals fp12_cyc_exp_xabs_gs on 200 easy-part outputs; the identity, an Fp4 element and 0 return the
    fallback flag with r untouched and the wrapper then gives Granger-Scott's words; a state with z2 = z3 = 0 at any
    one of the three saved powers raises the flag.  final_exp_is_one_l equals fp12_is_one(final_exponentiation(f)) on
    the Miller-loop outputs of valid triples, a wrong root, a swapped key, another signature, two signatures outside
    G2, f = 0 (not one, as the value form), f = 1, an Fp2 element and random elements; the statuses of the fused
    chain equal pairing_check_verify_sig's."""
    _build_and_run(tmp_path, [], "fe_hybrid_host")


def test_hybrid_power_under_asan_ubsan(tmp_path):
    # a stand-alone program with the sanitizers' runtimes linked into it; the fused chain on the comparison too
    r = _build_and_run(tmp_path, ["-DBLS_FE_CMP=1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                  "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan"],
                       "fe_hybrid_host_san")
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr


def test_the_two_switches(tmp_path):
    """-DBLS_FE_CMP=1 puts the fused chain's check on the comparison (the product keeps the value form, pairing_lds.h),
    -DBLS_FE_HYBRID=0 is the six-state power as it was: the same program passes on both."""
    _build_and_run(tmp_path, ["-DBLS_FE_CMP=1"], "fe_hybrid_host_cmp")
    _build_and_run(tmp_path, ["-DBLS_FE_HYBRID=0"], "fe_hybrid_host_six")


def test_fused_kernels_keep_their_resource_rows():
    assert os.path.exists(LIB), "libhipbls.so not built (run __graft_entry__.build())"
    rows = {r[0]: r for r in codeobj.resource_table(LIB)}
    for name in ("k_verify_fused", "k_verify_fused_lines"):
        fused = rows[name]
        print(name, fused)
        assert fused[2] == 512, fused            # one wave per SIMD
        assert fused[3] == 36 * 1024, fused      # LDS
        assert fused[1] <= PRIVATE_SEGMENT_BEFORE[name], fused  # the private segment may only shrink


# bytes per lane before the hybrid power (k_verify_fused, k_verify_fused_lines)
PRIVATE_SEGMENT_BEFORE = {"k_verify_fused": 10424, "k_verify_fused_lines": 10424}
