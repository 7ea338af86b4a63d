"""Every arithmetic layer of the DEVICE build against the oracle, one case per lane.

The device build of charon_amd/csrc is not the host build's program: Fp add / sub / neg, the Fp and Fp2 products and
squarings and the binary-GCD divstep are hand-written asm there, the modulus travels in SGPRs, and the Fp2 routines
take unreduced operands.  tests/test_host_arith.py and tests/test_arith_cases_host.py never run any of that.  This
file runs tests/arith_cases.py's lists (the same cases, the same expected values from oracle/bls12381.py and Python
integers) through tests/native/libgpu_units.so, whose gu_*_op kernels call the product's own device functions:

* Fp and Fp2 on raw limbs, at the edges and at the product routines' contract bounds (unreduced sums in [p, 2p),
  operands up to 2^382 - 1), the divstep inverse on Fibonacci-like and non-canonical inputs, the square roots;
* Fp12 ops; the curve additions' exceptional cases, scalar-multiple edges, subgroup checks and the decompression flag
  table for G1 and G2; hash to curve across the SHA-256 padding boundaries; one-lane pairings;
* the split-Fp2 build (BLS_FP2_PAIR, libgpu_units_pair.so): an Fp2 value on lanes l and l ^ 4, both lanes' results
  returned; the whole list, full waves and partial last groups.

Exact equality everywhere; no case is skipped or filtered at run time.
"""
import ctypes

import pytest

from tests import arith_cases as ac

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def run():
    from tests.hostlib import gpu_units_lib
    G = gpu_units_lib()
    sig = [ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_uint64]
    for fn in (G.gu_fp_op, G.gu_fp2_op, G.gu_fp12_op, G.gu_h2c_op, G.gu_pairing_op):
        fn.argtypes = sig
    G.gu_curve_op.argtypes = [ctypes.c_int] + sig
    fns = {ac.AU_FP: G.gu_fp_op, ac.AU_FP2: G.gu_fp2_op, ac.AU_FP12: G.gu_fp12_op, ac.AU_H2C: G.gu_h2c_op,
           ac.AU_PAIR: G.gu_pairing_op,
           ac.AU_CURVE_G1: lambda *a: G.gu_curve_op(1, *a), ac.AU_CURVE_G2: lambda *a: G.gu_curve_op(2, *a)}

    def call(layer, op, data, n):
        out = ctypes.create_string_buffer(ac.OUT_BYTES[layer] * n)
        assert fns[layer](op, data, out, n) == 0
        return out.raw
    return call


def _families(prefix):
    fams = [(i, f) for i, f in ac.all_families(host=False) if i.split("-")[0] in prefix]
    return pytest.mark.parametrize("make", [f for _, f in fams], ids=[i for i, _ in fams])


@_families(("fp",))
def test_fp(run, make):
    make().check(run)


def test_fp_inverses_agree_on_canonical_input(run):
    """The divstep inverse and the Fermat power give the same limbs on every canonical input of the list."""
    inv, powr = ac.fp_family("inv"), ac.fp_family("inv_pow")
    n = len(powr)
    assert inv.inputs[:n] == powr.inputs
    assert run(inv.layer, inv.op, b"".join(inv.inputs[:n]), n) == run(powr.layer, powr.op, b"".join(powr.inputs), n)


@_families(("fp2",))
def test_fp2(run, make):
    make().check(run)


@_families(("fp12",))
def test_fp12(run, make):
    make().check(run)


@_families(("g1", "g2"))
def test_curve(run, make):
    make().check(run)


@_families(("h2c",))
def test_hash_to_curve(run, make):
    make().check(run)


@_families(("pair",))
def test_pairing_one_lane(run, make):
    make().check(run)


# ---------------------------------------------------------------------------------------------- split-Fp2 build
@pytest.fixture(scope="module")
def pair_run():
    from tests.hostlib import gpu_units_pair_lib
    G = gpu_units_pair_lib()
    G.gup_run.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_uint32]

    def call(op, cases):
        n = len(cases)
        data = b"".join(ac.raw(a[0]) + ac.raw(a[1]) + ac.raw(b[0]) + ac.raw(b[1]) for a, b, _ in cases)
        out = ctypes.create_string_buffer(192 * n)
        assert G.gup_run(op, data, out, n) == 0
        return [(out.raw[192 * i:192 * i + 96], out.raw[192 * i + 96:192 * i + 192]) for i in range(n)]
    return call


@pytest.mark.parametrize("op,name", [(0, "fp2_mul"), (1, "fp2_sqr"), (2, "fp2_mul_fp"), (3, "fp_pow_sqrt"),
                                     (4, "fp_pow_sqrt_m1")])
def test_split_fp2_build(pair_run, op, name):
    """Lanes l and l ^ 4 agree and equal the one-lane routines' expected values.  Every case of the list runs in one
    launch; its longest prefix of whole waves (a multiple of 32 cases = 64 lanes) runs on its own, so every lane pair
    of a wave has live data; further launches of 4 k + 1, 2 and 3 cases end in a partial group of eight."""
    cases = ac.pair_cases(op)
    full = cases[:len(cases) - len(cases) % 32]
    parts = [cases[:5], cases[:30], cases[:7]]
    assert len(full) >= 32 and len(full) % 32 == 0 and [len(p) % 4 for p in parts] == [1, 2, 3]
    for part in [cases, full] + parts:
        for (a, b, r), (lo, hi) in zip(part, pair_run(op, part)):
            assert lo == hi, (name, hex(a[0]), hex(a[1]))
            assert lo == ac.raw(r[0]) + ac.raw(r[1]), (name, hex(a[0]), hex(a[1]), hex(b[0]), hex(b[1]))
