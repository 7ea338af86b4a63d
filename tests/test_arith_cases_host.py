"""The case lists of tests/arith_cases.py through the HOST build of the kernel arithmetic (tests/native/libhost_ops.so
ht_arith, the dispatchers of tests/native/arith_units.h compiled for x86).

This proves on the CPU that the expected values and the record plumbing are right before the same lists reach a GPU
(tests/test_gpu_arith_layers.py), and it closes the host suite's own gaps: Fp and Fp2 ops on raw limbs, the
exceptional cases of the curve additions, the scalar-multiple edges and the decompression flag table.  Exact equality
everywhere: this is integer arithmetic.
"""
import ctypes

import pytest

from tests import arith_cases as ac
from tests.hostlib import lib


@pytest.fixture(scope="module")
def run():
    L = lib()
    L.ht_arith.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_uint64]

    def call(layer, op, data, n):
        out = ctypes.create_string_buffer(ac.OUT_BYTES[layer] * n)
        assert L.ht_arith(layer, op, data, out, n) == 0
        return out.raw
    return call


_FAMILIES = ac.all_families(host=True)


@pytest.mark.parametrize("make", [f for _, f in _FAMILIES], ids=[i for i, _ in _FAMILIES])
def test_family(run, make):
    make().check(run)


def test_inverses_agree_on_canonical_input(run):
    """fp_inv (binary GCD) and fp_inv_pow (Fermat) give the same limbs on every canonical input of the list."""
    inv, powr = ac.fp_family("inv", True), ac.fp_family("inv_pow", True)
    n = len(powr)
    assert inv.inputs[:n] == powr.inputs
    assert run(inv.layer, inv.op, b"".join(inv.inputs[:n]), n) == run(powr.layer, powr.op, b"".join(powr.inputs), n)


def test_case_counts():
    """The lists keep their size: a family that lost its cases would pass vacuously."""
    counts = {i: len(f()) for i, f in _FAMILIES}
    assert counts["fp-add"] == 144 and counts["fp-mul"] == 144 + 140 and counts["fp-inv"] == 64 + 53 + 5
    assert counts["fp-inv_pow"] == 64 + 53 and counts["fp2-mul"] == 256 and counts["fp2-sqr"] == 100
    assert counts["g1-add"] == 10 and counts["g2-add"] == 10 and counts["g1-add_aff"] == 6
    assert counts["g1-decompress"] == 11 and counts["g2-decompress_check"] == 15
    assert counts["h2c-hash_to_g2"] == 11 and counts["h2c-map_to_curve"] == 12
    assert all(c > 0 for c in counts.values())
