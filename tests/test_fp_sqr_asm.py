"""The gfx950 Fp squaring routine (charon_amd/tools/gen_fp_asm.py gen_sqr / gen_sqr_routine), checked on the CPU.

The EMITTED text (BLS_FP_SQR_ASM_ROUTINE in charon_amd/csrc/fp_asm_gfx950.h) is interpreted lane-scalar from both of
its entries -- bls_fp_sqr_rt (one squaring) and bls_fp_sqr_run_rt (n squarings, n in s38) -- and compared limb for
limb with big-integer Montgomery squaring.  The strict interpreter raises when a v_mad_u64_u32 drops a carry that
no v_addc catches, and the bound walk of tests/test_fp_asm.py, which knows nothing of the generator's bookkeeping,
proves every elided carry impossible for operands below 2^382.
"""
import os
import random
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "charon_amd", "tools"))
import gen_fp_asm as g  # noqa: E402

from tests.test_fp_asm import _limbs, _symbolic_max, _val  # noqa: E402

R_INV = pow(pow(2, 384, g.P), -1, g.P)
TOP = (1 << 382) - 1  # the operand contract's largest value: every lower limb 0xFFFFFFFF, the top limb 2^30 - 1


def _routine():
    text = open(os.path.join(ROOT, "charon_amd", "csrc", "fp_asm_gfx950.h")).read()
    block = text.split("#define BLS_FP_SQR_ASM_ROUTINE \\", 1)[1].split("\n\n", 1)[0]
    return [s.replace("\\n", "").replace("\\t", "") for s in re.findall(r'^\s+"([^"]*)"', block, re.M)]


def _sqr_n(a, n):
    for _ in range(n):
        a = a * a * R_INV % g.P
    return a


def _edges():
    e = [0, 1, pow(2, 384, g.P), g.P - 1, g.P, 2 * g.P - 1, TOP, TOP - 1, 2 * g.P, g.P + 1, 1 << 381]
    e += [0xFFFFFFFF << (32 * k) for k in range(11)] + [0x3FFFFFFF << 352]  # one limb at its largest
    e += [1 << (32 * k) for k in range(12)] + [0x80000000 << (32 * k) for k in range(11)]  # the bit that leaves E into D
    alt = sum(0xFFFFFFFF << (32 * k) for k in range(0, 12, 2))
    e += [alt, (alt << 32) & TOP, sum(0xAAAAAAAA << (32 * k) for k in range(12)) & TOP,
          sum(0x55555555 << (32 * k) for k in range(12)) & TOP, sum(0x80000000 << (32 * k) for k in range(11))]
    assert all(0 <= x <= TOP for x in e)
    return e


@pytest.fixture(scope="module")
def routine():
    return _routine()


def _single(rt, a):
    return _val(g.emulate(rt, _limbs(a), _limbs(0), entry="bls_fp_sqr_rt"))


def _run(rt, a, n):
    return _val(g.emulate(rt, _limbs(a), _limbs(0), entry="bls_fp_sqr_run_rt", sregs={g.SQR_RUN_SGPR: n}))


def test_header_matches_generator(routine):
    assert routine == g.gen_sqr_routine(), "fp_asm_gfx950.h is stale: rerun charon_amd/tools/gen_fp_asm.py"
    body = g.gen_sqr()
    assert sum(x.startswith("v_mad_u64_u32") for x in body) == 78 + 144  # operand mads + reduction mads
    assert len(body) < len(g.gen_mul()) - 66  # at least the 66 repeated cross products are gone


def test_single_squaring_edges_and_random(routine):
    """One squaring (bls_fp_sqr_rt): limb-exact and canonical on the edge operands and 10,000 seeded random operands
    below 2^382 (lazy operands in [p, 2^382) included: three of four random ones)."""
    rnd = random.Random(1101)
    for a in _edges() + [rnd.randrange(1 << 382) for _ in range(10000)]:
        got = _single(routine, a)
        assert got == a * a * R_INV % g.P, hex(a)


@pytest.mark.parametrize("n", [1, 2, 5, 63])
def test_run_entry_equals_n_squarings(routine, n):
    """The run entry (bls_fp_sqr_run_rt, n in s38) equals n big-integer Montgomery squarings, canonical; the same
    edge operands, and random ones (fewer for the long runs: a run costs n squarings)."""
    rnd = random.Random(1102 + n)
    cases = _edges() + [rnd.randrange(1 << 382) for _ in range(max(40, 2000 // n))]
    for a in cases:
        got = _run(routine, a, n)
        assert got == _sqr_n(a, n) and got < g.P, (n, hex(a))


def test_run_of_one_is_the_single_entry(routine):
    rnd = random.Random(1103)
    for a in _edges() + [rnd.randrange(1 << 382) for _ in range(200)]:
        assert _run(routine, a, 1) == _single(routine, a)


def _bound(reg):
    """The largest value of a register a mad of the squaring reads: p's limbs exactly, the operand's top limb < 2^30,
    D_11 = a_11 << 1 | a_10 >> 31 < 2^31 (v23), every other limb, quotient digit, D_k and E_k up to 2^32 - 1."""
    if reg.startswith("s"):
        return (g.P >> (32 * (int(reg[1:]) - 16))) & 0xFFFFFFFF
    return {"v11": g.TOP_BOUND, "v23": 2 * g.TOP_BOUND + 1}.get(reg, 0xFFFFFFFF)


def test_carry_elision_bound_walk():
    """The independent bound walk over the squaring's column sums: no mad without a v_addc behind it can overflow its
    64-bit accumulator, and every other mad's carry is caught."""
    body = g.gen_sqr()
    free = _symbolic_max(body, _bound)
    mads = sum(x.startswith("v_mad_u64_u32") for x in body)
    assert free >= 50 and sum(x.startswith("v_addc") for x in body) == mads - free


def test_extreme_operands_keep_every_carry(routine):
    """Operands at the elision's limits in the strict interpreter, single and run entry."""
    ext = [TOP, TOP - 1, 0x3FFFFFFF << 352, (1 << 352) - 1, 2 * g.P - 1, 2 * g.P, g.P - 1,
           (0x340223D4 << 352) | ((1 << 352) - 1), TOP ^ 1, TOP ^ (1 << 351)]
    for a in ext:
        assert _single(routine, a) == a * a * R_INV % g.P
        assert _run(routine, a, 2) == _sqr_n(a, 2)


def test_strict_interpreter_is_live_on_the_squaring():
    """Removing a carry-catching v_addc from the squaring makes the interpreter raise on the largest operand."""
    body = g.gen_sqr()
    ks = [i for i, x in enumerate(body) if x.startswith("v_addc_co_u32_e32")]
    k = ks[len(ks) // 2]
    with pytest.raises(g.DroppedCarry):
        g.emulate(body[:k] + body[k + 1:], _limbs(TOP), _limbs(0))


def test_writes_stay_inside_the_declared_clobbers(routine):
    """Every destination of the routine is v0-v39, vcc, scc (implicit in s_sub_u32) or the run count: nothing
    else is written, and p's SGPRs (s16-s28) and the return address (s30/s31) are only read."""
    written = set()
    for ins in routine:
        if ins.endswith(":") or ins.startswith(("s_cbranch", "s_setpc")):
            continue
        op, rest = ins.split(" ", 1)
        o = [t.strip() for t in rest.split(",")]
        dsts = [o[0]] + ([o[1]] if op in ("v_mad_u64_u32", "v_sub_co_u32_e32", "v_subb_co_u32_e32", "v_add_co_u32_e32",
                                         "v_addc_co_u32_e32", "v_addc_co_u32_e64") else [])
        for d in dsts:
            written.update(g.regs_of(d) or [d])
    vg = {r for r in written if r.startswith("v") and r != "vcc"}
    assert vg <= {"v%d" % k for k in range(40)}
    assert {"v%d" % k for k in range(12)} <= vg
    assert written - vg == {"vcc", g.SQR_RUN_SGPR}
    assert g.SQR_RUN_SGPR not in ["s%d" % k for k in list(range(16, 29)) + [30, 31, 36, 37]]
