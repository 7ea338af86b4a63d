"""The device Fp squaring routine (bls_fp_sqr_rt / bls_fp_sqr_run_rt, tools/gen_fp_asm.py gen_sqr) on the GPU.

* One wave (64 lanes) of tests/native/libfp_units.so: fp_sqr and runs of n in {1, 2, 63} on edge, lazy and random
  operands == fp_mul(a, a) on the same lanes == Python integers, limb for limb; a run == n single calls.
* fp_pow for the two square-root exponents ((p + 1)/4 and (p - 3)/4, whose squarings now go in runs) on squares and
  non-squares == the host build's fp_pow == Python's pow.
* A 65-item wire-format Verify batch (one full wave plus one lane): valid items, the benchmark's three corruptions, a
  signature with x >= p, one off the curve, one on the curve outside G2, an infinity key.  Statuses == the oracle's
  (tests/golden/fp_sqr_verify_batch.json holds the batch and oracle/bls12381.py's verify_status of every item,
  recorded once: the oracle takes 0.6 s per item) == the host build's op_verify, through hipbls_verify_batch and
  through hipbls_batch_verify_rlc_device in both RLC modes.
"""
import ctypes
import json
import os
import random

import pytest

gpu = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
R = 1 << 384
R_INV = pow(R, -1, P)
TOP = (1 << 382) - 1
LANES = 64
OP_SQR, OP_MUL_AA, OP_SQR_RUN, OP_SQR_CALLS, OP_POW_SQRT, OP_POW_SQRT_M1 = range(6)


def _pack(vals):
    return (ctypes.c_uint32 * (12 * len(vals)))(*[(x >> (32 * k)) & 0xFFFFFFFF for x in vals for k in range(12)])


def _unpack(buf, n):
    return [sum(buf[12 * i + k] << (32 * k) for k in range(12)) for i in range(n)]


@pytest.fixture(scope="module")
def G():
    from tests.fp_units import gpu_lib
    return gpu_lib()


def _gpu(G, vals, op, n=0):
    out = (ctypes.c_uint32 * (12 * len(vals)))()
    assert G.fpu_run(_pack(vals), out, len(vals), op, n) == 0
    return _unpack(out, len(vals))


def _operands():
    """64 operands below 2^382: the edges of the CPU test, lazy values in [p, 2^382) and seeded random ones."""
    e = [0, 1, R % P, P - 1, P, 2 * P - 1, TOP, TOP - 1, P + 1, 2 * P, 1 << 381, 0x3FFFFFFF << 352]
    e += [0xFFFFFFFF << (32 * k) for k in (0, 5, 10)] + [0x80000000 << (32 * k) for k in (0, 6, 10)]
    e += [sum(0xFFFFFFFF << (32 * k) for k in range(0, 12, 2)), sum(0xFFFFFFFF << (32 * k) for k in range(1, 11, 2)),
          sum(0x80000000 << (32 * k) for k in range(11))]
    rnd = random.Random(1104)
    e += [rnd.randrange(P, 1 << 382) for _ in range(12)]
    e += [rnd.randrange(1 << 382) for _ in range(LANES - len(e))]
    assert len(e) == LANES and all(0 <= x <= TOP for x in e)
    return e


def _sqr_n(a, n):
    for _ in range(n):
        a = a * a * R_INV % P
    return a


@gpu
def test_single_squaring_one_wave(G):
    a = _operands()
    got = _gpu(G, a, OP_SQR)
    assert got == _gpu(G, a, OP_MUL_AA)
    assert got == [x * x * R_INV % P for x in a]


@gpu
@pytest.mark.parametrize("n", [1, 2, 63])
def test_squaring_run_one_wave(G, n):
    a = _operands()
    got = _gpu(G, a, OP_SQR_RUN, n)
    assert got == _gpu(G, a, OP_SQR_CALLS, n)
    assert got == [_sqr_n(x, n) for x in a]
    if n == 1:
        assert got == _gpu(G, a, OP_MUL_AA)


@gpu
def test_partial_wave_and_second_block(G):
    """65 lanes: a full wave and a one-lane wave (the run count is read from the first active lane)."""
    a = _operands() + [TOP]
    assert _gpu(G, a, OP_SQR_RUN, 5) == [_sqr_n(x, 5) for x in a]
    assert _gpu(G, a, OP_SQR) == [x * x * R_INV % P for x in a]


@gpu
@pytest.mark.parametrize("minus1", [0, 1])
def test_fp_pow_square_root_chains(G, minus1):
    """a^((p + 1)/4) and a^((p - 3)/4) in Montgomery form on 64 lanes: 0, 1, p - 1, squares and non-squares."""
    from tests.fp_units import host_lib
    rnd = random.Random(1105 + minus1)
    plain = [0, 1, P - 1, 4, P - 4]
    plain += [pow(rnd.randrange(2, P), 2, P) for _ in range(29)]
    while len(plain) < LANES:
        x = rnd.randrange(2, P)
        if pow(x, (P - 1) // 2, P) == P - 1:
            plain.append(x)
    assert any(pow(x, (P - 1) // 2, P) == 1 for x in plain) and len(plain) == LANES
    mont = [x * R % P for x in plain]
    got = _gpu(G, mont, OP_POW_SQRT_M1 if minus1 else OP_POW_SQRT)
    host = (ctypes.c_uint32 * (12 * LANES))()
    host_lib().fpuh_pow(_pack(mont), host, LANES, minus1)
    assert got == _unpack(host, LANES)
    e = (P - 3) // 4 if minus1 else (P + 1) // 4
    assert got == [pow(x, e, P) * R % P for x in plain]


# ---------------------------------------------------------------- the 65-item Verify batch
@pytest.fixture(scope="module")
def batch():
    with open(os.path.join(ROOT, "tests", "golden", "fp_sqr_verify_batch.json")) as f:
        items = json.load(f)["items"]
    assert len(items) == 65
    kinds = {it["kind"] for it in items}
    assert kinds == {"valid", "wrong_root", "swapped_share", "flipped_bit", "sig_x_ge_p", "sig_off_curve",
                     "sig_not_in_g2", "infinity_key"}
    b = lambda k: [bytes.fromhex(it[k]) for it in items]
    return b("pk"), b("msg"), b("sig"), [it["status"] for it in items]


@pytest.fixture(scope="module")
def impl():
    from charon_amd.tbls import RLC_AUTO, HipBLS
    h = HipBLS(device=0)
    yield h
    h.set_rlc_mode(RLC_AUTO)


def test_verify_batch_host_equals_oracle(batch):
    """No GPU: the host build's op_verify agrees with the recorded oracle statuses on every item."""
    from tests.hostlib import lib
    L = lib()
    pks, msgs, sigs, want = batch
    assert [L.ht_verify(p, m, len(m), s) for p, m, s in zip(pks, msgs, sigs)] == want


@gpu
def test_verify_batch_statuses(impl, batch):
    pks, msgs, sigs, want = batch
    assert impl.batch_verify_status(pks, msgs, sigs) == want  # key cache cold
    assert impl.batch_verify_status(pks, msgs, sigs) == want  # and warm


@gpu
@pytest.mark.parametrize("rlc_mode", ["windows", "batch"])
def test_verify_batch_through_rlc_device(impl, batch, rlc_mode):
    import torch
    from charon_amd.tbls import RLC_BATCH, RLC_WINDOWS
    pks, msgs, sigs, want = batch
    n = len(pks)
    dev = torch.device("cuda", 0)
    u8 = lambda parts: torch.frombuffer(bytearray(b"".join(parts)), dtype=torch.uint8).to(dev)
    d_pk, d_sig, d_msg = u8(pks), u8(sigs), u8(msgs)
    d_midx = torch.arange(n, dtype=torch.int32).to(dev)
    d_off = torch.arange(0, 32 * (n + 1), 32, dtype=torch.int64).to(dev)
    d_st = torch.full((n,), -7, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    prev = impl.set_rlc_mode({"windows": RLC_WINDOWS, "batch": RLC_BATCH}[rlc_mode])
    try:
        rc = impl.lib.hipbls_batch_verify_rlc_device(d_pk.data_ptr(), d_sig.data_ptr(), d_midx.data_ptr(), n,
                                                     d_msg.data_ptr(), d_off.data_ptr(), n, bytes(range(32)),
                                                     d_st.data_ptr(), ctypes.c_void_p(stream.cuda_stream))
        assert rc == 0
        torch.cuda.synchronize(dev)
        assert d_st.cpu().tolist() == want
    finally:
        impl.set_rlc_mode(prev)
