"""The fused Verify's shortened final exponentiation on the device (charon_amd/csrc/pairing_lds.h): the
hybrid a^|x| (and, in a -DBLS_FE_CMP=1 build, the comparison in place of the last product) gives the statuses the
oracle gives and the ones the prep + pair route gives (its kernels keep the six-state power).

Kernels covered: k_verify_fused_lines (recording cold, replaying warm) and, lines off, k_verify_fused, under
PAIR_SINGLE; k_verify_prep + k_verify_pair_lg2 under PAIR_LANES as the second reference.  One batch of 130 items (three
waves, the last partial) through hipbls_verify_batch_device, five calls in all.
"""
import random

import pytest

from tests.test_gpu_rootcache import DEFAULT_SLOTS, N_KEYS, R_ORDER, DevBatch
from tests.test_gpu_rootlines import G1_INF, G2_INF, _non_g2

pytestmark = pytest.mark.gpu

N = 130
KINDS = {3: "wrong root", 5: "swapped key", 7: "flipped bit", 9: "non-G2 signature", 11: "infinity key",
         12: "infinity signature"}  # by i % 13; every other item is valid


@pytest.fixture(scope="module")
def impl():
    from charon_amd.tbls import PAIR_AUTO, PAIR_SINGLE, HipBLS
    h = HipBLS()
    h.set_pair_mode(PAIR_SINGLE)
    yield h
    h.set_pair_mode(PAIR_AUTO)
    h.rootcache_config(DEFAULT_SLOTS)
    h.rootcache_lines_config(None)


@pytest.fixture(scope="module")
def items(impl):
    rng = random.Random(18057)
    sks = [rng.randrange(1, R_ORDER).to_bytes(32, "big") for _ in range(N_KEYS)]
    keys, st = impl.secret_to_public_key_batch(sks)
    assert set(st) == {0}
    owner = [i % N_KEYS for i in range(N)]
    msgs = [rng.randbytes(32) for _ in range(N)]
    sigs, st = impl.sign_batch([sks[o] for o in owner], msgs)
    assert set(st) == {0}
    pks, sigs = [keys[o] for o in owner], list(sigs)
    non_g2 = _non_g2(sigs[9])
    for i in range(N):
        kind = KINDS.get(i % 13)
        if kind == "wrong root":
            msgs[i] = rng.randbytes(32)
        elif kind == "swapped key":
            pks[i] = keys[(owner[i] + 1) % N_KEYS]
        elif kind == "flipped bit":
            b = bytearray(sigs[i])
            b[40] ^= 0x04
            sigs[i] = bytes(b)
        elif kind == "non-G2 signature":
            sigs[i] = non_g2
        elif kind == "infinity key":
            pks[i] = G1_INF
        elif kind == "infinity signature":
            sigs[i] = G2_INF
    assert len(set(msgs)) == N
    return pks, msgs, sigs


def test_fused_statuses_lines_on_off_cold_warm(impl, items):
    from charon_amd.tbls import PAIR_LANES, PAIR_SINGLE
    from oracle import bls12381 as bls
    pks, msgs, sigs = items
    b = DevBatch(pks, msgs, sigs)
    got = {}
    try:
        impl.rootcache_config(0)
        impl.rootcache_config(DEFAULT_SLOTS)      # an empty table
        impl.rootcache_lines_config(None)
        got["lines cold"] = b.run(impl)
        got["lines warm"] = b.run(impl)
        hits, published = impl.rootcache_lines_stats()[:2]
        assert published > 64 and hits == published  # the pairing-bound items recorded, then every one replayed
        impl.rootcache_config(DEFAULT_SLOTS)
        impl.rootcache_lines_config(0)            # as HIPBLS_ROOTCACHE_LINES=0: k_verify_fused
        got["no lines cold"] = b.run(impl)
        got["no lines warm"] = b.run(impl)
        assert impl.rootcache_lines_stats() == (0, 0, 0, 0)
        assert impl.rootcache_stats()[0] == published
        impl.set_pair_mode(PAIR_LANES)
        pair = b.run(impl)
    finally:
        impl.set_pair_mode(PAIR_SINGLE)
    for name, st in got.items():
        assert st == pair, name
    # the oracle on one item of each kind; every item of a kind has that status, the valid ones 0
    by_kind = {}
    for i in (0, 3, 5, 7, 9, 11, 12):
        by_kind[KINDS.get(i % 13)] = bls.verify_status(pks[i], msgs[i], sigs[i])
    assert by_kind[None] == 0 and by_kind["wrong root"] == 3 and by_kind["swapped key"] == 3
    assert pair == [by_kind[KINDS.get(i % 13)] for i in range(N)]
