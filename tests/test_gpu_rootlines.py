"""The root cache's line blocks in the wire-format fused Verify (charon_amd/csrc/rootcache.h): a root
whose Miller-loop lines were recorded by the lane that published it is verified by replaying them, with the same
statuses as the full loop gives, and the counters tell which lanes recorded, replayed or met a full pool.

Kernels covered: k_root_lookup, k_verify_fused_lines and (lines off) k_verify_fused, under PAIR_SINGLE.  Shapes stay at or below 256 items; every test is a
few calls of at most four waves.  Calls go through hipbls_verify_batch_device with a status buffer that starts at -7.
"""
import random
import threading

import pytest

from tests.test_gpu_keycache import _bad_keys
from tests.test_gpu_rootcache import DEFAULT_SLOTS, N_KEYS, R_ORDER, DevBatch, _fresh, _reaches_hash

pytestmark = pytest.mark.gpu

G2_INF = bytes([0xC0]) + bytes(95)
G1_INF = bytes([0xC0]) + bytes(47)


@pytest.fixture(scope="module")
def impl():
    from charon_amd.tbls import PAIR_AUTO, PAIR_SINGLE, HipBLS
    h = HipBLS()
    h.set_pair_mode(PAIR_SINGLE)
    yield h
    h.set_pair_mode(PAIR_AUTO)
    h.rootcache_config(DEFAULT_SLOTS)
    h.rootcache_lines_config(None)


def _non_g2(sig):
    """A signature's bytes with one bit flipped so that they still decode onto the curve (then outside G2)."""
    from oracle import bls12381 as bls
    for bit in range(8, 768):
        b = bytearray(sig)
        b[bit // 8] ^= 1 << (bit % 8)
        try:
            if bls.g2_decompress(bytes(b), subgroup_check=False) is not None:
                return bytes(b)
        except bls.BLSError:
            pass
    raise AssertionError("no flipped bit decodes")


@pytest.fixture(scope="module")
def items(impl):
    """192 items with distinct 32-byte roots: valid ones over 20 keys, wrong roots, swapped shares, flipped signature
    bits, bad key encodings, signatures on the curve outside G2 and the infinity key and signature.  `reach[i]`:
    whether item i gets as far as H(m) and the pairing."""
    rng = random.Random(31017)
    sks = [rng.randrange(1, R_ORDER).to_bytes(32, "big") for _ in range(N_KEYS)]
    keys, st = impl.secret_to_public_key_batch(sks)
    assert set(st) == {0}
    n = 192
    owner = [i % N_KEYS for i in range(n)]
    msgs = [rng.randbytes(32) for _ in range(n)]
    sigs, st = impl.sign_batch([sks[o] for o in owner], msgs)
    assert set(st) == {0}
    pks, sigs = [keys[o] for o in owner], list(sigs)
    bad = _bad_keys(keys[0])
    bad_key = [False] * n
    non_g2 = _non_g2(sigs[5])
    for i in range(n):
        kind = i % 16
        if kind == 3:
            msgs[i] = rng.randbytes(32)                    # wrong root
        elif kind == 6 and i + 1 < n:
            sigs[i] = sigs[i + 1]                          # swapped share
        elif kind == 9:
            b = bytearray(sigs[i])
            b[40] ^= 0x04                                  # flipped signature bit
            sigs[i] = bytes(b)
        elif kind == 11:
            pks[i] = bad[(i // 16) % len(bad)][1]           # a key error comes before the hash
            bad_key[i] = True
        elif kind == 13:
            sigs[i] = non_g2                               # reaches the pairing; the Miller loop's T1 rejects it
        elif kind == 14:
            sigs[i] = G2_INF
        elif kind == 15:
            pks[i] = G1_INF
    assert len(set(msgs)) == n
    reach = [_reaches_hash(bad_key[i], sigs[i]) and sigs[i] != G2_INF and pks[i] != G1_INF for i in range(n)]
    assert 100 < sum(reach) < n
    return dict(pks=pks, msgs=msgs, sigs=sigs, reach=reach, sks=sks, keys=keys)


def _delta(after, before):
    return tuple(a - b for a, b in zip(after, before))


# ---------------------------------------------------------------- 1: four configurations, one set of statuses
def test_off_cold_warm_equal_and_line_stats(impl, items):
    from oracle import bls12381 as bls
    pks, msgs, sigs = items["pks"], items["msgs"], items["sigs"]
    b = DevBatch(pks, msgs, sigs)
    reached = sum(items["reach"])
    impl.rootcache_config(0)
    off = b.run(impl)
    impl.rootcache_config(DEFAULT_SLOTS)
    impl.rootcache_lines_config(0)
    nolines = b.run(impl)
    assert impl.rootcache_lines_stats() == (0, 0, 0, 0)
    assert impl.rootcache_stats() == (0, 192, reached, 0)
    impl.rootcache_lines_config(None)
    cold = b.run(impl)
    assert impl.rootcache_stats() == (0, 192, reached, 0)
    assert impl.rootcache_lines_stats() == (0, reached, 0, 0)   # every H insert came with its block
    warm = b.run(impl)
    assert impl.rootcache_stats()[0] == reached
    assert impl.rootcache_lines_stats() == (reached, reached, 0, 0)  # every cached root that reaches the pairing replays
    assert nolines == off and cold == off and warm == off
    assert set(off) >= {0, 1, 2, 3}
    sample = [0, 3, 6, 9, 11, 13, 14, 15, 29, 191]
    assert [off[i] for i in sample] == [bls.verify_status(pks[i], msgs[i], sigs[i]) for i in sample]


# ---------------------------------------------------------------- 2: one root, 64 times, one wave
def test_one_root_64_times_publishes_one_block(impl, items):
    b = DevBatch([items["pks"][0]] * 64, [items["msgs"][0]] * 64, [items["sigs"][0]] * 64)
    impl.rootcache_lines_config(None)
    assert b.run(impl) == [0] * 64
    assert impl.rootcache_stats() == (0, 64, 1, 0)
    assert impl.rootcache_lines_stats() == (0, 1, 0, 0)
    assert b.run(impl) == [0] * 64
    assert impl.rootcache_lines_stats() == (64, 1, 0, 0)


# ---------------------------------------------------------------- 3: replaying lanes and full lanes in one call
def test_alternating_warm_and_new_roots(impl, items):
    wp, wm, ws = _fresh(impl, items, 64, 701)
    np_, nm, ns = _fresh(impl, items, 64, 702)
    pks, msgs, sigs = [], [], []
    for i in range(64):
        pks += [wp[i], np_[i]]
        msgs += [wm[i], nm[i]]
        sigs += [ws[i], ns[i]]
    mixed = DevBatch(pks, msgs, sigs)
    impl.rootcache_config(0)
    off = mixed.run(impl)
    assert off.count(3) == 2 and off.count(0) == 126
    impl.rootcache_config(DEFAULT_SLOTS)
    DevBatch(wp, wm, ws).run(impl)
    assert impl.rootcache_lines_stats() == (0, 64, 0, 0)
    assert mixed.run(impl) == off
    # the 64 warm roots replay (dealt to the front: one whole wave of replaying lanes), the 64 new ones record
    assert impl.rootcache_stats() == (64, 128, 128, 0)
    assert impl.rootcache_lines_stats() == (64, 128, 0, 0)
    assert mixed.run(impl) == off
    assert impl.rootcache_lines_stats() == (192, 128, 0, 0)


# ---------------------------------------------------------------- 4: a small pool fills; a rollover hands it out again
def test_small_pool_fills_and_rolls_over(impl, items):
    """64 slots, 4 blocks, 40 new roots.  A generation of a 64-slot table ends at 32 inserts, so the 40 roots come in
    two calls (24, then 16): the replay of the pool's four blocks is observed between them, within the generation.
    A wave replays only when every lane of it has a block (rootcache.h rl_wave_all), so "exactly those four replay"
    is observed with each root in a call of its own: four of the 24 calls replay, and the 24 together in one wave run
    the full loop."""
    pks, msgs, sigs = _fresh(impl, items, 40, 801)
    first = DevBatch(pks[:24], msgs[:24], sigs[:24])
    second = DevBatch(pks[24:], msgs[24:], sigs[24:])
    impl.rootcache_config(0)
    off1, off2 = first.run(impl), second.run(impl)
    assert off1 == [0] * 7 + [3] + [0] * 16 and off2 == [0] * 16
    try:
        impl.rootcache_config(64)
        impl.rootcache_lines_config(4)
        assert first.run(impl) == off1
        ins = impl.rootcache_stats()[2]
        assert 4 < ins <= 24
        assert impl.rootcache_lines_stats() == (0, 4, ins - 4, 0)     # four blocks, then a full pool: H alone
        assert first.run(impl) == off1                                # 4 lanes with a block among 24: the full loop
        assert impl.rootcache_lines_stats() == (0, 4, ins - 4, 0)
        singles = [DevBatch(pks[i:i + 1], msgs[i:i + 1], sigs[i:i + 1]) for i in range(24)]

        def replaying():
            """How many of the 24 roots replay when each is verified in a call of its own."""
            before = impl.rootcache_lines_stats()
            assert [b.run(impl)[0] for b in singles] == off1
            after = impl.rootcache_lines_stats()
            assert after[1:] == before[1:]
            return after[0] - before[0]

        assert replaying() == 4                                       # exactly those four replay
        assert impl.rootcache_stats()[3] == 0
        assert second.run(impl) == off2                               # 16 more roots: the generation is over
        hits, misses, ins2, rollovers = impl.rootcache_stats()
        assert ins2 >= 32 and rollovers == 0
        s0 = impl.rootcache_lines_stats()
        assert s0[:2] == (4, 4) and s0[3] == 0
        ins_before = ins2
        assert first.run(impl) == off1                                # emptied before this call: nothing to replay,
        assert impl.rootcache_stats()[3] == 1                         # and the pool is handed out from its start
        s1 = impl.rootcache_lines_stats()
        assert _delta(s1, s0)[:2] == (0, 4) and s1[3] == 0
        assert impl.rootcache_stats()[2] - ins_before <= 24           # so this generation is not over yet
        assert replaying() == 4
        assert impl.rootcache_stats()[3] == 1 and impl.rootcache_lines_stats()[3] == 0
    finally:
        impl.rootcache_config(DEFAULT_SLOTS)
        impl.rootcache_lines_config(None)


# ---------------------------------------------------------------- 5: racing recorders and readers
def test_racing_lines_on_four_streams(impl, items):
    """Once, not in a loop: four threads, three device calls of 256 items each on their own streams, over one shared
    set of 128 roots at other positions."""
    import torch
    p, m, s = _fresh(impl, items, 128, 901)  # every one reaches the pairing (one fails there)
    batches = []
    impl.rootcache_config(0)
    for t in range(4):
        r = 29 * t
        b = DevBatch((p[r:] + p[:r]) * 2, (m[r:] + m[:r]) * 2, (s[r:] + s[:r]) * 2)
        b.want = b.run(impl)
        b.rc, b.st = [], []
        batches.append(b)
    impl.rootcache_config(DEFAULT_SLOTS)
    impl.rootcache_lines_config(None)

    def worker(b):
        for _ in range(3):
            rc, st = b.launch(impl)
            b.rc.append(rc)
            b.st.append(st)

    th = [threading.Thread(target=worker, args=(b,)) for b in batches]
    for x in th:
        x.start()
    for x in th:
        x.join()
    torch.cuda.synchronize(batches[0].dev)
    for b in batches:
        assert b.rc == [0, 0, 0]
        for st in b.st:
            assert st.cpu().tolist() == b.want
    assert impl.rootcache_stats()[2] == 128
    line_hits, published, pool_full, _ = impl.rootcache_lines_stats()
    # only the lane that wins a root's insert takes a block, so no race hands out more than one per root
    assert 128 <= published <= DEFAULT_SLOTS // 2 and published == 128 and pool_full == 0
    assert line_hits <= 12 * 256


# ---------------------------------------------------------------- 6: the host-buffer call and the submission queue
def test_host_call_and_queue_with_lines_on_and_off(impl, items):
    k = 70
    pks, msgs, sigs = items["pks"][:k], items["msgs"][:k], items["sigs"][:k]
    got = {}
    for name, blocks in (("off", 0), ("on", None)):
        impl.rootcache_lines_config(blocks)
        cold = impl.batch_verify_status(pks, msgs, sigs)
        warm = impl.batch_verify_status(pks, msgs, sigs)
        tickets = [impl.verify_submit(p, m, s) for p, m, s in zip(pks[:24], msgs[:24], sigs[:24])]
        queued = [impl.verify_wait(t) for t in tickets]
        got[name] = (cold, warm, queued)
        assert cold == warm and queued == cold[:24]
    assert got["on"] == got["off"]
    assert impl.rootcache_lines_stats()[0] > 0 and impl.rootcache_lines_stats()[3] == 0
