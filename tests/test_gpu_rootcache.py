"""The device-resident root cache of the wire-format fused Verify (charon_amd/csrc/rootcache.h):
statuses with the cache off, cold and warm are the same integers, the counters tell which path every eligible item
took, a cached H(m) is only ever served for the 32 bytes it was computed from, and a full table is emptied.

Kernels covered: k_root_lookup and k_verify_fused (PAIR_SINGLE).  Shapes stay at or below 256 items.  Every call goes
through hipbls_verify_batch_device with a status buffer that starts at -7: no -7 may remain, so the lookup's order is
a permutation of the items.
"""
import ctypes
import random
import threading

import pytest

from tests.test_gpu_keycache import _bad_keys

pytestmark = pytest.mark.gpu

R_ORDER = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
DEFAULT_SLOTS = 262144
SIZES = (1, 63, 64, 65, 130)  # partial wave, exact wave, wave boundary, three waves
N_KEYS = 20
UNSET = -7


@pytest.fixture(scope="module")
def impl():
    from charon_amd.tbls import PAIR_AUTO, PAIR_SINGLE, HipBLS
    h = HipBLS()
    h.set_pair_mode(PAIR_SINGLE)
    yield h
    h.set_pair_mode(PAIR_AUTO)
    h.rootcache_config(DEFAULT_SLOTS)


class DevBatch:
    """A wire-format batch in device memory and one device call over it."""

    def __init__(self, pks, msgs, sigs, stream=None):
        import torch
        self.dev = torch.device("cuda", 0)
        self.n = len(pks)
        offs = [0]
        for m in msgs:
            offs.append(offs[-1] + len(m))

        def u8(blob):
            return torch.frombuffer(bytearray(blob if blob else b"\0"), dtype=torch.uint8).to(self.dev)

        self.pk, self.sig, self.msg = u8(b"".join(pks)), u8(b"".join(sigs)), u8(b"".join(msgs))
        self.off = torch.tensor(offs, dtype=torch.int64).to(self.dev)
        self.stream = stream or torch.cuda.Stream(self.dev)

    def launch(self, impl):
        """Enqueue one call; returns (rc, status tensor)."""
        import torch
        st = torch.full((self.n,), UNSET, dtype=torch.int32, device=self.dev)
        torch.cuda.synchronize(self.dev)
        rc = impl.lib.hipbls_verify_batch_device(self.pk.data_ptr(), self.msg.data_ptr(), self.off.data_ptr(),
                                                 self.sig.data_ptr(), self.n, st.data_ptr(),
                                                 ctypes.c_void_p(self.stream.cuda_stream))
        return rc, st

    def run(self, impl):
        import torch
        rc, st = self.launch(impl)
        assert rc == 0
        torch.cuda.synchronize(self.dev)
        out = st.cpu().tolist()
        assert UNSET not in out, out
        return out


def _reaches_hash(pk_bad, sig):
    """Whether the fused chain gets as far as H(m) for an item: a valid key and a signature that decodes onto the
    curve (its G2 membership comes later, from the Miller loop) and is not infinity."""
    from oracle import bls12381 as bls
    if pk_bad:
        return False
    try:
        return bls.g2_decompress(sig, subgroup_check=False) is not None
    except bls.BLSError:
        return False


@pytest.fixture(scope="module")
def items(impl):
    """130 items with distinct 32-byte roots: valid ones over 20 keys, wrong roots, swapped shares, flipped signature
    bits and every bad key encoding.  `hashed[i]`: whether item i reaches the hash."""
    rng = random.Random(20251)
    sks = [rng.randrange(1, R_ORDER).to_bytes(32, "big") for _ in range(N_KEYS)]
    keys, st = impl.secret_to_public_key_batch(sks)
    assert set(st) == {0}
    n = max(SIZES)
    owner = [i % N_KEYS for i in range(n)]
    msgs = [rng.randbytes(32) for _ in range(n)]
    sigs, st = impl.sign_batch([sks[o] for o in owner], msgs)
    assert set(st) == {0}
    pks, sigs = [keys[o] for o in owner], list(sigs)
    bad = _bad_keys(keys[0])
    bad_key = [False] * n
    for i in range(n):
        kind = i % 13
        if kind == 3:
            msgs[i] = rng.randbytes(32)                    # wrong root
        elif kind == 6 and i + 1 < n:
            sigs[i] = sigs[i + 1]                          # swapped share
        elif kind == 9:
            b = bytearray(sigs[i])
            b[40] ^= 0x04                                  # flipped signature bit
            sigs[i] = bytes(b)
        elif kind == 11:
            pks[i] = bad[(i // 13) % len(bad)][1]           # a key error comes before the hash
            bad_key[i] = True
    assert len(set(msgs)) == n
    hashed = [_reaches_hash(bad_key[i], sigs[i]) for i in range(n)]
    assert 0 < sum(hashed) < n and hashed[0]
    return dict(pks=pks, msgs=msgs, sigs=sigs, hashed=hashed, sks=sks, keys=keys)


def _fresh(impl, items, count, seed):
    """`count` valid items over fresh random 32-byte roots, one of them with a swapped share."""
    rng = random.Random(seed)
    owner = [i % N_KEYS for i in range(count)]
    msgs = [rng.randbytes(32) for _ in range(count)]
    sigs, st = impl.sign_batch([items["sks"][o] for o in owner], msgs)
    assert set(st) == {0}
    sigs = list(sigs)
    if count > 8:
        sigs[7] = sigs[8]
    return [items["keys"][o] for o in owner], msgs, sigs


# ---------------------------------------------------------------- 1: off = cold = warm, and the counters
def test_off_cold_warm_equal_and_stats(impl, items):
    from oracle import bls12381 as bls
    for n in SIZES:
        pks, msgs, sigs = items["pks"][:n], items["msgs"][:n], items["sigs"][:n]
        b = DevBatch(pks, msgs, sigs)
        impl.rootcache_config(0)
        off = b.run(impl)
        assert impl.rootcache_stats() == (0, 0, 0, 0)
        impl.rootcache_config(DEFAULT_SLOTS)
        cold = b.run(impl)
        s_cold = impl.rootcache_stats()
        warm = b.run(impl)
        s_warm = impl.rootcache_stats()
        assert cold == off and warm == off, n
        reached = sum(items["hashed"][:n])  # distinct roots: each one that reaches the hash is published once
        # cold: the lookup kernel ends before any insert of its call, so nothing hits; every item is eligible
        assert s_cold == (0, n, reached, 0), (n, s_cold)
        # warm: exactly the roots the cold call inserted are served; the others miss again and still publish nothing
        assert s_warm == (reached, n + (n - reached), reached, 0), (n, s_warm)
        if n == max(SIZES):
            sample = [0, 3, 6, 9, 11, 24]
            assert [off[i] for i in sample] == [bls.verify_status(pks[i], msgs[i], sigs[i]) for i in sample]
            assert set(off) >= {0, 1, 3}


# ---------------------------------------------------------------- 2: only 32-byte messages are eligible
def test_message_lengths_only_32_bytes_are_cached(impl, items):
    rng = random.Random(9)
    lengths = [0, 31, 32, 33, 64, 200, 32, 0, 200, 32, 31, 33]
    msgs = [rng.randbytes(k) for k in lengths]
    msgs[7] = b""  # the empty message twice
    owner = [i % N_KEYS for i in range(len(msgs))]
    sigs, st = impl.sign_batch([items["sks"][o] for o in owner], msgs)
    assert set(st) == {0}
    sigs = list(sigs)
    sigs[4], sigs[5] = sigs[5], sigs[4]  # two long messages fail
    pks = [items["keys"][o] for o in owner]
    b = DevBatch(pks, msgs, sigs)
    c32 = lengths.count(32)
    impl.rootcache_config(0)
    off = b.run(impl)
    assert off == [0, 0, 0, 0, 3, 3] + [0] * 6
    impl.rootcache_config(DEFAULT_SLOTS)
    assert b.run(impl) == off
    assert impl.rootcache_stats() == (0, c32, c32, 0)
    assert b.run(impl) == off
    assert impl.rootcache_stats() == (c32, c32, c32, 0)


# ---------------------------------------------------------------- 3: roots that differ in one bit
def test_near_equal_roots_never_share_an_entry(impl, items):
    pk, sk = items["keys"][0], items["sks"][0]
    A = bytes(range(32))
    B = A[:31] + bytes([A[31] ^ 1])
    (sigA,), st = impl.sign_batch([sk], [A])
    assert st == [0]
    ab = DevBatch([pk, pk], [A, B], [sigA, sigA])
    ba = DevBatch([pk, pk], [B, A], [sigA, sigA])
    impl.rootcache_config(DEFAULT_SLOTS)
    assert ab.run(impl) == [0, 3]   # cold
    assert impl.rootcache_stats() == (0, 2, 2, 0)
    assert ab.run(impl) == [0, 3]   # warm: each root finds its own entry
    assert ba.run(impl) == [3, 0]
    assert impl.rootcache_stats() == (4, 2, 2, 0)
    impl.rootcache_config(DEFAULT_SLOTS)
    assert ba.run(impl) == [3, 0]   # the other order, cold
    assert ab.run(impl) == [0, 3]
    assert impl.rootcache_stats() == (2, 2, 2, 0)


# ---------------------------------------------------------------- 4: one root, 64 times, one wave
def test_one_root_64_times_in_a_cold_wave_inserts_once(impl, items):
    b = DevBatch([items["pks"][0]] * 64, [items["msgs"][0]] * 64, [items["sigs"][0]] * 64)
    impl.rootcache_config(DEFAULT_SLOTS)
    assert b.run(impl) == [0] * 64
    assert impl.rootcache_stats() == (0, 64, 1, 0)
    assert b.run(impl) == [0] * 64
    assert impl.rootcache_stats() == (64, 64, 1, 0)


# ---------------------------------------------------------------- 5: hits to the front, the rest to the back
def test_partition_of_alternating_warm_and_new_roots(impl, items):
    wp, wm, ws = _fresh(impl, items, 65, 501)
    np_, nm, ns = _fresh(impl, items, 65, 502)
    pks, msgs, sigs = [], [], []
    for i in range(65):
        pks += [wp[i], np_[i]]
        msgs += [wm[i], nm[i]]
        sigs += [ws[i], ns[i]]
    mixed = DevBatch(pks, msgs, sigs)
    impl.rootcache_config(0)
    off = mixed.run(impl)
    assert off.count(3) == 2 and off.count(0) == 128
    impl.rootcache_config(DEFAULT_SLOTS)
    DevBatch(wp, wm, ws).run(impl)
    assert impl.rootcache_stats() == (0, 65, 65, 0)
    assert mixed.run(impl) == off
    assert impl.rootcache_stats() == (65, 130, 130, 0)


# ---------------------------------------------------------------- 6: a full table is emptied, never overwritten
def test_tiny_table_rolls_over(impl, items):
    batches = [DevBatch(*_fresh(impl, items, 40, 600 + k)) for k in range(3)]
    impl.rootcache_config(0)
    off = [b.run(impl) for b in batches]
    assert all(o == [0] * 7 + [3] + [0] * 32 for o in off)
    try:
        impl.rootcache_config(8)
        last = 0
        for k, b in enumerate(batches):
            assert b.run(impl) == off[k], k
            hits, misses, inserts, rollovers = impl.rootcache_stats()
            # a call lies within one generation (the table is only emptied before a call): eight slots, eight inserts
            assert 1 <= inserts - last <= 8, (k, inserts, last)
            assert hits == 0 and misses == 40 * (k + 1)
            last = inserts
        assert rollovers >= 1
        # what the last generation holds is still served, statuses unchanged
        assert batches[2].run(impl) == off[2]
        assert impl.rootcache_stats()[3] >= rollovers
    finally:
        impl.rootcache_config(DEFAULT_SLOTS)


# ---------------------------------------------------------------- 7: racing inserts and lookups
def test_racing_inserts_and_lookups_on_four_streams(impl, items):
    """Once, not in a loop: four threads, three device calls each on their own streams, overlapping root sets."""
    import torch
    n = 130
    batches = []
    impl.rootcache_config(0)
    for t in range(4):
        r = 13 * t  # the same roots at other positions and in other waves
        b = DevBatch(items["pks"][r:] + items["pks"][:r], items["msgs"][r:] + items["msgs"][:r],
                     items["sigs"][r:] + items["sigs"][:r])
        b.want = b.run(impl)
        b.rc, b.st = [], []
        batches.append(b)
    impl.rootcache_config(DEFAULT_SLOTS)  # cleared: the twelve calls race to fill it

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
    hits, misses, inserts, rollovers = impl.rootcache_stats()
    assert hits + misses == 12 * n and rollovers == 0
    assert inserts == sum(items["hashed"])  # write-once: each root that reached the hash is published exactly once


# ---------------------------------------------------------------- 8: config beside the submission queue's wire launches
def test_config_resizes_beside_queued_verifies(impl, items):
    """hipbls_rootcache_config (other sizes, off, on) from one thread while another sends ten Verify calls through the
    submission queue, whose worker launches wire batches without the context lock.  Once, not in a loop."""
    k = 10
    pks, msgs, sigs = items["pks"][:k], items["msgs"][:k], items["sigs"][:k]
    impl.rootcache_config(0)
    want = DevBatch(pks, msgs, sigs).run(impl)
    impl.rootcache_config(DEFAULT_SLOTS)
    got, errs = [], []

    def caller():
        try:
            for p, m, s in zip(pks, msgs, sigs):
                got.append(impl.verify_queued(p, m, s))
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    def resizer():
        try:
            for slots in (8, 0, 1024, 16, 0, DEFAULT_SLOTS):
                impl.rootcache_config(slots)
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    th = [threading.Thread(target=caller), threading.Thread(target=resizer)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errs, errs
    assert got == want
    assert DevBatch(pks, msgs, sigs).run(impl) == want
