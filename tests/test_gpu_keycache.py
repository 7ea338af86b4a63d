"""The device-resident key cache of the wire-format Verify and RLC kernels (charon_amd/csrc/keycache.h, DESIGN.md
4.10): statuses with the cache off, cold and warm are the same integers, the counters tell which path every item
took, and entries are only ever written for valid keys, once.

Kernels covered: k_verify_fused (PAIR_SINGLE), k_verify_prep (PAIR_LANES), k_rlc_items (RLC_WINDOWS) and k_rlcb_items
(RLC_BATCH).  Shapes stay at or below 256 items.
"""
import ctypes
import json
import os
import random
import threading

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R_ORDER = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
DEFAULT_SLOTS = 65536
ERR_PUBKEY = 1
SIZES = (1, 63, 64, 65, 130)  # partial wave, exact wave, wave boundary, three waves
N_KEYS = 20


@pytest.fixture(scope="module")
def impl():
    from charon_amd.tbls import PAIR_AUTO, RLC_AUTO, HipBLS
    h = HipBLS()
    yield h
    h.set_pair_mode(PAIR_AUTO)
    h.set_rlc_mode(RLC_AUTO)
    h.keycache_config(DEFAULT_SLOTS)


def _bad_keys(valid):
    """(name, 48 bytes) of every kind of key that must never become an entry."""
    from oracle import bls12381 as bls
    with open(os.path.join(ROOT, "tests", "golden", "fixtures.json")) as f:
        off_subgroup = bytes.fromhex(json.load(f)["small_order"]["verify"][16]["pk"])
    x = int.from_bytes(bytes([valid[0] & 0x1F]) + valid[1:], "big")
    off_curve = None
    for d in range(1, 64):
        cand = (x + d).to_bytes(48, "big")
        cand = bytes([cand[0] | 0x80]) + cand[1:]
        try:
            bls.g1_decompress(cand, subgroup_check=False)
        except bls.BLSError:
            off_curve = cand
            break
    assert off_curve is not None
    return [("x_ge_p", bytes([0x9F]) + b"\xff" * 47), ("off_curve", off_curve), ("off_subgroup", off_subgroup),
            ("infinity", b"\xc0" + bytes(47)), ("no_compression_flag", bytes([valid[0] & 0x7F]) + valid[1:]),
            ("infinity_flag_with_x", bytes([valid[0] | 0x40]) + valid[1:]), ("infinity_with_sign", b"\xe0" + bytes(47))]


@pytest.fixture(scope="module")
def items(impl):
    """130 items: valid ones over 20 keys, wrong roots, swapped shares, flipped signature bits and every bad key
    encoding.  Returns dict(pks, msgs, sigs, bad_key=[bool], keys=[valid key bytes], bad=[(name, bytes)])."""
    rng = random.Random(20250)
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
            pks[i] = bad[(i // 13) % len(bad)][1]           # a key that cannot be an entry
            bad_key[i] = True
    assert sum(bad_key) >= len(bad) and not bad_key[0]
    return dict(pks=pks, msgs=msgs, sigs=sigs, bad_key=bad_key, keys=keys, bad=bad)


def _off_cold_warm(impl, pks, msgs, sigs, slots=DEFAULT_SLOTS):
    """Statuses with the cache off, then cleared and cold, then warm; and the counters after the cold and warm calls."""
    impl.keycache_config(0)
    off = impl.batch_verify_status(pks, msgs, sigs)
    assert impl.keycache_stats() == (0, 0, 0)
    impl.keycache_config(slots)
    cold = impl.batch_verify_status(pks, msgs, sigs)
    s_cold = impl.keycache_stats()
    warm = impl.batch_verify_status(pks, msgs, sigs)
    s_warm = impl.keycache_stats()
    return off, cold, warm, s_cold, s_warm


# ---------------------------------------------------------------- 1, 2: cold = warm = off, and the counters
@pytest.mark.parametrize("mode", ["single", "lanes"])
def test_cold_warm_off_equal_and_stats(impl, items, mode):
    from charon_amd.tbls import PAIR_LANES, PAIR_SINGLE
    from oracle import bls12381 as bls
    prev = impl.set_pair_mode({"single": PAIR_SINGLE, "lanes": PAIR_LANES}[mode])
    try:
        for n in SIZES:
            pks, msgs, sigs = items["pks"][:n], items["msgs"][:n], items["sigs"][:n]
            bad = items["bad_key"][:n]
            off, cold, warm, s_cold, s_warm = _off_cold_warm(impl, pks, msgs, sigs)
            assert cold == off and warm == off, (mode, n)
            n_valid = n - sum(bad)
            distinct = len({p for p, b in zip(pks, bad) if not b})
            # cold: every item decodes; each distinct valid key is published exactly once.  (misses == n holds because
            # these launches are at most three waves, all resident at once and all past their lookups before the
            # first insert lands; the design allows hits inside one kernel, so at larger shapes only
            # hits + misses == n and inserts == distinct are properties of the cache.)
            assert s_cold == (0, n, distinct), (mode, n, s_cold)
            # warm: every valid key is served from the cache; every other key takes the decode again, and nothing new
            # is published
            assert s_warm == (n_valid, n + sum(bad), distinct), (mode, n, s_warm)
            if n == max(SIZES):
                # every bad-key item: the key error (infinity: KeyValidate fails the check), cold and warm alike
                want_bad = {name: (3 if name == "infinity" else ERR_PUBKEY) for name, _ in items["bad"]}
                by_bytes = {b: name for name, b in items["bad"]}
                seen = set()
                for i in range(n):
                    if bad[i]:
                        name = by_bytes[pks[i]]
                        seen.add(name)
                        assert off[i] == cold[i] == warm[i] == want_bad[name], (name, i, off[i])
                assert seen == set(want_bad)
                # a sample against the oracle: a valid item, a wrong root, a swapped share, a flipped bit, a bad key
                sample = [0, 3, 6, 9, 11, 24]
                assert [off[i] for i in sample] == [bls.verify_status(pks[i], msgs[i], sigs[i]) for i in sample]
    finally:
        impl.set_pair_mode(prev)


def test_off_subgroup_key_misses_both_times(impl, items):
    from charon_amd.tbls import PAIR_SINGLE
    small = dict(items["bad"])["off_subgroup"]
    pks = [items["keys"][0], small, items["keys"][1]]
    prev = impl.set_pair_mode(PAIR_SINGLE)
    try:
        off, cold, warm, s_cold, s_warm = _off_cold_warm(impl, pks, items["msgs"][:3], items["sigs"][:3])
        assert off[1] == cold[1] == warm[1] == ERR_PUBKEY
        assert off == cold == warm
        assert s_cold == (0, 3, 2) and s_warm == (2, 4, 2)
    finally:
        impl.set_pair_mode(prev)


# ---------------------------------------------------------------- 3: same x, other sign
def test_same_x_other_sign_are_two_keys(impl, items):
    from charon_amd.tbls import PAIR_SINGLE
    P = items["keys"][0]
    negP = bytes([P[0] ^ 0x20]) + P[1:]
    msgs = [items["msgs"][0], items["msgs"][0]]
    sigs = [items["sigs"][0], items["sigs"][0]]  # both under P's secret
    prev = impl.set_pair_mode(PAIR_SINGLE)
    try:
        off, cold, warm, s_cold, s_warm = _off_cold_warm(impl, [P, negP], msgs, sigs)
        assert off == cold == warm == [0, 3]
        assert s_cold == (0, 2, 2) and s_warm == (2, 2, 2)
        # the other order, warm: each tag finds its own entry
        assert impl.batch_verify_status([negP, P], msgs, sigs) == [3, 0]
        assert impl.keycache_stats() == (4, 2, 2)
    finally:
        impl.set_pair_mode(prev)


# ---------------------------------------------------------------- 4: one key, 64 times, one wave
def test_one_key_64_times_in_a_cold_wave_inserts_once(impl, items):
    from charon_amd.tbls import PAIR_SINGLE
    pks = [items["keys"][0]] * 64
    msgs = [items["msgs"][0]] * 64
    sigs = [items["sigs"][0]] * 64
    prev = impl.set_pair_mode(PAIR_SINGLE)
    try:
        off, cold, warm, s_cold, s_warm = _off_cold_warm(impl, pks, msgs, sigs)
        assert off == cold == warm == [0] * 64
        assert s_cold == (0, 64, 1)
        assert s_warm == (64, 64, 1)
    finally:
        impl.set_pair_mode(prev)


# ---------------------------------------------------------------- 5: tiny table
def test_tiny_table_never_overwrites(impl):
    from charon_amd.tbls import PAIR_SINGLE
    rng = random.Random(77)
    sks = [rng.randrange(1, R_ORDER).to_bytes(32, "big") for _ in range(40)]
    pks, _ = impl.secret_to_public_key_batch(sks)
    msgs = [rng.randbytes(32) for _ in range(40)]
    sigs, _ = impl.sign_batch(sks, msgs)
    sigs = list(sigs)
    sigs[7] = sigs[8]
    prev = impl.set_pair_mode(PAIR_SINGLE)
    try:
        impl.keycache_config(0)
        off = impl.batch_verify_status(pks, msgs, sigs)
        assert off == [0] * 7 + [3] + [0] * 32
        impl.keycache_config(8)
        last = 0
        for call in range(3):
            assert impl.batch_verify_status(pks, msgs, sigs) == off, call
            hits, misses, inserts = impl.keycache_stats()
            assert last <= inserts <= 8, (call, inserts)
            assert hits + misses == 40 * (call + 1)
            if call:
                assert hits >= last  # what was published stays served
            last = inserts
        assert last >= 1
    finally:
        impl.keycache_config(DEFAULT_SLOTS)
        impl.set_pair_mode(prev)


# ---------------------------------------------------------------- 6: the RLC wire-format path ([x] pk from the entry)
@pytest.mark.parametrize("rlc_mode", ["windows", "batch"])
def test_rlc_device_wire_format_cold_warm_off(impl, rlc_mode):
    import torch
    from charon_amd.tbls import RLC_BATCH, RLC_WINDOWS
    rng = random.Random(5)
    sks = [rng.randrange(1, R_ORDER).to_bytes(32, "big") for _ in range(64)]
    keys, _ = impl.secret_to_public_key_batch(sks)
    roots = [rng.randbytes(32) for _ in range(16)]
    owner = [v for v in range(64) for _ in range(4)]  # 64 validators x 4 partials
    midx = [(v + 5 * k) % 16 for v in range(64) for k in range(4)]
    sigs, st = impl.sign_batch([sks[o] for o in owner], [roots[m] for m in midx])
    assert set(st) == {0}
    sigs = list(sigs)
    sigs[37] = sigs[38]       # a share under another key
    midx[200] = (midx[200] + 1) % 16  # a wrong root
    pks = [keys[o] for o in owner]
    n = 256
    want = impl.batch_verify_status(pks, [roots[m] for m in midx], sigs)
    assert want.count(0) == n - 2 and want[37] == 3 and want[200] == 3

    dev = torch.device("cuda", 0)
    d_pk = torch.frombuffer(bytearray(b"".join(pks)), dtype=torch.uint8).to(dev)
    d_sig = torch.frombuffer(bytearray(b"".join(sigs)), dtype=torch.uint8).to(dev)
    d_midx = torch.tensor(midx, dtype=torch.int32).to(dev)
    d_msg = torch.frombuffer(bytearray(b"".join(roots)), dtype=torch.uint8).to(dev)
    d_off = torch.arange(0, 32 * 17, 32, dtype=torch.int64).to(dev)
    d_st = torch.full((n,), -7, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream(dev)

    def call():
        d_st.fill_(-7)
        torch.cuda.synchronize(dev)
        rc = impl.lib.hipbls_batch_verify_rlc_device(d_pk.data_ptr(), d_sig.data_ptr(), d_midx.data_ptr(), n,
                                                     d_msg.data_ptr(), d_off.data_ptr(), 16, bytes(range(32)),
                                                     d_st.data_ptr(), ctypes.c_void_p(stream.cuda_stream))
        assert rc == 0
        torch.cuda.synchronize(dev)
        return d_st.cpu().tolist()

    prev = impl.set_rlc_mode({"windows": RLC_WINDOWS, "batch": RLC_BATCH}[rlc_mode])
    try:
        impl.keycache_config(0)
        off = call()
        assert impl.keycache_stats() == (0, 0, 0)
        impl.keycache_config(DEFAULT_SLOTS)
        cold = call()
        h0, m0, i0 = impl.keycache_stats()
        warm = call()
        h1, m1, i1 = impl.keycache_stats()
        assert off == want and cold == want and warm == want
        # cold: nothing to hit, 64 distinct keys published; warm: every lookup hits (the batch mode's failed check runs
        # the item stage of the windows as well, so the lookups may be 256 or 512 per call)
        assert h0 == 0 and i0 == 64 and m0 in (256, 512), (h0, m0, i0)
        assert m1 == m0 and i1 == 64 and h1 == m0, (h1, m1, i1)
    finally:
        impl.set_rlc_mode(prev)


# ---------------------------------------------------------------- 7: racing inserts and lookups
def test_racing_inserts_and_lookups_on_four_streams(impl, items):
    import torch
    from charon_amd.tbls import PAIR_SINGLE
    n = 130
    dev = torch.device("cuda", 0)
    prev = impl.set_pair_mode(PAIR_SINGLE)
    try:
        impl.keycache_config(0)
        batches = []
        for t in range(4):
            # overlapping key sets: thread t's batch is the item list rotated by 13 t (the same 20 keys and the same
            # bad encodings, at other positions and in other waves)
            r = 13 * t
            pks = items["pks"][r:] + items["pks"][:r]
            msgs = items["msgs"][r:] + items["msgs"][:r]
            sigs = items["sigs"][r:] + items["sigs"][:r]
            want = impl.batch_verify_status(pks, msgs, sigs)
            batches.append(dict(
                pk=torch.frombuffer(bytearray(b"".join(pks)), dtype=torch.uint8).to(dev),
                sig=torch.frombuffer(bytearray(b"".join(sigs)), dtype=torch.uint8).to(dev),
                msg=torch.frombuffer(bytearray(b"".join(msgs)), dtype=torch.uint8).to(dev),
                off=torch.arange(0, 32 * (n + 1), 32, dtype=torch.int64).to(dev),
                st=[torch.full((n,), -7, dtype=torch.int32, device=dev) for _ in range(3)],
                stream=torch.cuda.Stream(dev), want=want, rc=[]))
        torch.cuda.synchronize(dev)
        impl.keycache_config(DEFAULT_SLOTS)  # cleared: the twelve calls race to fill it

        def worker(b):
            for k in range(3):
                b["rc"].append(impl.lib.hipbls_verify_batch_device(
                    b["pk"].data_ptr(), b["msg"].data_ptr(), b["off"].data_ptr(), b["sig"].data_ptr(), n,
                    b["st"][k].data_ptr(), ctypes.c_void_p(b["stream"].cuda_stream)))

        th = [threading.Thread(target=worker, args=(b,)) for b in batches]
        for x in th:
            x.start()
        for x in th:
            x.join()
        torch.cuda.synchronize(dev)
        for b in batches:
            assert b["rc"] == [0, 0, 0]
            for k in range(3):
                assert b["st"][k].cpu().tolist() == b["want"], k
        hits, misses, inserts = impl.keycache_stats()
        assert hits + misses == 12 * n
        assert inserts == N_KEYS  # write-once: however the calls interleave, each key is published exactly once
    finally:
        impl.set_pair_mode(prev)


# ---------------------------------------------------------------- config beside the submission queue's wire launches
def test_config_resizes_beside_queued_verifies(impl, items):
    """hipbls_keycache_config (other sizes, off, on) from one thread while another sends Verify calls through the
    submission queue, whose worker launches wire batches without the context lock: every launch takes the cache struct
    and enqueues under the cache's own lock, which config holds while it waits for the device and swaps the buffers.
    Statuses are those of the cache-off run.  Once, not in a loop."""
    from charon_amd.tbls import PAIR_SINGLE
    k = 10
    pks, msgs, sigs = items["pks"][:k], items["msgs"][:k], items["sigs"][:k]
    prev = impl.set_pair_mode(PAIR_SINGLE)  # the queue's wire batches then run k_verify_fused
    try:
        impl.keycache_config(0)
        want = impl.batch_verify_status(pks, msgs, sigs)
        impl.keycache_config(DEFAULT_SLOTS)
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
                    impl.keycache_config(slots)
            except Exception as e:  # noqa: BLE001
                errs.append(e)

        th = [threading.Thread(target=caller), threading.Thread(target=resizer)]
        for x in th:
            x.start()
        for x in th:
            x.join()
        assert not errs, errs
        assert got == want
        assert impl.batch_verify_status(pks, msgs, sigs) == want
    finally:
        impl.keycache_config(DEFAULT_SLOTS)
        impl.set_pair_mode(prev)
