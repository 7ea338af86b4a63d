"""The device-resident signature cache (charon_amd/csrc/sigcache.h): a partial signature is verified
when it arrives and handed to sigagg later; with the cache on the Verify side publishes what it decoded and sigagg's
scaling lanes look it up.  Outputs and statuses with the cache off, cold and warm are the same bytes and integers,
the counters tell which path every partial took, only valid points are ever entries, and a half-full table is emptied.

Kernels covered: k_sigcache_insert behind k_verify_prep / k_verify_prep_keys_sc + k_verify_pair_lg2 / _lq4,
k_rlc_items_sc, k_rlcb_items_sc (producers); k_tagg_scale_sc, k_tv_phase_a_sc, k_tv_phase_a_keys_sc (consumers).
Shapes stay at or below 256 partials.  A forced pair mode keeps sigagg off the lone route and Verify on prep + pair.
"""
import ctypes
import json
import os
import random
import threading

import pytest

from tests.test_gpu_lone_sigagg import _launches, _pack, _Reader, _t, _tv
from tests.test_gpu_sigagg_keys import _tvk

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R_ORDER = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
P_FIELD = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
OK, ERR_PUBKEY, ERR_SIGNATURE, ERR_VERIFY, ERR_COMBINE = 0, 1, 2, 3, 5
SLOTS = 4096  # 1 MiB: half of it holds every shape here many times over, so only the tiny-table test rolls over
UNSET = -7


@pytest.fixture(scope="module")
def impl():
    from charon_amd.tbls import PAIR_AUTO, PAIR_LANES, RLC_AUTO, HipBLS
    h = HipBLS()
    h.hcache_config(0)
    h.set_pair_mode(PAIR_LANES)
    yield h
    h.set_pair_mode(PAIR_AUTO)
    h.set_rlc_mode(RLC_AUTO)
    h.lib.hipbls_set_timing(0)
    h.sigcache_config(0)
    h.load_pubshares([])


class Validator:
    """One validator's duty: t of its `total` shares sign its 32-byte root."""

    def __init__(self, impl, seed, t, total):
        rng = random.Random(seed)
        secret = rng.randrange(1, R_ORDER).to_bytes(32, "big")
        self.msg = rng.randbytes(32)
        shares = impl.threshold_split_insecure(secret, total, t, _Reader(seed ^ 0x5EED))
        self.ids = sorted(rng.sample(range(1, total + 1), t))
        sks = [shares[i] for i in self.ids]
        sigs, st = impl.sign_batch(sks, [self.msg] * t)
        assert set(st) == {OK}
        self.parts = dict(zip(self.ids, sigs))
        self.pubshares, st = impl.secret_to_public_key_batch(sks)
        assert set(st) == {OK}
        self.pk = impl.secret_to_public_key(secret)


class Duty:
    """Some validators' partials as sigagg takes them (groups) and as Verify takes them (one item per partial)."""

    def __init__(self, vals, table):
        self.vals = vals
        self.groups = [v.parts for v in vals]
        self.pks = [v.pk for v in vals]
        self.msgs = [v.msg for v in vals]
        self.item_pks = [p for v in vals for p in v.pubshares]
        self.item_msgs = [v.msg for v in vals for _ in v.ids]
        self.item_sigs = [v.parts[i] for v in vals for i in v.ids]
        self.n = len(self.item_sigs)
        pos = {k: j for j, k in enumerate(table)}
        self.kidx = [pos[v.pk] for v in vals]
        self.item_kidx = [pos[p] for p in self.item_pks]


@pytest.fixture(scope="module")
def world(impl):
    """16 validators of 4-of-6 and 14 of 7-of-10 (ids 1..n: some c_k are negative), their keys in the resident table,
    and the four shapes: 7 partials, 64 (16 groups of 4: an exact wave), 71 (the wave boundary), 154 (three waves)."""
    v4 = [Validator(impl, 0x5C400 + k, 4, 6) for k in range(16)]
    v7 = [Validator(impl, 0x5C700 + k, 7, 10) for k in range(14)]
    table = list(dict.fromkeys([v.pk for v in v4 + v7] + [p for v in v4 + v7 for p in v.pubshares]))
    assert impl.load_pubshares(table) == [OK] * len(table)
    shapes = {7: Duty(v7[:1], table), 64: Duty(v4, table), 71: Duty(v4 + v7[:1], table),
              154: Duty(v7 + v4[:14], table)}
    assert {k: d.n for k, d in shapes.items()} == {7: 7, 64: 64, 71: 71, 154: 154}
    return dict(v4=v4, v7=v7, table=table, shapes=shapes)


def _sigagg(impl, entry, d):
    """One sigagg call over a duty: (96 bytes per group, aggregate statuses, verify statuses or None)."""
    if entry == "aggregate":
        aggs, st = _t(impl, d.groups)
        return aggs, st, None
    if entry == "aggregate_verify":
        return _tv(impl, d.groups, d.pks, d.msgs)
    rc, aggs, ast, vst = _tvk(impl, d.groups, d.kidx, d.msgs, list(range(len(d.msgs))))
    assert rc == 0, impl.lib.hipbls_last_error()
    return aggs, ast, vst


def _verify(impl, d):
    st = impl.batch_verify_status(d.item_pks, d.item_msgs, d.item_sigs)
    assert st == [OK] * d.n
    return st


# ---------------------------------------------------------------- 1: off = cold = warm, and the counters
@pytest.mark.parametrize("entry", ["aggregate", "aggregate_verify", "aggregate_verify_keys"])
def test_off_cold_warm_equal_and_stats(impl, world, entry):
    from charon_amd.tbls import PAIR_LANES, PAIR_QUADS
    from oracle import bls12381 as bls
    try:
        for n, d in world["shapes"].items():
            impl.set_pair_mode(PAIR_QUADS if n in (64, 154) else PAIR_LANES)
            impl.sigcache_config(0)
            off = _sigagg(impl, entry, d)
            assert impl.sigcache_stats() == (0, 0, 0, 0)
            assert set(off[1]) == {OK} and (off[2] is None or set(off[2]) == {OK})
            impl.sigcache_config(SLOTS)
            cold = _sigagg(impl, entry, d)
            # cold: the cache is on and nothing has been verified; sigagg never fills the cache
            assert impl.sigcache_stats() == (0, n, 0, 0), (n, impl.sigcache_stats())
            _verify(impl, d)
            assert impl.sigcache_stats() == (0, n, n, 0), (n, impl.sigcache_stats())
            warm = _sigagg(impl, entry, d)
            assert impl.sigcache_stats() == (n, n, n, 0), (n, impl.sigcache_stats())
            assert cold == off and warm == off, (entry, n)
            if n == 71:  # a sample against the oracle: a 4-of-6 and the 7-of-10 group
                for g in (0, len(d.groups) - 1):
                    assert off[0][g] == bls.threshold_aggregate(d.groups[g])
    finally:
        impl.set_pair_mode(PAIR_LANES)
        impl.sigcache_config(0)


# ---------------------------------------------------------------- 2: every producer route fills it
PRODUCERS = ["verify_lanes", "verify_quads", "verify_keys", "rlc_wire_windows", "rlc_wire_batch", "rlc_keys_windows",
             "rlc_keys_batch"]


def _produce(impl, route, pks, kidx, msgs, sigs):
    from charon_amd.tbls import PAIR_LANES, PAIR_QUADS, RLC_BATCH, RLC_WINDOWS
    impl.set_pair_mode(PAIR_QUADS if route == "verify_quads" else PAIR_LANES)
    if route.startswith("rlc"):
        impl.set_rlc_mode(RLC_BATCH if route.endswith("batch") else RLC_WINDOWS)
    seed = bytes(range(32))
    if route in ("verify_lanes", "verify_quads"):
        return impl.batch_verify_status(pks, msgs, sigs)
    if route == "verify_keys":
        return impl.batch_verify_keys_status(kidx, msgs, sigs)
    if route.startswith("rlc_wire"):
        return impl.batch_verify_rlc_status(pks, msgs, sigs, seed)
    return impl.batch_verify_rlc_keys_status(kidx, msgs, sigs, seed)


@pytest.mark.parametrize("route", PRODUCERS)
def test_every_producer_route_fills_it(impl, world, route):
    from charon_amd.tbls import PAIR_LANES, RLC_AUTO
    d = world["shapes"][71]
    other = world["shapes"][154].vals[1]  # a validator outside the 71-partial duty
    pks, kidx, msgs, sigs = list(d.item_pks), list(d.item_kidx), list(d.item_msgs), list(d.item_sigs)
    # beside the duty's 71 partials: one of them a second time, a flipped bit, and another validator's partial
    flipped = bytearray(sigs[5])
    flipped[50] ^= 0x10
    extra = [(0, sigs[0]), (5, bytes(flipped)), (9, other.parts[other.ids[0]])]
    for i, s in extra:
        pks.append(pks[i]), kidx.append(kidx[i]), msgs.append(msgs[i]), sigs.append(s)
    try:
        impl.sigcache_config(0)
        off = _produce(impl, route, pks, kidx, msgs, sigs)
        assert off == [OK] * 72 + [ERR_SIGNATURE, ERR_VERIFY]
        impl.sigcache_config(SLOTS)
        assert _produce(impl, route, pks, kidx, msgs, sigs) == off
        # the distinct insertable signatures: the duty's 71 and the valid point that is the wrong signature
        assert impl.sigcache_stats() == (0, 0, 72, 0), (route, impl.sigcache_stats())
        impl.set_pair_mode(PAIR_LANES)
        got = _sigagg(impl, "aggregate_verify", d)
        assert impl.sigcache_stats() == (71, 0, 72, 0), (route, impl.sigcache_stats())
        # partials nobody verified miss, every one of them
        rest = Duty(world["v7"][5:7], world["table"])
        _sigagg(impl, "aggregate", rest)
        assert impl.sigcache_stats() == (71, rest.n, 72, 0), (route, impl.sigcache_stats())
        impl.sigcache_config(0)
        assert _sigagg(impl, "aggregate_verify", d) == got
    finally:
        impl.set_pair_mode(PAIR_LANES)
        impl.set_rlc_mode(RLC_AUTO)
        impl.sigcache_config(0)


# ---------------------------------------------------------------- 3: never an entry
def _never_entries(sig):
    """Seven 96-byte strings that must never become entries, each with the status a Verify gives it."""
    with open(os.path.join(ROOT, "tests", "golden", "fixtures.json")) as f:
        small = bytes.fromhex(json.load(f)["small_order"]["verify"][0]["sig"])
    x_ge_p = bytearray((P_FIELD + 5).to_bytes(48, "big") + bytes(48))
    x_ge_p[0] |= 0x80
    off_curve = None
    from oracle import bls12381 as bls
    for k in range(1, 64):  # the first x near the signature's that is on no curve point
        cand = bytearray(sig)
        cand[95] = (cand[95] + k) & 0xFF
        try:
            bls.g2_decompress(bytes(cand), subgroup_check=False)
        except bls.BLSError:
            off_curve = bytes(cand)
            break
    assert off_curve is not None
    no_flag = bytearray(sig)
    no_flag[0] &= 0x7F
    inf_with_x = bytearray(sig)
    inf_with_x[0] |= 0x40
    flipped = bytearray(sig)
    flipped[70] ^= 0x02
    return [(bytes(x_ge_p), ERR_SIGNATURE), (off_curve, ERR_SIGNATURE), (small, ERR_SIGNATURE),
            (b"\xc0" + bytes(95), ERR_VERIFY), (bytes(no_flag), ERR_SIGNATURE), (bytes(inf_with_x), ERR_SIGNATURE),
            (bytes(flipped), ERR_SIGNATURE)]


@pytest.mark.parametrize("route", ["verify_lanes", "rlc_wire_windows", "rlc_keys_batch"])
def test_invalid_signatures_are_never_entries(impl, world, route):
    from charon_amd.tbls import PAIR_LANES, RLC_AUTO
    v = world["v7"][2]
    bad = _never_entries(v.parts[v.ids[0]])
    table = world["table"]
    pk, kid = v.pubshares[0], table.index(v.pubshares[0])
    # a Verify batch: the validator's own seven partials, then the seven strings under its first pubshare
    pks = list(v.pubshares) + [pk] * len(bad)
    kidx = [table.index(p) for p in v.pubshares] + [kid] * len(bad)
    msgs = [v.msg] * len(pks)
    sigs = [v.parts[i] for i in v.ids] + [b for b, _ in bad]
    # sigagg: one group per string, the string in place of the validator's first partial, and the intact group
    groups = [v.parts]
    for b, _ in bad:
        g = dict(v.parts)
        g[v.ids[0]] = b
        groups.append(g)
    d_pks, d_msgs = [v.pk] * len(groups), [v.msg] * len(groups)
    try:
        impl.sigcache_config(0)
        off_v = _produce(impl, route, pks, kidx, msgs, sigs)
        assert off_v[:7] == [OK] * 7 and off_v[7:] == [st for _, st in bad]
        impl.set_pair_mode(PAIR_LANES)
        off_a = _tv(impl, groups, d_pks, d_msgs)
        assert off_a[1][0] == OK and off_a[1][4] == OK  # the infinity partial aggregates (and fails the Verify)
        assert off_a[1][1:4] == [ERR_SIGNATURE] * 3 and off_a[1][5:] == [ERR_SIGNATURE] * 3
        impl.sigcache_config(SLOTS)
        assert _produce(impl, route, pks, kidx, msgs, sigs) == off_v
        assert impl.sigcache_stats() == (0, 0, 7, 0)  # the seven valid partials and nothing else
        impl.set_pair_mode(PAIR_LANES)
        for rep in (1, 2):  # they miss every time
            assert _tv(impl, groups, d_pks, d_msgs) == off_a
            hits = 7 + 6 * len(bad)  # the intact group, and each other group's six intact partials
            assert impl.sigcache_stats() == (rep * hits, rep * len(bad), 7, 0), impl.sigcache_stats()
    finally:
        impl.set_pair_mode(PAIR_LANES)
        impl.set_rlc_mode(RLC_AUTO)
        impl.sigcache_config(0)


# ---------------------------------------------------------------- 4: a valid point that is the wrong signature
def test_wrong_signature_is_cached_and_changes_nothing(impl, world):
    a, b = world["v7"][3], world["v7"][4]
    wrong = b.parts[b.ids[0]]  # another validator's partial: a point of G2, ERR_VERIFY under a's pubshare
    g = dict(a.parts)
    g[a.ids[0]] = wrong
    try:
        impl.sigcache_config(0)
        off = _tv(impl, [g, a.parts], [a.pk, a.pk], [a.msg, a.msg])
        assert off[1] == [OK, OK] and off[2] == [ERR_VERIFY, OK]
        impl.sigcache_config(SLOTS)
        st = impl.batch_verify_status(list(a.pubshares), [a.msg] * 7, [wrong] + [a.parts[i] for i in a.ids[1:]])
        assert st == [ERR_VERIFY] + [OK] * 6
        assert impl.sigcache_stats() == (0, 0, 7, 0)
        assert _tv(impl, [g, a.parts], [a.pk, a.pk], [a.msg, a.msg]) == off
        assert impl.sigcache_stats() == (13, 1, 7, 0)  # a's own first partial was never verified
    finally:
        impl.sigcache_config(0)


# ---------------------------------------------------------------- 5: one signature, 64 times, one wave
def test_one_signature_64_times_in_one_wave_inserts_once(impl, world):
    v = world["v4"][0]
    try:
        impl.sigcache_config(SLOTS)
        st = impl.batch_verify_status([v.pubshares[0]] * 64, [v.msg] * 64, [v.parts[v.ids[0]]] * 64)
        assert st == [OK] * 64
        assert impl.sigcache_stats() == (0, 0, 1, 0)
        st = impl.batch_verify_rlc_status([v.pubshares[0]] * 64, [v.msg] * 64, [v.parts[v.ids[0]]] * 64)
        assert st == [OK] * 64
        assert impl.sigcache_stats() == (0, 0, 1, 0)
    finally:
        impl.sigcache_config(0)


# ---------------------------------------------------------------- 6: a tiny table is emptied, never overwritten
def test_tiny_table_rolls_over(impl, world):
    d = Duty(world["v4"][:10], world["table"])  # 40 distinct signatures, three rounds of Verify then sigagg
    assert d.n == 40 and len(set(d.item_sigs)) == 40
    try:
        impl.sigcache_config(0)
        off = _sigagg(impl, "aggregate_verify", d)
        impl.sigcache_config(8)
        last_ins, last_hits = 0, 0
        for k in range(3):
            _verify(impl, d)
            hits, misses, inserts, rollovers = impl.sigcache_stats()
            # a call lies within one generation (the table is only emptied before a producer call): eight slots
            assert inserts - last_ins <= 8, (k, inserts, last_ins)
            assert k > 0 or inserts >= 4  # 40 signatures over eight slots and a 32-slot probe sequence
            assert _sigagg(impl, "aggregate_verify", d) == off, k
            hits, misses, inserts2, rollovers = impl.sigcache_stats()
            assert inserts2 == inserts  # sigagg never fills the cache
            # served is at most what the eight slots hold: an entry of an older generation is gone with its table
            assert hits - last_hits <= 8 and hits + misses == 40 * (k + 1), (k, hits, misses)
            last_ins, last_hits = inserts, hits
        assert rollovers >= 1
    finally:
        impl.sigcache_config(0)


# ---------------------------------------------------------------- 7: overlap of producers and consumers
class DevVerify:
    def __init__(self, d):
        import torch
        self.dev = torch.device("cuda", 0)
        self.n = d.n

        def u8(blob):
            return torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(self.dev)

        self.pk, self.sig, self.msg = u8(b"".join(d.item_pks)), u8(b"".join(d.item_sigs)), u8(b"".join(d.item_msgs))
        self.off = torch.tensor([32 * i for i in range(d.n + 1)], dtype=torch.int64).to(self.dev)
        self.stream = torch.cuda.Stream(self.dev)

    def launch(self, impl):
        import torch
        st = torch.full((self.n,), UNSET, dtype=torch.int32, device=self.dev)
        torch.cuda.synchronize(self.dev)
        rc = impl.lib.hipbls_verify_batch_device(self.pk.data_ptr(), self.msg.data_ptr(), self.off.data_ptr(),
                                                 self.sig.data_ptr(), self.n, st.data_ptr(),
                                                 ctypes.c_void_p(self.stream.cuda_stream))
        return rc, (st,)


class DevSigagg:
    def __init__(self, d):
        import torch
        self.dev = torch.device("cuda", 0)
        self.G, self.n = len(d.groups), d.n
        sigs, ids, offs, _ = _pack(d.groups)

        def u8(blob):
            return torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(self.dev)

        self.sig, self.pk, self.msg = u8(sigs), u8(b"".join(d.pks)), u8(b"".join(d.msgs))
        self.ids = torch.tensor(list(ids)[:d.n], dtype=torch.int64).to(self.dev)
        self.goff = torch.tensor(list(offs), dtype=torch.int64).to(self.dev)
        self.moff = torch.tensor([32 * g for g in range(self.G + 1)], dtype=torch.int64).to(self.dev)
        self.stream = torch.cuda.Stream(self.dev)

    def launch(self, impl):
        import torch
        out = torch.zeros((96 * self.G,), dtype=torch.uint8, device=self.dev)
        ast = torch.full((self.G,), UNSET, dtype=torch.int32, device=self.dev)
        vst = torch.full((self.G,), UNSET, dtype=torch.int32, device=self.dev)
        torch.cuda.synchronize(self.dev)
        rc = impl.lib.hipbls_threshold_aggregate_verify_batch_device(
            self.sig.data_ptr(), self.ids.data_ptr(), self.goff.data_ptr(), self.G, self.n, self.pk.data_ptr(),
            self.msg.data_ptr(), self.moff.data_ptr(), out.data_ptr(), ast.data_ptr(), vst.data_ptr(),
            ctypes.c_void_p(self.stream.cuda_stream))
        return rc, (out, ast, vst)


def test_overlapping_device_verify_and_sigagg_calls(impl, world):
    """Once, not in a loop: two threads on two streams, Verify calls on one and sigagg calls on the other, over
    overlapping partials, the cache cleared just before.  Every output equals the same call made alone."""
    import torch
    d71, d154 = world["shapes"][71], world["shapes"][154]
    ver = [DevVerify(d154), DevVerify(d71), DevVerify(d154)]
    agg = [DevSigagg(d71), DevSigagg(d154), DevSigagg(d71)]
    try:
        impl.sigcache_config(0)
        want = []
        for call in ver + agg:
            rc, outs = call.launch(impl)
            assert rc == 0
            torch.cuda.synchronize(call.dev)
            want.append([o.cpu().tolist() for o in outs])
        assert all(UNSET not in w[-1] for w in want)
        impl.sigcache_config(SLOTS)  # cleared: the calls race to fill and to read it
        got = {}

        def worker(calls, base):
            for k, call in enumerate(calls):
                got[base + k] = call.launch(impl)

        th = [threading.Thread(target=worker, args=(ver, 0)), threading.Thread(target=worker, args=(agg, 3))]
        for x in th:
            x.start()
        for x in th:
            x.join()
        torch.cuda.synchronize(ver[0].dev)
        for k in range(6):
            rc, outs = got[k]
            assert rc == 0
            assert [o.cpu().tolist() for o in outs] == want[k], k
        hits, misses, inserts, rollovers = impl.sigcache_stats()
        assert hits + misses == 71 + 154 + 71 and rollovers == 0
        assert inserts == len(set(d154.item_sigs) | set(d71.item_sigs))  # write-once: each signature exactly once
    finally:
        impl.sigcache_config(0)


# ---------------------------------------------------------------- 8: config beside the submission queue's wire launches
def test_config_resizes_beside_queued_verifies(impl, world):
    """hipbls_sigcache_config (other sizes, off, on) from one thread while another sends ten Verify calls through the
    submission queue, whose worker launches wire batches without the context lock.  Once, not in a loop."""
    d = world["shapes"][71]
    k = 10
    pks, msgs, sigs = d.item_pks[:k], d.item_msgs[:k], list(d.item_sigs[:k])
    sigs[3] = sigs[4]
    impl.load_pubshares([])  # an empty table: the queue's batches stay wire batches
    try:
        impl.sigcache_config(0)
        want = impl.batch_verify_status(pks, msgs, sigs)
        assert want == [OK] * 3 + [ERR_VERIFY] + [OK] * 6
        impl.sigcache_config(SLOTS)
        got, errs = [], []

        def caller():
            try:
                for p, m, s in zip(pks, msgs, sigs):
                    got.append(impl.verify_queued(p, m, s))
            except Exception as e:  # noqa: BLE001
                errs.append(e)

        def resizer():
            try:
                for slots in (8, 0, 1024, 16, 0, SLOTS):
                    impl.sigcache_config(slots)
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
        impl.sigcache_config(0)
        assert impl.load_pubshares(world["table"]) == [OK] * len(world["table"])


# ---------------------------------------------------------------- 9: routing
OLD = (b"verify_prep", b"verify_keys", b"rlc_items", b"rlcb_items", b"tagg_scale", b"tv_phase_a", b"tv_phase_a_keys")
NEW = (b"sigcache_insert", b"verify_prep_keys_sc", b"rlc_items_sc", b"rlcb_items_sc", b"tagg_scale_sc",
       b"tv_phase_a_sc", b"tv_phase_a_keys_sc")


def test_routing_by_launch_counts(impl, world):
    from charon_amd.tbls import PAIR_LANES, RLC_AUTO, RLC_BATCH, RLC_WINDOWS
    d = world["shapes"][7]
    seed = bytes(32)

    def one_of_each():
        impl.batch_verify_status(d.item_pks, d.item_msgs, d.item_sigs)
        impl.batch_verify_keys_status(d.item_kidx, d.item_msgs, d.item_sigs)
        impl.set_rlc_mode(RLC_WINDOWS)
        impl.batch_verify_rlc_status(d.item_pks, d.item_msgs, d.item_sigs, seed)
        impl.set_rlc_mode(RLC_BATCH)
        impl.batch_verify_rlc_keys_status(d.item_kidx, d.item_msgs, d.item_sigs, seed)
        _sigagg(impl, "aggregate", d)
        _sigagg(impl, "aggregate_verify", d)
        _sigagg(impl, "aggregate_verify_keys", d)

    def delta(names):
        before = [_launches(impl, n) for n in names]
        one_of_each()
        return tuple(_launches(impl, n) - b for n, b in zip(names, before))

    impl.lib.hipbls_set_timing(1)
    try:
        impl.set_pair_mode(PAIR_LANES)
        impl.sigcache_config(0)
        # off: each entry point launches the kernel it launched before the cache existed and none of the new ones
        assert delta(OLD + NEW) == (1, 1, 1, 1, 1, 1, 1) + (0,) * 7
        impl.sigcache_config(SLOTS)
        # on: the cache-taking kernels; the producer runs behind both prep + pair Verify calls; the wire Verify keeps
        # its prep, the keyed one takes the prep + pair twin instead of the one-lane kernel
        assert delta(OLD + NEW) == (1, 0, 0, 0, 0, 0, 0) + (2, 1, 1, 1, 1, 1, 1)
    finally:
        impl.lib.hipbls_set_timing(0)
        impl.set_pair_mode(PAIR_LANES)
        impl.set_rlc_mode(RLC_AUTO)
        impl.sigcache_config(0)
