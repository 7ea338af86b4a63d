"""The keyed Verify latency route: hipbls_verify_batch_keys and the submission queue's small keyed
batches on octets / sixteen lanes, keys from the resident table, H(m) read from and inserted into the H(m) cache.  It
is the wire-format call with two inputs found elsewhere: every case asserts that the statuses equal what
hipbls_verify_batch returns for pks[i] = the bytes loaded at table[key_idx[i]] -- at every size where a launch shape
changes, in the pair modes that choose between the routes, with the cache off, cold, warm, bypassed and wrapped.

The table and the cache are process-wide state: every test sets what it needs and restores it in `finally`; the module
leaves the table empty and the cache disabled.
"""
import ctypes
import json
import os
import random
import threading

import pytest

from tests.test_gpu_lone_sigagg import _launches, _tv
from tests.test_gpu_sigagg_keys import _tvk, _validator

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R_ORDER = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
OK, ERR_PUBKEY, ERR_SIGNATURE, ERR_VERIFY = 0, 1, 2, 3
INF_PK = b"\xc0" + bytes(47)
NVALID = 6
OFF_CURVE, OFF_SUBGROUP, INFINITY = NVALID, NVALID + 1, NVALID + 2  # the three bad table entries
KINDS = ("valid", "valid", "wrong_root", "another_key", "flag_cleared", "sig_off_subgroup", "valid", "entry_off_curve",
         "entry_off_subgroup", "entry_infinity")
# (items, distinct roots): sixteen lanes raced / the sixteen-lane - octet boundary / one workgroup against two, raced
# against unraced / partial last workgroups and different block counts for the two roles
SIZES = [(1, 1), (4, 2), (5, 3), (8, 3), (9, 4), (70, 9)]


@pytest.fixture(scope="module")
def impl():
    from charon_amd.tbls import PAIR_AUTO, HipBLS
    h = HipBLS()
    h.hcache_config(0)
    yield h
    h.set_pair_mode(PAIR_AUTO)
    h.lib.hipbls_set_timing(0)
    h.hcache_config(0)
    h.load_pubshares([])


@pytest.fixture(scope="module")
def world(impl):
    """The table (six valid keys, then an entry off the curve, one off the subgroup and the infinity key), the
    secrets of the valid keys and a signature off the subgroup."""
    from oracle import bls12381 as bls
    rng = random.Random(0x5A7)
    sks = [rng.randrange(1, R_ORDER).to_bytes(32, "big") for _ in range(NVALID)]
    pks, st = impl.secret_to_public_key_batch(sks)
    assert set(st) == {OK}
    with open(os.path.join(ROOT, "tests", "golden", "fixtures.json")) as f:
        so = json.load(f)["small_order"]
    x = int.from_bytes(bytes([pks[0][0] & 0x1F]) + pks[0][1:], "big")
    off_curve = None
    for d in range(1, 64):
        cand = (x + d).to_bytes(48, "big")
        cand = bytes([cand[0] | 0x80]) + cand[1:]
        try:
            bls.g1_decompress(cand)
        except bls.BLSError:
            off_curve = cand
            break
    assert off_curve is not None
    table = list(pks) + [off_curve, bytes.fromhex(so["verify"][16]["pk"]), INF_PK]
    return dict(sks=sks, table=table, load=[OK] * NVALID + [ERR_PUBKEY, ERR_PUBKEY, OK],
                small_sig=bytes.fromhex(so["verify"][0]["sig"]))


def _load(impl, world):
    assert impl.load_pubshares(world["table"]) == world["load"]


def _roots(tag, count):
    """`count` distinct messages: the empty one, then 32 and 200 bytes in turn."""
    rng = random.Random(tag)
    return [b""] + [rng.randbytes((200, 32)[r % 2]) for r in range(1, count)]


def _items(impl, world, n, roots, seed, kinds=KINDS):
    """n items over the roots, the kinds in rotation: (key indices, messages, signatures)."""
    rng = random.Random(seed)
    kidx, msgs, signer, signed = [], [], [], []
    for i in range(n):
        kind = kinds[i % len(kinds)]
        k = i % NVALID
        m = roots[i % len(roots)]
        kidx.append({"entry_off_curve": OFF_CURVE, "entry_off_subgroup": OFF_SUBGROUP,
                     "entry_infinity": INFINITY, "another_key": (k + 1) % NVALID}.get(kind, k))
        msgs.append(m)
        signer.append(world["sks"][k])
        signed.append(b"another root " + rng.randbytes(19) if kind == "wrong_root" else m)
    sigs, st = impl.sign_batch(signer, signed)
    assert set(st) == {OK}
    sigs = list(sigs)
    for i in range(n):
        kind = kinds[i % len(kinds)]
        if kind == "flag_cleared":
            sigs[i] = bytes([sigs[i][0] & 0x7F]) + sigs[i][1:]
        elif kind == "sig_off_subgroup":
            sigs[i] = world["small_sig"]
    return kidx, msgs, sigs


_ORACLE = {}


def _oracle_status(pk, msg, sig):
    from oracle import bls12381 as bls
    key = (pk, msg, sig)
    if key not in _ORACLE:
        _ORACLE[key] = bls.verify_status(pk, msg, sig)
    return _ORACLE[key]


@pytest.fixture(scope="module")
def cases(impl, world):
    """Per size: the items and the wire-format call's statuses for the same key bytes, computed once."""
    out = {}
    for n, nr in SIZES:
        kidx, msgs, sigs = _items(impl, world, n, _roots(0xC0 + n, nr), 0xD0 + n)
        assert len(set(msgs)) == nr and sorted({len(m) for m in msgs}) == [0, 32, 200][:min(nr, 3)]
        want = impl.batch_verify_status([world["table"][k] for k in kidx], msgs, sigs)
        out[n] = (kidx, msgs, sigs, want)
    # the kinds give what they are built for
    assert out[70][3][:10] == [OK, OK, ERR_VERIFY, ERR_VERIFY, ERR_SIGNATURE, ERR_SIGNATURE, OK, ERR_PUBKEY,
                               ERR_PUBKEY, ERR_VERIFY]
    return out


def _keyed(impl, case):
    kidx, msgs, sigs, want = case
    got = impl.batch_verify_keys_status(kidx, msgs, sigs)
    assert got == want
    return got


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("n,nr", SIZES)
def test_parity_cache_off_cold_warm_bypass(impl, world, cases, n, nr):
    _load(impl, world)
    case = cases[n]
    try:
        impl.hcache_config(0)
        _keyed(impl, case)
        assert impl.hcache_stats() == (0, 0, 0)
        impl.hcache_config(64)
        _keyed(impl, case)  # cold: every root missed and inserted
        assert impl.hcache_stats() == (0, nr, nr)
        _keyed(impl, case)  # warm
        assert impl.hcache_stats() == (nr, nr, nr)
        impl.hcache_config(nr - 1)  # fewer columns than roots (none at all for one root): the call's own table
        _keyed(impl, case)
        assert impl.hcache_stats() == (0, 0, 0)
    finally:
        impl.hcache_config(0)
    # the oracle on the first (valid) and the last item
    kidx, msgs, sigs, want = case
    for i in sorted({0, n - 1}):
        assert _oracle_status(world["table"][kidx[i]], msgs[i], sigs[i]) == want[i], i


@pytest.mark.parametrize("n,nr", SIZES)
def test_parity_forced_octets_and_forced_single(impl, world, cases, n, nr):
    from charon_amd.tbls import PAIR_AUTO, PAIR_OCTETS, PAIR_SINGLE
    _load(impl, world)
    case = cases[n]
    names = (b"verify_prep8_keys", b"verify_gather_keys", b"verify_pair_lq8", b"verify_keys")
    impl.lib.hipbls_set_timing(1)
    try:
        impl.hcache_config(64)
        assert impl.set_pair_mode(PAIR_OCTETS) == PAIR_AUTO
        before = [_launches(impl, x) for x in names]
        _keyed(impl, case)
        _keyed(impl, case)
        assert [_launches(impl, x) - b for x, b in zip(names, before)] == [2, 2, 2, 0]  # eight lanes at every size
        assert impl.hcache_stats() == (nr, nr, nr)
        impl.set_pair_mode(PAIR_SINGLE)  # keeps k_verify_keys, and the cache out of it
        before = [_launches(impl, x) for x in names]
        _keyed(impl, case)
        assert [_launches(impl, x) - b for x, b in zip(names, before)] == [0, 0, 0, 1]
        assert impl.hcache_stats() == (nr, nr, nr)
    finally:
        impl.set_pair_mode(PAIR_AUTO)
        impl.lib.hipbls_set_timing(0)
        impl.hcache_config(0)


def test_parity_every_kind_as_a_lone_call(impl, world):
    """n = 1 for each kind of item: the sixteen-lane raced check composes every status by itself."""
    _load(impl, world)
    kinds = tuple(dict.fromkeys(KINDS))
    kidx, msgs, sigs = _items(impl, world, len(kinds), _roots(0xE1, 3), 0xE2, kinds=kinds)
    want = impl.batch_verify_status([world["table"][k] for k in kidx], msgs, sigs)
    assert want == [OK, ERR_VERIFY, ERR_VERIFY, ERR_SIGNATURE, ERR_SIGNATURE, ERR_PUBKEY, ERR_PUBKEY, ERR_VERIFY]
    try:
        impl.hcache_config(64)
        for rnd in range(2):  # cold, then warm
            for i in range(len(kinds)):
                assert impl.batch_verify_keys_status(kidx[i:i + 1], msgs[i:i + 1], sigs[i:i + 1]) == want[i:i + 1], \
                    (rnd, kinds[i])
        assert impl.hcache_stats() == (len(kinds) + len(kinds) - 3, 3, 3)
    finally:
        impl.hcache_config(0)
    for i in (1, 3):  # wrong root, cleared flag
        assert _oracle_status(world["table"][kidx[i]], msgs[i], sigs[i]) == want[i]


def test_parity_capacity_4_wrap_and_demotion(impl, world):
    """Capacity 4, successive calls of 5 items over 3 new roots each: the ring wraps in the second call, later calls
    overwrite columns, and a call that repeats one cached root beside two new ones has that hit demoted."""
    _load(impl, world)
    sets = [_roots(0xF0 + c, 4)[1:] for c in range(4)]  # 3 non-empty roots per call
    calls = [_items(impl, world, 5, r, 0xF8 + c) for c, r in enumerate(sets)]
    # the fifth call: the oldest root still cached beside two new ones
    mixed_roots = [sets[3][0]] + _roots(0xF7, 3)[1:]
    calls.append(_items(impl, world, 5, mixed_roots, 0xFD))
    wants = [impl.batch_verify_status([world["table"][k] for k in c[0]], c[1], c[2]) for c in calls]
    try:
        impl.hcache_config(4)
        for j, (c, w) in enumerate(zip(calls[:4], wants)):
            assert impl.batch_verify_keys_status(*c) == w, j
            assert impl.hcache_stats() == (0, 3 * (j + 1), min(4, 3 * (j + 1)))
        # ring = 0 now; sets[3] sits in columns 1, 2, 3 and sets[2][2] in column 0
        assert impl.batch_verify_keys_status(*calls[3]) == wants[3]  # warm after the wrap
        assert impl.hcache_stats() == (3, 12, 4)
        # sets[3][0] is in column 1; the two new roots would take 0 and 1: demoted, three misses
        assert impl.batch_verify_keys_status(*calls[4]) == wants[4]
        assert impl.hcache_stats() == (3, 15, 4)
        assert impl.batch_verify_keys_status(*calls[4]) == wants[4]
        assert impl.hcache_stats() == (6, 15, 4)
    finally:
        impl.hcache_config(0)
    assert _oracle_status(world["table"][calls[4][0][0]], calls[4][1][0], calls[4][2][0]) == wants[4][0] == OK


# ------------------------------------------------------------------------------------------------ 2. accounting
def test_accounting_and_routes(impl, world, cases):
    from charon_amd.tbls import PAIR_AUTO, PAIR_SINGLE
    _load(impl, world)
    case = cases[5]
    names = (b"verify_prep8_keys", b"verify_gather_keys", b"verify_keys")
    impl.lib.hipbls_kernel_timing_reset()
    impl.lib.hipbls_set_timing(1)
    try:
        impl.hcache_config(64)
        kidx, msgs, sigs, want = case
        assert impl.batch_verify_keys_status(kidx, msgs, sigs) == want
        assert impl.hcache_stats() == (0, 3, 3)
        assert impl.batch_verify_keys_status(kidx, msgs, sigs) == want
        assert impl.hcache_stats() == (3, 3, 3)
        got = [_launches(impl, x) for x in names]
        assert got[0] >= 1 and got[1] >= 1 and got[2] == 0, got
        assert impl.set_pair_mode(PAIR_SINGLE) == PAIR_AUTO
        assert impl.batch_verify_keys_status(kidx, msgs, sigs) == want
        assert _launches(impl, b"verify_keys") == 1
        assert impl.hcache_stats() == (3, 3, 3)
    finally:
        impl.set_pair_mode(PAIR_AUTO)
        impl.lib.hipbls_set_timing(0)
        impl.hcache_config(0)


def test_lone_call_of_the_binding(impl, world):
    from charon_amd.tbls import TBLSError
    _load(impl, world)
    kidx, msgs, sigs = _items(impl, world, 3, _roots(0x111, 2), 0x112, kinds=("valid", "another_key", "flag_cleared"))
    assert impl.verify_keys(kidx[0], msgs[0], sigs[0]) is None
    with pytest.raises(TBLSError, match="signature not verified"):
        impl.verify_keys(kidx[1], msgs[1], sigs[1])
    with pytest.raises(TBLSError, match="cannot unmarshal signature"):
        impl.verify_keys(kidx[2], msgs[2], sigs[2])
    with pytest.raises(TBLSError, match="cannot set compressed public key"):
        impl.verify_keys(OFF_CURVE, msgs[0], sigs[0])
    with pytest.raises(ValueError):
        impl.verify_keys(len(world["table"]), msgs[0], sigs[0])  # outside the table: refused up front


# ------------------------------------------------------------------------------------------------ 3. one cache
def test_one_cache_three_users(impl):
    vs = [_validator(impl, 0x8100 + k, 4, 6) for k in range(2)]
    assert impl.load_pubshares([v[1] for v in vs]) == [OK, OK]
    try:
        impl.hcache_config(16)
        # a lone Verify misses root r and inserts it; the sigagg over r that follows hits
        parts, pk, msg, agg = vs[0]
        impl.verify_keys(0, msg, agg)
        assert impl.hcache_stats() == (0, 1, 1)
        got = _tvk(impl, [parts], [0], [msg], [0])
        assert impl.hcache_stats() == (1, 1, 1)
        assert got == (0,) + _tv(impl, [parts], [pk], [msg])
        assert got == (0, [agg], [OK], [OK])
        # a keyed RLC call inserts a new root; the lone Verify over it hits
        parts, pk, msg, agg = vs[1]
        assert impl.batch_verify_rlc_keys_status([1], [msg], [agg], seed=bytes(range(32))) == [OK]
        assert impl.hcache_stats() == (1, 2, 2)
        assert impl.batch_verify_keys_status([1], [msg], [agg]) == impl.batch_verify_status([pk], [msg], [agg]) == [OK]
        assert impl.hcache_stats() == (2, 2, 2)
        # and with the other validator's key: the cached H(m), the wire-format status
        assert impl.batch_verify_keys_status([0], [msg], [agg]) == \
            impl.batch_verify_status([vs[0][1]], [msg], [agg]) == [ERR_VERIFY]
        assert impl.hcache_stats() == (3, 2, 2)
    finally:
        impl.hcache_config(0)


# ------------------------------------------------------------------------------------------------ 4. queue
def test_queue_in_the_production_configuration(impl, world):
    """The Go binding's configuration (table loaded, cache enabled), serial callers: every batch is one item, runs
    keyed and takes the latency route, never the RLC kernels."""
    _load(impl, world)
    roots = _roots(0x9A, 7)[1:]
    kidx, msgs, sigs = _items(impl, world, 18, roots, 0x9B, kinds=("valid",))
    order = sorted(range(18), key=lambda i: (i % 6, i))  # root by root: 6 roots x 3 partials
    kidx, msgs, sigs = [kidx[i] for i in order], [msgs[i] for i in order], [sigs[i] for i in order]
    sigs[4] = bytes([sigs[4][0] & 0x7F]) + sigs[4][1:]
    sigs[11], sigs[12] = sigs[12], sigs[11]
    pks = [world["table"][k] for k in kidx]
    want = impl.batch_verify_status(pks, msgs, sigs)
    assert want.count(OK) == 15 and want[4] == ERR_SIGNATURE and want[11] == want[12] == ERR_VERIFY
    names = (b"verify_prep8_keys", b"rlc_items")
    impl.lib.hipbls_set_timing(1)
    try:
        impl.hcache_config(256)
        h0, m0, _ = impl.hcache_stats()
        k0, (b0, _) = impl.queue_keyed_batches(), impl.queue_stats()
        before = [_launches(impl, x) for x in names]
        got = [impl.verify_queued(pks[i], msgs[i], sigs[i]) for i in range(18)]
        assert got == want
        h1, m1, e1 = impl.hcache_stats()
        k1, (b1, _) = impl.queue_keyed_batches(), impl.queue_stats()
        assert k1 - k0 == b1 - b0 == 18
        assert m1 - m0 == len(set(msgs)) == 6 and h1 - h0 == 12 and e1 == 6
        after = [_launches(impl, x) for x in names]
        assert after[0] - before[0] == 18 and after[1] - before[1] == 0
    finally:
        impl.lib.hipbls_set_timing(0)
        impl.hcache_config(0)


# ------------------------------------------------------------------------------------------------ 5. overwrite
def test_columns_overwritten_beside_a_sigagg_gather(impl):
    """Capacity 4.  Thread A: 20 keyed lone sigagg calls over two cached roots (each gathers H(m) from the cache and
    returns before its kernels end).  Thread B: 20 lone Verify calls, each over a new root, so the ring overwrites every
    column, the two roots' among them.  Every output is the wire-format call's."""
    vs = [_validator(impl, 0xA100 + k, 4, 6) for k in range(2)]
    assert impl.load_pubshares([v[1] for v in vs]) == [OK, OK]
    want_a = [_tv(impl, [v[0]], [v[1]], [v[2]]) for v in vs]
    assert [w[2] for w in want_a] == [[OK], [OK]]
    rng = random.Random(0xA2)
    new_roots = [rng.randbytes(32) for _ in range(20)]
    # thread B: validator k's aggregate under its root key, but over a fresh root each time: "signature not verified"
    b_calls = [(j % 2, new_roots[j], vs[j % 2][3]) for j in range(20)]
    want_b = impl.batch_verify_status([vs[k][1] for k, _, _ in b_calls], [m for _, m, _ in b_calls],
                                      [s for _, _, s in b_calls])
    assert want_b == [ERR_VERIFY] * 20
    errors = []
    try:
        impl.hcache_config(4)
        for k, v in enumerate(vs):  # both roots cached
            impl.verify_keys(k, v[2], v[3])
        assert impl.hcache_stats() == (0, 2, 2)

        def thread_a():
            try:
                for j in range(20):
                    k = j % 2
                    got = _tvk(impl, [vs[k][0]], [k], [vs[k][2]], [0])
                    if got != (0,) + want_a[k]:
                        errors.append(("sigagg", j, got[0], got[2], got[3]))
            except Exception as e:  # a thread's exception must fail the test, not vanish
                errors.append(("sigagg", repr(e)))

        def thread_b():
            try:
                for j, (k, m, s) in enumerate(b_calls):
                    got = impl.batch_verify_keys_status([k], [m], [s])
                    if got != want_b[j:j + 1]:
                        errors.append(("verify", j, got))
            except Exception as e:
                errors.append(("verify", repr(e)))

        ths = [threading.Thread(target=thread_a), threading.Thread(target=thread_b)]
        for t in ths:
            t.start()
        for t in ths:
            t.join()
        hits, misses, entries = impl.hcache_stats()
        assert misses >= 22 and entries == 4  # thread B's 20 new roots all inserted
    finally:
        impl.hcache_config(0)
    assert not errors, errors[:5]
