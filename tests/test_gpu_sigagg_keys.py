"""sigagg with the root keys by resident-table index and the hashes from the H(m) cache
(hipbls_threshold_aggregate_verify_batch_keys[_device]).  It is the wire-format call with two inputs
found elsewhere, not new semantics: every case asserts that the 96-byte aggregates and both status arrays equal what
hipbls_threshold_aggregate_verify_batch returns for dv_pks[g] = the bytes loaded at table[dv_key_idx[g]] and message
g = msgs[msg_idx[g]] -- on the lone route and the throughput route, in every pair mode, with the cache off, cold, warm
and evicted.  The aggregate of a valid group also equals Sign(secret), and the oracle confirms a seeded sample.

Inputs as tests/test_gpu_lone_sigagg.py: seeded secrets split by the engine's own threshold_split, partials by
sign_batch.  The table and the cache are process-wide state: every test loads what it needs, and the module leaves the
table empty and the cache disabled, as it found them.
"""
import ctypes
import json
import os
import random
import subprocess
import sys
import threading
import time

import pytest

from tests.test_gpu_lone_sigagg import _Pairs, _Reader, _launches, _oracle, _pack, _tv

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R_ORDER = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
OK, ERR_PUBKEY, ERR_SIGNATURE, ERR_VERIFY, ERR_COMBINE, ERR_ARG = 0, 1, 2, 3, 5, 16
INF_PK = b"\xc0" + bytes(47)


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


def _validator(impl, seed, t, total, ids=None, msg=None, msg_len=32):
    """One validator's duty: (partials {id: sig} of t of its `total` shares, root key, message, Sign(secret))."""
    rng = random.Random(seed)
    secret = rng.randrange(1, R_ORDER).to_bytes(32, "big")
    own = rng.randbytes(msg_len)
    msg = own if msg is None else msg
    shares = impl.threshold_split_insecure(secret, total, t, _Reader(seed ^ 0x5EED))
    ids = sorted(rng.sample(range(1, total + 1), t)) if ids is None else list(ids)
    sigs, st = impl.sign_batch([shares[i] for i in ids], [msg] * len(ids))
    assert set(st) <= {OK}
    return dict(zip(ids, sigs)), impl.secret_to_public_key(secret), msg, impl.sign(secret, msg)


def _tvk(impl, groups, kidx, msgs, midx):
    """hipbls_threshold_aggregate_verify_batch_keys, raw: (rc, per-group 96 bytes, aggregate statuses, verify
    statuses); msgs are the distinct messages."""
    G = len(groups)
    sigs, ids, offs, _ = _pack(groups)
    moffs = (ctypes.c_uint64 * (len(msgs) + 1))()
    for m in range(len(msgs)):
        moffs[m + 1] = moffs[m] + len(msgs[m])
    out = ctypes.create_string_buffer(96 * max(G, 1))
    ast, vst = (ctypes.c_int32 * max(G, 1))(*[-1] * G), (ctypes.c_int32 * max(G, 1))(*[-1] * G)
    rc = impl.lib.hipbls_threshold_aggregate_verify_batch_keys(
        sigs, ids, offs, G, (ctypes.c_uint32 * max(G, 1))(*kidx), (ctypes.c_uint32 * max(G, 1))(*midx),
        b"".join(msgs), moffs, len(msgs), out, ast, vst)
    raw = out.raw
    return rc, [raw[96 * g:96 * g + 96] for g in range(G)], list(ast)[:G], list(vst)[:G]


def _index(items):
    """Distinct items in first-use order and each item's index among them."""
    table = list(dict.fromkeys(items))
    pos = {x: j for j, x in enumerate(table)}
    return table, [pos[x] for x in items]


def _load(impl, table, want=None):
    assert impl.load_pubshares(table) == (want if want is not None else [OK] * len(table))


def _same(impl, groups, pks, msgs, load=True):
    """The keyed call over (table of the distinct keys, distinct messages) must equal the wire-format call on the same
    bytes.  Returns (bytes, aggregate statuses, verify statuses)."""
    table, kidx = _index(pks)
    roots, midx = _index(msgs)
    if load:
        impl.load_pubshares(table)
    rc, aggs, ast, vst = _tvk(impl, groups, kidx, roots, midx)
    assert rc == 0, impl.lib.hipbls_last_error()
    want = _tv(impl, groups, pks, msgs)
    assert (aggs, ast, vst) == want
    return aggs, ast, vst


def _cols(vs):
    return [v[0] for v in vs], [v[1] for v in vs], [v[2] for v in vs]


def _delta(impl, names, fn):
    before = [_launches(impl, n) for n in names]
    fn()
    return tuple(_launches(impl, n) - b for n, b in zip(names, before))


# ------------------------------------------------------------------------------------------------ 1. routes
NAMES = (b"tv_prep8_keys", b"tv_gather_keys", b"tv_lq16", b"tv_prep8", b"tv_phase_a_keys", b"tv_phase_a")


def test_routes_by_launch_counts(impl):
    from charon_amd.tbls import PAIR_AUTO, PAIR_QUADS
    five = [_validator(impl, 0x1100 + k, 2, 3) for k in range(5)]
    one = five[:1]
    impl.lib.hipbls_set_timing(1)
    try:
        # the lone route: the keyed prep, the gather, the unchanged sixteen-lane check (the second tv_lq16 launch is
        # the wire-format call _same compares with, which also accounts for the one tv_prep8)
        assert _delta(impl, NAMES, lambda: _same(impl, *_cols(one))) == (1, 1, 2, 1, 0, 0)
        table, kidx = _index([v[1] for v in one])
        assert _delta(impl, NAMES, lambda: _tvk(impl, [one[0][0]], kidx, [one[0][2]], [0])) == (1, 1, 1, 0, 0, 0)
        # just past the lone envelope
        table, kidx = _index([v[1] for v in five])
        _load(impl, table)
        roots, midx = _index([v[2] for v in five])
        assert _delta(impl, NAMES, lambda: _tvk(impl, [v[0] for v in five], kidx, roots, midx)) == (0, 0, 0, 0, 1, 0)
        # a forced pair mode keeps the throughput kernels, keyed
        assert impl.set_pair_mode(PAIR_QUADS) == PAIR_AUTO
        assert _delta(impl, NAMES, lambda: _tvk(impl, [five[0][0]], kidx[:1], roots[:1], [0])) == (0, 0, 0, 0, 1, 0)
        impl.set_pair_mode(PAIR_AUTO)
        # the wire-format call launches neither keyed kernel
        assert _delta(impl, NAMES, lambda: _tv(impl, *_cols(one))) == (0, 0, 1, 1, 0, 0)
        assert _delta(impl, NAMES, lambda: _tv(impl, *_cols(five))) == (0, 0, 0, 0, 0, 1)
    finally:
        impl.set_pair_mode(PAIR_AUTO)
        impl.lib.hipbls_set_timing(0)


# ------------------------------------------------------------------------------------------------ 2. lone shapes
@pytest.mark.parametrize("t,total,ids", [(1, 3, [3]), (2, 3, None), (7, 10, None)])
def test_lone_one_group(impl, t, total, ids):
    parts, pk, msg, want = _validator(impl, 0x1200 + t, t, total, ids=ids)
    assert _same(impl, [parts], [pk], [msg]) == ([want], [OK], [OK])
    if t == 7:
        assert _oracle(parts, pk, msg) == (want, OK, OK)


def test_lone_four_groups_64_partials_two_sharing_a_root(impl):
    root = bytes(range(32))
    vs = [_validator(impl, 0x1300 + k, t, t + 2, msg=root if k in (1, 3) else None)
          for k, t in enumerate((7, 20, 33, 4))]
    assert sum(len(v[0]) for v in vs) == 64 and vs[1][2] == vs[3][2] == root
    aggs, ast, vst = _same(impl, *_cols(vs))
    assert aggs == [v[3] for v in vs] and ast == [OK] * 4 and vst == [OK] * 4


def test_lone_one_group_of_64_partials(impl):
    parts, pk, msg, want = _validator(impl, 0x1340, 64, 64)
    assert _same(impl, [parts], [pk], [msg]) == ([want], [OK], [OK])


def test_lone_four_groups_one_empty(impl):
    vs = [_validator(impl, 0x1350 + k, t, 10) for k, t in enumerate((4, 7, 2))]
    groups = [vs[0][0], {}, vs[1][0], vs[2][0]]
    pks = [vs[0][1], vs[0][1], vs[1][1], vs[2][1]]
    msgs = [vs[0][2], b"empty", vs[1][2], vs[2][2]]
    aggs, ast, vst = _same(impl, groups, pks, msgs)
    assert ast == [OK, ERR_COMBINE, OK, OK] and vst == [OK, ERR_COMBINE, OK, OK]
    assert aggs == [vs[0][3], bytes(96), vs[1][3], vs[2][3]]
    assert _same(impl, [{}, {}], [vs[1][1]] * 2, [b"", b"x"]) == ([bytes(96)] * 2, [ERR_COMBINE] * 2, [ERR_COMBINE] * 2)


def test_lone_message_lengths_0_32_33(impl):
    vs = [_validator(impl, 0x1360 + n, 4, 6, msg_len=n) for n in (0, 32, 33)]
    assert [len(v[2]) for v in vs] == [0, 32, 33]
    aggs, ast, vst = _same(impl, *_cols(vs))
    assert aggs == [v[3] for v in vs] and ast == [OK] * 3 and vst == [OK] * 3
    for v in vs:
        assert _same(impl, [v[0]], [v[1]], [v[2]]) == ([v[3]], [OK], [OK])


# ------------------------------------------------------------------------------------------------ 3. throughput shapes
@pytest.fixture(scope="module")
def wide(impl):
    """65 groups of 2-of-3 over 5 distinct roots: 130 partials, so the key role, the partial role and the gather all
    cross a 64-lane workgroup, and roots repeat."""
    roots = [bytes([0xA0 + r]) * 32 for r in range(5)]
    return [_validator(impl, 0x2000 + g, 2, 3, msg=roots[g % 5]) for g in range(65)]


def test_throughput_65_groups_5_roots_every_pair_mode(impl, wide):
    from charon_amd.tbls import PAIR_AUTO, PAIR_LANES, PAIR_QUADS, PAIR_SINGLE
    groups, pks, msgs = _cols(wide)
    assert len(set(msgs)) == 5
    try:
        for mode in (PAIR_SINGLE, PAIR_LANES, PAIR_QUADS, PAIR_AUTO):
            impl.set_pair_mode(mode)
            aggs, ast, vst = _same(impl, groups, pks, msgs)
            assert aggs == [v[3] for v in wide] and ast == [OK] * 65 and vst == [OK] * 65, mode
    finally:
        impl.set_pair_mode(PAIR_AUTO)
    g = 37
    assert _oracle(groups[g], pks[g], msgs[g]) == (wide[g][3], OK, OK)


# ------------------------------------------------------------------------------------------------ 4. cache states
@pytest.fixture(scope="module")
def ten(impl):
    """Ten 2-of-3 duties on ten roots."""
    return [_validator(impl, 0x3000 + k, 2, 3) for k in range(10)]


def _warm(impl, vs, kidx):
    """The keyed RLC BatchVerify over the duties' roots (here: the aggregates under the root keys), which caches H(m)
    of every root it sees."""
    st = impl.batch_verify_rlc_keys_status(kidx, [v[2] for v in vs], [v[3] for v in vs], seed=bytes(range(32)))
    assert st == [OK] * len(vs)


def _keyed_ok(impl, vs, kidx):
    roots, midx = _index([v[2] for v in vs])
    got = _tvk(impl, [v[0] for v in vs], kidx, roots, midx)
    assert got == (0, [v[3] for v in vs], [OK] * len(vs), [OK] * len(vs))


def test_cache_off_cold_warm_and_mixed(impl, ten):
    vs = ten[:5]
    table, kidx = _index([v[1] for v in vs])
    _load(impl, table)
    try:
        impl.hcache_config(0)  # disabled: every root is hashed by the call, and counted
        _keyed_ok(impl, vs, kidx)
        assert impl.hcache_stats() == (0, 5, 0)
        impl.hcache_config(16)  # cold
        _keyed_ok(impl, vs, kidx)
        assert impl.hcache_stats() == (0, 5, 0)  # sigagg inserts nothing
        _warm(impl, vs, kidx)
        assert impl.hcache_stats() == (0, 10, 5)
        _keyed_ok(impl, vs, kidx)  # warm: all five from their columns
        assert impl.hcache_stats() == (5, 10, 5)
        _keyed_ok(impl, vs[:1], kidx[:1])  # and on the lone route
        assert impl.hcache_stats() == (6, 10, 5)
        impl.hcache_config(16)  # three of five warm: hits and misses in one call
        _warm(impl, vs[1:4], kidx[1:4])
        assert impl.hcache_stats() == (0, 3, 3)
        _keyed_ok(impl, vs, kidx)
        assert impl.hcache_stats() == (3, 5, 3)
        _keyed_ok(impl, vs[:4], kidx[:4])  # lone route, mixed
        assert impl.hcache_stats() == (6, 6, 3)
    finally:
        impl.hcache_config(0)


def test_cache_eviction_between_warm_up_and_sigagg(impl, ten):
    first, other = ten[:4], ten[4:8]
    table, kidx = _index([v[1] for v in ten[:8]])
    _load(impl, table)
    try:
        impl.hcache_config(4)
        _warm(impl, first, kidx[:4])
        _warm(impl, other, kidx[4:])  # takes all four columns
        assert impl.hcache_stats() == (0, 8, 4)
        _keyed_ok(impl, first, kidx[:4])
        assert impl.hcache_stats() == (0, 12, 4)
        _keyed_ok(impl, other, kidx[4:])
        assert impl.hcache_stats() == (4, 12, 4)
    finally:
        impl.hcache_config(0)


# ------------------------------------------------------------------------------------------------ 5. failures
@pytest.fixture(scope="module")
def base(impl):
    with open(os.path.join(ROOT, "tests", "golden", "fixtures.json")) as f:
        so = json.load(f)["small_order"]
    return dict(v=_validator(impl, 0x4000, 4, 6), other=_validator(impl, 0x4001, 4, 6),
                nb=[_validator(impl, 0x4010 + k, t, 10) for k, t in enumerate((7, 4, 2))],
                small_sig=bytes.fromhex(so["verify"][0]["sig"]), small_pk=bytes.fromhex(so["verify"][16]["pk"]))


FAILURES = ["table_entry_bad_encoding", "table_entry_off_subgroup", "infinity_key", "another_validators_key",
            "msg_idx_names_another_root", "partial_not_in_g2", "duplicate_id", "id_zero", "empty_group"]


def _failure(base, case):
    """(partials, root key bytes in the table, message, aggregate status, verify status, table load status)."""
    parts, pk, msg, _ = base["v"]
    parts = dict(parts)
    ids = list(parts)
    if case == "table_entry_bad_encoding":
        return parts, bytes([pk[0] & 0x7F]) + pk[1:], msg, OK, ERR_PUBKEY, ERR_PUBKEY
    if case == "table_entry_off_subgroup":
        return parts, base["small_pk"], msg, OK, ERR_PUBKEY, ERR_PUBKEY
    if case == "infinity_key":
        return parts, INF_PK, msg, OK, ERR_VERIFY, OK
    if case == "another_validators_key":
        return parts, base["other"][1], msg, OK, ERR_VERIFY, OK
    if case == "msg_idx_names_another_root":
        return parts, pk, base["nb"][0][2], OK, ERR_VERIFY, OK
    if case == "partial_not_in_g2":
        parts[ids[2]] = base["small_sig"]
        return parts, pk, msg, ERR_SIGNATURE, ERR_SIGNATURE, OK
    if case == "duplicate_id":
        return _Pairs([(ids[0], parts[ids[0]]), (ids[1], parts[ids[1]]), (ids[0], parts[ids[2]])]), pk, msg, \
            ERR_COMBINE, ERR_COMBINE, OK
    if case == "id_zero":
        return {0: parts[ids[0]], **{i: parts[i] for i in ids[1:]}}, pk, msg, ERR_COMBINE, ERR_COMBINE, OK
    if case == "empty_group":
        return {}, pk, msg, ERR_COMBINE, ERR_COMBINE, OK
    raise AssertionError(case)


@pytest.mark.parametrize("case", FAILURES)
def test_failure_alone_and_beside_valid_groups(impl, base, case):
    parts, pk, msg, want_ast, want_vst, want_load = _failure(base, case)
    nb = base["nb"]
    _load(impl, [pk], [want_load])
    aggs, ast, vst = _same(impl, [parts], [pk], [msg], load=False)
    assert (ast, vst) == ([want_ast], [want_vst])
    if want_ast != OK:
        assert aggs == [bytes(96)]
    o_agg, o_ast, o_vst = _oracle(parts, pk, msg)
    assert (o_ast, o_vst) == (want_ast, want_vst) and (o_agg is None or o_agg == aggs[0])
    # beside three valid groups, at the second place (the lone route), and with two more (the throughput route)
    for extra in ((), (base["other"], base["v"])):
        vs = [nb[0], (parts, pk, msg, aggs[0]), nb[1], nb[2], *extra]
        got = _same(impl, *_cols(vs))
        want_a = [OK, want_ast, OK, OK] + [OK] * len(extra)
        want_v = [OK, want_vst, OK, OK] + [OK] * len(extra)
        assert got == ([v[3] for v in vs], want_a, want_v)


# ------------------------------------------------------------------------------------------------ 6. arguments
def test_host_arguments(impl, base):
    vs = base["nb"]
    groups, pks, msgs = _cols(vs)
    _load(impl, pks)
    assert _tvk(impl, groups, [0, 1, 2], msgs, [0, 1, 2])[0] == 0
    assert _tvk(impl, groups, [0, 3, 2], msgs, [0, 1, 2])[0] == ERR_ARG  # index equal to the table size
    assert _tvk(impl, groups, [0, 1, 2], msgs, [0, 3, 2])[0] == ERR_ARG  # msg_idx == n_msgs
    assert _tvk(impl, groups, [0, 1, 2], [], [0, 0, 0])[0] == ERR_ARG
    assert _tvk(impl, [], [], [], [])[0] == 0  # n_groups == 0
    _load(impl, [])
    assert _tvk(impl, groups, [0, 1, 2], msgs, [0, 1, 2])[0] == ERR_ARG  # an empty table
    with pytest.raises(ValueError):
        impl.batch_threshold_aggregate_verify_keys(groups, [0, 1, 2], msgs, [0, 1, 2])
    _load(impl, pks)
    aggs, vst = impl.batch_threshold_aggregate_verify_keys(groups, [0, 1, 2], msgs, [0, 1, 2])
    assert aggs == [v[3] for v in vs] and vst == [OK] * 3


def _device_call(impl, groups, kidx, roots, midx, stream, torch, dev):
    def u8(b):
        return torch.frombuffer(bytearray(b) or bytearray(1), dtype=torch.uint8).to(dev)

    G = len(groups)
    sigs, ids, offs, n_parts = _pack(groups)
    moffs = [0]
    for m in roots:
        moffs.append(moffs[-1] + len(m))
    b = dict(sig=u8(sigs), ids=torch.tensor(list(ids), dtype=torch.int64).to(dev),
             off=torch.tensor(list(offs), dtype=torch.int64).to(dev),
             kidx=torch.tensor(kidx, dtype=torch.int64).to(torch.int32).to(dev),
             midx=torch.tensor(midx, dtype=torch.int64).to(torch.int32).to(dev), msg=u8(b"".join(roots)),
             moff=torch.tensor(moffs, dtype=torch.int64).to(dev),
             out=torch.full((96 * G,), 0xEE, dtype=torch.uint8, device=dev),
             ast=torch.full((G,), -1, dtype=torch.int32, device=dev),
             vst=torch.full((G,), -1, dtype=torch.int32, device=dev))
    torch.cuda.synchronize(dev)
    rc = impl.lib.hipbls_threshold_aggregate_verify_batch_keys_device(
        b["sig"].data_ptr(), b["ids"].data_ptr(), b["off"].data_ptr(), G, n_parts, b["kidx"].data_ptr(),
        b["midx"].data_ptr(), b["msg"].data_ptr(), b["moff"].data_ptr(), len(roots), b["out"].data_ptr(),
        b["ast"].data_ptr(), b["vst"].data_ptr(), ctypes.c_void_p(stream.cuda_stream))
    assert rc == 0, impl.lib.hipbls_last_error()
    return b


def _device_result(b, G):
    raw = bytes(b["out"].cpu().numpy().tobytes())
    return [raw[96 * g:96 * g + 96] for g in range(G)], b["ast"].cpu().tolist(), b["vst"].cpu().tolist()


@pytest.mark.parametrize("n_groups", [4, 6])  # the lone route and the throughput route
def test_device_variant_bad_indices_in_one_group(impl, base, n_groups):
    """A key index equal to the table size, a message index equal to n_msgs, and both on a group whose aggregation
    fails: verify_status is ERR_ARG there, that group's aggregate bytes and status are the aggregation's, and the other
    groups are right."""
    import torch
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(dev)
    vs = [base["nb"][0], base["v"], base["nb"][1], base["nb"][2], base["other"], base["nb"][0]][:n_groups]
    groups, pks, msgs = _cols(vs)
    table, kidx = _index(pks)
    roots, midx = _index(msgs)
    _load(impl, table)
    want = _tv(impl, groups, pks, msgs)
    ids = list(vs[1][0])
    dup = _Pairs([(ids[0], vs[1][0][ids[0]]), (ids[0], vs[1][0][ids[1]])])
    want_dup = _tv(impl, [dup], [pks[1]], [msgs[1]])
    assert want_dup[1] == [ERR_COMBINE]
    cases = [(groups, [kidx[0], len(table)] + kidx[2:], midx, want[0][1], OK),
             (groups, kidx, [midx[0], len(roots)] + midx[2:], want[0][1], OK),
             ([groups[0], dup] + groups[2:], [kidx[0], len(table)] + kidx[2:], [midx[0], len(roots)] + midx[2:],
              bytes(96), ERR_COMBINE),
             (groups, kidx, midx, want[0][1], OK)]
    bufs = [_device_call(impl, g, k, roots, m, s, torch, dev) for g, k, m, _, _ in cases]
    torch.cuda.synchronize(dev)
    for j, (b, (_, _, _, agg1, ast1)) in enumerate(zip(bufs, cases)):
        aggs, ast, vst = _device_result(b, n_groups)
        bad_v = ERR_ARG if j < 3 else want[2][1]
        assert aggs == [want[0][0], agg1] + want[0][2:], j
        assert ast == [OK, ast1] + [OK] * (n_groups - 2), j
        assert vst == [OK, bad_v] + [OK] * (n_groups - 2), j


# ------------------------------------------------------------------------------------------------ 7. reuse
def _five_calls(impl, base):
    calls = []
    for k in range(5):
        t, total = ((7, 10), (4, 6))[k % 2]
        parts, pk, msg, want = _validator(impl, 0x6000 + k, t, total)
        if k == 1:  # a partial of another duty: bytes, but not verified
            parts = dict(parts)
            parts[list(parts)[0]] = base["v"][0][list(base["v"][0])[0]]
        elif k == 3:  # an undecodable partial
            parts = dict(parts)
            i = list(parts)[-1]
            parts[i] = bytes([parts[i][0] & 0x7F]) + parts[i][1:]
        calls.append((parts, pk, msg))
    return calls


def test_five_consecutive_host_calls_use_both_workspace_sets(impl, base):
    calls = _five_calls(impl, base)
    table, kidx = _index([c[1] for c in calls])
    _load(impl, table)
    want = [_tv(impl, [c[0]], [c[1]], [c[2]]) for c in calls]
    assert [w[2] for w in want] == [[OK], [ERR_VERIFY], [OK], [ERR_SIGNATURE], [OK]]
    for _ in range(2):
        for c, k, w in zip(calls, kidx, want):
            assert _tvk(impl, [c[0]], [k], [c[2]], [0]) == (0,) + w


def test_five_consecutive_device_calls_on_a_torch_stream(impl, base):
    import torch
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(dev)
    calls = _five_calls(impl, base)
    table, kidx = _index([c[1] for c in calls])
    _load(impl, table)
    want = [_tv(impl, [c[0]], [c[1]], [c[2]]) for c in calls]
    bufs = [_device_call(impl, [c[0]], [k], [c[2]], [0], s, torch, dev) for c, k in zip(calls, kidx)]
    torch.cuda.synchronize(dev)
    for b, w in zip(bufs, want):
        assert _device_result(b, 1) == w


def test_four_threads_mixing_keyed_rlc_and_keyed_sigagg(impl):
    """Four threads, each alternating keyed RLC calls (which fill and evict cache columns) and keyed sigagg calls
    (which read them) over 12 rotating roots with 8 cache columns, for at most two seconds: every status and byte is
    right.  Ordinary use of the ordering rule, nothing more."""
    vs = [_validator(impl, 0x7000 + k, 2, 3) for k in range(12)]
    table, kidx = _index([v[1] for v in vs])
    _load(impl, table)
    errors = []
    deadline = time.monotonic() + 1.5
    try:
        impl.hcache_config(8)

        def worker(th):
            try:
                k = 0
                while k < 6 or (time.monotonic() < deadline and k < 200):
                    lo = (3 * th + 5 * k) % 12
                    n = (1, 4, 5)[k % 3]  # lone calls and a throughput call
                    pick = [(lo + j) % 12 for j in range(n)]
                    if k % 2 == 0:
                        st = impl.batch_verify_rlc_keys_status([kidx[i] for i in pick], [vs[i][2] for i in pick],
                                                               [vs[i][3] for i in pick])
                        if st != [OK] * n:
                            errors.append((th, k, "rlc", st))
                    else:
                        roots, midx = _index([vs[i][2] for i in pick])
                        got = _tvk(impl, [vs[i][0] for i in pick], [kidx[i] for i in pick], roots, midx)
                        if got != (0, [vs[i][3] for i in pick], [OK] * n, [OK] * n):
                            errors.append((th, k, "sigagg", got[0], got[2], got[3]))
                    k += 1
            except Exception as e:  # a thread's exception must fail the test, not vanish
                errors.append((th, repr(e)))

        threads = [threading.Thread(target=worker, args=(th,)) for th in range(4)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
    finally:
        impl.hcache_config(0)
    assert not errors, errors[:5]


def test_table_reload_between_calls(impl, base):
    """The indices name whatever the table holds now."""
    a, b = base["v"], base["other"]
    _load(impl, [a[1], b[1]])
    assert _tvk(impl, [a[0], b[0]], [0, 1], [a[2], b[2]], [0, 1]) == (0, [a[3], b[3]], [OK, OK], [OK, OK])
    _load(impl, [b[1], a[1]])
    got = _tvk(impl, [a[0], b[0]], [0, 1], [a[2], b[2]], [0, 1])
    assert got == (0,) + _tv(impl, [a[0], b[0]], [b[1], a[1]], [a[2], b[2]])
    assert got[2:] == ([OK, OK], [ERR_VERIFY, ERR_VERIFY])
    assert _tvk(impl, [a[0], b[0]], [1, 0], [a[2], b[2]], [0, 1]) == (0, [a[3], b[3]], [OK, OK], [OK, OK])


# ------------------------------------------------------------------------------------------------ 8. two contexts
def test_two_contexts_split_equals_the_wire_format_call(tmp_path):
    """HipBLS(devices=[0, 0]) in a child process (the binding is per process): 2,050 groups of 2-of-3 over 7 roots
    are cut into two ranges of whole groups, each with its own renumbered message table, table copy and cache."""
    out = tmp_path / "out.json"
    r = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "tests", "sigagg_keys_child.py"), str(out)],
                       capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    with open(out) as f:
        got = json.load(f)
    assert got["contexts"] == 2 and got["groups"] == 2050
    assert got["equal"] is True
    assert got["ok_groups"] == 2050 - got["bad_groups"] and got["bad_groups"] > 0
    # both ranges use all 7 roots: each context looked up its own renumbered table
    assert got["misses"] == 14 and got["hits"] == 0 and got["entries"] == 0
