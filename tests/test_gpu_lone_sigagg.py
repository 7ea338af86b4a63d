"""The lone sigagg route: a threshold-aggregate(-verify) call of at most 4 groups and 64 partials in
AUTO pair mode runs on lane groups -- octets for the keys, hashes and partials (verify_lat.hip k_tv_prep8), then per
group the sum, the sixteen-lane check and [L^-1] S (verify_hex.hip k_tv_pair_lq16; k_tagg_sum8 for the aggregate-only
call) -- instead of one lane per unit of work.  It is a route, not new semantics: every byte and status equals the
throughput kernels', which the forced pair modes keep (PAIR_QUADS is the reference run here), the aggregate of a
valid group equals Sign(secret), and the oracle (pure-Python pairing, at most four groups per test) confirms a sample.

Inputs: seeded secrets split by the engine's own threshold_split (ids 1..n); the one group whose ids leave 1..n
({1, 2^40, -5}, the field path) evaluates its seeded polynomial on the host, as tests/test_gpu_r04.py does.
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
OK, ERR_PUBKEY, ERR_SIGNATURE, ERR_VERIFY, ERR_COMBINE = 0, 1, 2, 3, 5
INF = b"\xc0" + bytes(95)


@pytest.fixture(scope="module")
def impl():
    from charon_amd.tbls import HipBLS
    return HipBLS()


class _Reader:
    """A seeded reader for threshold_split_insecure (herumi.go:84-132 takes an io.Reader)."""

    def __init__(self, seed):
        self.rng = random.Random(seed)

    def read(self, n):
        return (self.rng.randrange(1, R_ORDER)).to_bytes(n, "big")


def _validator(impl, seed, t, total, ids=None, msg_len=32):
    """One validator's duty: (partials {id: sig} of t of its `total` shares, root key, message, Sign(secret))."""
    rng = random.Random(seed)
    secret = rng.randrange(1, R_ORDER).to_bytes(32, "big")
    msg = rng.randbytes(msg_len)
    shares = impl.threshold_split_insecure(secret, total, t, _Reader(seed ^ 0x5EED))
    ids = sorted(rng.sample(range(1, total + 1), t)) if ids is None else list(ids)
    sigs, st = impl.sign_batch([shares[i] for i in ids], [msg] * len(ids))
    assert set(st) <= {OK}
    pk = impl.secret_to_public_key(secret)
    return dict(zip(ids, sigs)), pk, msg, impl.sign(secret, msg)


def _field_validator(impl, seed, ids, t):
    """Shares at arbitrary int64 ids: the seeded polynomial evaluated on the host (ids mod r, as fr_from_i64)."""
    rng = random.Random(seed)
    poly = [rng.randrange(1, R_ORDER) for _ in range(t)]
    msg = rng.randbytes(32)

    def ev(x):
        acc = 0
        for c in reversed(poly):
            acc = (acc * (x % R_ORDER) + c) % R_ORDER
        return acc

    sigs, st = impl.sign_batch([ev(i).to_bytes(32, "big") for i in ids], [msg] * len(ids))
    assert set(st) == {OK}
    secret = poly[0].to_bytes(32, "big")
    return dict(zip(ids, sigs)), impl.secret_to_public_key(secret), msg, impl.sign(secret, msg)


def _pack(groups):
    offs = (ctypes.c_uint64 * (len(groups) + 1))()
    ids, sigs = [], []
    for g, grp in enumerate(groups):
        offs[g] = len(ids)
        for i, s in grp.items():
            ids.append(int(i))
            sigs.append(bytes(s))
    offs[len(groups)] = len(ids)
    return b"".join(sigs), (ctypes.c_int64 * max(1, len(ids)))(*ids), offs, len(ids)


def _tv(impl, groups, pks, msgs):
    """hipbls_threshold_aggregate_verify_batch, raw: (per-group 96 bytes, aggregate statuses, verify statuses)."""
    G = len(groups)
    sigs, ids, offs, _ = _pack(groups)
    moffs = (ctypes.c_uint64 * (G + 1))()
    for g in range(G):
        moffs[g + 1] = moffs[g] + len(msgs[g])
    out = ctypes.create_string_buffer(96 * G)
    ast, vst = (ctypes.c_int32 * G)(*[-1] * G), (ctypes.c_int32 * G)(*[-1] * G)
    rc = impl.lib.hipbls_threshold_aggregate_verify_batch(sigs, ids, offs, G, b"".join(pks), b"".join(msgs), moffs,
                                                          out, ast, vst)
    assert rc == 0, impl.lib.hipbls_last_error()
    raw = out.raw
    return [raw[96 * g:96 * g + 96] for g in range(G)], list(ast), list(vst)


def _t(impl, groups):
    """hipbls_threshold_aggregate_batch, raw: (per-group 96 bytes, statuses)."""
    G = len(groups)
    sigs, ids, offs, _ = _pack(groups)
    out = ctypes.create_string_buffer(96 * G)
    st = (ctypes.c_int32 * G)(*[-1] * G)
    rc = impl.lib.hipbls_threshold_aggregate_batch(sigs, ids, offs, G, out, st)
    assert rc == 0, impl.lib.hipbls_last_error()
    raw = out.raw
    return [raw[96 * g:96 * g + 96] for g in range(G)], list(st)


def _forced(impl, fn, *args):
    """The same call on the throughput kernels (a forced pair mode never takes the route)."""
    from charon_amd.tbls import PAIR_AUTO, PAIR_QUADS
    assert impl.set_pair_mode(PAIR_QUADS) == PAIR_AUTO
    try:
        return fn(impl, *args)
    finally:
        impl.set_pair_mode(PAIR_AUTO)


def _both(impl, groups, pks, msgs):
    """The fused and the aggregate-only call on the route; both must equal their forced-mode runs.  Returns the fused
    call's (bytes, aggregate statuses, verify statuses)."""
    got = _tv(impl, groups, pks, msgs)
    assert got == _forced(impl, _tv, groups, pks, msgs)
    agg = _t(impl, groups)
    assert agg == _forced(impl, _t, groups)
    assert agg == (got[0], got[1])
    return got


def _launches(impl, name):
    a, c = ctypes.c_double(), ctypes.c_uint64()
    impl.lib.hipbls_kernel_timing(name, ctypes.byref(a), ctypes.byref(c))
    return c.value


def _oracle(group, pk, msg):
    """(aggregate or None, aggregate status, verify status) by the oracle, in sigagg's order."""
    from oracle import bls12381 as bls
    try:
        agg = bls.threshold_aggregate(group)
    except bls.BLSError as e:
        st = ERR_SIGNATURE if "unmarshal" in str(e) else ERR_COMBINE
        return None, st, st
    return agg, OK, bls.verify_status(pk, msg, agg)


# ------------------------------------------------------------------------------------------------ 1. route taken
def test_route_taken_only_inside_its_envelope(impl):
    """One group in AUTO launches tv_prep8 + tv_lq16 (tv_prep8 + tagg_sum8 for the aggregate-only call); the forced
    modes, a 5-group call and a 65-partial call keep the throughput kernels."""
    from charon_amd.tbls import PAIR_AUTO, PAIR_QUADS, PAIR_SINGLE
    names = (b"tv_prep8", b"tv_lq16", b"tagg_sum8")
    one = _validator(impl, 0x101, 7, 10)
    five = [_validator(impl, 0x110 + k, 2, 3) for k in range(5)]
    wide = [_validator(impl, 0x120, 33, 33), _validator(impl, 0x121, 32, 32)]  # 65 partials in 2 groups

    def delta(fn):
        before = [_launches(impl, n) for n in names]
        fn()
        return tuple(_launches(impl, n) - b for n, b in zip(names, before))

    def fused(vs):
        aggs, ast, vst = _tv(impl, [v[0] for v in vs], [v[1] for v in vs], [v[2] for v in vs])
        assert aggs == [v[3] for v in vs] and ast == [OK] * len(vs) and vst == [OK] * len(vs)

    def plain(vs):
        aggs, st = _t(impl, [v[0] for v in vs])
        assert aggs == [v[3] for v in vs] and st == [OK] * len(vs)

    impl.lib.hipbls_set_timing(1)
    try:
        assert delta(lambda: fused([one])) == (1, 1, 0)
        assert delta(lambda: plain([one])) == (1, 0, 1)
        for mode in (PAIR_QUADS, PAIR_SINGLE):
            impl.set_pair_mode(mode)
            assert delta(lambda: fused([one])) == (0, 0, 0), mode
            assert delta(lambda: plain([one])) == (0, 0, 0), mode
        impl.set_pair_mode(PAIR_AUTO)
        assert delta(lambda: fused(five)) == (0, 0, 0)
        assert delta(lambda: plain(five)) == (0, 0, 0)
        assert delta(lambda: fused(wide)) == (0, 0, 0)
        assert delta(lambda: plain(wide)) == (0, 0, 0)
        assert delta(lambda: fused(five[:4])) == (1, 1, 0)  # 4 groups: still inside
    finally:
        impl.set_pair_mode(PAIR_AUTO)
        impl.lib.hipbls_set_timing(0)


# ------------------------------------------------------------------------------------------------ 2. shapes
# t = 8 fills one 64-lane workgroup of octets, t = 9 spills into a second; t = 20 is above lagrange_small's 16
@pytest.mark.parametrize("t,total,ids", [(1, 3, [3]), (2, 3, None), (4, 6, None), (7, 10, None), (8, 10, None),
                                         (9, 10, None), (20, 24, None)])
def test_one_group_shapes(impl, t, total, ids):
    parts, pk, msg, want = _validator(impl, 0x200 + t, t, total, ids=ids)
    aggs, ast, vst = _both(impl, [parts], [pk], [msg])
    assert (aggs, ast, vst) == ([want], [OK], [OK])


def test_four_groups_totalling_64_partials(impl):
    """7 + 20 + 33 + 4 = 64 partials: the envelope's edge, two groups on the field path (t > 16)."""
    vs = [_validator(impl, 0x300 + k, t, t + 2) for k, t in enumerate((7, 20, 33, 4))]
    aggs, ast, vst = _both(impl, [v[0] for v in vs], [v[1] for v in vs], [v[2] for v in vs])
    assert aggs == [v[3] for v in vs] and ast == [OK] * 4 and vst == [OK] * 4


def test_one_group_holding_all_64_partials(impl):
    parts, pk, msg, want = _validator(impl, 0x340, 64, 64)
    assert _both(impl, [parts], [pk], [msg]) == ([want], [OK], [OK])


def test_four_groups_one_empty(impl):
    vs = [_validator(impl, 0x350 + k, t, 10) for k, t in enumerate((4, 7, 2))]
    groups = [vs[0][0], {}, vs[1][0], vs[2][0]]
    pks = [vs[0][1], vs[0][1], vs[1][1], vs[2][1]]
    msgs = [vs[0][2], b"empty", vs[1][2], vs[2][2]]
    aggs, ast, vst = _both(impl, groups, pks, msgs)
    assert ast == [OK, ERR_COMBINE, OK, OK] and vst == [OK, ERR_COMBINE, OK, OK]
    assert aggs == [vs[0][3], bytes(96), vs[1][3], vs[2][3]]
    # empty groups at the edges, and nothing but empty groups (no partial at all)
    assert _both(impl, [{}, vs[1][0], {}], [vs[1][1]] * 3, [vs[1][2]] * 3) == \
        ([bytes(96), vs[1][3], bytes(96)], [ERR_COMBINE, OK, ERR_COMBINE], [ERR_COMBINE, OK, ERR_COMBINE])
    assert _both(impl, [{}, {}], [vs[1][1]] * 2, [b"", b"x"]) == ([bytes(96)] * 2, [ERR_COMBINE] * 2, [ERR_COMBINE] * 2)


def test_message_lengths_0_32_33(impl):
    vs = [_validator(impl, 0x360 + n, 4, 6, msg_len=n) for n in (0, 32, 33)]
    assert [len(v[2]) for v in vs] == [0, 32, 33]
    aggs, ast, vst = _both(impl, [v[0] for v in vs], [v[1] for v in vs], [v[2] for v in vs])
    assert aggs == [v[3] for v in vs] and ast == [OK] * 3 and vst == [OK] * 3
    for v in vs:  # and each alone
        assert _both(impl, [v[0]], [v[1]], [v[2]]) == ([v[3]], [OK], [OK])
    assert _oracle(vs[0][0], vs[0][1], vs[0][2]) == (vs[0][3], OK, OK)


# ------------------------------------------------------------------------------------------------ 3. ids
def test_non_contiguous_and_field_path_ids(impl):
    small = _validator(impl, 0x400, 3, 10, ids=[2, 5, 9])
    field = _field_validator(impl, 0x401, [1, 2 ** 40, -5], 3)
    for v in (small, field):
        assert _both(impl, [v[0]], [v[1]], [v[2]]) == ([v[3]], [OK], [OK])
        assert _oracle(v[0], v[1], v[2]) == (v[3], OK, OK)
    # side by side, either order: the path is the group's
    for vs in ((small, field), (field, small)):
        aggs, ast, vst = _both(impl, [v[0] for v in vs], [v[1] for v in vs], [v[2] for v in vs])
        assert aggs == [v[3] for v in vs] and ast == [OK, OK] and vst == [OK, OK]


# ------------------------------------------------------------------------------------------------ 4. failures
@pytest.fixture(scope="module")
def base(impl):
    """A valid 4-of-6 duty to break, three valid neighbours, and small-order points from the stored fixture."""
    with open(os.path.join(ROOT, "tests", "golden", "fixtures.json")) as f:
        so = json.load(f)["small_order"]
    return dict(v=_validator(impl, 0x500, 4, 6), other=_validator(impl, 0x501, 4, 6),
                nb=[_validator(impl, 0x510 + k, t, 10) for k, t in enumerate((7, 4, 2))],
                small_sig=bytes.fromhex(so["verify"][0]["sig"]), small_pk=bytes.fromhex(so["verify"][16]["pk"]))


def _failure(base, case):
    """(partials, root key, message, expected aggregate status, expected verify status) of a failure case."""
    parts, pk, msg, _ = base["v"]
    parts = dict(parts)
    ids = list(parts)
    if case == "partial_bad_encoding":
        parts[ids[1]] = bytes([parts[ids[1]][0] & 0x7F]) + parts[ids[1]][1:]  # compression flag cleared
        return parts, pk, msg, ERR_SIGNATURE, ERR_SIGNATURE
    if case == "partial_off_subgroup":
        parts[ids[2]] = base["small_sig"]
        return parts, pk, msg, ERR_SIGNATURE, ERR_SIGNATURE
    if case == "partial_at_infinity":  # deserializes; the aggregate is then of another polynomial
        parts[ids[0]] = INF
        return parts, pk, msg, OK, ERR_VERIFY
    if case == "duplicate_id":  # the Go map cannot hold one, the C ABI can: packed by hand below
        return [(ids[0], parts[ids[0]]), (ids[1], parts[ids[1]]), (ids[0], parts[ids[2]])], pk, msg, ERR_COMBINE, \
            ERR_COMBINE
    if case == "id_zero":
        parts = {0: parts[ids[0]], **{i: parts[i] for i in ids[1:]}}
        return parts, pk, msg, ERR_COMBINE, ERR_COMBINE
    if case == "bad_encoding_and_duplicate_id":  # the deserialization error is reported first
        bad = bytes([parts[ids[1]][0] & 0x7F]) + parts[ids[1]][1:]
        return [(ids[0], parts[ids[0]]), (ids[0], parts[ids[2]]), (ids[1], bad)], pk, msg, ERR_SIGNATURE, ERR_SIGNATURE
    if case == "swapped_share":  # another validator's partial under this id: aggregate bytes, failed Verify
        parts[ids[3]] = base["other"][0][list(base["other"][0])[0]]
        return parts, pk, msg, OK, ERR_VERIFY
    if case == "wrong_message":
        return parts, pk, msg[:-1] + bytes([msg[-1] ^ 1]), OK, ERR_VERIFY
    if case == "root_key_bad_encoding":
        return parts, bytes([pk[0] & 0x7F]) + pk[1:], msg, OK, ERR_PUBKEY
    if case == "root_key_off_subgroup":
        return parts, base["small_pk"], msg, OK, ERR_PUBKEY
    if case == "root_key_at_infinity":
        return parts, b"\xc0" + bytes(47), msg, OK, ERR_VERIFY
    if case == "sum_to_infinity":  # ids {1, 2, 3}: lambda = 3, -3, 1, so P, P, infinity cancel
        p = parts[ids[0]]
        return {1: p, 2: p, 3: INF}, pk, msg, OK, ERR_VERIFY
    if case == "two_infinity_partials":
        return {1: INF, 2: INF}, pk, msg, OK, ERR_VERIFY
    raise AssertionError(case)


class _Pairs:
    """A group with a repeated id, which a dict cannot hold: items() yields the pairs in order (all that _pack and the
    oracle's threshold_aggregate read of a group)."""

    def __init__(self, pairs):
        self.pairs = list(pairs)

    def items(self):
        return list(self.pairs)


FAILURES = ["partial_bad_encoding", "partial_off_subgroup", "partial_at_infinity", "duplicate_id", "id_zero",
            "bad_encoding_and_duplicate_id", "swapped_share", "wrong_message", "root_key_bad_encoding",
            "root_key_off_subgroup", "root_key_at_infinity", "sum_to_infinity", "two_infinity_partials"]


@pytest.mark.parametrize("case", FAILURES)
def test_failure_alone_and_beside_valid_groups(impl, base, case):
    parts, pk, msg, want_ast, want_vst = _failure(base, case)
    if isinstance(parts, list):
        parts = _Pairs(parts)
    aggs, ast, vst = _both(impl, [parts], [pk], [msg])
    assert (ast, vst) == ([want_ast], [want_vst])
    if want_ast != OK:
        assert aggs == [bytes(96)]
    elif case in ("sum_to_infinity", "two_infinity_partials"):
        assert aggs == [INF]
    else:
        assert aggs[0][0] & 0x80 and aggs != [INF]
    o_agg, o_ast, o_vst = _oracle(parts, pk, msg)
    assert (o_ast, o_vst) == (want_ast, want_vst)
    if o_agg is not None:
        assert o_agg == aggs[0]
    # beside three valid groups, at the second place: theirs are untouched, its own as alone
    nb = base["nb"]
    groups = [nb[0][0], parts, nb[1][0], nb[2][0]]
    got = _both(impl, groups, [nb[0][1], pk, nb[1][1], nb[2][1]], [nb[0][2], msg, nb[1][2], nb[2][2]])
    assert got == ([nb[0][3], aggs[0], nb[1][3], nb[2][3]], [OK, want_ast, OK, OK], [OK, want_vst, OK, OK])


# ------------------------------------------------------------------------------------------------ 5. workspace reuse
def _five_calls(impl, base):
    """Five consecutive lone calls' inputs, alternating 7-of-10 / 4-of-6 and valid / invalid, with what each returns."""
    calls = []
    for k in range(5):
        t, total = ((7, 10), (4, 6))[k % 2]
        parts, pk, msg, want = _validator(impl, 0x600 + k, t, total)
        if k % 2 == 0:
            calls.append((parts, pk, msg, want, OK, OK))
        elif k == 1:  # a partial of another duty: bytes, but not verified
            parts = dict(parts)
            parts[list(parts)[0]] = base["v"][0][list(base["v"][0])[0]]
            calls.append((parts, pk, msg, None, OK, ERR_VERIFY))
        else:  # an undecodable partial
            parts = dict(parts)
            i = list(parts)[-1]
            parts[i] = bytes([parts[i][0] & 0x7F]) + parts[i][1:]
            calls.append((parts, pk, msg, bytes(96), ERR_SIGNATURE, ERR_SIGNATURE))
    return calls


def test_five_consecutive_calls_reuse_both_workspace_sets(impl, base):
    calls = _five_calls(impl, base)
    forced = [_forced(impl, _tv, [c[0]], [c[1]], [c[2]]) for c in calls]
    for _ in range(2):
        for c, f in zip(calls, forced):
            aggs, ast, vst = _tv(impl, [c[0]], [c[1]], [c[2]])
            assert (ast, vst) == ([c[4]], [c[5]])
            if c[3] is not None:
                assert aggs == [c[3]]
            assert (aggs, ast, vst) == f


def test_five_consecutive_device_calls_on_a_torch_stream(impl, base):
    """hipbls_threshold_aggregate_verify_batch_device with resident inputs: the five calls enqueued back to back on one
    stream, read after one synchronize."""
    import torch
    dev = torch.device("cuda", 0)
    calls = _five_calls(impl, base)
    forced = [_forced(impl, _tv, [c[0]], [c[1]], [c[2]]) for c in calls]

    def u8(b):
        return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)

    bufs = []
    for parts, pk, msg, _, _, _ in calls:
        ids = list(parts)
        bufs.append(dict(sig=u8(b"".join(parts[i] for i in ids)), ids=torch.tensor(ids, dtype=torch.int64).to(dev),
                         off=torch.tensor([0, len(ids)], dtype=torch.int64).to(dev), pk=u8(pk), msg=u8(msg),
                         moff=torch.tensor([0, len(msg)], dtype=torch.int64).to(dev),
                         out=torch.full((96,), 0xEE, dtype=torch.uint8, device=dev),
                         ast=torch.full((1,), -1, dtype=torch.int32, device=dev),
                         vst=torch.full((1,), -1, dtype=torch.int32, device=dev), n=len(ids)))
    s = torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    for b in bufs:
        rc = impl.lib.hipbls_threshold_aggregate_verify_batch_device(
            b["sig"].data_ptr(), b["ids"].data_ptr(), b["off"].data_ptr(), 1, b["n"], b["pk"].data_ptr(),
            b["msg"].data_ptr(), b["moff"].data_ptr(), b["out"].data_ptr(), b["ast"].data_ptr(), b["vst"].data_ptr(),
            ctypes.c_void_p(s.cuda_stream))
        assert rc == 0
    torch.cuda.synchronize(dev)
    for b, f in zip(bufs, forced):
        got = ([bytes(b["out"].cpu().numpy().tobytes())], b["ast"].cpu().tolist(), b["vst"].cpu().tolist())
        assert got == f


# ------------------------------------------------------------------------------------------------ 6. concurrency
def test_four_threads_of_lone_calls(impl, base):
    """Four host threads, eight lone sigagg calls each, every thread on inputs of its own (a 7-of-10 and a 4-of-6 duty,
    a failing one every fourth call)."""
    duties = []
    for th in range(4):
        mine = []
        for k in range(2):
            t, total = ((7, 10), (4, 6))[k]
            parts, pk, msg, want = _validator(impl, 0x700 + 16 * th + k, t, total)
            mine.append((parts, pk, msg, ([want], [OK], [OK])))
        parts, pk, msg, _ = mine[0]
        bad = dict(parts)
        bad[list(bad)[0]] = base["v"][0][list(base["v"][0])[0]]
        mine.append((bad, pk, msg, _forced(impl, _tv, [bad], [pk], [msg])))
        assert mine[2][3][1:] == ([OK], [ERR_VERIFY])
        duties.append(mine)
    errors = []

    def worker(th):
        try:
            for k in range(8):
                parts, pk, msg, want = duties[th][2 if k % 4 == 3 else k % 2]
                got = _tv(impl, [parts], [pk], [msg])
                if got != want:
                    errors.append((th, k, got[1], got[2]))
        except Exception as e:  # a thread's exception must fail the test, not vanish
            errors.append((th, repr(e)))

    threads = [threading.Thread(target=worker, args=(th,)) for th in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
