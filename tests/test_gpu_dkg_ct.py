"""A joint-Feldman dealing round on the GPU (charon_amd/csrc/dkg_ct.hip):
hipbls_deal_commit_batch_ct, hipbls_verify_secret_shares_batch_ct and hipbls_combine_shares_batch_ct against the oracle
(tests/dkg_vectors.py, computed once per process) with guarded output buffers, lane counts around the workgroup
(kBlock = 64 = one wave) with the faults at the wave boundaries, the round trip with the existing split and share
calls, a whole ceremony at the smallest honest size, the argument errors, the _device forms, two contexts on one GPU,
and which kernels each call launches.
"""
import ctypes
import itertools
import os
import random
import re
import subprocess
import sys

import pytest

from tests import dkg_vectors as V

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_BLOCK = 64
ERR_ARG = 16
R = V.R


@pytest.fixture(scope="module")
def impl():
    from charon_amd.tbls import HipBLS
    return HipBLS()


def _guarded(n, width):
    return ctypes.create_string_buffer(b"\xee" * (width * (n + 1)), width * (n + 1))


def _status(n):
    return (ctypes.c_int32 * (n + 1))(*([-7] * (n + 1)))


def _c_deal(lib, d):
    """hipbls_deal_commit_batch_ct through ctypes with 0xee-filled outputs one entry too long and -7-filled status
    arrays one entry too long: (rc, shares, status, commitments, com_status); the extra entries must come back
    untouched."""
    n, t, tot = d.n_val, d.threshold, d.total
    out, com = _guarded(n * tot, 32), _guarded(n * t, 48)
    st, cst = _status(n), _status(n * t)
    tails = b"".join(b"".join(x) for x in d.tails())
    rc = lib.hipbls_deal_commit_batch_ct(b"".join(d.secrets()), tails or None, n, tot, t, out, st, com, cst)
    raw, craw = out.raw, com.raw
    assert raw[32 * n * tot:] == b"\xee" * 32 and craw[48 * n * t:] == b"\xee" * 48 and st[n] == -7 and cst[n * t] == -7
    return (rc, [[raw[32 * (tot * v + i):32 * (tot * v + i) + 32] for i in range(tot)] for v in range(n)], list(st)[:n],
            [[craw[48 * (t * v + j):48 * (t * v + j) + 48] for j in range(t)] for v in range(n)],
            [list(cst)[t * v:t * v + t] for v in range(n)])


def _c_check(lib, c):
    n = c.n_val * c.n_dealers
    st = _status(n)
    rc = lib.hipbls_verify_secret_shares_batch_ct(c.flat_shares(), c.flat_commitments(), c.n_val, c.n_dealers,
                                                  c.threshold, c.my_id, st)
    assert st[n] == -7
    return rc, [list(st)[c.n_dealers * v:c.n_dealers * (v + 1)] for v in range(c.n_val)]


def _c_combine(lib, c, with_pubs=True):
    n = c.n_val
    out, pubs = _guarded(n, 32), _guarded(n, 48)
    st, pst = _status(n), _status(n)
    rc = lib.hipbls_combine_shares_batch_ct(c.flat_shares(), c.flat_include(), n, c.n_dealers, out, st,
                                            pubs if with_pubs else None, pst if with_pubs else None)
    raw, praw = out.raw, pubs.raw
    assert raw[32 * n:] == b"\xee" * 32 and st[n] == -7
    if with_pubs:
        assert praw[48 * n:] == b"\xee" * 48 and pst[n] == -7
    else:
        assert praw == b"\xee" * (48 * (n + 1)) and list(pst) == [-7] * (n + 1)
    return (rc, [raw[32 * v:32 * v + 32] for v in range(n)], list(st)[:n],
            [praw[48 * v:48 * v + 48] for v in range(n)], list(pst)[:n])


def _check_dealing(impl, d):
    rc, shares, st, com, cst = _c_deal(impl.lib, d)
    assert rc == 0 and st == d.status, (d.name, st, d.status)
    assert shares == d.shares and com == d.commitments and cst == d.com_status, d.name
    got = impl.deal_commit_batch_ct(d.secrets(), d.tails(), d.total, d.threshold)
    want_shares = [{i + 1: s for i, s in enumerate(row)} for row in d.shares]
    assert got == (want_shares, d.status, d.commitments, d.com_status), d.name


def _check_check(impl, c):
    rc, st = _c_check(impl.lib, c)
    assert rc == 0 and st == c.status, (c.name, st, c.status)
    assert impl.verify_secret_shares_batch_ct(c.shares, c.commitments, c.my_id) == c.status, c.name


def _check_combine(impl, c):
    rc, out, st, pubs, pst = _c_combine(impl.lib, c)
    assert rc == 0 and st == c.status, (c.name, st, c.status)
    assert out == c.out and pubs == c.pubs and pst == c.pub_status, c.name
    rc, out, st, _, _ = _c_combine(impl.lib, c, with_pubs=False)
    assert rc == 0 and st == c.status and out == c.out, c.name
    assert impl.combine_shares_batch_ct(c.shares, c.include) == (c.out, c.status, c.pubs, c.pub_status), c.name
    assert impl.combine_shares_batch_ct(c.shares, c.include, with_pubs=False) == (c.out, c.status, None, None), c.name


# ------------------------------------------------------------------------------------------------ 1. the vectors
def test_deal_commit_against_the_oracle(impl):
    for d in V.dealings():
        _check_dealing(impl, d)


def test_share_check_against_the_oracle(impl):
    for c in V.checks():
        _check_check(impl, c)


def test_combine_against_the_oracle(impl):
    for c in V.combines():
        _check_combine(impl, c)


# ------------------------------------------------------------------------------------------------ 2. wave boundaries
def _positions(n):
    return sorted({0, n - 1} | {p for p in (K_BLOCK - 1, K_BLOCK) if p < n})


LANES = [(63, 1), (64, 1), (65, 1), (129, 1), (21, 3), (13, 5), (43, 3)]  # 63, 64, 65, 129, 63, 65, 129 lanes


@pytest.mark.parametrize("n_val,threshold", LANES)
def test_commitment_lane_counts_around_the_workgroup(impl, n_val, threshold):
    assert n_val * threshold in (63, 64, 65, 129)
    bad_at = {p // threshold for p in _positions(n_val * threshold)}  # the validators that own lanes 0, 63, 64, last
    polys = []
    for v in range(n_val):
        p = [3 + (v + 5 * j) % 11 for j in range(threshold)]  # a small pool: the oracle multiplies each value once
        if v in bad_at:
            p[v % threshold] = R + v
        polys.append(p)
    d = V.Dealing("lanes", threshold, 2, polys)
    assert [v for v, s in enumerate(d.status) if s != V.OK] == sorted(bad_at)
    _check_dealing(impl, d)


@pytest.mark.parametrize("n_val,n_dealers", LANES)
def test_check_lane_counts_around_the_workgroup(impl, n_val, n_dealers):
    n = n_val * n_dealers
    assert n in (63, 64, 65, 129)
    faults = dict(zip(_positions(n), itertools.cycle((V.ERR_SECRET, V.ERR_VERIFY, V.ERR_PUBKEY))))
    bad_enc = sorted(V.VS.bad_encodings().values())
    shares, com = [], []
    for v in range(n_val):
        srow, crow = [], []
        for d in range(n_dealers):
            lane = v * n_dealers + d
            coeffs = [3 + lane % 11, 20 + lane % 7]  # at id 1 the share is their sum
            share, poly = V.b32(sum(coeffs)), [V.enc(c) for c in coeffs]
            f = faults.get(lane)
            if f == V.ERR_SECRET:
                share = V.b32(R + lane)
            elif f == V.ERR_VERIFY:
                share = V.b32(sum(coeffs) + 1)
            elif f == V.ERR_PUBKEY:
                poly[lane % 2] = bad_enc[lane % len(bad_enc)]
            srow.append(share)
            crow.append(poly)
        shares.append(srow)
        com.append(crow)
    c = V.Check("lanes", shares, com, 1)
    flat = [s for row in c.status for s in row]
    assert {i: s for i, s in enumerate(flat) if s != V.OK} == faults
    _check_check(impl, c)


@pytest.mark.parametrize("n_val", [63, 64, 65, 129])
def test_sum_lane_counts_around_the_workgroup(impl, n_val):
    pos = _positions(n_val)
    shares = [[V.b32(1000 * (v % 5) + 10 * d + 1) for d in range(3)] for v in range(n_val)]  # sums from a small pool
    include = [[1, 1, 1] for _ in range(n_val)]
    want = {}
    for k, p in enumerate(pos):  # an excluded dealer, a bad share, an excluded bad share, nobody: in turn
        kind = k % 4
        if kind == 0:
            include[p][1] = 0
        elif kind == 1:
            shares[p][2] = V.b32(R + p)
            want[p] = V.ERR_SECRET
        elif kind == 2:
            shares[p][0] = V.b32(2**256 - 1)
            include[p][0] = 0
        else:
            include[p] = [0, 0, 0]
            want[p] = V.ERR_COMBINE
    c = V.Combine("lanes", shares, include)
    assert {v: s for v, s in enumerate(c.status) if s != V.OK} == want
    _check_combine(impl, c)


# ------------------------------------------------------------------------------------------------ 3. the existing calls
def test_round_trip_with_the_split_and_the_share_call(impl):
    rng = random.Random(2121)
    n, total, threshold = 8, 10, 7
    secrets = [V.b32(rng.randrange(1, R)) for _ in range(n)]
    tails = [[V.b32(rng.randrange(1, R)) for _ in range(threshold - 1)] for _ in range(n)]
    shares, st, com, cst = impl.deal_commit_batch_ct(secrets, tails, total, threshold)
    assert st == [V.OK] * n and cst == [[V.OK] * threshold] * n
    s_shares, s_st, s_pubs, s_pst = impl.threshold_split_batch_ct(secrets, tails, total, threshold)
    assert (shares, st) == (s_shares, s_st)
    got, gst = impl.public_key_share_batch([[c] for c in com], list(range(total + 1)))
    assert gst == [V.OK] * n
    assert got == s_pubs  # k = 0 the root key, k = 1..10 the pubshares, entry for entry
    # and the dealer's own shares pass the receivers' check at every id
    for my_id in (1, 10):
        vst = impl.verify_secret_shares_batch_ct([[shares[v][my_id]] for v in range(n)], [[c] for c in com], my_id)
        assert vst == [[V.OK]] * n


# ------------------------------------------------------------------------------------------------ 4. a whole ceremony
def test_whole_ceremony(impl):
    """4 operators, threshold 3, 5 validators: every operator deals, every operator checks what it received and sums
    the qualified dealers' shares; the cluster then holds a 3-of-4 sharing of the sum of the qualified secrets."""
    rng = random.Random(4355)
    ops, threshold, n_val = 4, 3, 5
    secret = [[rng.randrange(1, R) for _ in range(n_val)] for _ in range(ops)]  # [dealer][validator]
    dealt = []
    for d in range(ops):
        tails = [[V.b32(rng.randrange(1, R)) for _ in range(threshold - 1)] for _ in range(n_val)]
        shares, st, com, cst = impl.deal_commit_batch_ct([V.b32(s) for s in secret[d]], tails, ops, threshold)
        assert st == [V.OK] * n_val and cst == [[V.OK] * threshold] * n_val
        dealt.append((shares, com))
    # what goes wrong: dealer 3 sends operator 2 a forged share for validator 1, and dealer 0 publishes another
    # validator's commitment list for validator 3
    published = [[dealt[d][1][v] for d in range(ops)] for v in range(n_val)]  # [validator][dealer]
    published[3][0] = dealt[0][1][4]
    complaints = set()
    received = {}
    for i in range(1, ops + 1):
        mine = [[dealt[d][0][v][i] for d in range(ops)] for v in range(n_val)]
        if i == 2:
            forged = bytearray(mine[1][3])
            forged[31] ^= 1
            mine[1][3] = bytes(forged)
        vst = impl.verify_secret_shares_batch_ct(mine, published, i)
        want = [[V.OK] * ops for _ in range(n_val)]
        want[3][0] = V.ERR_VERIFY
        if i == 2:
            want[1][3] = V.ERR_VERIFY
        assert vst == want, i
        complaints |= {(v, d) for v in range(n_val) for d in range(ops) if vst[v][d] != V.OK}
        received[i] = mine
    assert complaints == {(1, 3), (3, 0)}
    include = [[(v, d) not in complaints for d in range(ops)] for v in range(n_val)]
    final, final_pub = {}, {}
    for i in range(1, ops + 1):
        out, st, pubs, pst = impl.combine_shares_batch_ct(received[i], include)
        assert st == [V.OK] * n_val and pst == [V.OK] * n_val
        final[i], final_pub[i] = out, pubs
    group_secret = [sum(secret[d][v] for d in range(ops) if include[v][d]) % R for v in range(n_val)]
    subsets = list(itertools.combinations(range(1, ops + 1), threshold))
    secs, rst, pks, kst = impl.recover_secret_batch_ct([{i: final[i][v] for i in ids} for v in range(n_val)
                                                        for ids in subsets])
    assert rst == [V.OK] * len(secs) and kst == [V.OK] * len(secs)
    assert secs == [V.b32(group_secret[v]) for v in range(n_val) for _ in subsets]
    # the public side: a disqualified dealer's polynomial is replaced by the identity polynomial
    qualified = [[published[v][d] if include[v][d] else [V.INF48] * threshold for d in range(ops)]
                 for v in range(n_val)]
    pubs, pst = impl.public_key_share_batch(qualified, list(range(ops + 1)))
    assert pst == [V.OK] * n_val
    for v in range(n_val):
        assert [final_pub[i][v] for i in range(1, ops + 1)] == pubs[v][1:], v
        assert pubs[v][0] == pks[v * len(subsets)], v
    msg = b"a duty signed by the dealt cluster"
    ids = (1, 3, 4)
    sigs, sst = impl.sign_batch_ct([final[i][2] for i in ids], [msg] * 3)
    assert sst == [V.OK] * 3
    impl.verify(pubs[2][0], msg, impl.threshold_aggregate(dict(zip(ids, sigs))))


# ------------------------------------------------------------------------------------------------ 5. forms, arguments
def test_argument_rules(impl):
    lib = impl.lib
    sec = V.b32(5) * 4
    com = V.enc(5) * 8
    out = ctypes.create_string_buffer(b"\xee" * 480, 480)
    out2 = ctypes.create_string_buffer(b"\xee" * 480, 480)
    st = (ctypes.c_int32 * 8)(*([-7] * 8))
    st2 = (ctypes.c_int32 * 8)(*([-7] * 8))
    inc = bytes([1] * 8)

    deal = lib.hipbls_deal_commit_batch_ct
    assert deal(None, None, 0, 1, 1, None, None, None, None) == 0  # a count of 0
    bad = [(sec, sec, 1, 1, 0, out, st, out2, st2),         # threshold == 0
           (sec, sec, 1, 0, 1, out, st, out2, st2),         # total == 0
           (sec, sec, 0, 0, 1, out, st, out2, st2),         # ... with nothing to do
           (None, sec, 1, 3, 2, out, st, out2, st2), (sec, None, 1, 3, 2, out, st, out2, st2),
           (sec, sec, 1, 3, 2, None, st, out2, st2), (sec, sec, 1, 3, 2, out, None, out2, st2),
           (sec, sec, 1, 3, 2, out, st, None, st2),         # only one of the output pair
           (sec, sec, 1, 3, 2, out, st, out2, None),
           (sec, sec, 1, 3, 2, out, st, None, None),
           (sec, sec, 1 << 31, 1, 1, out, st, out2, st2),   # lane counts >= 2^31
           (sec, sec, 1 << 20, (1 << 11) - 1, 1, out, st, out2, st2),
           (sec, sec, 1 << 16, 1, 1 << 15, out, st, out2, st2),
           (sec, sec, 1, 1, 65536, out, st, out2, st2)]     # threshold > 65,535
    for args in bad:
        assert deal(*args) == ERR_ARG, args[2:5]
        assert lib.hipbls_last_error() == b"bad deal arguments"
        assert lib.hipbls_deal_commit_batch_ct_device(*args, None) == ERR_ARG, args[2:5]

    check = lib.hipbls_verify_secret_shares_batch_ct
    assert check(None, None, 0, 1, 1, 1, None) == 0
    bad = [(sec, com, 1, 1, 0, 1, st), (sec, com, 1, 0, 1, 1, st), (sec, com, 0, 0, 1, 1, st),
           (None, com, 1, 1, 1, 1, st), (sec, None, 1, 1, 1, 1, st), (sec, com, 1, 1, 1, 1, None),
           (sec, com, 1 << 31, 1, 1, 1, st), (sec, com, 1 << 16, 1 << 15, 1, 1, st),
           (sec, com, 1 << 16, 1, 1 << 15, 1, st), (sec, com, 1, 1 << 16, 1 << 15, 1, st),
           (sec, com, 1, 1, 65536, 1, st)]
    for args in bad:
        assert check(*args) == ERR_ARG, args[2:5]
        assert lib.hipbls_last_error() == b"bad share check arguments"
        assert lib.hipbls_verify_secret_shares_batch_ct_device(*args, None) == ERR_ARG, args[2:5]

    combine = lib.hipbls_combine_shares_batch_ct
    assert combine(None, None, 0, 1, None, None, None, None) == 0
    bad = [(sec, inc, 1, 0, out, st, out2, st2), (sec, inc, 0, 0, out, st, out2, st2),
           (None, inc, 1, 2, out, st, out2, st2), (sec, inc, 1, 2, None, st, out2, st2),
           (sec, inc, 1, 2, out, None, out2, st2), (sec, inc, 1, 2, out, st, None, st2),
           (sec, inc, 1, 2, out, st, out2, None), (sec, inc, 1 << 31, 1, out, st, out2, st2),
           (sec, inc, 1 << 16, 1 << 15, out, st, out2, st2), (sec, None, 1, 1 << 31, out, st, out2, st2)]
    for args in bad:
        assert combine(*args) == ERR_ARG, args[2:4]
        assert lib.hipbls_last_error() == b"bad combine arguments"
        assert lib.hipbls_combine_shares_batch_ct_device(*args, None) == ERR_ARG, args[2:4]
    assert out.raw == out2.raw == b"\xee" * 480 and list(st) == list(st2) == [-7] * 8
    # a null include mask is every dealer, not an error
    assert combine(sec, None, 2, 2, out, st, None, None) == 0 and list(st)[:3] == [0, 0, -7]
    assert out.raw[:64] == V.b32(10) * 2 and out.raw[64:] == b"\xee" * 416


def test_device_forms_equal_host_calls(impl):
    import torch
    lib = impl.lib
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(dev)
    stream = ctypes.c_void_p(s.cuda_stream)

    def dbytes(b):
        return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)

    def guarded(n, width):
        return torch.full((width * (n + 1),), 0xEE, dtype=torch.uint8, device=dev)

    def status(n):
        return torch.full((n + 1,), -7, dtype=torch.int32, device=dev)

    def raw(t):
        return bytes(t.cpu().numpy().tobytes())

    d = V.dealings()[2]
    n, t, tot = d.n_val, d.threshold, d.total
    d_sec, d_tail = dbytes(b"".join(d.secrets())), dbytes(b"".join(b"".join(x) for x in d.tails()))
    d_out, d_com, d_st, d_cst = guarded(n * tot, 32), guarded(n * t, 48), status(n), status(n * t)
    torch.cuda.synchronize(dev)
    assert lib.hipbls_deal_commit_batch_ct_device(d_sec.data_ptr(), d_tail.data_ptr(), n, tot, t, d_out.data_ptr(),
                                                  d_st.data_ptr(), d_com.data_ptr(), d_cst.data_ptr(), stream) == 0
    torch.cuda.synchronize(dev)
    assert raw(d_out) == b"".join(x for row in d.shares for x in row) + b"\xee" * 32
    assert raw(d_com) == b"".join(x for row in d.commitments for x in row) + b"\xee" * 48
    assert d_st.cpu().tolist() == d.status + [-7]
    assert d_cst.cpu().tolist() == [x for row in d.com_status for x in row] + [-7]

    for c in V.checks():
        if c.name not in ("edge_shares", "bad_encodings", "t7_id-9223372036854775808"):
            continue
        m = c.n_val * c.n_dealers
        d_sh, d_cm, d_st = dbytes(c.flat_shares()), dbytes(c.flat_commitments()), status(m)
        torch.cuda.synchronize(dev)
        assert lib.hipbls_verify_secret_shares_batch_ct_device(d_sh.data_ptr(), d_cm.data_ptr(), c.n_val, c.n_dealers,
                                                               c.threshold, c.my_id, d_st.data_ptr(), stream) == 0
        torch.cuda.synchronize(dev)
        assert d_st.cpu().tolist() == [x for row in c.status for x in row] + [-7], c.name

    for c in V.combines():
        n = c.n_val
        d_sh = dbytes(c.flat_shares())
        d_inc = dbytes(c.flat_include()) if c.include is not None else None
        d_out, d_pub, d_st, d_pst = guarded(n, 32), guarded(n, 48), status(n), status(n)
        torch.cuda.synchronize(dev)
        assert lib.hipbls_combine_shares_batch_ct_device(d_sh.data_ptr(), d_inc.data_ptr() if d_inc is not None else None,
                                                         n, c.n_dealers, d_out.data_ptr(), d_st.data_ptr(),
                                                         d_pub.data_ptr(), d_pst.data_ptr(), stream) == 0
        torch.cuda.synchronize(dev)
        assert raw(d_out) == b"".join(c.out) + b"\xee" * 32 and raw(d_pub) == b"".join(c.pubs) + b"\xee" * 48, c.name
        assert d_st.cpu().tolist() == c.status + [-7] and d_pst.cpu().tolist() == c.pub_status + [-7], c.name
    # nothing to do: no launch, nothing touched
    assert lib.hipbls_deal_commit_batch_ct_device(None, None, 0, 1, 1, None, None, None, None, None) == 0
    assert lib.hipbls_verify_secret_shares_batch_ct_device(None, None, 0, 1, 1, 1, None, None) == 0
    assert lib.hipbls_combine_shares_batch_ct_device(None, None, 0, 1, None, None, None, None, None) == 0


def test_two_contexts_equal_one(impl):
    """2,200 validators are split over two contexts (whole validators) by each of the three calls; the child process
    binds both to device 0 and must return this process's bytes."""
    from tests import dkg_child as C
    want = C.digest(impl)
    r = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "tests", "dkg_child.py"), "2"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == want, r.stdout


# ------------------------------------------------------------------------------------------------ 6. routing
def _timed_names():
    with open(os.path.join(ROOT, "charon_amd", "csrc", "hipbls.hip")) as f:
        return sorted(set(re.findall(r'timed\(c, "([a-z0-9_]+)"', f.read())))


def _launched(impl):
    got = {}
    for name in _timed_names():
        a, c = ctypes.c_double(), ctypes.c_uint64()
        assert impl.lib.hipbls_kernel_timing(name.encode(), ctypes.byref(a), ctypes.byref(c)) == 0
        if c.value:
            got[name] = c.value
    return got


def test_routing(impl):
    assert {"commit_ct", "share_check_ct", "share_sum_ct"} <= set(_timed_names())
    d = V.dealings()[1]
    c = V.checks()[1]
    u = V.combines()[1]
    impl.threshold_split_batch_ct(d.secrets()[:1], d.tails()[:1], 3, 2)  # the comb is built by the first deal of a context
    lib = impl.lib
    lib.hipbls_set_timing(1)
    try:
        lib.hipbls_kernel_timing_reset()
        impl.deal_commit_batch_ct(d.secrets(), d.tails(), d.total, d.threshold)
        assert _launched(impl) == {"deal_ct": 1, "commit_ct": 1}
        lib.hipbls_kernel_timing_reset()
        impl.verify_secret_shares_batch_ct(c.shares, c.commitments, c.my_id)
        assert _launched(impl) == {"g1_decode": 1, "vss_eval": 1, "share_check_ct": 1}
        lib.hipbls_kernel_timing_reset()
        impl.combine_shares_batch_ct(u.shares, u.include)
        assert _launched(impl) == {"share_sum_ct": 1}
        # the calls that were there before launch what they launched before
        lib.hipbls_kernel_timing_reset()
        impl.threshold_split_batch_ct(d.secrets(), d.tails(), d.total, d.threshold)
        assert _launched(impl) == {"deal_ct": 1}
        lib.hipbls_kernel_timing_reset()
        impl.public_key_share_batch([[x] for x in d.commitments[:2]], [0, 1])
        assert _launched(impl) == {"g1_decode": 1, "vss_eval": 1}
    finally:
        lib.hipbls_set_timing(0)
