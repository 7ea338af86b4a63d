"""Batched PublicKeyShare / PublicKeyRecover on the GPU (charon_amd/csrc/vss.hip):
hipbls_public_key_share_batch and hipbls_public_key_recover_batch against the oracle (tests/vss_vectors.py, computed
once per process), against the existing deal (threshold_split_batch_ct's public keys), joint dealings, the Feldman
checks of the binding, lane counts around the workgroup (kBlock = 64 = one wave) with bad validators / groups at the
wave boundaries and guarded output buffers, the _device forms, the argument errors, two contexts on one GPU, and which
kernels each call launches.
"""
import ctypes
import os
import random
import re
import subprocess
import sys

import pytest

from oracle import bls12381 as O
from tests import vss_vectors as V

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_BLOCK = 64
ERR_ARG = 16
VSS_NAMES = {"g1_decode", "vss_dealer_sum", "vss_eval", "vss_scale", "vss_sum"}


@pytest.fixture(scope="module")
def impl():
    from charon_amd.tbls import HipBLS
    return HipBLS()


@pytest.fixture(scope="module")
def deal(impl):
    """8 random validators at 7-of-10 dealt by the existing call: (secrets, tails, shares, pubs, commitments)."""
    rng = random.Random(2020)
    n, total, threshold = 8, 10, 7
    secrets = [rng.randrange(1, V.R).to_bytes(32, "big") for _ in range(n)]
    tails = [[rng.randrange(1, V.R).to_bytes(32, "big") for _ in range(threshold - 1)] for _ in range(n)]
    shares, st, pubs, pst = impl.threshold_split_batch_ct(secrets, tails, total, threshold)
    assert st == [V.OK] * n and all(s == V.OK for row in pst for s in row)
    flat, cst = impl.secret_to_public_key_batch([c for v in range(n) for c in [secrets[v]] + tails[v]])
    assert cst == [V.OK] * (n * threshold)
    com = [[flat[threshold * v:threshold * (v + 1)]] for v in range(n)]
    return secrets, tails, shares, pubs, com


def _c_share(lib, commitments, n_val, n_dealers, threshold, ids):
    """hipbls_public_key_share_batch through ctypes with 0xee-filled outputs one entry too long: (rc, pubs, status);
    the extra entries must come back untouched."""
    m = len(ids)
    out = ctypes.create_string_buffer(b"\xee" * (48 * (n_val * m + 1)), 48 * (n_val * m + 1))
    st = (ctypes.c_int32 * (n_val + 1))(*([-7] * (n_val + 1)))
    arr = (ctypes.c_int64 * max(m, 1))(*ids)
    rc = lib.hipbls_public_key_share_batch(commitments, n_val, n_dealers, threshold, arr, m, out, st)
    raw = out.raw
    assert raw[48 * n_val * m:] == b"\xee" * 48 and st[n_val] == -7
    return rc, [[raw[48 * (m * v + i):48 * (m * v + i) + 48] for i in range(m)] for v in range(n_val)], list(st)[:n_val]


def _c_recover(lib, gs):
    """hipbls_public_key_recover_batch through ctypes, guarded as _c_share: (rc, keys, status)."""
    n = len(gs)
    ids = [i for g in gs for i, _ in g.pairs]
    offs = [0]
    for g in gs:
        offs.append(offs[-1] + len(g.pairs))
    out = ctypes.create_string_buffer(b"\xee" * (48 * (n + 1)), 48 * (n + 1))
    st = (ctypes.c_int32 * (n + 1))(*([-7] * (n + 1)))
    rc = lib.hipbls_public_key_recover_batch(b"".join(p for g in gs for _, p in g.pairs) or None,
                                             (ctypes.c_int64 * max(len(ids), 1))(*ids),
                                             (ctypes.c_uint64 * (n + 1))(*offs), n, out, st)
    raw = out.raw
    assert raw[48 * n:] == b"\xee" * 48 and st[n] == -7
    return rc, [raw[48 * g:48 * g + 48] for g in range(n)], list(st)[:n]


def _check_call(impl, c):
    rc, pubs, st = _c_share(impl.lib, c.flat(), c.n_val, c.n_dealers, c.threshold, c.ids)
    assert rc == 0 and st == c.status, (c.name, st, c.status)
    assert pubs == c.pubs, c.name
    assert impl.public_key_share_batch(c.commitments, c.ids) == (c.pubs, c.status), c.name


def _check_groups(impl, gs):
    rc, keys, st = _c_recover(impl.lib, gs)
    assert rc == 0 and st == [g.status for g in gs], [(g.name, s, g.status) for g, s in zip(gs, st) if s != g.status]
    assert keys == [g.pubkey for g in gs], [g.name for g, k in zip(gs, keys) if k != g.pubkey]


# ------------------------------------------------------------------------------------------------ 1. the vectors
def test_share_batch_against_the_oracle(impl):
    for c in V.share_calls():
        _check_call(impl, c)


def test_recover_batch_against_the_oracle(impl):
    gs = list(V.groups())
    _check_groups(impl, gs)
    for g in gs:  # every group alone, and through the binding
        _check_groups(impl, [g])
    assert impl.public_key_recover_batch([g.pairs for g in gs]) == ([g.pubkey for g in gs], [g.status for g in gs])


# ------------------------------------------------------------------------------------------------ 2. the existing deal
def test_share_batch_equals_the_deal(impl, deal):
    secrets, tails, shares, pubs, com = deal
    got, st = impl.public_key_share_batch(com, list(range(11)))
    assert st == [V.OK] * 8
    assert got == pubs  # k = 0 the root key, k = 1..10 the pubshares, entry for entry


# ------------------------------------------------------------------------------------------------ 3. recover
def test_recover_any_seven_and_verify_pubshares(impl, deal):
    secrets, tails, shares, pubs, com = deal
    subsets = ([1, 2, 3, 4, 5, 6, 7], [10, 9, 8, 6, 4, 3, 1], [2, 9, 4, 7, 10, 5, 8])
    groups = [{i: pubs[v][i] for i in ids} for v in range(8) for ids in subsets]
    keys, st = impl.public_key_recover_batch(groups)
    assert st == [V.OK] * len(groups)
    assert keys == [pubs[v][0] for v in range(8) for _ in subsets]
    for v in (0, 5):
        good = {i: pubs[v][i] for i in range(1, 11)}
        assert impl.verify_pubshares(pubs[v][0], good, 7) is True
        assert impl.verify_pubshares(pubs[v][0], dict(reversed(list(good.items()))), 7) is True
        for pos in (3, 9):  # among the first seven, and among the rest
            other = dict(good)
            other[pos] = pubs[(v + 1) % 8][pos]
            assert impl.verify_pubshares(pubs[v][0], other, 7) is False
        for a, b in ((2, 6), (4, 10), (8, 9)):
            swapped = dict(good)
            swapped[a], swapped[b] = good[b], good[a]
            assert impl.verify_pubshares(pubs[v][0], swapped, 7) is False
        assert impl.verify_pubshares(pubs[(v + 1) % 8][0], good, 7) is False  # another validator's key
        assert impl.verify_pubshares(pubs[v][0], {i: good[i] for i in range(1, 7)}, 7) is False  # too few


# ------------------------------------------------------------------------------------------------ 4. joint dealing
def test_joint_dealing_and_verify_secret_shares(impl, deal):
    secrets, tails, shares, pubs, com = deal
    ids = list(range(11))
    joint = [[com[3 * v + d][0] for d in range(3)] for v in range(2)]  # two validators, three dealers each
    got, st = impl.public_key_share_batch(joint, ids)
    assert st == [V.OK, V.OK]
    single, sst = impl.public_key_share_batch(com[:6], ids)
    assert sst == [V.OK] * 6
    for v in range(2):
        for i in range(11):
            acc = None
            for d in range(3):
                acc = O.g1_add(acc, O.g1_decompress(single[3 * v + d][i]))
            assert got[v][i] == O.g1_compress(acc), (v, i)
    my_id = 4
    mine = [shares[d][my_id] for d in range(3)]  # what dealers 0..2 sent operator 4
    coms = [com[d][0] for d in range(3)]
    assert impl.verify_secret_shares(mine, coms, my_id) == [True, True, True]
    flipped = bytearray(mine[1])
    flipped[31] ^= 1
    assert impl.verify_secret_shares([mine[0], bytes(flipped), mine[2]], coms, my_id) == [True, False, True]
    assert impl.verify_secret_shares(mine, [coms[0], coms[2], coms[1]], my_id) == [True, False, False]
    assert impl.verify_secret_shares(mine, coms, my_id + 1) == [False, False, False]
    assert impl.verify_secret_shares([], [], my_id) == []


# ------------------------------------------------------------------------------------------------ 5. wave boundaries
def _bad_positions(n):
    return sorted({0, n - 1} | {p for p in (K_BLOCK - 1, K_BLOCK) if p < n})


@pytest.mark.parametrize("n_val,n_ids", [(63, 1), (64, 1), (65, 1), (129, 1), (21, 3), (13, 5), (43, 3)])
def test_share_lane_counts_around_the_workgroup(impl, n_val, n_ids):
    assert n_val * n_ids in (63, 64, 65, 129)
    bad = sorted(V.bad_encodings().values())
    # lanes run validator-fastest: lane l is validator l % n_val, so these validators own lanes 0, 63, 64 and the last
    bad_at = {p % n_val for p in _bad_positions(n_val * n_ids)} | {n_val - 1}
    com = []
    for v in range(n_val):
        poly = [V.enc(3 + v % 11), V.enc(20 + v % 7)]
        if v in bad_at:
            poly[v % 2] = bad[v % len(bad)]
        com.append([poly])
    c = V.ShareCall("lanes", com, [1, -2, 0, 3, 1][:n_ids])
    assert [v for v, s in enumerate(c.status) if s != V.OK] == sorted(bad_at)
    _check_call(impl, c)


@pytest.mark.parametrize("n", [63, 64, 65, 129])
def test_recover_group_counts_around_the_workgroup(impl, n):
    base = list(V.groups())
    rng = random.Random(n)
    gs = [base[rng.randrange(len(base))] for _ in range(n)]
    bad = [g for g in base if g.status != V.OK]
    for j, p in enumerate(_bad_positions(n)):
        gs[p] = bad[j % len(bad)]
    _check_groups(impl, gs)


# ------------------------------------------------------------------------------------------------ 6. forms, arguments
def test_device_forms_equal_host_calls(impl):
    import torch
    lib = impl.lib
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(dev)

    def dbytes(b):
        return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)

    for c in V.share_calls():
        if c.name not in ("shape_t7_i11_d3", "bad_encodings", "exceptional"):
            continue
        m = len(c.ids)
        d_com = dbytes(c.flat())
        d_ids = torch.tensor(c.ids, dtype=torch.int64).to(dev)
        d_out = torch.full((48 * (c.n_val * m + 1),), 0xEE, dtype=torch.uint8, device=dev)
        d_st = torch.full((c.n_val + 1,), -7, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        rc = lib.hipbls_public_key_share_batch_device(d_com.data_ptr(), c.n_val, c.n_dealers, c.threshold,
                                                      d_ids.data_ptr(), m, d_out.data_ptr(), d_st.data_ptr(),
                                                      ctypes.c_void_p(s.cuda_stream))
        assert rc == 0
        torch.cuda.synchronize(dev)
        assert bytes(d_out.cpu().numpy().tobytes()) == b"".join(p for row in c.pubs for p in row) + b"\xee" * 48
        assert d_st.cpu().tolist() == c.status + [-7]

    gs = list(V.groups())
    ids = [i for g in gs for i, _ in g.pairs]
    offs = [0]
    for g in gs:
        offs.append(offs[-1] + len(g.pairs))
    n = len(gs)
    d_sh = dbytes(b"".join(p for g in gs for _, p in g.pairs))
    d_ids = torch.tensor(ids, dtype=torch.int64).to(dev)
    d_off = torch.tensor(offs, dtype=torch.int64).to(dev)
    d_out = torch.full((48 * (n + 1),), 0xEE, dtype=torch.uint8, device=dev)
    d_st = torch.full((n + 1,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    rc = lib.hipbls_public_key_recover_batch_device(d_sh.data_ptr(), d_ids.data_ptr(), d_off.data_ptr(), n, len(ids),
                                                    d_out.data_ptr(), d_st.data_ptr(), ctypes.c_void_p(s.cuda_stream))
    assert rc == 0
    torch.cuda.synchronize(dev)
    assert bytes(d_out.cpu().numpy().tobytes()) == b"".join(g.pubkey for g in gs) + b"\xee" * 48
    assert d_st.cpu().tolist() == [g.status for g in gs] + [-7]
    # nothing to do: no launch, nothing touched
    assert lib.hipbls_public_key_share_batch_device(None, 0, 1, 1, None, 1, None, None, None) == 0
    assert lib.hipbls_public_key_recover_batch_device(None, None, None, 0, 0, None, None, None) == 0


def test_argument_rules(impl):
    lib = impl.lib
    com = V.enc(5) * 4
    ids = (ctypes.c_int64 * 4)(1, 2, 3, 4)
    out = ctypes.create_string_buffer(b"\xee" * 480, 480)
    st = (ctypes.c_int32 * 8)(*([-7] * 8))
    share = lib.hipbls_public_key_share_batch
    assert share(None, 0, 1, 1, None, 1, None, None) == 0  # n_val == 0
    assert share(com, 0, 2, 2, ids, 2, out, st) == 0
    bad = [(com, 1, 1, 0, ids, 1, out, st),        # threshold == 0
           (com, 1, 0, 1, ids, 1, out, st),        # n_dealers == 0
           (com, 1, 1, 1, ids, 0, out, st),        # n_ids == 0
           (com, 0, 1, 0, ids, 1, out, st),        # threshold == 0 with nothing to do
           (None, 1, 1, 1, ids, 1, out, st), (com, 1, 1, 1, None, 1, out, st),
           (com, 1, 1, 1, ids, 1, None, st), (com, 1, 1, 1, ids, 1, out, None),
           (com, 1 << 31, 1, 1, ids, 1, out, st),  # counts >= 2^31
           (com, 1, 1, 1, ids, 1 << 31, out, st),
           (com, 1 << 16, 1, 1, ids, 1 << 15, out, st),
           (com, 1 << 16, 1 << 15, 1, ids, 1, out, st),
           (com, 1, 1 << 16, 1 << 15, ids, 1, out, st),
           (com, 1, 1, 65536, ids, 1, out, st)]    # threshold > 65,535
    for args in bad:
        assert share(*args) == ERR_ARG, args[1:4]
        assert lib.hipbls_last_error() == b"bad public key share arguments"
        assert lib.hipbls_public_key_share_batch_device(*args, None) == ERR_ARG, args[1:4]
    assert out.raw == b"\xee" * 480 and list(st) == [-7] * 8
    recover = lib.hipbls_public_key_recover_batch
    offs = (ctypes.c_uint64 * 2)(0, 2)
    assert recover(None, None, None, 0, None, None) == 0  # n_groups == 0
    for args in ((com, ids, None, 1, out, st), (com, ids, offs, 1, None, st), (com, ids, offs, 1, out, None),
                 (None, ids, offs, 1, out, st), (com, None, offs, 1, out, st), (com, ids, offs, 1 << 31, out, st)):
        assert recover(*args) == ERR_ARG
        assert lib.hipbls_last_error() == b"bad public key recover arguments"
    assert recover(com, ids, (ctypes.c_uint64 * 2)(0, 1 << 31), 1, out, st) == ERR_ARG  # the pubshare count
    assert recover(com, ids, (ctypes.c_uint64 * 3)(0, 2, 1), 2, out, st) == ERR_ARG     # offsets that go down
    rdev = lib.hipbls_public_key_recover_batch_device
    for args in ((com, ids, None, 1, 2, out, st), (com, ids, offs, 1, 2, None, st), (com, ids, offs, 1, 2, out, None),
                 (None, ids, offs, 1, 2, out, st), (com, None, offs, 1, 2, out, st),
                 (com, ids, offs, 1 << 31, 2, out, st), (com, ids, offs, 1, 1 << 31, out, st)):
        assert rdev(*args, None) == ERR_ARG
    assert out.raw == b"\xee" * 480 and list(st) == [-7] * 8
    assert recover(None, None, (ctypes.c_uint64 * 2)(0, 0), 1, out, st) == 0 and st[0] == V.ERR_COMBINE  # one empty group
    assert out.raw[:48] == bytes(48) and out.raw[48:] == b"\xee" * 432


def test_two_contexts_equal_one(impl):
    """640 validators and 2,304 groups are split over two contexts (whole validators, whole groups); the child process
    binds both to device 0 and must return this process's bytes."""
    from tests import vss_child as C
    want = C.digest(impl)
    r = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "tests", "vss_child.py"), "2"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == want, r.stdout


# ------------------------------------------------------------------------------------------------ 7. routing
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


def test_routing(impl, deal):
    from charon_amd.tbls import PAIR_SINGLE
    secrets, tails, shares, pubs, com = deal
    assert VSS_NAMES <= set(_timed_names())
    impl.threshold_split_batch_ct(secrets[:1], tails[:1], 10, 7)  # the comb is built by the first deal of a context
    sk = (12345).to_bytes(32, "big")
    msg = b"routing"
    pk, sig = impl.secret_to_public_key(sk), impl.sign(sk, msg)
    lib = impl.lib
    lib.hipbls_set_timing(1)
    prev = impl.set_pair_mode(PAIR_SINGLE)
    try:
        lib.hipbls_kernel_timing_reset()
        impl.public_key_share_batch(com, [0, 1])
        assert _launched(impl) == {"g1_decode": 1, "vss_eval": 1}
        lib.hipbls_kernel_timing_reset()
        impl.public_key_share_batch([[com[0][0], com[1][0]]], [0, 1])
        assert _launched(impl) == {"g1_decode": 1, "vss_dealer_sum": 1, "vss_eval": 1}
        lib.hipbls_kernel_timing_reset()
        impl.public_key_recover_batch([{i: pubs[0][i] for i in range(1, 8)}])
        assert _launched(impl) == {"vss_scale": 1, "vss_sum": 1}
        lib.hipbls_kernel_timing_reset()
        impl.public_key_recover_batch([{}])
        assert _launched(impl) == {"vss_sum": 1}
        # the calls that were there before launch what they launched before
        lib.hipbls_kernel_timing_reset()
        impl.threshold_split_batch_ct(secrets, tails, 10, 7)
        assert _launched(impl) == {"deal_ct": 1}
        lib.hipbls_kernel_timing_reset()
        assert impl.batch_verify_status([pk] * 3, [msg] * 3, [sig] * 3) == [0, 0, 0]
        got = _launched(impl)
        assert got in ({"verify": 1}, {"verify": 1, "root_lookup": 1}), got  # the lookup only with the root cache on
    finally:
        impl.set_pair_mode(prev)
        lib.hipbls_set_timing(0)
