"""Batched, secret-independent ThresholdSplit / RecoverSecret on the GPU (charon_amd/csrc/deal_ct.hip):
hipbls_threshold_split_batch_ct and hipbls_recover_secret_batch_ct against the oracle (tests/deal_ct_vectors.py,
computed once per process), the single calls and secret_to_public_key_batch_ct, lane counts around the workgroup
(kBlock = 64 = one wave) with bad validators at the wave boundaries, null public-key outputs, the _device forms, the
round trip split -> recover, and two contexts on one GPU.
"""
import ctypes
import os
import random
import subprocess
import sys

import pytest

from tests import deal_ct_vectors as V

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_BLOCK = 64


@pytest.fixture(scope="module")
def impl():
    from charon_amd.tbls import HipBLS
    return HipBLS()


def _deal(impl, vs, with_pubs=True):
    total, threshold = vs[0].total, vs[0].threshold
    return impl.threshold_split_batch_ct([v.secret_bytes() for v in vs], [v.tail_bytes() for v in vs], total,
                                         threshold, with_pubs=with_pubs)


def _check_deal(impl, vs):
    shares, st, pubs, pst = _deal(impl, vs)
    assert st == [v.status for v in vs]
    for v, sh, pk, ps in zip(vs, shares, pubs, pst):
        assert [sh[i] for i in range(1, v.total + 1)] == v.shares
        assert ps == [w[0] for w in v.pubs]
        assert pk == [w[1] for w in v.pubs]
    return shares, st, pubs, pst


def _c_split(lib, v):
    """hipbls_threshold_split itself, through ctypes: (rc, status, the total x 32 output bytes)."""
    out = ctypes.create_string_buffer(b"\xee" * (32 * v.total), 32 * v.total)
    st = (ctypes.c_int32 * 1)(-7)
    rc = lib.hipbls_threshold_split(v.secret_bytes(), b"".join(v.tail_bytes()) or None, v.total, v.threshold, out, st)
    return rc, st[0], out.raw


def _c_recover(lib, pairs):
    """hipbls_recover_secret itself, through ctypes: (rc, status, the 32 output bytes)."""
    n = len(pairs)
    ids = (ctypes.c_int64 * max(n, 1))(*[i for i, _ in pairs])
    out = ctypes.create_string_buffer(b"\xee" * 32, 32)
    st = (ctypes.c_int32 * 1)(-7)
    rc = lib.hipbls_recover_secret(b"".join(s for _, s in pairs) or None, ids if n else None, n, out, st)
    return rc, st[0], out.raw


def test_split_batch_against_the_oracle(impl):
    for shape, vs in V.by_shape().items():
        _check_deal(impl, vs)


def test_split_batch_equals_single_calls_and_sk_to_pk_ct(impl):
    from charon_amd.tbls import TBLSError
    for shape, vs in V.by_shape().items():
        shares, st, pubs, pst = _deal(impl, vs)
        for v, sh, s in zip(vs, shares, st):
            # the C-ABI's single call: the oracle's bytes and status, which are the batch call's (zero bytes when bad)
            rc, cst, raw = _c_split(impl.lib, v)
            assert (rc, cst) == (0, v.status) and cst == s
            assert raw == b"".join(v.shares) == b"".join(sh[i] for i in range(1, v.total + 1))
            if s == V.OK:
                assert impl._split(v.secret_bytes(), v.total, v.threshold, v.tail_bytes()) == sh
            else:
                with pytest.raises(TBLSError, match="cannot unmarshal bytes into Herumi secret key"):
                    impl._split(v.secret_bytes(), v.total, v.threshold, v.tail_bytes())
        # the public keys are secret_to_public_key_batch_ct's for the same scalars (a bad validator's scalars are 0)
        scalars = [V.b32(s) for v in vs for s in v.scalars]
        pk2, st2 = impl.secret_to_public_key_batch_ct(scalars)
        assert [p for row in pubs for p in row] == pk2
        assert [s for row in pst for s in row] == st2


def test_single_calls_keep_their_errors(impl):
    from charon_amd.tbls import TBLSError
    with pytest.raises(ValueError, match="bad split arguments"):
        impl._split(V.b32(5), 0, 1, [])
    with pytest.raises(ValueError, match="bad split arguments"):
        impl._split(V.b32(5), 3, 0, [])
    with pytest.raises(TBLSError, match="cannot recover full private key from partial keys"):
        impl.recover_secret({})
    with pytest.raises(TBLSError, match="cannot recover full private key from partial keys"):
        impl.recover_secret({0: V.b32(5), 1: V.b32(6)})
    with pytest.raises(TBLSError, match="cannot unmarshal key with into Herumi secret key"):
        impl.recover_secret({1: V.b32(V.R)})
    assert impl.recover_secret({1: V.b32(7)}) == V.b32(7)
    lib = impl.lib
    st = (ctypes.c_int32 * 4)()
    out = ctypes.create_string_buffer(32 * 4)
    # hipbls_threshold_split's own argument checks: HIPBLS_ERR_ARG with its text, nothing written
    one, tail = V.b32(1), V.b32(2)
    for args in ((None, tail, 2, 2, out, st), (one, tail, 2, 2, None, st), (one, tail, 2, 2, out, None),
                 (one, tail, 0, 2, out, st), (one, tail, 2, 0, out, st), (one, None, 2, 2, out, st)):
        st[0] = -7
        assert lib.hipbls_threshold_split(*args) == 16, args[2:4]
        assert lib.hipbls_last_error() == b"bad split arguments" and st[0] == -7
    assert lib.hipbls_threshold_split(one, None, 2, 1, out, st) == 0 and st[0] == 0  # threshold 1 needs no tail
    assert out.raw[:64] == one + one
    # hipbls_recover_secret's
    ids = (ctypes.c_int64 * 2)(1, 2)
    for args in ((one + tail, ids, 2, None, st), (one + tail, ids, 2, out, None), (None, ids, 2, out, st),
                 (one + tail, None, 2, out, st)):
        st[0] = -7
        assert lib.hipbls_recover_secret(*args) == 16
        assert lib.hipbls_last_error() == b"bad recover arguments" and st[0] == -7
    assert lib.hipbls_recover_secret(None, None, 0, out, st) == 0 and st[0] == V.ERR_COMBINE  # n = 0: not an argument error
    assert out.raw[:32] == bytes(32)
    assert lib.hipbls_threshold_split_batch_ct(V.b32(1), None, 0, 0, 1, out, st, None, None) == 16  # total == 0
    assert lib.hipbls_threshold_split_batch_ct(V.b32(1), None, 0, 1, 0, out, st, None, None) == 16  # threshold == 0
    assert lib.hipbls_threshold_split_batch_ct(None, None, 0, 1, 1, None, None, None, None) == 0    # n_val == 0
    assert lib.hipbls_threshold_split_batch_ct(V.b32(1), None, 1, 1, 1, out, st, out, None) == 16   # pubs without status
    assert lib.hipbls_threshold_split_batch_ct(V.b32(1), None, 1, 2, 2, out, st, None, None) == 16  # no tail
    assert lib.hipbls_recover_secret_batch_ct(None, None, None, 0, None, None, None, None) == 0     # n_groups == 0


def _lanes_case(n_val, total, threshold, seed):
    """n_val validators with a bad one at the first lane, the last lane and on both sides of every wave boundary."""
    rng = random.Random(seed)
    row = total + 1
    n = n_val * row
    bad_at = sorted({0, n_val - 1} | {p // row for b in range(K_BLOCK, n, K_BLOCK) for p in (b - 1, b)})
    bads = [V.R, 2**256 - 1, V.R + 1]
    vs = []
    for v in range(n_val):
        tail = [rng.randrange(V.R) for _ in range(threshold - 1)]
        secret = rng.randrange(1, V.R)
        if v in bad_at and n_val > 2:
            j = bad_at.index(v)
            if j % 2 == 0 or threshold == 1:
                secret = bads[j % 3]
            else:
                tail[rng.randrange(threshold - 1)] = bads[j % 3]
        vs.append(V.Validator(total, threshold, secret, tail))
    return vs


@pytest.mark.parametrize("n_val,total,threshold", [(21, 2, 2), (16, 3, 2), (13, 4, 3), (43, 2, 1), (1, 1, 1)])
def test_split_lane_counts_around_the_workgroup(impl, n_val, total, threshold):
    assert n_val * (total + 1) in (63, 64, 65, 129, 2)
    vs = _lanes_case(n_val, total, threshold, seed=n_val)
    if n_val > 2:
        assert any(v.status != V.OK for v in vs) and any(v.status == V.OK for v in vs)
    _check_deal(impl, vs)


def test_split_without_public_keys(impl):
    vs = V.by_shape()[(4, 3)]
    shares, st, pubs, pst = _deal(impl, vs, with_pubs=False)
    assert pubs is None and pst is None
    assert st == [v.status for v in vs]
    assert [[sh[i] for i in range(1, 5)] for sh in shares] == [v.shares for v in vs]


def _check_recover(impl, gs):
    secs, st, pks, pst = impl.recover_secret_batch_ct([_Pairs(g.pairs) for g in gs])
    assert st == [g.status for g in gs]
    assert secs == [g.secret for g in gs]
    assert pst == [g.pk_status for g in gs]
    assert pks == [g.pk for g in gs]


class _Pairs:
    """A group as the binding takes it (.items()), duplicates kept."""

    def __init__(self, pairs):
        self.pairs = pairs

    def items(self):
        return list(self.pairs)


def test_recover_batch_against_the_oracle(impl):
    gs = list(V.groups())
    _check_recover(impl, gs)
    # every group alone (its own largest group size), without keys, and through the single call
    from charon_amd.tbls import TBLSError
    for g in gs:
        secs, st, pks, pst = impl.recover_secret_batch_ct([_Pairs(g.pairs)], with_pubkeys=False)
        assert (secs, st, pks, pst) == ([g.secret], [g.status], None, None)
        # the C-ABI's single call: the oracle's secret and status (n = 0, id 0, a duplicate, a share >= r among them)
        assert _c_recover(impl.lib, g.pairs) == (0, g.status, g.secret)
        ids = [i for i, _ in g.pairs]
        if len(set(ids)) != len(ids):
            continue  # a map cannot hold it
        if g.status == V.OK:
            assert impl.recover_secret(dict(g.pairs)) == g.secret
        else:
            with pytest.raises(TBLSError):
                impl.recover_secret(dict(g.pairs))


@pytest.mark.parametrize("n", [63, 64, 65, 129])
def test_recover_group_counts_around_the_workgroup(impl, n):
    base = list(V.groups())
    rng = random.Random(n)
    gs = [base[rng.randrange(len(base))] for _ in range(n)]
    bad = [g for g in base if g.status != V.OK]
    for j, p in enumerate(sorted({0, n - 1} | {p for b in range(K_BLOCK, n, K_BLOCK) for p in (b - 1, b)})):
        gs[p] = bad[j % len(bad)]
    _check_recover(impl, gs)


def test_split_then_recover_any_threshold_shares(impl):
    rng = random.Random(77)
    total, threshold, n = 10, 7, 24
    vs = [V.Validator(total, threshold, rng.randrange(1, V.R), [rng.randrange(V.R) for _ in range(threshold - 1)])
          for _ in range(n)]
    shares, st, pubs, pst = _deal(impl, vs)
    assert st == [V.OK] * n
    groups = []
    for sh in shares:
        ids = rng.sample(range(1, total + 1), threshold)
        groups.append({i: sh[i] for i in ids})
    secs, rst, pks, rpst = impl.recover_secret_batch_ct(groups)
    assert rst == [V.OK] * n and rpst == [V.OK] * n
    assert secs == [v.secret_bytes() for v in vs]
    assert pks == [row[0] for row in pubs]  # the root key of entry k = 0


def test_device_forms_equal_host_calls(impl):
    import torch
    lib = impl.lib
    dev = torch.device("cuda", 0)
    vs = _lanes_case(13, 4, 3, seed=5)
    n_val, total, threshold, row = 13, 4, 3, 5
    shares, st, pubs, pst = _deal(impl, vs)

    def dbytes(b):
        return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)

    sec = b"".join(v.secret_bytes() for v in vs)
    d_sec = dbytes(sec)
    d_tail = dbytes(b"".join(b"".join(v.tail_bytes()) for v in vs))
    d_sh = torch.full((32 * n_val * total,), 0xEE, dtype=torch.uint8, device=dev)
    d_st = torch.full((n_val,), -7, dtype=torch.int32, device=dev)
    d_pub = torch.full((48 * n_val * row,), 0xEE, dtype=torch.uint8, device=dev)
    d_pst = torch.full((n_val * row,), -7, dtype=torch.int32, device=dev)
    s = torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    rc = lib.hipbls_threshold_split_batch_ct_device(d_sec.data_ptr(), d_tail.data_ptr(), n_val, total, threshold,
                                                    d_sh.data_ptr(), d_st.data_ptr(), d_pub.data_ptr(),
                                                    d_pst.data_ptr(), ctypes.c_void_p(s.cuda_stream))
    assert rc == 0
    torch.cuda.synchronize(dev)
    raw = bytes(d_sh.cpu().numpy().tobytes())
    assert raw == b"".join(sh[i] for sh in shares for i in range(1, total + 1))
    assert d_st.cpu().tolist() == st
    assert bytes(d_pub.cpu().numpy().tobytes()) == b"".join(p for r in pubs for p in r)
    assert d_pst.cpu().tolist() == [x for r in pst for x in r]
    assert bytes(d_sec.cpu().numpy().tobytes()) == sec  # the caller's secrets stay the caller's
    # without keys: the key buffers are not touched
    d_sh.fill_(0xEE)
    rc = lib.hipbls_threshold_split_batch_ct_device(d_sec.data_ptr(), d_tail.data_ptr(), n_val, total, threshold,
                                                    d_sh.data_ptr(), d_st.data_ptr(), None, None,
                                                    ctypes.c_void_p(s.cuda_stream))
    assert rc == 0
    torch.cuda.synchronize(dev)
    assert bytes(d_sh.cpu().numpy().tobytes()) == raw

    gs = list(V.groups())
    want = impl.recover_secret_batch_ct([_Pairs(g.pairs) for g in gs])
    ids = [i for g in gs for i, _ in g.pairs]
    offs = [0]
    for g in gs:
        offs.append(offs[-1] + len(g.pairs))
    n = len(gs)
    d_shares = dbytes(b"".join(sh for g in gs for _, sh in g.pairs))
    d_ids = torch.tensor(ids, dtype=torch.int64).to(dev)
    d_off = torch.tensor(offs, dtype=torch.int64).to(dev)
    d_out = torch.full((32 * n,), 0xEE, dtype=torch.uint8, device=dev)
    d_rst = torch.full((n,), -7, dtype=torch.int32, device=dev)
    d_pk = torch.full((48 * n,), 0xEE, dtype=torch.uint8, device=dev)
    d_pkst = torch.full((n,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    rc = lib.hipbls_recover_secret_batch_ct_device(d_shares.data_ptr(), d_ids.data_ptr(), d_off.data_ptr(), n,
                                                   len(ids), d_out.data_ptr(), d_rst.data_ptr(), d_pk.data_ptr(),
                                                   d_pkst.data_ptr(), ctypes.c_void_p(s.cuda_stream))
    assert rc == 0
    torch.cuda.synchronize(dev)
    assert bytes(d_out.cpu().numpy().tobytes()) == b"".join(want[0])
    assert d_rst.cpu().tolist() == want[1]
    assert bytes(d_pk.cpu().numpy().tobytes()) == b"".join(want[2])
    assert d_pkst.cpu().tolist() == want[3]


def test_two_contexts_equal_one(impl):
    """4,608 validators x 1-of-1 and 2,304 groups are split over two contexts (whole validators, whole groups); the
    child process binds both to device 0 and must return this process's bytes."""
    from tests import deal_ct_child as C
    want = C.digest(impl)
    r = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "tests", "deal_ct_child.py"), "2"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == want, r.stdout
