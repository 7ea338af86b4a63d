"""Secret-independent Sign / SecretToPublicKey on the GPU (charon_amd/csrc/sign_ct.hip): the bytes
and statuses of hipbls_sign_batch_ct / hipbls_secret_to_public_key_batch_ct against the oracle, the reference KATs and
the existing (variable-time) batch calls, over the edge scalars of the digit decomposition and the batch sizes around
the workgroup size (kBlock = 64 = one wave).

The oracle's answers are computed once per module (one hash per message, one multiplication per distinct item) and
shared by the tests.
"""
import ctypes
import json
import os
import random

import pytest

from tests import sign_ct_vectors as V

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_BLOCK = 64  # hipbls.hip kBlock: one wave per workgroup
SIZES = (1, 63, K_BLOCK - 1, K_BLOCK, K_BLOCK + 1, 65, 2 * K_BLOCK + 17)  # the last: two blocks and a partial wave
ZERO96, ZERO48 = bytes(96), bytes(48)


def h(s):
    return bytes.fromhex(s)


@pytest.fixture(scope="module")
def impl():
    from charon_amd.tbls import HipBLS
    return HipBLS()


@pytest.fixture(scope="module")
def kat():
    with open(os.path.join(ROOT, "tests", "golden", "kat_reference.json")) as f:
        return json.load(f)


class Oracle:
    """oracle/bls12381.py's Sign and SecretToPublicKey with H(m) and the answers memoized: (status, bytes)."""

    def __init__(self):
        from oracle import bls12381 as bls
        self.bls = bls
        self.hm, self.sig, self.pk = {}, {}, {}

    def sign(self, s, msg):
        if s >= V.R:
            return V.ERR_SECRET, ZERO96
        if (s, msg) not in self.sig:
            if msg not in self.hm:
                self.hm[msg] = self.bls.hash_to_g2(msg)
            self.sig[(s, msg)] = self.bls.g2_compress(self.bls.g2_mul(self.hm[msg], s))
        return 0, self.sig[(s, msg)]

    def pubkey(self, s):
        if s >= V.R or s == 0:
            return V.ERR_SECRET, ZERO48
        if s not in self.pk:
            self.pk[s] = self.bls.secret_to_public_key(V.sk_bytes(s))
        return 0, self.pk[s]


@pytest.fixture(scope="module")
def oracle():
    o = Oracle()
    # the memoized form is the oracle's own sign()
    s, m = V.random_secrets(1, seed=5)[0], V.MESSAGES[0]
    assert o.sign(s, m)[1] == o.bls.sign(V.sk_bytes(s), m)
    return o


@pytest.fixture(scope="module")
def pool():
    """(secret, message) pairs: the edge list x the three messages, then seeded random secrets, 2 blocks + 17 in all
    at least."""
    items = [(s, m) for m in V.MESSAGES for s in V.edge_secrets()]
    rnd = V.random_secrets(40)
    items += [(s, V.MESSAGES[i % 3]) for i, s in enumerate(rnd)]
    assert len(items) >= max(SIZES)
    return items


def _check_sign(impl, oracle, items):
    sks = [V.sk_bytes(s) for s, _ in items]
    msgs = [m for _, m in items]
    got, st = impl.sign_batch_ct(sks, msgs)
    want = [oracle.sign(s, m) for s, m in items]
    assert st == [w[0] for w in want]
    assert got == [w[1] for w in want]
    # statuses and zero-filled outputs are sign_batch's for the same input
    old, ost = impl.sign_batch(sks, msgs)
    assert (got, st) == (old, ost)


def _check_pk(impl, oracle, secrets):
    sks = [V.sk_bytes(s) for s in secrets]
    got, st = impl.secret_to_public_key_batch_ct(sks)
    want = [oracle.pubkey(s) for s in secrets]
    assert st == [w[0] for w in want]
    assert got == [w[1] for w in want]
    old, ost = impl.secret_to_public_key_batch(sks)
    assert (got, st) == (old, ost)


def test_sign_ct_reference_kats(impl, kat):
    from oracle import ssz
    k = kat["prysm"]
    sks, roots, want = [h(k["sk"])], [h(k["signing_root"])], [k["sig"]]
    k = kat["teku"]
    obj = ssz.validator_registration_root(h(k["fee_recipient"]), k["gas_limit"], k["timestamp"], h(k["pubkey"]))
    sks.append(h(k["sk"]))
    roots.append(ssz.signing_data_root(obj, h(k["domain"])))
    want.append(k["sig"])
    k = kat["deposit"]
    by_pk = {e["pubkey"]: e for e in k["entries"]}
    domain = ssz.compute_domain(ssz.DOMAIN_DEPOSIT, h("00001020"))
    dsks = [h(s) for s in k["sks"]]
    pks, st = impl.secret_to_public_key_batch_ct(dsks)
    assert st == [0] * len(dsks) and all(pk.hex() in by_pk for pk in pks)
    for sk, pk in zip(dsks, pks):
        sks.append(sk)
        roots.append(ssz.signing_data_root(h(by_pk[pk.hex()]["deposit_message_root"]), domain))
        want.append(by_pk[pk.hex()]["signature"])
    sigs, st = impl.sign_batch_ct(sks, roots)
    assert st == [0] * len(sks)
    assert [s.hex() for s in sigs] == want


def test_sign_ct_edge_scalars_three_messages(impl, oracle, pool):
    edge = V.edge_secrets()
    items = pool[:3 * len(edge)]
    assert {s for s, _ in items} == set(edge) and {m for _, m in items} == set(V.MESSAGES)
    _check_sign(impl, oracle, items)
    # sk = 0 signs to the infinity encoding with status OK, as herumi's Sign does
    from charon_amd.tbls import INFINITY_G2
    assert oracle.sign(0, V.MESSAGES[0]) == (0, INFINITY_G2)


def _mixture(pool, n, seed):
    """The first n pool items in a seeded order, with secrets >= r and sk = 0 forced at the first lane, the last lane
    and both sides of every wave boundary."""
    rng = random.Random(seed)
    items = list(pool[:max(n, 8)])
    rng.shuffle(items)
    items = items[:n]
    bad = [V.R, 0, 2**256 - 1, V.R + 1]
    spots = sorted({0, n - 1} | {p for b in range(K_BLOCK, n, K_BLOCK) for p in (b - 1, b)})
    if n > 2:  # at n = 1, 2 keep a valid lane as well (n = 1: the forced lane is the only one)
        for j, p in enumerate(spots):
            items[p] = (bad[j % len(bad)], items[p][1])
    return items


@pytest.mark.parametrize("n", sorted(set(SIZES)))
def test_sign_ct_batch_sizes_with_bad_lanes(impl, oracle, pool, n):
    items = _mixture(pool, n, seed=n)
    _check_sign(impl, oracle, items)
    if n == 1:  # the lone lane with each bad secret too
        for s in (V.R, 0):
            _check_sign(impl, oracle, [(s, V.MESSAGES[0])])


@pytest.mark.parametrize("n", sorted(set(SIZES)))
def test_sk_to_pk_ct_batch_sizes_with_bad_lanes(impl, oracle, pool, n):
    _check_pk(impl, oracle, [s for s, _ in _mixture(pool, n, seed=100 + n)])
    if n == 1:
        for s in (V.R, 0):
            _check_pk(impl, oracle, [s])


def test_sk_to_pk_ct_edge_scalars(impl, oracle):
    _check_pk(impl, oracle, V.edge_secrets())


@pytest.fixture(scope="module")
def thousand(impl):
    rng = random.Random(1000)
    sks = [V.sk_bytes(s) for s in V.random_secrets(1000, seed=77)]
    roots = [rng.randbytes(32) for _ in range(1000)]
    sigs, st = impl.sign_batch_ct(sks, roots)
    return sks, roots, sigs, st


def test_sign_ct_equals_sign_batch_on_1000_random(impl, thousand):
    sks, roots, sigs, st = thousand
    old, ost = impl.sign_batch(sks, roots)
    assert st == ost == [0] * 1000
    assert sigs == old


def test_ct_signatures_verify_under_ct_public_keys(impl, thousand):
    sks, roots, sigs, st = thousand
    pks, pst = impl.secret_to_public_key_batch_ct(sks)
    assert pst == [0] * 1000
    assert impl.batch_verify_status(pks, roots, sigs) == [0] * 1000


def test_device_variants_equal_host_calls(impl, pool):
    import torch
    from charon_amd.tbls import load_library
    lib = load_library()
    dev = torch.device("cuda", 0)
    n = 65
    items = _mixture(pool, n, seed=65)
    sks = [V.sk_bytes(s) for s, _ in items]
    msgs = [m for _, m in items]
    want_sig, want_st = impl.sign_batch_ct(sks, msgs)
    want_pk, want_pst = impl.secret_to_public_key_batch_ct(sks)
    offs, o = [0], 0
    for m in msgs:
        o += len(m)
        offs.append(o)
    d_sk = torch.frombuffer(bytearray(b"".join(sks)), dtype=torch.uint8).to(dev)
    d_msg = torch.frombuffer(bytearray(b"".join(msgs)), dtype=torch.uint8).to(dev)
    d_off = torch.tensor(offs, dtype=torch.int64).to(dev)
    d_sig = torch.full((96 * n,), 0xEE, dtype=torch.uint8, device=dev)
    d_pk = torch.full((48 * n,), 0xEE, dtype=torch.uint8, device=dev)
    d_st = torch.full((n,), -7, dtype=torch.int32, device=dev)
    d_pst = torch.full((n,), -7, dtype=torch.int32, device=dev)
    s = torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    rc = lib.hipbls_sign_batch_ct_device(d_sk.data_ptr(), d_msg.data_ptr(), d_off.data_ptr(), n, d_sig.data_ptr(),
                                         d_st.data_ptr(), ctypes.c_void_p(s.cuda_stream))
    assert rc == 0
    rc = lib.hipbls_secret_to_public_key_batch_ct_device(d_sk.data_ptr(), n, d_pk.data_ptr(), d_pst.data_ptr(),
                                                         ctypes.c_void_p(s.cuda_stream))
    assert rc == 0
    torch.cuda.synchronize(dev)
    raw = bytes(d_sig.cpu().numpy().tobytes())
    assert [raw[96 * i:96 * i + 96] for i in range(n)] == want_sig
    assert d_st.cpu().tolist() == want_st
    raw = bytes(d_pk.cpu().numpy().tobytes())
    assert [raw[48 * i:48 * i + 48] for i in range(n)] == want_pk
    assert d_pst.cpu().tolist() == want_pst
    # the caller's secrets are the caller's: the device calls leave them as they were
    assert bytes(d_sk.cpu().numpy().tobytes()) == b"".join(sks)


def test_implementation_methods_reproduce_the_prysm_kat(impl, kat):
    from charon_amd.tbls import TBLSError
    from oracle import bls12381 as bls
    k = kat["prysm"]
    sk, root = h(k["sk"]), h(k["signing_root"])
    assert impl.sign(sk, root).hex() == k["sig"]
    assert impl.secret_to_public_key(sk) == bls.secret_to_public_key(sk)
    # the reference's errors, unchanged
    with pytest.raises(TBLSError, match="cannot unmarshal secret into Herumi secret key"):
        impl.sign(V.sk_bytes(V.R), root)
    with pytest.raises(TBLSError, match="cannot unmarshal secret into Herumi secret key"):
        impl.secret_to_public_key(V.sk_bytes(V.R))
    with pytest.raises(TBLSError, match="cannot obtain public key from secret"):
        impl.secret_to_public_key(bytes(32))
