"""FastAggregateVerify by resident key index (hipbls_verify_aggregate_batch_keys[_device]).  It is the
wire-format call with two inputs found elsewhere -- the keys in the resident table, H(m) in the H(m) cache -- so every
case asserts that the statuses equal what hipbls_verify_aggregate_batch returns for the bytes loaded at
table[key_idx[k]]: on the lone route and the throughput route, in the pair modes that choose between them, with the
cache off, cold, warm and bypassed, from host buffers and from torch tensors, with and without the split key sum, on
one context and on two.  The oracle confirms the honest sample groups, and the reference's locks are known answers.

The table and the cache are process-wide state: every test sets what it needs, and the module leaves the table empty
and the cache disabled, as it found them.
"""
import ctypes
import json
import os
import random
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_PUBKEY, ERR_SIGNATURE, ERR_VERIFY, ERR_ARG = 0, 1, 2, 3, 16
NK = 512
NEG0, BAD, INF, SMALL = NK, NK + 1, NK + 2, NK + 3  # table entries behind the 512 valid keys
MATRIX_WANT = [0, 3, 2, 1, 3, 3, 3, 2, 2, 1, 0, 3]
h = bytes.fromhex


def _launches(impl, name):
    a, c = ctypes.c_double(), ctypes.c_uint64()
    impl.lib.hipbls_kernel_timing(name, ctypes.byref(a), ctypes.byref(c))
    return c.value


@pytest.fixture(scope="module")
def impl():
    from charon_amd.tbls import PAIR_AUTO, HipBLS
    hb = HipBLS()
    hb.hcache_config(0)
    yield hb
    hb.set_pair_mode(PAIR_AUTO)
    hb.lib.hipbls_set_timing(0)
    hb.hcache_config(0)
    hb.load_pubshares([])


@pytest.fixture(scope="module")
def world(impl):
    """The twelve-group matrix of tests/test_gpu_r05.py test_fav_octet_and_sixteen_lane_layouts_match_fav_batch, by
    key index: the table holds the 512 valid keys, -P of the first, the bad encoding, the identity key and the
    small-order key of tests/golden/fixtures.json.  The wire-format statuses are computed once."""
    with open(os.path.join(ROOT, "tests", "golden", "fixtures.json")) as f:
        so = json.load(f)["small_order"]
    rng = random.Random(55)
    sks = [rng.randrange(1, 2 ** 254).to_bytes(32, "big") for _ in range(NK)]
    pks, st = impl.secret_to_public_key_batch(sks)
    assert set(st) == {OK}
    msg = b"sync committee root".ljust(32, b"\0")
    msg2 = b"another root of 200 bytes".ljust(200, b"\x07")
    sigs, _ = impl.sign_batch(sks, [msg] * NK)
    sigs2, _ = impl.sign_batch(sks[:3], [msg2] * 3)
    agg3, agg512, agg3b = impl.aggregate(sigs[:3]), impl.aggregate(sigs), impl.aggregate(sigs2)
    bad_sig = bytes([agg3[0] & 0x7F]) + agg3[1:]
    neg0 = bytes([pks[0][0] ^ 0x20]) + pks[0][1:]  # the sign flag: -P
    small_sig, small_pk = h(so["verify"][0]["sig"]), h(so["verify"][16]["pk"])
    table = list(pks) + [neg0, bytes(48), bytes([0xC0]) + bytes(47), small_pk]
    load = [OK] * (NK + 1) + [ERR_PUBKEY, OK, ERR_PUBKEY]
    all_k = list(range(NK))
    matrix = [
        ([0, 1, 2], agg3, msg),                # 0
        ([0, 1, 2], agg3, msg[::-1]),          # 3
        ([0, 1, 2], bad_sig, msg),             # 2
        ([0, BAD, 2], agg3, msg),              # 1
        ([], agg3, msg),                       # 3
        ([0, 1, 2, INF], agg3, msg),           # 3
        ([0, NEG0], agg3, msg),                # 3: the key sum is the identity
        ([0, 1, 2], small_sig, msg),           # 2
        ([0, BAD], small_sig, msg),            # 2: the signature's membership error before the key's
        ([0, 1, 2, SMALL], agg3, msg),         # 1
        (all_k, agg512, msg),                  # 0
        (all_k[:511], agg512, msg),            # 3
    ]
    w = dict(sks=sks, pks=pks, sigs=sigs, table=table, load=load, msg=msg, msg2=msg2, agg3=agg3, agg3b=agg3b,
             agg512=agg512, matrix=matrix)
    w["want"] = impl.batch_verify_aggregate_status(_wire(w, matrix))
    assert w["want"] == MATRIX_WANT
    return w


def _wire(world, groups):
    return [([world["table"][k] for k in idx], sig, m) for idx, sig, m in groups]


def _load(impl, world):
    assert impl.load_pubshares(world["table"]) == world["load"]


# ------------------------------------------------------------------------------------------------ 1. statuses, routes
def test_status_matrix_on_both_routes_equals_the_wire_format_call(impl, world):
    """PAIR_SINGLE and 24 groups take k_fav_batch_keys behind k_rlc_hash (one distinct message, hashed once); 12
    groups in AUTO take the octet prep and k_fav_pair_lq16_keys; then one group per call."""
    from charon_amd.tbls import PAIR_AUTO, PAIR_SINGLE
    _load(impl, world)
    groups, want = world["matrix"], world["want"]
    impl.lib.hipbls_set_timing(1)
    try:
        for mode, batch, hexl in ((PAIR_SINGLE, groups, 0), (PAIR_AUTO, groups, 1), (PAIR_AUTO, groups * 2, 0)):
            impl.set_pair_mode(mode)
            names = (b"fav_lq16_keys", b"fav_prep8_keys", b"fav_keys", b"rlc_hash", b"fav_sum_keys",
                     b"fav_lq16", b"fav_prep8", b"fav")
            before = [_launches(impl, n) for n in names]
            got = impl.batch_verify_aggregate_keys_status(batch)
            print("keyed FAV", mode, len(batch), got)
            assert got == want * (len(batch) // len(groups)), (mode, len(batch))
            delta = [_launches(impl, n) - b for n, b in zip(names, before)]
            # no 512-key group is cut at the default threshold, and no wire-format kernel runs
            assert delta == [hexl, hexl, 1 - hexl, 1 - hexl, 0, 0, 0, 0], (mode, len(batch), delta)
        impl.set_pair_mode(PAIR_AUTO)
        for g, w in zip(groups, want):  # one group per call, as the sync-committee duty sends it
            assert impl.batch_verify_aggregate_keys_status([g]) == [w]
        impl.verify_aggregate_keys(*groups[0])
        from charon_amd.tbls import TBLSError
        for g, text in ((groups[1], "signature verification failed"),
                        (groups[2], "cannot unmarshal signature into Herumi signature"),
                        (groups[3], "cannot set compressed public key in Herumi format")):
            with pytest.raises(TBLSError) as e:
                impl.verify_aggregate_keys(*g)
            assert str(e.value) == text
    finally:
        impl.set_pair_mode(PAIR_AUTO)
        impl.lib.hipbls_set_timing(0)


def test_oracle_confirms_the_honest_sample(impl, world):
    from oracle import bls12381 as bls
    _load(impl, world)
    rng = random.Random(0x0FA)
    for _ in range(2):
        idx = rng.sample(range(NK), 3)
        sig = impl.aggregate([world["sigs"][k] for k in idx])
        bls.verify_aggregate([world["table"][k] for k in idx], sig, world["msg"])  # raises unless it verifies
        assert impl.batch_verify_aggregate_keys_status([(idx, sig, world["msg"])]) == [OK]
        with pytest.raises(bls.BLSError):
            bls.verify_aggregate([world["table"][k] for k in idx[:2]], sig, world["msg"])
        assert impl.batch_verify_aggregate_keys_status([(idx[:2], sig, world["msg"])]) == [ERR_VERIFY]


# ------------------------------------------------------------------------------------------------ 2. duplicate keys
def test_duplicate_keys_double_in_the_strided_sum(impl, world):
    """One key twice (lanes 0 and 1 meet in the tree with equal points), and 130 keys with key[k] == key[k + 64]: lane
    k's second mixed addition adds a point to itself."""
    from charon_amd.tbls import PAIR_AUTO, PAIR_SINGLE
    _load(impl, world)
    sigs, msg = world["sigs"], world["msg"]
    twice = [7, 7]
    idx130 = list(range(130))
    for k in (3, 40, 63):
        idx130[k + 64] = idx130[k]
    groups = [(twice, impl.aggregate([sigs[k] for k in twice]), msg),
              (idx130, impl.aggregate([sigs[k] for k in idx130]), msg),
              (idx130, impl.aggregate([sigs[k] for k in range(130)]), msg)]  # the aggregate without the repeats
    want = impl.batch_verify_aggregate_status(_wire(world, groups))
    assert want == [OK, OK, ERR_VERIFY]
    try:
        for mode in (PAIR_AUTO, PAIR_SINGLE):
            impl.set_pair_mode(mode)
            assert impl.batch_verify_aggregate_keys_status(groups) == want, mode
    finally:
        impl.set_pair_mode(PAIR_AUTO)


# ------------------------------------------------------------------------------------------------ 3. the H(m) cache
def test_cache_off_cold_warm_bypassed_and_shared_roots(impl, world):
    from charon_amd.tbls import PAIR_AUTO, PAIR_SINGLE
    _load(impl, world)
    msg, msg2 = world["msg"], world["msg2"]
    two_roots = [([0, 1, 2], world["agg3"], msg), ([0, 1, 2], world["agg3b"], msg2), ([0, 1], world["agg3"], msg)]
    want = impl.batch_verify_aggregate_status(_wire(world, two_roots))
    assert want == [OK, OK, ERR_VERIFY]
    impl.lib.hipbls_set_timing(1)
    try:
        # off
        impl.hcache_config(0)
        assert impl.batch_verify_aggregate_keys_status(two_roots) == want
        assert impl.hcache_stats() == (0, 0, 0)
        # cold: three groups over two roots are two lookups, both misses, and the call inserts nothing
        impl.hcache_config(8)
        assert impl.batch_verify_aggregate_keys_status(two_roots) == want
        assert impl.hcache_stats() == (0, 2, 0)
        assert impl.batch_verify_aggregate_keys_status(two_roots) == want  # still cold: the call never inserts
        assert impl.hcache_stats() == (0, 4, 0)
        # warm: after the prefetch of both roots the hits rise by the distinct messages, the prep still runs (its
        # signature role) and the statuses stay
        assert impl.hcache_prefetch([msg, msg2]) == (2, 0)
        prep = _launches(impl, b"fav_prep8_keys")
        assert impl.batch_verify_aggregate_keys_status(two_roots) == want
        assert impl.hcache_stats() == (2, 4, 2)
        assert _launches(impl, b"fav_prep8_keys") == prep + 1
        # two groups sharing one root count as one lookup; one warm and one cold root in one call
        assert impl.batch_verify_aggregate_keys_status([two_roots[0], two_roots[2]]) == [want[0], want[2]]
        assert impl.hcache_stats() == (3, 4, 2)
        other = ([0, 1, 2], world["agg3"], msg[::-1])
        assert impl.batch_verify_aggregate_keys_status([two_roots[1], other]) == [OK, ERR_VERIFY]
        assert impl.hcache_stats() == (4, 5, 2)
        # the throughput route reads the same columns
        impl.set_pair_mode(PAIR_SINGLE)
        assert impl.batch_verify_aggregate_keys_status(two_roots) == want
        impl.set_pair_mode(PAIR_AUTO)
        assert impl.hcache_stats() == (6, 5, 2)
        # a capacity below the call's distinct messages: bypassed, nothing counted
        impl.hcache_config(1)
        assert impl.hcache_prefetch([msg]) == (1, 0)
        assert impl.batch_verify_aggregate_keys_status(two_roots) == want
        assert impl.hcache_stats() == (0, 0, 1)
        assert impl.batch_verify_aggregate_keys_status([two_roots[0]]) == [OK]  # a call that fits reads it
        assert impl.hcache_stats() == (1, 0, 1)
    finally:
        impl.set_pair_mode(PAIR_AUTO)
        impl.lib.hipbls_set_timing(0)
        impl.hcache_config(0)


# ------------------------------------------------------------------------------------------------ 4. arguments
def _raw_call(impl, groups, fill=0x55555555):
    g = len(groups)
    idx = [k for ks, _, _ in groups for k in ks]
    koffs = (ctypes.c_uint64 * (g + 1))()
    n = 0
    for j, (ks, _, _) in enumerate(groups):
        koffs[j] = n
        n += len(ks)
    koffs[g] = n
    from charon_amd.tbls import _offsets
    blob, moffs = _offsets([m for _, _, m in groups])
    st = (ctypes.c_int32 * g)(*([fill] * g))
    arr = (ctypes.c_uint32 * max(n, 1))(*idx)
    rc = impl.lib.hipbls_verify_aggregate_batch_keys(arr, koffs, g, b"".join(s for _, s, _ in groups), blob, moffs, st)
    return rc, list(st)


def test_host_call_refuses_an_index_outside_the_table(impl, world):
    _load(impl, world)
    good = world["matrix"][0]
    T = len(world["table"])
    for groups in ([good, ([0, T], world["agg3"], world["msg"])], [([T], world["agg3"], world["msg"])] + [good] * 20):
        rc, st = _raw_call(impl, groups)
        assert rc == ERR_ARG and st == [0x55555555] * len(groups)  # the status array is untouched
    rc, st = _raw_call(impl, [good])
    assert (rc, st) == (0, [OK])
    try:
        assert impl.load_pubshares([]) == []
        rc, st = _raw_call(impl, [good])
        assert rc == ERR_ARG and st == [0x55555555]
    finally:
        _load(impl, world)


def _device_call(impl, groups, torch, dev, stream):
    def u8(b):
        return torch.frombuffer(bytearray(b) or bytearray(1), dtype=torch.uint8).to(dev)

    g = len(groups)
    idx = [k for ks, _, _ in groups for k in ks]
    koffs, moffs = [0], [0]
    for ks, _, m in groups:
        koffs.append(koffs[-1] + len(ks))
        moffs.append(moffs[-1] + len(m))
    b = dict(kidx=torch.tensor(idx or [0], dtype=torch.int64).to(torch.int32).to(dev),
             koff=torch.tensor(koffs, dtype=torch.int64).to(dev), sig=u8(b"".join(s for _, s, _ in groups)),
             msg=u8(b"".join(m for _, _, m in groups)), moff=torch.tensor(moffs, dtype=torch.int64).to(dev),
             st=torch.full((g,), -7, dtype=torch.int32, device=dev))
    torch.cuda.synchronize(dev)
    rc = impl.lib.hipbls_verify_aggregate_batch_keys_device(
        b["kidx"].data_ptr(), len(idx), b["koff"].data_ptr(), g, b["sig"].data_ptr(), b["msg"].data_ptr(),
        b["moff"].data_ptr(), b["st"].data_ptr(), ctypes.c_void_p(stream.cuda_stream))
    assert rc == 0, impl.lib.hipbls_last_error()
    return b


def test_device_call_on_torch_tensors(impl, world):
    """The statuses of the host call, on both routes; an index outside the table is ERR_ARG for its group alone,
    whatever else the group holds, and the loads stay inside the table."""
    import torch
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(dev)
    _load(impl, world)
    T = len(world["table"])
    groups, want = world["matrix"], world["want"]
    msg = world["msg"]
    outside = [([0, 1, T], world["agg3"], msg), ([0xFFFFFFFF], world["agg3"], msg),
               ([BAD, T + 5], bytes([world["agg3"][0] & 0x7F]) + world["agg3"][1:], msg)]
    mixed = groups[:3] + outside + groups[3:6]
    calls = [(groups, want), (groups * 2, want * 2), (mixed, want[:3] + [ERR_ARG] * 3 + want[3:6]),
             (mixed * 3, (want[:3] + [ERR_ARG] * 3 + want[3:6]) * 3)]
    hits0 = None
    impl.hcache_config(8)
    try:
        assert impl.hcache_prefetch([msg]) == (1, 0)
        hits0 = impl.hcache_stats()
        bufs = [_device_call(impl, g, torch, dev, s) for g, _ in calls]
        torch.cuda.synchronize(dev)
        for b, (g, w) in zip(bufs, calls):
            assert b["st"].cpu().tolist() == w, len(g)
        assert impl.hcache_stats() == hits0  # the device call leaves the cache alone
    finally:
        impl.hcache_config(0)


# ------------------------------------------------------------------------------------------------ 5. known answers
def test_reference_locks_by_key_index(impl, kat):
    """The four example locks and the manifest's lock2: keyed FastAggregateVerify of the lock's aggregate over every
    pubshare on the lock hash; one index replaced by another key's does not verify."""
    locks = [([h(s) for v in lk["validators"] for s in v["public_shares"]], h(lk["signature_aggregate"]),
              h(lk["lock_hash"])) for lk in kat["locks"]]
    m = kat["manifest"]["lock2"]
    locks.append(([h(s) for s in m["public_shares"]], h(m["signature_aggregate"]), h(m["lock_hash"])))
    assert len(locks) == 5
    try:
        for pks, sig, root in locks:
            n = len(pks)
            assert n >= 2 and set(impl.load_pubshares(pks)) == {OK}
            assert impl.batch_verify_aggregate_status([(pks, sig, root)]) == [OK]
            assert impl.batch_verify_aggregate_keys_status([(range(n), sig, root)]) == [OK]
            swapped = list(range(n))
            swapped[n // 2] = (n // 2 + 1) % n
            assert impl.batch_verify_aggregate_keys_status([(swapped, sig, root)]) == [ERR_VERIFY]
            impl.verify_aggregate_keys(range(n), sig, root)
    finally:
        impl.load_pubshares([])


# ------------------------------------------------------------------------------------------------ 6. child processes
def _child(tmp_path, mode, env=None):
    out = tmp_path / ("%s.json" % mode)
    e = dict(os.environ)
    e.pop("HIPBLS_FAV_SUM_SPLIT", None)
    e.update(env or {})
    r = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "tests", "fav_keys_child.py"), mode, str(out)],
                       capture_output=True, text=True, timeout=120, cwd=ROOT, env=e)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    with open(out) as f:
        return json.load(f)


@pytest.mark.parametrize("split", [64, 0])
def test_split_key_sum(tmp_path, split):
    """HIPBLS_FAV_SUM_SPLIT=64 (read at init, hence the child): the 200-key groups are cut into four slices and summed
    by k_fav_sum_keys -- honest, a failed key in the last slice, the identity key in slice 1, P in slice 0 and -P in
    slice 2 with the total at the identity -- and a 64-key group sits at the threshold and is not cut.  0 turns the
    split off: same statuses, no slice sum."""
    got = _child(tmp_path, "split", {"HIPBLS_FAV_SUM_SPLIT": str(split)})
    print("split", split, got)
    assert got["want"] == [OK, ERR_PUBKEY, ERR_VERIFY, ERR_VERIFY, OK]
    assert got["lone"] == got["want"] and got["batch"] == got["want"]
    if split:
        assert got["lone_sums"] == [1, 1, 1, 1, 0] and got["batch_sums"] == 1
    else:
        assert got["lone_sums"] == [0] * 5 and got["batch_sums"] == 0


def test_two_contexts(tmp_path):
    got = _child(tmp_path, "ctx")
    assert got["contexts"] == 2
    for name, n in (("four_a", 4), ("four_b", 4), ("split", 130)):
        assert len(got[name]["want"]) == n and got[name]["got"] == got[name]["want"], name
    assert set(got["split"]["want"]) == {OK, ERR_PUBKEY, ERR_VERIFY}
