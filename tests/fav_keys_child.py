"""Child process of tests/test_gpu_fav_keys.py, for what is fixed per process.  Usage: fav_keys_child.py MODE OUT.json

  split  the split key sum under whatever HIPBLS_FAV_SUM_SPLIT the parent set (read at init): a
         200-key honest group, the same group with a failed key in the last slice, with the identity key in a middle
         slice, with P in slice 0 and -P in slice 2 and a total at the identity, and a 64-key group -- one group per
         call on the lone route, then all in one call on the throughput route, beside the wire-format call on the same
         bytes, with the number of slice-sum launches each call made.
  ctx    two contexts on device 0: 4 groups twice (a single range runs on a round-robin context, so both contexts
         serve one) and 130 groups (two ranges of whole groups), beside the wire-format call.
"""
import ctypes
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

R_ORDER = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
BAD_PK, INF_PK = bytes(48), b"\xc0" + bytes(47)


def _launches(impl, name):
    a, c = ctypes.c_double(), ctypes.c_uint64()
    impl.lib.hipbls_kernel_timing(name, ctypes.byref(a), ctypes.byref(c))
    return c.value


def _neg(pk):
    return bytes([pk[0] ^ 0x20]) + pk[1:]  # the sign flag: -P


def split(impl):
    from charon_amd.tbls import PAIR_AUTO, PAIR_SINGLE
    rng = random.Random(0xFA5)
    sks = [rng.randrange(1, R_ORDER).to_bytes(32, "big") for _ in range(200)]
    pks, st = impl.secret_to_public_key_batch(sks)
    assert set(st) == {0}
    msg = rng.randbytes(32)
    sigs, st = impl.sign_batch(sks, [msg] * 200)
    assert set(st) == {0}
    agg200, agg64 = impl.aggregate(sigs), impl.aggregate(sigs[:64])
    table = list(pks) + [_neg(p) for p in pks[:100]] + [BAD_PK, INF_PK]
    NEG, BAD, INF = 200, 300, 301
    assert impl.load_pubshares(table) == [0] * 300 + [1, 0]
    honest = list(range(200))
    bad_last = honest[:195] + [BAD] + honest[196:]       # slice 3 = keys 192 .. 199
    inf_mid = honest[:100] + [INF] + honest[101:]        # slice 1 = keys 64 .. 127
    # P_0 .. P_99, then -P_(j + 72) for j = 0 .. 99: -P_0 sits at key 128, the first of slice 2; no slice sums to the
    # identity, the total does
    cancel = honest[:100] + [NEG + (j + 72) % 100 for j in range(100)]
    assert cancel[0] == 0 and cancel[128] == NEG
    cases = [(honest, agg200), (bad_last, agg200), (inf_mid, agg200), (cancel, agg200), (honest[:64], agg64)]
    keyed = [(idx, sig, msg) for idx, sig in cases]
    wire = [([table[k] for k in idx], sig, msg) for idx, sig in cases]
    out = dict(want=impl.batch_verify_aggregate_status(wire), lone=[], lone_sums=[])
    impl.lib.hipbls_set_timing(1)
    for g in keyed:
        before = _launches(impl, b"fav_sum_keys")
        out["lone"] += impl.batch_verify_aggregate_keys_status([g])
        out["lone_sums"].append(_launches(impl, b"fav_sum_keys") - before)
    impl.set_pair_mode(PAIR_SINGLE)
    before = _launches(impl, b"fav_sum_keys")
    out["batch"] = impl.batch_verify_aggregate_keys_status(keyed)
    out["batch_sums"] = _launches(impl, b"fav_sum_keys") - before
    impl.set_pair_mode(PAIR_AUTO)
    impl.lib.hipbls_set_timing(0)
    return out


def ctx(impl):
    rng = random.Random(0xFA6)
    sks = [rng.randrange(1, R_ORDER).to_bytes(32, "big") for _ in range(8)]
    pks, st = impl.secret_to_public_key_batch(sks)
    assert set(st) == {0}
    roots = [rng.randbytes(32) for _ in range(3)]
    table = list(pks) + [BAD_PK]
    assert impl.load_pubshares(table) == [0] * 8 + [1]
    aggs = {}

    def group(g):
        """Group g: 1 to 4 keys from key g % 8 on, over root g % 3; every 13th has a key swapped, every 17th a key
        that failed to load."""
        idx = [(g + j) % 8 for j in range(1 + g % 4)]
        key = (tuple(idx), g % 3)
        if key not in aggs:
            s, st = impl.sign_batch([sks[k] for k in idx], [roots[g % 3]] * len(idx))
            assert set(st) == {0}
            aggs[key] = impl.aggregate(s)
        if g % 13 == 5:
            idx = idx[:-1] + [(idx[-1] + 3) % 8]
        elif g % 17 == 3:
            idx = idx + [8]
        return idx, aggs[key], roots[g % 3]

    out = dict(contexts=len(impl.device_slots()))
    for name, n in (("four_a", 4), ("four_b", 4), ("split", 130)):
        keyed = [group(g) for g in range(n)]
        wire = [([table[k] for k in idx], sig, m) for idx, sig, m in keyed]
        out[name] = dict(got=impl.batch_verify_aggregate_keys_status(keyed),
                         want=impl.batch_verify_aggregate_status(wire))
    return out


def main():
    mode, dst = sys.argv[1], sys.argv[2]
    from charon_amd.tbls import HipBLS
    if mode == "split":
        out = split(HipBLS())
    else:
        impl = HipBLS(devices=[0, 0])
        assert impl.device_slots() == [0, 0]
        out = ctx(impl)
    with open(dst, "w") as f:
        json.dump(out, f)
    print("fav keys child:", mode, "ok")


if __name__ == "__main__":
    main()
