"""Child process of tests/test_gpu_deal_ct.py: binds the library to K contexts on device 0, so that the batched split
and recover calls are cut into K ranges of whole validators / whole groups, and prints a digest of everything they
return.  The parent computes the same digest on its one context.  Usage: deal_ct_child.py K
"""
import hashlib
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
N_VAL, N_GROUPS = 4608, 2304  # above twice the library's per-context minimum for 1-of-1 deals and for groups


def digest(impl):
    rng = random.Random(4608)
    secrets = [rng.randrange(1, R).to_bytes(32, "big") for _ in range(N_VAL)]
    for p in (0, N_VAL // 2 - 1, N_VAL // 2, N_VAL - 1):  # bad validators where the ranges meet
        secrets[p] = (R + p).to_bytes(32, "big")
    h = hashlib.sha256()
    shares, st, pubs, pst = impl.threshold_split_batch_ct(secrets, [[]] * N_VAL, 1, 1)
    assert st.count(4) == 4 and st.count(0) == N_VAL - 4
    for v in range(N_VAL):
        h.update(shares[v][1] + bytes([st[v]]) + b"".join(pubs[v]) + bytes(pst[v]))
    groups = []
    for g in range(N_GROUPS):
        groups.append({1 + g % 5: rng.randrange(R).to_bytes(32, "big"), 7 + g % 3: rng.randrange(R).to_bytes(32, "big")})
    groups[N_GROUPS // 2] = {}
    groups[N_GROUPS // 2 - 1] = {3: R.to_bytes(32, "big")}
    secs, rst, pks, rpst = impl.recover_secret_batch_ct(groups)
    assert rst.count(5) == 1 and rst.count(4) == 1
    for g in range(N_GROUPS):
        h.update(secs[g] + bytes([rst[g]]) + pks[g] + bytes([rpst[g]]))
    return h.hexdigest()


def main():
    k = int(sys.argv[1])
    from charon_amd.tbls import HipBLS
    impl = HipBLS(devices=[0] * k)
    assert impl.device_slots() == [0] * k
    print(digest(impl))


if __name__ == "__main__":
    main()
