"""Child process of tests/test_gpu_vss.py: binds the library to K contexts on device 0, so that the batched
PublicKeyShare / PublicKeyRecover calls are cut into K ranges of whole validators / whole groups, and prints a digest
of everything they return.  The parent computes the same digest on its one context.  Usage: vss_child.py K
"""
import hashlib
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
N_VAL, N_GROUPS = 640, 2304  # above twice the library's per-context minimum for validators and for groups


def digest(impl):
    rng = random.Random(640)
    keys, st = impl.secret_to_public_key_batch([rng.randrange(1, R).to_bytes(32, "big") for _ in range(2 * N_VAL)])
    assert st == [0] * (2 * N_VAL)
    com = [[[keys[2 * v], keys[2 * v + 1]]] for v in range(N_VAL)]
    for p in (0, N_VAL // 2 - 1, N_VAL // 2, N_VAL - 1):  # bad validators where the ranges meet
        com[p][0][p % 2] = bytes(48)
    h = hashlib.sha256()
    pubs, pst = impl.public_key_share_batch(com, [0, 3])
    assert pst.count(1) == 4 and pst.count(0) == N_VAL - 4
    for v in range(N_VAL):
        h.update(b"".join(pubs[v]) + bytes([pst[v]]))
    groups = [{1 + g % 5: keys[g % len(keys)], 7 + g % 3: keys[(g + 1) % len(keys)]} for g in range(N_GROUPS)]
    groups[N_GROUPS // 2] = {}
    groups[N_GROUPS // 2 - 1] = {3: bytes(48)}
    pks, rst = impl.public_key_recover_batch(groups)
    assert rst.count(5) == 1 and rst.count(1) == 1
    for g in range(N_GROUPS):
        h.update(pks[g] + bytes([rst[g]]))
    return h.hexdigest()


def main():
    k = int(sys.argv[1])
    from charon_amd.tbls import HipBLS
    impl = HipBLS(devices=[0] * k)
    assert impl.device_slots() == [0] * k
    print(digest(impl))


if __name__ == "__main__":
    main()
