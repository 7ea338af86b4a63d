"""Child process of tests/test_gpu_dkg_ct.py: binds the library to K contexts on device 0, so that the three calls of a
joint-Feldman round are cut into K ranges of whole validators, and prints a digest of everything they return.  The
parent computes the same digest on its one context.  Usage: dkg_child.py K
"""
import hashlib
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
N_VAL = 2200  # above twice the library's per-context minimum of every call at these shapes (2-of-3, 2 and 3 dealers)


def digest(impl):
    rng = random.Random(2200)
    secrets = [rng.randrange(1, R).to_bytes(32, "big") for _ in range(N_VAL)]
    tails = [[rng.randrange(1, R).to_bytes(32, "big")] for _ in range(N_VAL)]
    meet = (0, N_VAL // 2 - 1, N_VAL // 2, N_VAL - 1)  # bad validators where the ranges meet
    for p in meet:
        tails[p] = [R.to_bytes(32, "big")]
    h = hashlib.sha256()
    shares, st, com, cst = impl.deal_commit_batch_ct(secrets, tails, 3, 2)
    assert st.count(4) == 4 and st.count(0) == N_VAL - 4
    for v in range(N_VAL):
        h.update(b"".join(shares[v][i] for i in (1, 2, 3)) + bytes([st[v]]) + b"".join(com[v]) + bytes(cst[v]))
    # operator 3 checks what "dealers" 2w and 2w + 1 sent it for validator w; forged shares where the ranges meet
    nw = N_VAL // 2
    mine = [[shares[2 * w + d][3] for d in range(2)] for w in range(nw)]
    for w, d in ((nw // 2 - 1, 0), (nw // 2, 1)):  # dealers that are good validators of the deal above
        mine[w][d] = shares[2 * w + d][1]
    vst = impl.verify_secret_shares_batch_ct(mine, [[com[2 * w], com[2 * w + 1]] for w in range(nw)], 3)
    flat = [s for row in vst for s in row]
    assert flat.count(3) == 2 and flat.count(1) == 4 and flat.count(0) == N_VAL - 6
    h.update(bytes(flat))
    rows = [[shares[v][i] for i in (1, 2, 3)] for v in range(N_VAL)]
    include = [[(v + d) % 5 != 0 for d in range(3)] for v in range(N_VAL)]
    rows[N_VAL // 2][1] = R.to_bytes(32, "big")
    include[N_VAL // 2] = [True, True, True]
    include[N_VAL // 2 - 1] = [False, False, False]
    for inc in (include, None):
        out, ost, pubs, pst = impl.combine_shares_batch_ct(rows, inc)
        assert ost.count(4) == 1 and ost.count(5) == (1 if inc else 0)
        for v in range(N_VAL):
            h.update(out[v] + bytes([ost[v]]) + pubs[v] + bytes([pst[v]]))
    return h.hexdigest()


def main():
    k = int(sys.argv[1])
    from charon_amd.tbls import HipBLS
    impl = HipBLS(devices=[0] * k)
    assert impl.device_slots() == [0] * k
    print(digest(impl))


if __name__ == "__main__":
    main()
