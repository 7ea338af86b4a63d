"""Child process of tests/test_gpu_sigagg_keys.py: binds the library to two contexts on device 0, so the keyed sigagg
call over 2,050 groups is cut into two ranges of whole groups (kSplitGroups = 1,024 per range), and compares it with
the wire-format call on the same bytes.  Usage: sigagg_keys_child.py OUT.json
"""
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.test_gpu_lone_sigagg import _Reader, _tv  # noqa: E402
from tests.test_gpu_sigagg_keys import R_ORDER, _tvk  # noqa: E402

G = 2050
SUBSETS = ((1, 2), (1, 3), (2, 3))


def main():
    from charon_amd.tbls import HipBLS
    impl = HipBLS(devices=[0, 0])
    assert impl.device_slots() == [0, 0]
    rng = random.Random(0x2C0)
    vals = []  # seven validators, one root each: (shares' partials by id, root key, root)
    for k in range(7):
        secret = rng.randrange(1, R_ORDER).to_bytes(32, "big")
        root = rng.randbytes(32)
        shares = impl.threshold_split_insecure(secret, 3, 2, _Reader(0x2C1 + k))
        sigs, st = impl.sign_batch([shares[i] for i in (1, 2, 3)], [root] * 3)
        assert set(st) == {0}
        vals.append((dict(zip((1, 2, 3), sigs)), impl.secret_to_public_key(secret), root))
    groups, kidx, midx = [], [], []
    bad = 0
    for g in range(G):
        parts, _, _ = vals[g % 7]
        ids = SUBSETS[(g // 7) % 3]
        grp = {i: parts[i] for i in ids}
        k = g % 7
        if g % 257 == 5:  # another validator's key: not verified
            k = (k + 1) % 7
            bad += 1
        elif g % 257 == 9:  # another validator's partial under this id
            grp[ids[0]] = vals[(g + 3) % 7][0][ids[0]]
            bad += 1
        groups.append(grp)
        kidx.append(k)
        midx.append(g % 7)
    table = [v[1] for v in vals]
    roots = [v[2] for v in vals]
    assert impl.load_pubshares(table) == [0] * 7
    want = _tv(impl, groups, [table[k] for k in kidx], [roots[m] for m in midx])
    impl.hcache_config(16)
    rc, aggs, ast, vst = _tvk(impl, groups, kidx, roots, midx)
    hits, misses, entries = impl.hcache_stats()
    impl.hcache_config(0)
    out = dict(contexts=len(impl.device_slots()), groups=G, rc=rc, equal=(rc == 0 and (aggs, ast, vst) == want),
               ok_groups=sum(1 for s in vst if s == 0), bad_groups=bad, hits=hits, misses=misses, entries=entries)
    with open(sys.argv[1], "w") as f:
        json.dump(out, f)
    print("sigagg keys child:", out)


if __name__ == "__main__":
    main()
