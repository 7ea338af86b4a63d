"""Share calls and recover groups shared by the PublicKeyShare / PublicKeyRecover tests (tests/test_vss_host.py,
tests/test_gpu_vss.py), with what the Python oracle expects for each: g1_decompress, g1_mul, g1_add, g1_neg,
g1_compress and lagrange_coeffs_at_zero composed here.  The expectations are computed once per process."""
import functools
import random

from oracle import bls12381 as O

R, P = O.R, O.P
OK, ERR_PUBKEY, ERR_COMBINE = 0, 1, 5
INT64_MIN = -(1 << 63)
ZERO48 = bytes(48)
INF48 = bytes([0xC0]) + bytes(47)
SHAPES = ((1, 1), (2, 3), (7, 11))  # (threshold, n_ids)
DEALERS = (1, 3)
IDS = {1: [5], 3: [-1, INT64_MIN, (1 << 40) + 3],
       11: [0, 1, 2, 3, 4, 5, -1, (1 << 40) + 7, INT64_MIN, 2, 10]}  # 2 is repeated


@functools.lru_cache(maxsize=None)
def point(k):
    """[k] g1 (None for k = 0 mod r)"""
    return O.g1_mul(O.G1_GEN, k % R)


def enc(k):
    return O.g1_compress(point(k))


@functools.lru_cache(maxsize=None)
def decode(b):
    """(True, point) or (False, None) as the library decodes a 48-byte key: subgroup test included."""
    try:
        return True, O.g1_decompress(b)
    except O.BLSError:
        return False, None


def mul_i64(pt, x):
    """[x] P for an int64 x, as x mod r"""
    return O.g1_mul(pt, x % R)


@functools.lru_cache(maxsize=None)
def bad_encodings():
    """{name: 48 bytes the library must refuse}"""
    good = bytearray(enc(7))
    out = {}
    b = bytearray((P + 1).to_bytes(48, "big"))  # x >= p (p + 1 < 2^381: the flag bits stay free)
    b[0] |= 0x80
    out["x_ge_p"] = bytes(b)
    x = 1
    while O.fp_sqrt((x * x * x + 4) % P) is not None:
        x += 1
    b = bytearray(x.to_bytes(48, "big"))
    b[0] |= 0x80
    out["not_on_curve"] = bytes(b)
    b = bytearray(good)
    b[0] &= 0x7F
    out["flag_clear"] = bytes(b)
    b = bytearray(INF48)
    b[47] = 1
    out["inf_nonzero"] = bytes(b)
    x = 1
    while True:  # on the curve, outside G1: found without the subgroup test, refused with it
        b = bytearray(x.to_bytes(48, "big"))
        b[0] |= 0x80
        try:
            pt = O.g1_decompress(bytes(b), subgroup_check=False)
        except O.BLSError:
            pt = None
        if pt is not None and O.g1_mul(pt, R) is not None:
            break
        x += 1
    out["not_in_g1"] = bytes(b)
    for name, v in out.items():
        assert not decode(v)[0], name
    return out


class ShareCall:
    """One hipbls_public_key_share_batch call: commitments[v][d][j] (bytes), ids, and the oracle's pubs[v][i] and
    status[v]."""

    def __init__(self, name, commitments, ids):
        self.name, self.commitments, self.ids = name, commitments, list(ids)
        self.n_val, self.n_dealers, self.threshold = len(commitments), len(commitments[0]), len(commitments[0][0])
        self.pubs, self.status = [], []
        for val in commitments:
            dec = [[decode(c) for c in poly] for poly in val]
            if not all(ok for poly in dec for ok, _ in poly):
                self.status.append(ERR_PUBKEY)
                self.pubs.append([ZERO48] * len(self.ids))
                continue
            A = []
            for j in range(self.threshold):
                s = None
                for d in range(self.n_dealers):
                    s = O.g1_add(s, dec[d][j][1])
                A.append(s)
            row = []
            for x in self.ids:
                acc = A[-1]
                for j in range(self.threshold - 2, -1, -1):
                    acc = O.g1_add(mul_i64(acc, x), A[j])
                row.append(O.g1_compress(acc))
            self.status.append(OK)
            self.pubs.append(row)

    def flat(self):
        return b"".join(c for val in self.commitments for poly in val for c in poly)


@functools.lru_cache(maxsize=None)
def share_calls():
    rng = random.Random(20261024)
    bad = bad_encodings()
    out = []
    for threshold, n_ids in SHAPES:
        for nd in DEALERS:
            com = [[[enc(rng.randrange(1, R)) for _ in range(threshold)] for _ in range(nd)] for _ in range(3)]
            out.append(ShareCall("shape_t%d_i%d_d%d" % (threshold, n_ids, nd), com, IDS[n_ids]))
    # the exceptional additions: threshold 2, id 1, P = [5] g1; a polynomial is [C0, C1]
    Pb, Nb = enc(5), enc(-5)
    out.append(ShareCall("exceptional", [[[Pb, Pb]],      # [1] C1 == C0: a doubling
                                         [[Nb, Pb]],      # [1] C1 == -C0: the identity
                                         [[Pb, INF48]],   # C1 the identity
                                         [[INF48, Pb]]],  # C0 the identity
                         [1]))
    assert out[-1].pubs[0][0] == enc(10) and out[-1].pubs[1][0] == INF48 and out[-1].status == [OK] * 4
    assert out[-1].pubs[2][0] == Pb and out[-1].pubs[3][0] == Pb
    Q = enc(rng.randrange(1, R))
    out.append(ShareCall("dealer_sum_exceptional",
                         [[[Pb, Q], [Pb, Q], [Q, Pb]],      # two dealers' points equal, in both coefficients
                          [[Pb, Q], [Nb, INF48], [Q, Nb]],  # two opposite, one the identity
                          [[Pb, Pb], [Nb, Nb], [INF48, INF48]]],  # every sum the identity
                         [1, 0, -2]))
    assert out[-1].pubs[2] == [INF48] * 3
    # bad encodings: exactly one validator fails, its neighbours do not; the bad commitment at either coefficient
    com = []
    for k, name in enumerate(sorted(bad)):
        com.append([[enc(rng.randrange(1, R)), enc(rng.randrange(1, R))]])
        poly = [enc(rng.randrange(1, R)), enc(rng.randrange(1, R))]
        poly[k % 2] = bad[name]
        com.append([poly])
    com.append([[enc(rng.randrange(1, R)), enc(rng.randrange(1, R))]])
    out.append(ShareCall("bad_encodings", com, [1, 2]))
    assert out[-1].status == [OK, ERR_PUBKEY] * len(bad) + [OK]
    com = [[[enc(rng.randrange(1, R)) for _ in range(2)] for _ in range(3)] for _ in range(3)]
    com[1][2][1] = bad["not_in_g1"]
    out.append(ShareCall("bad_in_third_dealer", com, [0, 3]))
    assert out[-1].status == [OK, ERR_PUBKEY, OK]
    return tuple(out)


class Group:
    """One recover group: [(id, pubshare bytes)] and the oracle's status and key."""

    def __init__(self, name, pairs):
        self.name, self.pairs = name, list(pairs)
        ids = [i for i, _ in self.pairs]
        dec = [decode(p) for _, p in self.pairs]
        if not ids or 0 in ids or len(set(ids)) != len(ids):
            self.status = ERR_COMBINE  # public, decided first
        elif not all(ok for ok, _ in dec):
            self.status = ERR_PUBKEY
        else:
            self.status = OK
        self.pubkey = ZERO48
        if self.status == OK:
            acc = None
            for lam, (_, pt) in zip(O.lagrange_coeffs_at_zero(ids), dec):
                acc = O.g1_add(acc, O.g1_mul(pt, lam))
            self.pubkey = O.g1_compress(acc)


def _poly_pubshare(coeffs, x):
    return enc(sum(c * pow(x, j, R) for j, c in enumerate(coeffs)) % R)


@functools.lru_cache(maxsize=None)
def groups():
    rng = random.Random(20261025)
    bad = bad_encodings()
    out = []

    def real(name, ids, degree=None):
        """pubshares of a real polynomial at ids: the group recovers [f(0)] g1 when it has degree + 1 shares"""
        coeffs = [rng.randrange(1, R) for _ in range((degree if degree is not None else len(ids) - 1) + 1)]
        g = Group(name, [(i, _poly_pubshare(coeffs, i)) for i in ids])
        assert g.status == OK and g.pubkey == enc(coeffs[0]), name
        out.append(g)

    out.append(Group("empty", []))
    real("size1", [4])
    real("size3", rng.sample(range(1, 11), 3))
    real("size7", rng.sample(range(1, 11), 7))
    real("size17_leaves_small_by_t", list(range(1, 18)))
    real("size3_big_ids", [(1 << 40) + k for k in (1, 2, 5)])
    real("bound_inside", [1 << 20, -(1 << 20), 5])
    real("bound_outside", [(1 << 20) + 1, 1, 2])
    real("negative_id", [-3, 2, 7])
    real("int64_min", [INT64_MIN, 1, (1 << 62) + 5])
    out.append(Group("id0", [(1, enc(5)), (0, enc(6)), (2, enc(7))]))
    out.append(Group("duplicate", [(4, enc(5)), (9, enc(6)), (4, enc(7))]))
    out.append(Group("bad_and_duplicate", [(4, bad["x_ge_p"]), (9, enc(6)), (4, enc(7))]))
    assert out[-1].status == ERR_COMBINE
    for k, name in enumerate(sorted(bad)):
        pairs = [(1, enc(rng.randrange(1, R))), (2, enc(rng.randrange(1, R))), (3, enc(rng.randrange(1, R)))]
        pairs[k % 3] = (pairs[k % 3][0], bad[name])
        out.append(Group("bad_" + name, pairs))
        assert out[-1].status == ERR_PUBKEY
        real("after_bad_" + name, [2, 5])
    out.append(Group("identity_share", [(1, enc(9)), (2, INF48), (3, enc(11))]))
    out.append(Group("identity_result", [(1, INF48), (2, INF48)]))
    out.append(Group("identity_big_ids", [((1 << 40) + 1, INF48), (3, enc(4))]))
    assert out[-2].status == OK and out[-2].pubkey == INF48
    out.append(Group("empty_at_the_end", []))
    return tuple(out)


def write_host_file(path):
    """The vectors as tests/native/vss_host.cpp reads them.  Returns (share calls, share lanes, groups)."""
    lines = []
    lanes = 0
    for c in share_calls():
        lines.append("S %d %d %d %d %s" % (c.n_val, c.n_dealers, c.threshold, len(c.ids), " ".join(map(str, c.ids))))
        for v in range(c.n_val):
            lines.append("V %d %s" % (c.status[v], " ".join(x.hex() for poly in c.commitments[v] for x in poly)))
            lines.append("O " + " ".join(p.hex() for p in c.pubs[v]))
        lanes += c.n_val * len(c.ids)
    for g in groups():
        lines.append("G %d %d %s" % (len(g.pairs), g.status, g.pubkey.hex()))
        for i, p in g.pairs:
            lines.append("I %d %s" % (i, p.hex()))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return len(share_calls()), lanes, len(groups())
