"""Dealings, share checks and share sums shared by the joint-Feldman round tests (tests/test_dkg_ct_host.py,
tests/test_gpu_dkg_ct.py), with what the Python oracle expects for each: g1_mul, g1_add, g1_compress, g1_decompress and
recover_secret composed here (the polynomial evaluation of a share check is vss_vectors.ShareCall's).  Every secret,
coefficient and share is compared with r here; nothing is assumed about it.  The expectations are computed once per
process."""
import functools
import random

from oracle import bls12381 as O
from tests import vss_vectors as VS

R = O.R
OK, ERR_PUBKEY, ERR_VERIFY, ERR_SECRET, ERR_COMBINE = 0, 1, 3, 4, 5
INT64_MIN = -(1 << 63)
ZERO32, ZERO48, INF48 = bytes(32), bytes(48), VS.INF48
SHAPES = ((1, 1), (2, 3), (7, 10))  # (threshold, total)
COEFFS = (0, 1, R, R - 1, 2**256 - 1)  # the bad ones between good ones
MY_IDS = (1, 10, -1, INT64_MIN, 0)


def b32(v):
    return v.to_bytes(32, "big")


@functools.lru_cache(maxsize=None)
def enc(k):
    """[k] g1 compressed for any integer k (the infinity encoding for k = 0 mod r)"""
    return VS.enc(k)


def pub(scalar):
    """(status, 48 bytes) of SecretToPublicKey for a scalar below r: zero is refused."""
    return (ERR_SECRET, ZERO48) if scalar == 0 else (OK, enc(scalar))


def poly_at(coeffs, x):
    """f(x mod r) for coefficients below r"""
    return sum(c * pow(x % R, j, R) for j, c in enumerate(coeffs)) % R


class Dealing:
    """One hipbls_deal_commit_batch_ct call: polys[v] = [secret, tail...] as integers below 2^256, and the oracle's
    shares[v][i-1], status[v], commitments[v][j], com_status[v][j]."""

    def __init__(self, name, threshold, total, polys):
        self.name, self.threshold, self.total, self.polys = name, threshold, total, [list(p) for p in polys]
        self.shares, self.status, self.commitments, self.com_status = [], [], [], []
        for p in self.polys:
            assert len(p) == threshold and all(0 <= c < 2**256 for c in p)
            if all(c < R for c in p):
                sh = O.threshold_split_poly(p[0], p[1:], total)
                self.shares.append([sh[i] for i in range(1, total + 1)])
                self.status.append(OK)
                self.commitments.append([enc(c) for c in p])
                self.com_status.append([OK] * threshold)
            else:
                self.shares.append([ZERO32] * total)
                self.status.append(ERR_SECRET)
                self.commitments.append([ZERO48] * threshold)
                self.com_status.append([ERR_SECRET] * threshold)

    @property
    def n_val(self):
        return len(self.polys)

    def secrets(self):
        return [b32(p[0]) for p in self.polys]

    def tails(self):
        return [[b32(c) for c in p[1:]] for p in self.polys]


@functools.lru_cache(maxsize=None)
def dealings():
    rng = random.Random(20261101)
    out = []
    for threshold, total in SHAPES:
        def tail(n=threshold - 1):
            return [rng.randrange(1, R) for _ in range(n)]
        polys = [[c] + tail() for c in COEFFS]  # every listed value as the secret: a zero secret among them
        polys.append([rng.randrange(1, R)] + tail())
        if threshold > 1:
            for c in COEFFS:  # every listed value as the TOP coefficient: a zero top coefficient among them
                polys.append([rng.randrange(1, R)] + tail(threshold - 2) + [c])
            polys.append([rng.randrange(1, R)] + tail())
        if threshold > 2:
            p = [rng.randrange(1, R)] + tail()
            p[threshold // 2] = R  # a bad coefficient in the middle of the tail
            polys += [p, [0] * threshold, [rng.randrange(1, R)] + tail()]
        d = Dealing("shape_t%d_n%d" % (threshold, total), threshold, total, polys)
        bad = [v for v, s in enumerate(d.status) if s != OK]
        assert bad and all(d.status[v - 1] == OK and d.status[v + 1] == OK for v in bad if 0 < v < d.n_val - 1)
        out.append(d)
    assert out[0].commitments[0] == [INF48] and out[0].com_status[0] == [OK]  # a zero secret: the identity, legal
    assert out[2].commitments[-2] == [INF48] * 7
    return tuple(out)


class Check:
    """One hipbls_verify_secret_shares_batch_ct call: shares[v][d] (bytes), commitments[v][d][j] (bytes), my_id, and
    the oracle's expected[v][d] (what the share call gives for (v, d) at my_id, zero bytes when a commitment does not
    decode), decode_status[v][d] and status[v][d]."""

    def __init__(self, name, shares, commitments, my_id):
        self.name, self.shares, self.commitments, self.my_id = name, shares, commitments, my_id
        self.n_val, self.n_dealers, self.threshold = len(shares), len(shares[0]), len(commitments[0][0])
        call = VS.ShareCall(name, [[poly] for val in commitments for poly in val], [my_id])
        nd = self.n_dealers
        self.expected = [[call.pubs[v * nd + d][0] for d in range(nd)] for v in range(self.n_val)]
        self.decode_status = [call.status[v * nd:v * nd + nd] for v in range(self.n_val)]
        self.status = []
        for v in range(self.n_val):
            row = []
            for d in range(nd):
                s = int.from_bytes(shares[v][d], "big")
                if self.decode_status[v][d] != OK:
                    row.append(ERR_PUBKEY)  # public, decided first
                elif s >= R:
                    row.append(ERR_SECRET)
                elif enc(s) != self.expected[v][d]:
                    row.append(ERR_VERIFY)
                else:
                    row.append(OK)
            self.status.append(row)

    def flat_shares(self):
        return b"".join(s for row in self.shares for s in row)

    def flat_commitments(self):
        return b"".join(c for val in self.commitments for poly in val for c in poly)


def _honest(rng, threshold, my_id, coeffs=None):
    """(share bytes, commitments) of one dealer's polynomial at my_id"""
    coeffs = coeffs if coeffs is not None else [rng.randrange(1, R) for _ in range(threshold)]
    return b32(poly_at(coeffs, my_id)), [enc(c) for c in coeffs]


@functools.lru_cache(maxsize=None)
def checks():
    rng = random.Random(20261102)
    bad = VS.bad_encodings()
    out = []
    for (threshold, _), my_id in zip(SHAPES + ((2, 3), (7, 10)), MY_IDS):
        # 3 validators x 2 dealers of honest shares at this id, then the faults, each between honest neighbours
        sh, com = [], []
        nv = 3 if threshold < 7 else 2
        for v in range(nv):
            pairs = [_honest(rng, threshold, my_id) for _ in range(2)]
            sh.append([p[0] for p in pairs])
            com.append([p[1] for p in pairs])
        s = int.from_bytes(sh[1][0], "big")
        sh[1][0] = b32((s + 1) % R)  # off by one
        c = Check("t%d_id%d" % (threshold, my_id), sh, com, my_id)
        assert c.status == [[OK, OK], [ERR_VERIFY, OK], [OK, OK]][:nv], (c.name, c.status)
        out.append(c)
    # shares 0, r, 2^256 - 1; a zero share that IS the polynomial's value; a share of the identity polynomial
    my_id = 3
    a0 = rng.randrange(1, R)
    zero_poly = [a0, (-a0 * pow(my_id, -1, R)) % R]  # f(3) = 0
    rows = [_honest(rng, 2, my_id), (b32(0), _honest(rng, 2, my_id)[1]), (b32(R), _honest(rng, 2, my_id)[1]),
            (b32(2**256 - 1), _honest(rng, 2, my_id)[1]), _honest(rng, 2, my_id, zero_poly),
            (b32(0), [INF48, INF48]), (b32(1), [INF48, INF48]), _honest(rng, 2, my_id)]
    c = Check("edge_shares", [[r[0]] for r in rows], [[r[1]] for r in rows], my_id)
    assert c.status == [[OK], [ERR_VERIFY], [ERR_SECRET], [ERR_SECRET], [OK], [OK], [ERR_VERIFY], [OK]], c.status
    assert c.shares[4][0] == ZERO32 and c.expected[4][0] == INF48
    out.append(c)
    # commitments that do not decode, at either coefficient, with a right share, a wrong one and one >= r: the public
    # error wins every time; the other dealer of the same validator is not touched
    sh, com = [], []
    for k, name in enumerate(sorted(bad)):
        good = _honest(rng, 2, 5)
        poly = [enc(rng.randrange(1, R)), enc(rng.randrange(1, R))]
        poly[k % 2] = bad[name]
        sh.append([good[0], (b32(7), b32(R), b32(0))[k % 3]])
        com.append([good[1], poly])
    c = Check("bad_encodings", sh, com, 5)
    assert c.status == [[OK, ERR_PUBKEY]] * len(bad), c.status
    out.append(c)
    assert {c.my_id for c in out} >= set(MY_IDS)
    return tuple(out)


class Combine:
    """One hipbls_combine_shares_batch_ct call: shares[v][d] (bytes), include[v][d] (or None for all), and the oracle's
    out[v], status[v], pubs[v], pub_status[v]."""

    def __init__(self, name, shares, include):
        self.name, self.shares, self.include = name, shares, include
        self.n_val, self.n_dealers = len(shares), len(shares[0])
        self.out, self.status, self.pubs, self.pub_status = [], [], [], []
        for v in range(self.n_val):
            inc = [True] * self.n_dealers if include is None else [bool(f) for f in include[v]]
            vals = [int.from_bytes(s, "big") for s, f in zip(shares[v], inc) if f]
            if not vals:
                st = ERR_COMBINE  # public, decided first
            elif any(x >= R for x in vals):
                st = ERR_SECRET
            else:
                st = OK
            x = sum(vals) % R if st == OK else 0
            self.status.append(st)
            self.out.append(b32(x) if st == OK else ZERO32)
            pst, pk = pub(x) if st == OK else (ERR_SECRET, ZERO48)
            self.pub_status.append(pst)
            self.pubs.append(pk)

    def flat_shares(self):
        return b"".join(s for row in self.shares for s in row)

    def flat_include(self):
        return None if self.include is None else bytes(f for row in self.include for f in row)  # non-zero: included


@functools.lru_cache(maxsize=None)
def combines():
    rng = random.Random(20261103)

    def row(n):
        return [b32(rng.randrange(1, R)) for _ in range(n)]

    out = []
    for nd in (1, 3, 9):
        out.append(Combine("all_d%d" % nd, [row(nd) for _ in range(4)], None))
    nd = 4
    a, b = rng.randrange(1, R), rng.randrange(1, R)
    zero_sum = [b32(a), b32(b), b32((-a - b) % R), b32(rng.randrange(1, R))]  # the first three add up to 0 mod r
    with_bad = row(nd)
    with_bad[2] = b32(R)
    top = [b32(R - 1)] * nd
    shares = [row(nd), row(nd), row(nd), with_bad, with_bad, zero_sum, top, [b32(2**256 - 1)] + row(nd - 1), row(nd)]
    include = [[1, 1, 1, 1], [0, 0, 0, 0], [0, 0, 1, 0], [1, 1, 0, 1], [1, 1, 1, 1], [1, 1, 1, 0], [1, 1, 1, 1],
               [2, 0, 0, 0], [0, 255, 1, 0]]
    c = Combine("masks", shares, include)
    assert c.status == [OK, ERR_COMBINE, OK, OK, ERR_SECRET, OK, OK, ERR_SECRET, OK], c.status
    assert c.out[2] == shares[2][2] and c.out[5] == ZERO32 and c.pub_status[5] == ERR_SECRET
    assert c.out[6] == b32((4 * (R - 1)) % R)
    out.append(c)
    out.append(Combine("masks_ignored", shares[:3] + shares[5:7], None))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def joint_dealing():
    """A joint dealing on the oracle alone: 3 dealers, 2-of-3.  Returns (dealer polynomials, final shares by id, the
    commitments' sums by coefficient as points)."""
    rng = random.Random(20261104)
    polys = [[rng.randrange(1, R) for _ in range(2)] for _ in range(3)]
    final = {i: sum(poly_at(p, i) for p in polys) % R for i in (1, 2, 3)}
    sums = []
    for j in range(2):
        acc = None
        for p in polys:
            acc = O.g1_add(acc, VS.point(p[j]))
        sums.append(acc)
    return polys, final, sums


def trace_secrets():
    rng = random.Random(20261105)
    return list(COEFFS) + [R - 2, R + 1, 2**255, 16**63, 16**63 - 1] + [rng.randrange(1, R) for _ in range(12)]


def write_host_file(path):
    """The vectors as tests/native/dkg_ct_host.cpp reads them.  Returns (commitment lanes, check lanes, sums, trace
    secrets)."""
    lines = []
    n_com = n_chk = n_sum = 0
    for d in dealings():
        for v in range(d.n_val):
            lines.append("C %d %d %s %s" % (d.threshold, d.status[v], d.secrets()[v].hex(),
                                            " ".join(t.hex() for t in d.tails()[v])))
            for j in range(d.threshold):
                lines.append("M %d %d %s" % (j, d.com_status[v][j], d.commitments[v][j].hex()))
                n_com += 1
    for c in checks():
        for v in range(c.n_val):
            for d in range(c.n_dealers):
                lines.append("K %d %s %s %d" % (c.decode_status[v][d], c.shares[v][d].hex(), c.expected[v][d].hex(),
                                                c.status[v][d]))
                n_chk += 1
    for c in combines():
        for v in range(c.n_val):
            lines.append("U %d %d %d %s %d %s" % (c.n_dealers, 0 if c.include is None else 1, c.status[v],
                                                  c.out[v].hex(), c.pub_status[v], c.pubs[v].hex()))
            for d in range(c.n_dealers):
                lines.append("H %d %s" % (1 if c.include is None else c.include[v][d], c.shares[v][d].hex()))
            n_sum += 1
    for s in trace_secrets():
        lines.append("S %s" % b32(s).hex())
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return n_com, n_chk, n_sum, len(trace_secrets())
