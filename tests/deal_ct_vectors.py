"""Validators and share groups shared by the batched split / recover tests (tests/test_deal_ct_host.py,
tests/test_gpu_deal_ct.py), with what the Python oracle expects for each.  Every secret, coefficient and share is
compared with r here; nothing is assumed about it.  The expectations are computed once per process."""
import functools
import random

from oracle import bls12381 as O

R = O.R
OK, ERR_SECRET, ERR_COMBINE = 0, 4, 5
SHAPES = ((1, 1), (4, 3), (10, 7), (3, 5))  # (total, threshold)
ROOTS = (0, 1, R - 1, R, 2**256 - 1)
ZERO32, ZERO48 = bytes(32), bytes(48)


def b32(v):
    return v.to_bytes(32, "big")


@functools.lru_cache(maxsize=None)
def _pub(scalar):
    """(status, 48 bytes) of SecretToPublicKey for a scalar below r: zero is refused."""
    if scalar == 0:
        return ERR_SECRET, ZERO48
    return OK, O.secret_to_public_key(b32(scalar))


class Validator:
    """One polynomial: total, threshold, secret and tail as integers below 2^256, and the oracle's outputs."""

    def __init__(self, total, threshold, secret, tail):
        assert len(tail) == threshold - 1 and all(0 <= c < 2**256 for c in [secret] + list(tail))
        self.total, self.threshold, self.secret, self.tail = total, threshold, secret, list(tail)
        self.status = OK if all(c < R for c in [secret] + self.tail) else ERR_SECRET
        if self.status == OK:
            sh = O.threshold_split_poly(secret, self.tail, total)
            self.scalars = [secret] + [int.from_bytes(sh[i], "big") for i in range(1, total + 1)]
            self.shares = [sh[i] for i in range(1, total + 1)]
        else:
            self.scalars = [0] * (total + 1)
            self.shares = [ZERO32] * total

    @property
    def pubs(self):
        """[(status, bytes)] for k = 0..total: the root key, then the pubshares."""
        if self.status != OK:
            return [(ERR_SECRET, ZERO48)] * (self.total + 1)
        return [_pub(s) for s in self.scalars]

    def secret_bytes(self):
        return b32(self.secret)

    def tail_bytes(self):
        return [b32(c) for c in self.tail]


@functools.lru_cache(maxsize=None)
def validators():
    rng = random.Random(20261021)
    out = []
    for total, threshold in SHAPES:
        for s in ROOTS:  # every root secret of the list, a random tail
            out.append(Validator(total, threshold, s, [rng.randrange(R) for _ in range(threshold - 1)]))
        if threshold > 1:  # a tail coefficient >= r, at either end of the tail
            for pos, bad in ((0, R), (threshold - 2, 2**256 - 1)):
                tail = [rng.randrange(R) for _ in range(threshold - 1)]
                tail[pos] = bad
                out.append(Validator(total, threshold, rng.randrange(1, R), tail))
    # one share exactly 0: threshold 2, a1 = -s / i
    for total, i in ((4, 3), (1, 1)):
        s = rng.randrange(1, R)
        v = Validator(total, 2, s, [(-s * pow(i, -1, R)) % R])
        assert v.scalars[i] == 0 and v.pubs[i] == (ERR_SECRET, ZERO48)
        out.append(v)
    for n in range(32):  # seeded random validators over the shapes
        total, threshold = SHAPES[n % len(SHAPES)]
        out.append(Validator(total, threshold, rng.randrange(1, R), [rng.randrange(R) for _ in range(threshold - 1)]))
    assert sum(1 for v in out if v.status != OK) == 2 * len(SHAPES) + 2 * 3
    return tuple(out)


def by_shape():
    """{(total, threshold): [validators]} in list order: one batched call per shape."""
    d = {}
    for v in validators():
        d.setdefault((v.total, v.threshold), []).append(v)
    return d


class Group:
    """One recover group: [(id, share bytes)] and the oracle's secret, status and public key."""

    def __init__(self, pairs):
        self.pairs = list(pairs)
        ids = [i for i, _ in self.pairs]
        if not ids or 0 in ids or len(set(ids)) != len(ids):
            self.status = ERR_COMBINE  # public, decided first
        elif any(int.from_bytes(s, "big") >= R for _, s in self.pairs):
            self.status = ERR_SECRET
        else:
            self.status = OK
        if self.status == OK:
            self.secret = O.recover_secret(dict(self.pairs))
            self.pk_status, self.pk = _pub(int.from_bytes(self.secret, "big"))
        else:
            self.secret, self.pk_status, self.pk = ZERO32, ERR_SECRET, ZERO48


@functools.lru_cache(maxsize=None)
def groups():
    rng = random.Random(20261022)
    out = []
    for m in (1, 3, 7):
        for _ in range(2):  # shares of a real polynomial of degree m - 1 at ids 1..10: recovers its secret
            s = rng.randrange(1, R)
            sh = O.threshold_split_poly(s, [rng.randrange(R) for _ in range(m - 1)], 10)
            ids = rng.sample(range(1, 11), m)
            g = Group([(i, sh[i]) for i in ids])
            assert g.status == OK and g.secret == b32(s)
            out.append(g)
        out.append(Group([(rng.randrange(1, 2**40), b32(rng.randrange(R))) for _ in range(m)]))  # any shares
    big = [(-3, b32(rng.randrange(R))), (2**62 + 5, b32(rng.randrange(R))), (7, b32(rng.randrange(R)))]
    out.append(Group(big))  # a negative id (r - 3) and one above 2^62
    out.append(Group([(1, b32(5)), (0, b32(6)), (2, b32(7))]))  # id 0
    out.append(Group([(4, b32(5)), (9, b32(6)), (4, b32(7))]))  # a duplicate id
    out.append(Group([]))  # empty
    out.append(Group([(1, b32(5)), (2, b32(R)), (3, b32(7))]))  # a share >= r
    out.append(Group([(1, b32(2**256 - 1))]))
    out.append(Group([(0, b32(R)), (1, b32(1))]))  # id 0 and a share >= r: the public error wins
    out.append(Group([(1, b32(0)), (2, b32(0))]))  # recovers 0: a secret without a public key
    assert out[-1].status == OK and out[-1].pk_status == ERR_SECRET and out[-2].status == ERR_COMBINE
    out.append(Group([]))  # an empty group at the very end
    return tuple(out)


def trace_secrets():
    rng = random.Random(20261023)
    return list(ROOTS) + [R - 2, R + 1, 2**255, 16**63, 16**63 - 1] + [rng.randrange(1, R) for _ in range(16)]


def write_host_file(path):
    """The vectors as tests/native/deal_ct_host.cpp reads them."""
    lines = []
    for v in validators():
        lines.append("D %d %d %d %s %s" % (v.total, v.threshold, v.status, v.secret_bytes().hex(),
                                           " ".join(t.hex() for t in v.tail_bytes())))
        for k, (pst, pk) in enumerate(v.pubs):
            lines.append("P %d %s %d %s" % (k, v.shares[k - 1].hex() if k else "-", pst, pk.hex()))
    for g in groups():
        lines.append("R %d %d %s %d %s" % (len(g.pairs), g.status, g.secret.hex(), g.pk_status, g.pk.hex()))
        for i, s in g.pairs:
            lines.append("I %d %s" % (i, s.hex()))
    for s in trace_secrets():
        lines.append("S %s" % b32(s).hex())
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return len(validators()), len(groups()), len(trace_secrets())
