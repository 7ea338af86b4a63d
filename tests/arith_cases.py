"""Case lists for the per-layer arithmetic tests, shared by the host build (tests/test_arith_cases_host.py, through
tests/native/libhost_ops.so ht_arith) and the device build (tests/test_gpu_arith_layers.py, through
tests/native/libgpu_units.so gu_*_op and libgpu_units_pair.so).  Both run the dispatchers of
tests/native/arith_units.h, whose record layouts the packers below follow.

Every input comes from a fixed seed and every expected value from oracle/bls12381.py or Python integers, never from
the code under test.  A family is a list of (input record, want): want is the exact output record, or a function of
the output record that asserts (square roots are fixed only up to sign; Jacobian results are compared after dividing
by Z in Python, so the check does not lean on the kernel's own inversion).  Each list asserts its own preconditions, so
it cannot quietly degenerate.

`host=True` gives the host build's documented view of two contracts (field.h "host builds keep every value
canonical"): fp_add_lazy / fp_sub_lazy return the reduced sum there, and fp2_mul takes canonical coefficients only, so
its unreduced operands are reduced before they go in.  The values mod p are the same cases.
"""
import functools
import random
import struct

from oracle import bls12381 as bls

P = bls.P
R = bls.R
X_ABS = bls.X_ABS
MONT = 1 << 384  # the Montgomery radix of field.h
MONT_INV = pow(MONT, -1, P)
AU_FP, AU_FP2, AU_FP12, AU_CURVE_G1, AU_CURVE_G2, AU_H2C, AU_PAIR = range(7)
IN_BYTES = (100, 192, 1152, 720, 720, 208, 576)
OUT_BYTES = (52, 100, 576, 296, 296, 288, 576)

EDGE = [0, 1, 2, P - 1, P - 2, (P - 1) // 2, 1 << 380, P - (1 << 32)]  # tests/test_fp_asm.py _cases()
LAZY = [P, P + 1, 2 * P - 2, 2 * P - 1]  # unreduced sums in [p, 2p)
# the product routine's contract bound (operands below 2^382): test_product_extreme_operands_keep_every_carry's ext
TOP = (1 << 382) - 1
EXT = [TOP, TOP - 1, 0x3FFFFFFF << 352, (1 << 352) - 1, 2 * P - 1, 2 * P, P - 1, 0, 1,
       (0x340223D4 << 352) | ((1 << 352) - 1)]
MUL_SMALL_K = [0, 1, 2, 3, 12, 16]  # 16: fp_mul_small's documented bound (field.h); nothing in csrc calls it today

FP_OPS = {"add": 0, "sub": 1, "neg": 2, "half": 3, "dbl": 4, "mul_small": 5, "add_lazy": 6, "sub_lazy": 7, "mul": 8,
          "inv": 9, "inv_pow": 10, "sqrt": 11}
FP2_OPS = {"mul": 0, "sqr": 1, "sqr_c": 2, "mul_fp": 3, "mul_xi": 4, "mul_3b2": 5, "inv": 6, "sqrt": 7}
FP12_OPS = {"mul": 0, "sqr": 1, "inv": 2, "frob1": 3, "frob2": 4, "frob3": 5, "cyc_sqr": 6, "mul_line": 7}
CURVE_OPS = {"add": 0, "add_aff": 1, "dbl": 2, "mul_limbs": 3, "mul_u64": 4, "eq": 5, "in_subgroup": 6,
             "mul_glv4": 7, "clear_cofactor": 8, "subgroup_and_mul_i64": 9, "decompress": 10, "decompress_check": 11}
G2_ONLY = ("mul_glv4", "clear_cofactor", "subgroup_and_mul_i64")
H2C_OPS = {"expand_message": 0, "hash_to_g2": 1, "map_to_curve": 2}
PAIR_OPS = {"pairing": 0, "product_n": 1, "product_2": 2}
H2C_LENGTHS = [0, 1, 31, 32, 33, 55, 56, 63, 64, 65, 200]


class Family:
    def __init__(self, layer, op, cases):
        self.layer, self.op = layer, op
        self.inputs = [c[0] for c in cases]
        self.wants = [c[1] for c in cases]
        assert self.inputs and all(len(b) == IN_BYTES[layer] for b in self.inputs)

    def __len__(self):
        return len(self.inputs)

    def check(self, run):
        """run(layer, op, input bytes, n) -> output bytes: every case's output record against its want."""
        n, ob = len(self.inputs), OUT_BYTES[self.layer]
        out = run(self.layer, self.op, b"".join(self.inputs), n)
        assert len(out) == n * ob
        for i, want in enumerate(self.wants):
            got = out[ob * i:ob * (i + 1)]
            if callable(want):
                want(got)
            else:
                assert got == want, (self.layer, self.op, i, self.inputs[i].hex())


def mont(x):
    return x * MONT % P


def unmont(x):
    return x * MONT_INV % P


def raw(x):  # 12 little-endian 32-bit limbs
    return x.to_bytes(48, "little")


def be(x):
    return x.to_bytes(48, "big")


def _pairs(seed, extra=4):
    rng = random.Random(seed)
    xs = EDGE + [rng.randrange(P) for _ in range(extra)]
    return [(a, b) for a in xs for b in xs]


# ------------------------------------------------------------------------------------------------ Fp, raw limbs
def _fp_in(a, b=0, k=0):
    return raw(a) + raw(b) + struct.pack("<I", k)


def _fp_out(r, flag=0):
    return raw(r) + struct.pack("<I", flag)


@functools.lru_cache(None)
def fp_family(name, host=False):
    op = FP_OPS[name]
    if name in ("add", "sub", "neg", "half", "dbl", "add_lazy", "sub_lazy"):
        fn = {"add": lambda a, b: (a + b) % P, "sub": lambda a, b: (a - b) % P, "neg": lambda a, b: -a % P,
              "half": lambda a, b: a * pow(2, -1, P) % P, "dbl": lambda a, b: 2 * a % P,
              # unreduced, as test_lazy_add_sub_blocks expects them (the host build reduces: see the module docstring)
              "add_lazy": lambda a, b: (a + b) % P if host else a + b,
              "sub_lazy": lambda a, b: (a - b) % P if host else a + P - b}[name]
        cases = [(_fp_in(a, b), _fp_out(fn(a, b))) for a, b in _pairs(101)]
        assert all(a < P and b < P for a, b in _pairs(101))
    elif name == "mul_small":
        rng = random.Random(102)
        xs = EDGE + [rng.randrange(P) for _ in range(4)]
        cases = [(_fp_in(a, 0, k), _fp_out(k * a % P)) for k in MUL_SMALL_K for a in xs]
    elif name == "mul":
        rng = random.Random(606)
        prs = _pairs(103) + [(a, b) for a in EXT for b in EXT + [rng.randrange(1 << 382) for _ in range(4)]]
        assert all(a <= TOP and b <= TOP for a, b in prs)
        cases = [(_fp_in(a, b), _fp_out(a * b * MONT_INV % P)) for a, b in prs]
    elif name in ("inv", "inv_pow"):
        rng = random.Random(11)
        fib = [1, 1]
        while fib[-1] < P:
            fib.append(fib[-1] + fib[-2])
        xs = [0, 1, 2, P - 1, P - 2, (P - 1) // 2] + [(1 << k) % P for k in range(0, 381, 17)] + fib[-12:] + \
            [f % P for f in fib[-12:]] + [rng.randrange(P) for _ in range(64)]
        assert fib[-1] > P > fib[-2]
        ms = [mont(x % P) for x in xs]  # Montgomery form of x: what the kernels hand fp_inv
        if name == "inv":  # the divstep bound covers operands below 2^382; the Fermat power takes canonical ones
            ms += [P, P + 1, 2 * P - 1, 2 * P - 2, TOP]
        cases = [(_fp_in(m), _fp_out(mont(pow(unmont(m), P - 2, P)))) for m in ms]
    elif name == "sqrt":
        squares = [e * e % P for e in EDGE]
        non_res = [-s % P for s in squares if s]  # p = 3 mod 4: -1 is a non-residue
        assert all(bls.fp_sqrt(s) is not None for s in squares) and all(bls.fp_sqrt(s) is None for s in non_res)

        def want(a, square):
            def chk(got):
                assert struct.unpack("<I", got[48:])[0] == int(square), hex(a)
                if square:
                    s = unmont(int.from_bytes(got[:48], "little"))
                    assert int.from_bytes(got[:48], "little") < P and s * s % P == a, hex(a)
            return chk
        cases = [(_fp_in(mont(a)), want(a, True)) for a in squares] + \
                [(_fp_in(mont(a)), want(a, False)) for a in non_res]
        assert 0 in squares
    return Family(AU_FP, op, cases)


# ------------------------------------------------------------------------------------------------ Fp2, raw limbs
def _fp2_in(a, b=(0, 0)):
    return raw(a[0]) + raw(a[1]) + raw(b[0]) + raw(b[1])


def _fp2_out(r, flag=0):
    return raw(r[0]) + raw(r[1]) + struct.pack("<I", flag)


def _f2_mont(a):
    return (mont(a[0]), mont(a[1]))


def fp2_mul_cases():
    """(a, b, product) on raw limbs: coefficients from the edge set and the unreduced bounds (tower.h: operands may be
    sums in [0, 2p)); the formulas of test_fp2_product_routine."""
    rng = random.Random(42)
    pool = EDGE + LAZY + [rng.randrange(P) for _ in range(2)]
    quads = [tuple(rng.choice(pool) for _ in range(4)) for _ in range(248)]
    quads += [(x, x, x, x) for x in (2 * P - 1, 2 * P - 2, P, P - 1)] + \
             [(2 * P - 1, 0, 2 * P - 1, 0), (0, 2 * P - 1, 0, 2 * P - 1), (2 * P - 1, 2 * P - 1, 0, 2 * P - 1),
              (2 * P - 1, 2 * P - 1, 2 * P - 1, 0)]
    assert any(max(q) >= P for q in quads) and all(max(q) < 2 * P for q in quads)
    return [((a0, a1), (b0, b1), ((a0 * b0 - a1 * b1) * MONT_INV % P, (a0 * b1 + a1 * b0) * MONT_INV % P))
            for a0, a1, b0, b1 in quads]


def fp2_sqr_cases():
    """(a, square), canonical operands only (tower.h fp2_sqr's contract)."""
    return [((a0, a1), ((a0 * a0 - a1 * a1) * MONT_INV % P, 2 * a0 * a1 * MONT_INV % P)) for a0, a1 in _pairs(52, 2)]


def fp2_mul_fp_cases():
    rng = random.Random(53)
    return [((a0, a1), (b, 0), (a0 * b * MONT_INV % P, a1 * b * MONT_INV % P))
            for a0, a1 in _pairs(53, 0) for b in (rng.choice(EDGE), rng.randrange(P))]


@functools.lru_cache(None)
def fp2_family(name, host=False):
    op = FP2_OPS[name]
    if name == "mul":
        red = (lambda a: (a[0] % P, a[1] % P)) if host else (lambda a: a)
        cases = [(_fp2_in(red(a), red(b)), _fp2_out(r)) for a, b, r in fp2_mul_cases()]
    elif name in ("sqr", "sqr_c"):
        cases = [(_fp2_in(a), _fp2_out(r)) for a, r in fp2_sqr_cases()]
    elif name == "mul_fp":
        cases = [(_fp2_in(a, b), _fp2_out(r)) for a, b, r in fp2_mul_fp_cases()]
    elif name == "mul_xi":
        cases = [(_fp2_in((a0, a1)), _fp2_out(((a0 - a1) % P, (a0 + a1) % P))) for a0, a1 in _pairs(54, 2)]
    elif name == "mul_3b2":
        cases = [(_fp2_in((a0, a1)), _fp2_out((12 * (a0 - a1) % P, 12 * (a0 + a1) % P))) for a0, a1 in _pairs(55, 2)]
    elif name == "inv":
        rng = random.Random(56)
        xs = [(0, 0)] + [(e, 0) for e in EDGE[1:]] + [(0, e) for e in EDGE[1:]] + \
            [(rng.choice(EDGE), rng.choice(EDGE)) for _ in range(16)] + \
            [(rng.randrange(P), rng.randrange(P)) for _ in range(16)]
        cases = [(_fp2_in(_f2_mont(a)), _fp2_out(_f2_mont(bls.f2_inv(a) if a != (0, 0) else (0, 0)))) for a in xs]
        assert all(bls.f2_mul(a, bls.f2_inv(a)) == (1, 0) for a in xs[1:])
    elif name == "sqrt":
        rng = random.Random(57)
        res = [e * e % P for e in EDGE[1:]]
        xs = [(0, 0)] + [(c, 0) for c in res] + [(-c % P, 0) for c in res] + [(0, e) for e in EDGE[1:]]
        assert all(bls.fp_sqrt(c) is not None and bls.fp_sqrt(-c % P) is None for c in res)
        xs += [bls.f2_sqr((rng.choice(EDGE), rng.choice(EDGE))) for _ in range(8)]
        xs += [bls.f2_sqr((rng.randrange(P), rng.randrange(P))) for _ in range(8)]
        non = []
        while len(non) < 8:
            a = (rng.randrange(P), rng.randrange(P))
            if not bls.f2_is_square(a):
                non.append(a)
        xs += non
        squares = [a == (0, 0) or bls.f2_is_square(a) for a in xs]
        assert squares.count(False) == 8 and all(squares[:-8])

        def want(a, square):
            def chk(got):
                assert struct.unpack("<I", got[96:])[0] == int(square), a
                if square:
                    m = (int.from_bytes(got[:48], "little"), int.from_bytes(got[48:96], "little"))
                    assert max(m) < P and bls.f2_sqr((unmont(m[0]), unmont(m[1]))) == a, a
            return chk
        cases = [(_fp2_in(_f2_mont(a)), want(a, s)) for a, s in zip(xs, squares)]
    return Family(AU_FP2, op, cases)


# ------------------------------------------------------------------------------------------------ split-Fp2 build
def pair_cases(op):
    """(a, b, r) raw for tests/native/gpu_units_pair.hip: 0 fp2_mul, 1 fp2_sqr, 2 fp2_mul_fp (the cases of the
    one-lane routines above), 3 / 4 fp_pow to (p + 1) / 4 and (p - 3) / 4 on the inputs of test_fp_pow_square_root_chains
    (result in c0, c1 = 0)."""
    if op == 0:
        return fp2_mul_cases()
    if op == 1:
        return [(a, (0, 0), r) for a, r in fp2_sqr_cases()]
    if op == 2:
        return fp2_mul_fp_cases()
    # tests/test_gpu_fp_sqr.py test_fp_pow_square_root_chains' list: 0, 1, p - 1, 4, p - 4, then 29 squares and 30
    # non-residues by construction, 64 per exponent (two full waves of the split build)
    minus1 = op - 3
    rng = random.Random(1105 + minus1)
    plain = [0, 1, P - 1, 4, P - 4]
    plain += [pow(rng.randrange(2, P), 2, P) for _ in range(29)]
    while len(plain) < 64:
        x = rng.randrange(2, P)
        if pow(x, (P - 1) // 2, P) == P - 1:
            plain.append(x)
    legendre = [pow(x, (P - 1) // 2, P) for x in plain]
    assert len(plain) == 64 and legendre.count(1) >= 29 and legendre.count(P - 1) >= 30
    e = (P - 3) // 4 if minus1 else (P + 1) // 4
    return [((mont(x), 0), (0, 0), (mont(pow(x, e, P)), 0)) for x in plain]


# ------------------------------------------------------------------------------------------------ Fp12
def f12_bytes(f):
    return b"".join(be(c) for f6 in f for f2 in f6 for c in f2)


def rand_f12(rng):
    return tuple(tuple((rng.randrange(P), rng.randrange(P)) for _ in range(3)) for _ in range(2))


def _cyclotomic(a):  # a^((p^6 - 1)(p^2 + 1))
    c = bls.f12_mul(bls.f12_conj(a), bls.f12_inv(a))
    return bls.f12_mul(bls.f12_pow(c, P * P), c)


@functools.lru_cache(None)
def fp12_family(name):
    op = FP12_OPS[name]
    rng = random.Random(9)
    z = (0, 0)
    r1, r2, b1, b2 = (rand_f12(rng) for _ in range(4))
    top = tuple(tuple((P - 1, P - 1) for _ in range(3)) for _ in range(2))
    in_fp2 = (((rng.randrange(P), rng.randrange(P)), z, z), (z, z, z))
    elems = [r1, r2, bls.F12_ONE, top, in_fp2]
    if name == "mul":
        prs = [(r1, b1), (r2, b2), (bls.F12_ONE, b1), (top, b2), (top, top), (in_fp2, b1), (b2, in_fp2)]
        cases = [(f12_bytes(a) + f12_bytes(b), f12_bytes(bls.f12_mul(a, b))) for a, b in prs]
    elif name in ("sqr", "inv"):
        fn = bls.f12_sqr if name == "sqr" else bls.f12_inv
        cases = [(f12_bytes(a) + f12_bytes(b1), f12_bytes(fn(a))) for a in elems]
    elif name.startswith("frob"):
        cases = [(f12_bytes(a) + f12_bytes(b1), f12_bytes(bls.f12_pow(a, P ** int(name[4])))) for a in elems]
    elif name == "cyc_sqr":
        cyc = [_cyclotomic(r1), _cyclotomic(r2), bls.F12_ONE, _cyclotomic(top)]
        for c in cyc:  # in the cyclotomic subgroup: c^(p^4 - p^2 + 1) = 1
            assert bls.f12_mul(bls.f12_pow(c, P ** 4), c) == bls.f12_pow(c, P * P)
        assert cyc[0] != bls.F12_ONE and cyc[1] != bls.F12_ONE
        cases = [(f12_bytes(c) + f12_bytes(b1), f12_bytes(bls.f12_mul(c, c))) for c in cyc]
    elif name == "mul_line":
        def line(g0, g1, h1):  # (g0 + g1 v) + (h1 v) w
            return ((g0, g1, z), (z, h1, z))
        g0, g1, h1 = b1[0][0], b1[0][1], b1[1][1]
        lines = [line(g0, g1, h1), line(g0, z, h1), line(g0, g1, z), line(b2[0][0], b2[0][1], b2[1][1])]
        cases = [(f12_bytes(a) + f12_bytes(ln), f12_bytes(bls.f12_mul(a, ln))) for a in elems for ln in lines]
    return Family(AU_FP12, op, cases)


# ------------------------------------------------------------------------------------------------ curve
class _Group:
    """The oracle's affine arithmetic (None = infinity) and the record packing for F = fp (g = 1) or fp2 (g = 2)."""

    def __init__(self, g):
        self.g = g
        self.layer = AU_CURVE_G1 if g == 1 else AU_CURVE_G2
        self.add, self.mul, self.neg = (bls.g1_add, bls.g1_mul, bls.g1_neg) if g == 1 else \
            (bls.g2_add, bls.g2_mul, bls.g2_neg)
        self.gen = bls.G1_GEN if g == 1 else bls.G2_GEN
        self.compress = bls.g1_compress if g == 1 else bls.g2_compress
        self.decompress_fn = bls.g1_decompress if g == 1 else bls.g2_decompress
        self.csize = 48 * g  # bytes per coordinate; also the compressed size

    # field helpers on ints (g = 1) or pairs (g = 2)
    def fmul(self, a, b):
        return a * b % P if self.g == 1 else bls.f2_mul(a, b)

    def finv(self, a):
        return pow(a, -1, P) if self.g == 1 else bls.f2_inv(a)

    def fbytes(self, a):
        return be(a) if self.g == 1 else be(a[0]) + be(a[1])

    def ffrom(self, b):
        v = [int.from_bytes(b[48 * i:48 * i + 48], "big") for i in range(self.g)]
        return v[0] if self.g == 1 else (v[0], v[1])

    def frand(self, rng):
        return rng.randrange(1, P) if self.g == 1 else (rng.randrange(1, P), rng.randrange(P))

    @property
    def zero(self):
        return 0 if self.g == 1 else (0, 0)

    @property
    def one(self):
        return 1 if self.g == 1 else (1, 0)

    def jac(self, pt, lam=None):
        """Jacobian coordinates of an affine point scaled through by lam (X lam^2, Y lam^3, lam); None -> Z = 0."""
        if pt is None:
            return (lam or self.one, lam or self.one, self.zero)
        lam = lam or self.one
        l2 = self.fmul(lam, lam)
        return (self.fmul(pt[0], l2), self.fmul(pt[1], self.fmul(l2, lam)), lam)

    def jbytes(self, j):
        return b"".join(self.fbytes(c) for c in j).ljust(288, b"\0")

    def record(self, p=None, q=None, k=0, c=0, comp=b""):
        return (self.jbytes(p or self.jac(None)) + self.jbytes(q or self.jac(None)) + k.to_bytes(32, "little") +
                struct.pack("<q", c) + comp.ljust(96, b"\0")).ljust(720, b"\0")

    def affine(self, got):
        """(flag, affine point or None) of an output record: the Jacobian result divided through by Z."""
        flag = struct.unpack("<i", got[:4])[0]
        s = self.csize
        x, y, zc = (self.ffrom(got[8 + s * i:8 + s * (i + 1)]) for i in range(3))
        if zc == self.zero:
            return flag, None
        zi = self.finv(zc)
        zi2 = self.fmul(zi, zi)
        return flag, (self.fmul(x, zi2), self.fmul(y, self.fmul(zi2, zi)))

    def want_point(self, pt, flag=0):
        def chk(got):
            assert self.affine(got) == (flag, pt)
        return chk

    def want_flag(self, flag):
        def chk(got):
            assert struct.unpack("<i", got[:4])[0] == flag
        return chk

    def random_point(self, rng):
        """A point of the curve almost surely outside the prime-order subgroup."""
        while True:
            if self.g == 1:
                x = rng.randrange(P)
                y = bls.fp_sqrt((x ** 3 + 4) % P)
            else:
                x = (rng.randrange(P), rng.randrange(P))
                y = bls.f2_sqrt(bls.f2_add(bls.f2_mul(bls.f2_sqr(x), x), bls.B2))
            if y is not None:
                return (x, y)


def _decompress_cases(G, rng, outside):
    c = G.csize
    pt = G.mul(G.gen, rng.randrange(1, R))
    enc = bytearray(G.compress(pt))
    flipped = bytes([enc[0] ^ 0x20]) + bytes(enc[1:])
    inf = bytes([0xC0]) + bytes(c - 1)
    x_is_p = bytearray(bytes(c - 48) + be(P))  # G2: x.c1 = 0, x.c0 = p
    x_is_p[0] |= 0x80
    not_on_curve = None
    while not_on_curve is None:
        body = bytearray(b"".join(be(rng.randrange(P)) for _ in range(G.g)))
        body[0] |= 0x80
        try:
            G.decompress_fn(bytes(body), False)
        except bls.BLSError:
            not_on_curve = bytes(body)
    cases = [bytes(enc), flipped, inf, bytes([0xC0]) + bytes(c - 2) + b"\x01", bytes([0xE0]) + bytes(c - 1),
             bytes([enc[0] & 0x7F]) + bytes(enc[1:]), bytes(c), bytes(x_is_p), bytes([0x9F]) + b"\xff" * (c - 1),
             not_on_curve, G.compress(outside)]
    if G.g == 2:
        x1_is_p = bytearray(be(P) + be(5))  # x.c1 = p, x.c0 fine
        x1_is_p[0] |= 0x80
        # x.c0 = p + k with (k, 0) on the curve: only the range check of c0 rejects it (x.c0 = p reduces to x = 0,
        # which is off the curve anyway)
        k = next(k for k in range(1, 64) if bls.f2_sqrt(bls.f2_add((k ** 3 % P, 0), bls.B2)) is not None)
        assert bls.g2_on_curve(((k, 0), bls.f2_sqrt(bls.f2_add((k ** 3 % P, 0), bls.B2))))
        x0_wraps = bytearray(bytes(48) + be(P + k))
        x0_wraps[0] |= 0x80
        cases += [bytes(x1_is_p), bytes([0x9F]) + b"\xff" * 47 + bytes(enc[48:]), bytes(enc[:48]) + b"\xff" * 48,
                  bytes(x0_wraps)]
    return cases


@functools.lru_cache(None)
def curve_family(g, name):
    G = _Group(g)
    op = CURVE_OPS[name]
    rng = random.Random(300 + 10 * g + op)
    pt, qt = G.mul(G.gen, rng.randrange(2, R)), G.mul(G.gen, rng.randrange(2, R))
    l1, l2 = G.frand(rng), G.frand(rng)
    inf = G.jac(None)
    inf_xy = G.jac(None, G.frand(rng))  # Z = 0 with other X, Y
    outside = G.random_point(rng)
    assert G.mul(outside, R) is not None and G.mul(pt, R) is None  # really outside / inside the subgroup
    assert G.jac(pt, l1) != G.jac(pt, l2) and G.jac(pt, l1)[0] != pt[0]  # P = Q is not visible in the coordinates
    if name == "add":
        prs = [(G.jac(pt, l1), G.jac(qt, l2), G.add(pt, qt)), (G.jac(pt, l1), G.jac(pt, l2), G.add(pt, pt)),
               (G.jac(pt, l1), G.jac(pt), G.add(pt, pt)), (G.jac(pt, l1), G.jac(G.neg(pt), l2), None),
               (inf, G.jac(qt, l2), qt), (inf_xy, G.jac(qt), qt), (G.jac(pt, l1), inf, pt), (G.jac(pt, l1), inf_xy, pt),
               (inf, inf_xy, None), (G.jac(outside, l1), G.jac(outside, l2), G.add(outside, outside))]
        cases = [(G.record(p, q), G.want_point(w)) for p, q, w in prs]
    elif name == "add_aff":  # the second operand is affine: it cannot be infinity
        prs = [(G.jac(pt, l1), qt, G.add(pt, qt)), (G.jac(pt, l1), pt, G.add(pt, pt)), (G.jac(pt), pt, G.add(pt, pt)),
               (G.jac(pt, l1), G.neg(pt), None), (inf, qt, qt), (inf_xy, qt, qt)]
        cases = [(G.record(p, G.jac(q)), G.want_point(w)) for p, q, w in prs]
    elif name == "dbl":
        prs = [(inf, None), (inf_xy, None), (G.jac(pt, l1), G.add(pt, pt)), (G.jac(qt), G.add(qt, qt)),
               (G.jac(outside, l2), G.add(outside, outside))]
        assert G.add(pt, pt) is not None  # no 2-torsion in play
        cases = [(G.record(p), G.want_point(w)) for p, w in prs]
    elif name == "mul_limbs":
        ks = [0, 1, 2, R - 1, R, R + 1, (1 << 255) - 1, (1 << 256) - 1, rng.randrange(R)]
        cases = [(G.record(G.jac(pt, l1), k=k), G.want_point(G.mul(pt, k))) for k in ks]
        cases += [(G.record(inf, k=5), G.want_point(None)),
                  (G.record(G.jac(outside, l2), k=R), G.want_point(G.mul(outside, R)))]
        assert G.mul(pt, R) is None and G.mul(pt, R + 1) == pt and G.mul(pt, R - 1) == G.neg(pt)
    elif name == "mul_u64":
        ks = [0, 1, 2, 3, X_ABS, 1 << 63, (1 << 64) - 1, rng.randrange(1 << 64)]
        cases = [(G.record(G.jac(pt, l1), k=k), G.want_point(G.mul(pt, k))) for k in ks]
        cases.append((G.record(inf, k=X_ABS), G.want_point(None)))
    elif name == "eq":
        prs = [(G.jac(pt, l1), G.jac(pt, l2), 1), (G.jac(pt, l1), G.jac(pt), 1), (G.jac(pt, l1), G.jac(qt, l1), 0),
               (G.jac(pt, l1), G.jac(G.neg(pt), l2), 0), (inf, inf_xy, 1), (G.jac(pt, l1), inf, 0),
               (inf_xy, G.jac(qt), 0)]
        cases = [(G.record(p, q), G.want_flag(f)) for p, q, f in prs]
    elif name == "in_subgroup":
        h1 = 0x396C8C005555E1568C00AAAB0000AAAB  # G1's cofactor
        inside = G.mul(outside, h1 if g == 1 else bls.H_EFF_G2)
        assert inside is not None and G.mul(inside, R) is None
        prs = [(G.jac(pt, l1), 1), (G.jac(inside, l2), 1), (G.jac(inside), 1), (G.jac(outside, l1), 0),
               (G.jac(outside), 0), (inf, 1), (inf_xy, 1)]
        cases = [(G.record(p), G.want_flag(f)) for p, f in prs]
    elif name == "mul_glv4":  # plain scalars below r, subgroup points
        ks = [0, 1, R - 1, X_ABS, X_ABS ** 2, X_ABS ** 3, X_ABS - 1, rng.randrange(R)]
        assert all(k < R for k in ks)
        cases = [(G.record(G.jac(pt, l1), k=k), G.want_point(G.mul(pt, k))) for k in ks]
    elif name == "clear_cofactor":
        img = bls.iso_map_g2(bls.map_to_curve_sswu((rng.randrange(P), rng.randrange(P))))
        assert bls.g2_on_curve(img) and G.mul(img, R) is not None
        cases = [(G.record(G.jac(img)), G.want_point(G.mul(img, bls.H_EFF_G2))),
                 (G.record(G.jac(img, l1)), G.want_point(G.mul(img, bls.H_EFF_G2)))]
    elif name == "subgroup_and_mul_i64":  # affine input (Z = 1), as k_tagg_scale passes it
        cases = []
        for p, member in ((pt, 1), (outside, 0)):
            for c in (1, -1, -36, (1 << 63) - 1, 5, -(1 << 62) - 12345):
                w = G.mul(p, c) if c > 0 else G.neg(G.mul(p, -c))
                cases.append((G.record(G.jac(p), c=c), G.want_point(w, member)))
    elif name in ("decompress", "decompress_check"):
        check = name == "decompress_check"
        cases, statuses = [], []
        for enc in _decompress_cases(G, rng, outside):
            try:  # the oracle's deserialiser decides: a point -> DEC_OK, infinity -> DEC_INF, an error -> DEC_BAD
                w = G.decompress_fn(enc, check)
                st = 0 if w is not None else 2
            except bls.BLSError:
                w, st = None, 1
            statuses.append(st)
            cases.append((G.record(comp=enc), G.want_point(w, st)))
        want = [0, 0, 2, 1, 1, 1, 1, 1, 1, 1, 1 if check else 0] + [1, 1, 1, 1] * (g - 1)
        assert statuses == want, statuses  # the list holds what it says, in order
    return Family(G.layer, op, cases)


def curve_ops(g):
    return [n for n in CURVE_OPS if g == 2 or n not in G2_ONLY]


# ------------------------------------------------------------------------------------------------ hash to curve
def _g2_jac_want(pt):
    G = _Group(2)

    def chk(got):
        assert G.affine(b"\0" * 8 + got)[1] == pt
    return chk


@functools.lru_cache(None)
def h2c_family(name):
    op = H2C_OPS[name]
    rng = random.Random(400 + op)
    if name in ("expand_message", "hash_to_g2"):
        msgs = [bytes(rng.randrange(256) for _ in range(n)) for n in H2C_LENGTHS]
        assert len(bls.DST_POP) == 43

        def rec(m):
            return (struct.pack("<I", len(m)) + m).ljust(208, b"\0")
        if name == "expand_message":
            cases = [(rec(m), bls.expand_message_xmd(m, bls.DST_POP, 256).ljust(288, b"\0")) for m in msgs]
        else:
            cases = [(rec(m), _g2_jac_want(bls.hash_to_g2(m, bls.DST_POP))) for m in msgs]
    else:
        us = [(0, 0), (1, 0), (0, 1), (P - 1, P - 1)] + [(rng.randrange(P), rng.randrange(P)) for _ in range(8)]
        branches = set()
        for u in us:  # which candidate the RFC picks (tests/test_host_arith.py test_map_to_curve): is gx1 a square?
            zu2 = bls.f2_mul(bls.SSWU_Z, bls.f2_sqr(u))
            den = bls.f2_add(bls.f2_sqr(zu2), zu2)
            if bls.f2_is_zero(den):
                x1 = bls.f2_mul(bls.SSWU_B, bls.f2_inv(bls.f2_mul(bls.SSWU_Z, bls.SSWU_A)))
            else:
                x1 = bls.f2_mul(bls.f2_mul(bls.f2_neg(bls.SSWU_B), bls.f2_inv(bls.SSWU_A)),
                                bls.f2_add((1, 0), bls.f2_inv(den)))
            gx1 = bls.f2_add(bls.f2_add(bls.f2_mul(bls.f2_sqr(x1), x1), bls.f2_mul(bls.SSWU_A, x1)), bls.SSWU_B)
            branches.add(bls.f2_is_square(gx1))
        assert branches == {True, False}

        def out(pt):
            (x0, x1), (y0, y1) = pt
            return (be(x0) + be(x1) + be(y0) + be(y1)).ljust(288, b"\0")
        cases = [((struct.pack("<I", 96) + be(u[0]) + be(u[1])).ljust(208, b"\0"), out(bls.map_to_curve_sswu(u)))
                 for u in us]
    return Family(AU_H2C, op, cases)


# ------------------------------------------------------------------------------------------------ pairing, one lane
@functools.lru_cache(None)
def pairing_family(name):
    op = PAIR_OPS[name]
    p1 = bls.g1_mul(bls.G1_GEN, 0x1234567)
    q1 = bls.g2_mul(bls.G2_GEN, 0x89ABCDEF)

    def rec(pa, qa, pb, qb):
        def g2b(q):
            return be(q[0][0]) + be(q[0][1]) + be(q[1][0]) + be(q[1][1])
        return be(pa[0]) + be(pa[1]) + g2b(qa) + be(pb[0]) + be(pb[1]) + g2b(qb)
    if name == "pairing":  # the kernels' final exponentiation gives the pairing cubed (test_pairing_matches_oracle_cubed)
        e = bls.pairing(p1, q1)
        assert e != bls.F12_ONE
        cases = [(rec(p1, q1, p1, q1), f12_bytes(bls.f12_mul(bls.f12_mul(e, e), e)))]
    else:  # e(P, Q) e(-P, Q) = 1, and e(P, Q) e(P, -Q) = 1
        cases = [(rec(p1, q1, bls.g1_neg(p1), q1), f12_bytes(bls.F12_ONE)),
                 (rec(p1, q1, p1, bls.g2_neg(q1)), f12_bytes(bls.F12_ONE))]
    return Family(AU_PAIR, op, cases)


def all_families(host=False):
    """(id, family constructor) of every op family: the two test files parametrize over this one list."""
    fams = [("fp-" + n, functools.partial(fp_family, n, host)) for n in FP_OPS]
    fams += [("fp2-" + n, functools.partial(fp2_family, n, host)) for n in FP2_OPS]
    fams += [("fp12-" + n, functools.partial(fp12_family, n)) for n in FP12_OPS]
    fams += [("g%d-%s" % (g, n), functools.partial(curve_family, g, n)) for g in (1, 2) for n in curve_ops(g)]
    fams += [("h2c-" + n, functools.partial(h2c_family, n)) for n in H2C_OPS]
    fams += [("pair-" + n, functools.partial(pairing_family, n)) for n in PAIR_OPS]
    return fams
