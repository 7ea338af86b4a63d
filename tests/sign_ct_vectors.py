"""Secrets and messages shared by the secret-independent Sign / SecretToPublicKey tests (tests/test_sign_ct_host.py,
tests/test_gpu_sign_ct.py): the edge scalars of the base-|x| digit decomposition and of the fixed 4-bit window, the
values around r, and seeded random ones.  Every entry is compared with r here; nothing is assumed about it."""
import random

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
X_ABS = 0xd201000000010000
ERR_SECRET = 4


def edge_secrets():
    """The list of the kernels' edge scalars, each below 2^256 (what 32 bytes hold)."""
    v = [0, 1, 2, 3, 15, 16, 17, 2**32 - 1, 2**32 + 1, 2**64 - 1, 2**64]
    for k in (1, 2, 3):
        v += [X_ABS**k - 1, X_ABS**k, X_ABS**k + 1]
    ones = 1 + X_ABS + X_ABS**2 + X_ABS**3
    v += [d * ones for d in (1, 2, 2**62)]
    v += [2**k for k in (63, 127, 128, 191, 192, 254)]
    v += [(R - 1) // 2, (R + 1) // 2, R - 2, R - 1]
    v += [R, R + 1, 2**256 - 1]
    out = []
    for s in v:
        if 0 <= s < 2**256 and s not in out:
            out.append(s)
    return out


def random_secrets(n, seed=20261021):
    rng = random.Random(seed)
    return [rng.randrange(1, R) for _ in range(n)]


def expected_status(s):
    """Sign's status for the secret s (SecretToPublicKey also refuses 0)."""
    return 0 if s < R else ERR_SECRET


def sk_bytes(s):
    return s.to_bytes(32, "big")


MESSAGES = (bytes((0xA5 ^ (7 * i)) & 0xFF for i in range(32)), b"", bytes((i * i + 3) & 0xFF for i in range(100)))
