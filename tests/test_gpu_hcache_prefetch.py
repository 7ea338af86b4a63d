"""The H(m) prefetch (hipbls_hcache_prefetch): signing roots hashed into the H(m) cache before any
signature over them exists, so that the first keyed Verify, queued Verify or keyed sigagg of each root is a hit.  The
consumers are the unchanged hit paths of test_gpu_verify_keys_lat.py and test_gpu_sigagg_keys.py: every case asserts
the wire-format call's statuses (and bytes) for the same key bytes, and the accounting that tells a prefetched hash from
a Verify's own (hits / misses of hipbls_hcache_stats, the launch counts of "hcache_fill8" and "rlc_hash").

The table and the cache are process-wide state: every test sets what it needs and restores it in `finally`; the module
leaves the table empty, the cache disabled and the pair mode AUTO.
"""
import os
import random
import subprocess
import sys
import threading

import pytest

from tests.test_gpu_lone_sigagg import _launches, _tv
from tests.test_gpu_sigagg_keys import _tvk, _validator
from tests.test_gpu_verify_keys_lat import NVALID, _items, _load, world  # noqa: F401 (world: a fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_VERIFY = 0, 3
FILL, RLC_HASH, PREP = b"hcache_fill8", b"rlc_hash", b"verify_prep8_keys"


@pytest.fixture(scope="module")
def impl():
    from charon_amd.tbls import PAIR_AUTO, HipBLS
    h = HipBLS()
    h.hcache_config(0)
    yield h
    h.set_pair_mode(PAIR_AUTO)
    h.lib.hipbls_set_timing(0)
    h.hcache_config(0)
    h.load_pubshares([])


def _roots(tag, count):
    """`count` distinct roots: the empty message, then 200 and 32 bytes in turn."""
    rng = random.Random(tag)
    return [b""] + [rng.randbytes((32, 200)[r % 2]) for r in range(1, count)]


def _signed(impl, world, roots, wrong=False):
    """One item per root under the table's valid keys in turn: (key indices, roots, signatures); wrong = each
    signature is over another root."""
    kidx = [r % NVALID for r in range(len(roots))]
    sigs, st = impl.sign_batch([world["sks"][k] for k in kidx], [b"another root " + m if wrong else m for m in roots])
    assert set(st) == {OK}
    return kidx, list(roots), list(sigs)


def _verify(impl, world, call):
    """The keyed call; asserts it equals the wire-format call on the same key bytes."""
    kidx, msgs, sigs = call
    got = impl.batch_verify_keys_status(kidx, msgs, sigs)
    assert got == impl.batch_verify_status([world["table"][k] for k in kidx], msgs, sigs)
    return got


# ------------------------------------------------------------------------------------------------ 1. miss counts
# 1 root / the empty message and a 200-byte one / a full workgroup of 8 octets / two workgroups, the last one partial
@pytest.mark.parametrize("nr", [1, 2, 8, 9])
def test_prefetch_then_verify(impl, world, nr):
    _load(impl, world)
    roots = _roots(0x1A0 + nr, nr)
    assert len(set(roots)) == nr and [len(m) for m in roots[:2]] == [0, 200][:nr]
    good, bad = _signed(impl, world, roots), _signed(impl, world, roots, wrong=True)
    mix = _items(impl, world, 10, roots, 0x1B0 + nr)  # every kind of item, over every root
    assert set(mix[1]) == set(roots)
    impl.lib.hipbls_set_timing(1)
    try:
        impl.hcache_config(64)
        fill0, prep0 = _launches(impl, FILL), _launches(impl, PREP)
        assert impl.hcache_prefetch(roots) == (nr, 0)
        assert impl.hcache_stats() == (0, 0, nr)  # entries move, the consumers' counters do not
        assert _launches(impl, FILL) == fill0 + 1
        assert _verify(impl, world, good) == [OK] * nr
        assert impl.hcache_stats() == (nr, 0, nr)  # one hit per distinct root per call
        assert _verify(impl, world, bad) == [ERR_VERIFY] * nr
        assert impl.hcache_stats() == (2 * nr, 0, nr)
        want = _verify(impl, world, mix)
        assert want[:10] == [OK, OK, ERR_VERIFY, ERR_VERIFY, 2, 2, OK, 1, 1, ERR_VERIFY]
        assert impl.hcache_stats() == (3 * nr, 0, nr)
        for r in sorted({0, nr - 1}):  # and as lone calls: the sixteen-lane check
            assert _verify(impl, world, [x[r:r + 1] for x in good]) == [OK]
            assert _verify(impl, world, [x[r:r + 1] for x in bad]) == [ERR_VERIFY]
        lone = 2 * len({0, nr - 1})
        assert impl.hcache_stats() == (3 * nr + lone, 0, nr)
        assert impl.hcache_prefetch(roots) == (0, nr)  # all present: nothing launched, nothing counted
        assert impl.hcache_stats() == (3 * nr + lone, 0, nr)
        assert _launches(impl, FILL) == fill0 + 1
        assert _launches(impl, PREP) == prep0 + 3 + lone  # the Verifies ran their own prep (with no hash blocks)
    finally:
        impl.lib.hipbls_set_timing(0)
        impl.hcache_config(0)


# ------------------------------------------------------------------------------------------------ 2. a reader
def test_keyed_sigagg_reads_a_prefetched_root(impl):
    """The keyed sigagg never writes the cache: after a prefetch its 7-of-10 call hits, and returns the wire-format
    call's bytes and statuses."""
    parts, pk, msg, agg = _validator(impl, 0x2A00, 7, 10)
    assert impl.load_pubshares([pk]) == [OK]
    try:
        impl.hcache_config(16)
        assert impl.hcache_prefetch([msg]) == (1, 0)
        got = _tvk(impl, [parts], [0], [msg], [0])
        assert got == (0,) + _tv(impl, [parts], [pk], [msg])
        assert got == (0, [agg], [OK], [OK])
        assert impl.hcache_stats() == (1, 0, 1)
    finally:
        impl.hcache_config(0)


# ------------------------------------------------------------------------------------------------ 3. mixed call
def test_mixed_call_counts_and_ring_slots(impl, world):
    _load(impl, world)
    a, b, c, d, e, f, g, h = _roots(0x3A, 9)[1:]
    impl.lib.hipbls_set_timing(1)
    try:
        impl.hcache_config(8)
        fill0 = _launches(impl, FILL)
        assert impl.hcache_prefetch([a, b]) == (2, 0)
        assert impl.hcache_prefetch([b, c, c, a, d, c]) == (2, 2)  # c, d hashed once each; a, b present
        assert impl.hcache_stats() == (0, 0, 4)
        assert _verify(impl, world, _signed(impl, world, [a, b, c, d])) == [OK] * 4
        assert impl.hcache_stats() == (4, 0, 4)
        # only c and d took ring slots: four more roots fill the ring without evicting a
        assert impl.hcache_prefetch([e, f, g, h]) == (4, 0)
        assert impl.hcache_stats() == (4, 0, 8)
        assert _verify(impl, world, _signed(impl, world, [a, h, e, d])) == [OK] * 4
        assert impl.hcache_stats() == (8, 0, 8)
        assert _launches(impl, FILL) == fill0 + 3
    finally:
        impl.lib.hipbls_set_timing(0)
        impl.hcache_config(0)


# ------------------------------------------------------------------------------------------------ 4. bypass
def test_bypass_cache_off_and_more_roots_than_columns(impl, world):
    _load(impl, world)
    roots = _roots(0x4A, 6)[1:]
    call = _signed(impl, world, roots[:1])
    impl.lib.hipbls_set_timing(1)
    try:
        fill0, hash0 = _launches(impl, FILL), _launches(impl, RLC_HASH)
        impl.hcache_config(0)
        assert impl.hcache_prefetch(roots[:1]) == (0, 0)
        assert impl.hcache_stats() == (0, 0, 0)
        assert _verify(impl, world, call) == [OK]
        impl.hcache_config(4)
        assert impl.hcache_prefetch(roots) == (0, 0)  # 5 roots into 4 columns
        assert impl.hcache_stats() == (0, 0, 0)
        assert (_launches(impl, FILL), _launches(impl, RLC_HASH)) == (fill0, hash0)
        assert _verify(impl, world, call) == [OK]  # the Verify hashes the root itself
        assert impl.hcache_stats() == (0, 1, 1)
        assert impl.hcache_prefetch(roots[:3] + roots[:2]) == (2, 1)  # five items, three distinct: goes through
    finally:
        impl.lib.hipbls_set_timing(0)
        impl.hcache_config(0)


# ------------------------------------------------------------------------------------------------ 5. wrap
def test_wrap_and_demotion_at_capacity_4(impl, world):
    _load(impl, world)
    r = _roots(0x5A, 9)[1:]
    x, y = r[6], r[7]
    calls = {k: _signed(impl, world, [m]) for k, m in (("r0", r[0]), ("r2", r[2]), ("r5", r[5]), ("x", x), ("y", y))}
    try:
        impl.hcache_config(4)
        assert impl.hcache_prefetch(r[0:3]) == (3, 0)  # columns 0, 1, 2
        assert impl.hcache_prefetch(r[3:6]) == (3, 0)  # columns 3, 0, 1: r0 and r1 evicted, r2 stays
        assert impl.hcache_stats() == (0, 0, 4)
        # r2 sits in column 2 = ring, which x and y are about to take: demoted and hashed again, into columns 2, 3, 0
        assert impl.hcache_prefetch([r[2], x, y]) == (3, 0)
        assert impl.hcache_stats() == (0, 0, 4)
        for k in ("r2", "x", "y", "r5"):
            assert _verify(impl, world, calls[k]) == [OK], k
        assert impl.hcache_stats() == (4, 0, 4)
        assert _verify(impl, world, calls["r0"]) == [OK]  # evicted by the second prefetch: a miss, and correct
        assert impl.hcache_stats() == (4, 1, 4)
        assert _verify(impl, world, calls["r5"]) == [OK]  # r0 took column 1, r5's: a miss again, and correct
        assert impl.hcache_stats() == (4, 2, 4)
    finally:
        impl.hcache_config(0)


# ------------------------------------------------------------------------------------------------ 6. route boundary
def test_route_boundary_4096_and_4097(impl, world):
    """Up to 4,096 misses take octets (hcache_fill8), more take one lane per root (rlc_hash, on the same stream)."""
    _load(impl, world)
    rng = random.Random(0x6A)
    first = [rng.randbytes(32) for _ in range(4096)]
    second = [rng.randbytes(32) for _ in range(4097)]
    impl.lib.hipbls_set_timing(1)
    try:
        impl.hcache_config(8192)
        hits = 0
        for roots, want in ((first, (1, 0)), (second, (0, 1))):
            before = (_launches(impl, FILL), _launches(impl, RLC_HASH))
            assert impl.hcache_prefetch(roots) == (len(roots), 0)
            assert (_launches(impl, FILL) - before[0], _launches(impl, RLC_HASH) - before[1]) == want
            picks = [roots[0], roots[len(roots) // 2], roots[-1]]
            assert _verify(impl, world, _signed(impl, world, picks)) == [OK] * 3
            assert _verify(impl, world, _signed(impl, world, picks, wrong=True)) == [ERR_VERIFY] * 3
            hits += 6
            assert impl.hcache_stats()[:2] == (hits, 0)
        assert impl.hcache_stats() == (hits, 0, 8192)  # the 8,193rd root took the first one's column
    finally:
        impl.lib.hipbls_set_timing(0)
        impl.hcache_config(0)


# ------------------------------------------------------------------------------------------------ 7. other users
def test_prefetch_beside_verify_and_sigagg(impl):
    """Capacity 8.  Thread A: 20 prefetch calls of 1 to 3 fresh roots each, so the ring wraps several times.  Thread B:
    keyed Verifies and keyed 4-of-6 sigagg calls on its own two roots, whose columns thread A keeps taking.  Every
    status and aggregate byte is the wire-format call's throughout."""
    vs = [_validator(impl, 0x7A00 + k, 4, 6) for k in range(2)]
    assert impl.load_pubshares([v[1] for v in vs]) == [OK, OK]
    want_tv = [_tv(impl, [v[0]], [v[1]], [v[2]]) for v in vs]
    assert [w[2] for w in want_tv] == [[OK], [OK]]
    rng = random.Random(0x7B)
    fresh = [[rng.randbytes(32) for _ in range(1 + j % 3)] for j in range(20)]
    errors = []
    try:
        impl.hcache_config(8)
        assert impl.hcache_prefetch([v[2] for v in vs]) == (2, 0)

        def thread_a():
            try:
                for j, roots in enumerate(fresh):
                    got = impl.hcache_prefetch(roots)
                    if got != (len(roots), 0):
                        errors.append(("prefetch", j, got))
            except Exception as e:  # a thread's exception must fail the test, not vanish
                errors.append(("prefetch", repr(e)))

        def thread_b():
            try:
                for j in range(20):
                    k = j % 2
                    parts, pk, msg, agg = vs[k]
                    got = impl.batch_verify_keys_status([k, 1 - k], [msg, msg], [agg, agg])
                    if got != [OK, ERR_VERIFY]:
                        errors.append(("verify", j, got))
                    got = _tvk(impl, [parts], [k], [msg], [0])
                    if got != (0,) + want_tv[k]:
                        errors.append(("sigagg", j, got[0], got[2], got[3]))
            except Exception as e:
                errors.append(("consumer", repr(e)))

        ths = [threading.Thread(target=thread_a), threading.Thread(target=thread_b)]
        for t in ths:
            t.start()
        for t in ths:
            t.join()
        assert impl.hcache_stats()[2] == 8  # 40 fresh roots went through 8 columns
    finally:
        impl.hcache_config(0)
    assert not errors, errors[:5]


# ------------------------------------------------------------------------------------------------ 8. two contexts
def test_two_contexts_every_cache_gets_the_roots():
    """A fresh process bound to two contexts (tests/hcache_prefetch_child.py): one prefetch inserts into both caches, so
    host calls (round-robin over the contexts) and the queued Verify (the context its message hashes to) all hit."""
    r = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "tests", "hcache_prefetch_child.py")],
                       capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "hcache prefetch child: 2 contexts ok" in r.stdout
