"""Latency of lone calls on the proposer path (INTEGRATION.md latency table).

A proposal runs randao Verify -> sigagg of one validator -> block Verify -> sigagg of one validator, each step waiting
for the one before (core/validatorapi/validatorapi.go:320,379,420,479,609; core/sigagg/sigagg.go:138-159).  This tool
times each of those calls alone, and the chain as one unit, through the synchronous host API (every call ends in a
device sync and the copy-back, so the host clock covers the whole call):

    HIPBLS_LIB=<another build> python3 charon_amd/tools/lone_latency.py [--calls 200] [--warmup 20]

One process per run; the library comes from HIPBLS_LIB as charon_amd/tbls.py allows (an A/B against another commit's
build is two processes).  After the clocked pass, a second pass with hipbls_set_timing(1) reports the per-kernel
averages of the stages the shapes launched.  Prints one JSON object.

The sigagg_keys_* shapes are the same duties through hipbls_threshold_aggregate_verify_batch_keys: the root keys in the
resident table, the H(m) cache enabled and warmed by one keyed RLC BatchVerify over the duty's partials (what parsigex
has done by the time charon aggregates); sigagg_keys_7of10_nocache runs with cache capacity 0, so the call hashes the
root itself.

The verify_keys_* shapes are the lone tbls.Verify by key index (hipbls_verify_batch_keys): _cold
empties the H(m) cache before every call (outside the clock), so the call misses and inserts; _warm repeats the call on
a cached root.  verify_keys_n<N> are N items over N / 4 roots with the cache disabled (every root hashed by the call),
verify_keys_n<N>_warm the same on cached roots.  queued_verify_keyed_* is a lone hipbls_verify with the table loaded
and the cache enabled, the Go binding's configuration.  chain_verify_keys_sigagg_keys_x2 is the proposer chain with
keyed Verify and keyed sigagg and no warm-up call: the cache is emptied before every chain, the first Verify of each
root inserts and the sigagg that follows hits.

The prefetch shapes (hipbls_hcache_prefetch): prefetch_<N> is the call itself over N roots the cache
does not hold (emptied before every call, outside the clock; 4,097 roots take the one-lane route).  The *_prefetched
shapes are verify_keys_1_cold, queued_verify_keyed_cold and the keyed chain with each root prefetched outside the
clock, after the cache was emptied and before the root's first Verify.  verify_keys_1_warm_beside_prefetch_<N> is the
warm lone Verify while another thread issues prefetch calls of N fresh roots back to back: what the prefetch's hold of
the context lock costs a caller that collides with it (the other thread also takes Python's interpreter lock between
its calls, so the row is an upper bound).  Back to back, the two threads take the context lock (an unfair mutex) in long
turns, so the row's max_ms and pass_wall_ms show starvation rather than one collision; the _beside_paced_prefetch_<N>
rows rest the other thread 5 ms between its calls, so that a clocked call waits for at most one prefetch.

The fav_keys_* shapes are the lone FastAggregateVerify by key index (hipbls_verify_aggregate_batch_keys, DESIGN.md
4.7.1) beside the wire-format fav_* rows over the same keys: 4, 12 and 512 keys, _warm on a prefetched root (the call
only reads the cache, so it stays warm) and _nocache with the cache disabled (the call hashes the root itself).  The
lock shape is cluster/lock.go:162-178 for 10,000 validators x 4 shares: one group of 40,000 keys (--lock-keys), wire
format (fav_lock_<N>), keyed with the split key sum at its default threshold (fav_keys_lock_<N>) and keyed with the
split off (fav_keys_lock_<N>_nosplit).  HIPBLS_FAV_SUM_SPLIT is read at init, so the last row comes from a child
process of this tool run with HIPBLS_FAV_SUM_SPLIT=0 and the one shape.

--shapes takes name prefixes (comma-separated) to run a subset.
"""
import argparse
import ctypes
import json
import os
import random
import statistics
import subprocess
import sys
import threading
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

R_ORDER = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
STAGES = ("verify_prep8", "verify_pair_lq16", "verify_pair_lq8", "fav_prep8", "fav_lq16", "fav", "tv_prep8", "tv_lq16",
          "tagg_sum8", "tv_phase_a", "tv_prep_pk", "tagg_scale", "tagg_sum", "tv_check_unscale", "tagg_unscale",
          "verify_pair_lq4", "verify_pair_lg2", "tv_prep8_keys", "tv_gather_keys", "tv_phase_a_keys",
          "verify_prep8_keys", "verify_gather_keys", "verify_keys", "rlc_hash", "rlc_items", "rlc_window",
          "rlc_window_lg2", "hcache_fill8", "fav_prep8_keys", "fav_lq16_keys", "fav_keys", "fav_sum_keys")
FAV_SIZES = (4, 12, 512)
SIZES = (8, 64, 512, 4096)
PREFETCH_SIZES = (1, 64, 4097)
BESIDE_SIZES = (1, 4096)
PACED_PAUSE_S = 0.005  # the paced collision rows: the other thread rests this long between its prefetch calls


def _duty(impl, rng, t, total):
    """One validator's duty: t of its `total` partials, its root key, its 32-byte signing root and Sign(secret); and
    the pubshares of those partials by id."""
    secret = rng.randrange(1, R_ORDER).to_bytes(32, "big")
    msg = rng.randbytes(32)
    shares = impl.threshold_split(secret, total, t)
    ids = sorted(rng.sample(range(1, total + 1), t))
    sigs, st = impl.sign_batch([shares[i] for i in ids], [msg] * t)
    assert set(st) == {0}
    pubshares, st = impl.secret_to_public_key_batch([shares[i] for i in ids])
    assert set(st) == {0}
    return (dict(zip(ids, sigs)), impl.secret_to_public_key(secret), msg, impl.sign(secret, msg)), \
        (dict(zip(ids, pubshares)), ids), [shares[i] for i in ids]


def _fav(impl, rng, nkeys):
    """One FastAggregateVerify group: nkeys keys over one message and the sum of their signatures."""
    sks = [rng.randrange(1, R_ORDER).to_bytes(32, "big") for _ in range(nkeys)]
    msg = rng.randbytes(32)
    pks, _ = impl.secret_to_public_key_batch(sks)
    sigs, _ = impl.sign_batch(sks, [msg] * nkeys)
    return pks, impl.aggregate(sigs), msg


def _stats(ms):
    ms = sorted(ms)
    return {"p50_ms": round(statistics.median(ms), 4), "p90_ms": round(ms[int(0.9 * (len(ms) - 1))], 4),
            "min_ms": round(ms[0], 4), "calls": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--timing-calls", type=int, default=20)
    ap.add_argument("--shapes", default="", help="comma-separated name prefixes; default: every shape")
    ap.add_argument("--lock-keys", type=int, default=40000, help="keys of the lock-shape FastAggregateVerify group")
    a = ap.parse_args()
    if a.calls < 200:
        ap.error("--calls must be at least 200")
    from charon_amd import tbls
    impl = tbls.HipBLS()
    rng = random.Random(0x10E)
    made = [_duty(impl, rng, 4, 6), _duty(impl, rng, 7, 10), _duty(impl, rng, 7, 10)]
    (d46, d710, d710b), shares = [m[0] for m in made], [m[1] for m in made]
    share_secrets = made[0][2]  # duty 0's four share secrets, in the order of its sorted ids
    fav4, fav12 = _fav(impl, rng, 4), _fav(impl, rng, 12)
    # the keyed FastAggregateVerify shapes; the large groups are only made when a shape that uses them is selected
    prefixes = tuple(a.shapes.split(",")) if a.shapes else ("",)
    lock_name = "lock_%d" % a.lock_keys

    def selected(*names):
        return any(n.startswith(prefixes) for n in names)

    favs = {4: fav4, 12: fav12}
    if selected("fav_1x512", "fav_keys_1x512"):
        favs[512] = _fav(impl, rng, 512)
    if selected("fav_" + lock_name, "fav_keys_" + lock_name):
        favs[lock_name] = _fav(impl, random.Random(0x10C), a.lock_keys)

    def verify(d):  # a Verify of the duty's aggregate: the randao / block signature check
        assert impl.batch_verify_status([d[1]], [d[2]], [d[3]]) == [0]

    def sigagg(d):
        aggs, vst = impl.batch_threshold_aggregate_verify([d[0]], [d[1]], [d[2]])
        assert aggs == [d[3]] and vst == [0]

    def tagg(d):
        assert impl.batch_threshold_aggregate([d[0]]) == [d[3]]

    def fav(f):
        assert impl.batch_verify_aggregate_status([f]) == [0]

    def chain():
        verify(d710)
        sigagg(d710)
        verify(d710b)
        sigagg(d710b)

    # the keyed shapes: table = each duty's pubshares (for the warm-up RLC call) and root key
    duties = (d46, d710, d710b)
    table, root_idx, share_idx = [], [], []
    for d, (sh, _) in zip(duties, shares):
        share_idx.append({i: len(table) + k for k, i in enumerate(sorted(sh))})
        table.extend(sh[i] for i in sorted(sh))
        root_idx.append(len(table))
        table.append(d[1])
    fav_idx = {}
    for size, f in favs.items():
        fav_idx[size] = list(range(len(table), len(table) + len(f[0])))
        table.extend(f[0])
    assert set(impl.load_pubshares(table)) == {0}

    def fav_keys(size):
        f = favs[size]
        assert impl.batch_verify_aggregate_keys_status([(fav_idx[size], f[1], f[2])]) == [0]

    def fav_warm(size):  # the root hashed ahead of the call, which only reads the cache
        cache(65536)
        assert impl.hcache_prefetch([favs[size][2]]) == (1, 0)

    def warm(k):  # parsigex's keyed RLC BatchVerify over the duty's partials: caches H(root)
        d = duties[k]
        ids = list(d[0])
        st = impl.batch_verify_rlc_keys_status([share_idx[k][i] for i in ids], [d[2]] * len(ids), [d[0][i] for i in ids])
        assert st == [0] * len(ids)

    def sigagg_keys(k):
        d = duties[k]
        aggs, vst = impl.batch_threshold_aggregate_verify_keys([d[0]], [root_idx[k]], [d[2]], [0])
        assert aggs == [d[3]] and vst == [0]

    def cache(capacity, ks=()):
        impl.hcache_config(capacity)
        for k in ks:
            warm(k)

    def chain_keys():
        verify(d710)
        sigagg_keys(1)
        verify(d710b)
        sigagg_keys(2)

    def verify_keys(k):  # the same check as verify(duties[k]), the key by its table index
        d = duties[k]
        assert impl.batch_verify_keys_status([root_idx[k]], [d[2]], [d[3]]) == [0]

    def verify_queued(k):
        d = duties[k]
        assert impl.verify_queued(d[1], d[2], d[3]) == 0

    def chain_keys_all():
        verify_keys(1)
        sigagg_keys(1)
        verify_keys(2)
        sigagg_keys(2)

    # N items over N / 4 roots: partial signatures of duty 0's four shares (their pubshares are table entries)
    ids0 = sorted(d46[0])
    sk_rng = random.Random(0x51E)
    big = {}
    for n in SIZES:
        roots = [sk_rng.randbytes(32) for _ in range(max(1, n // 4))]
        msgs = [roots[i // 4 % len(roots)] for i in range(n)]
        big[n] = ([share_idx[0][ids0[i % 4]] for i in range(n)], msgs,
                  impl.sign_batch([share_secrets[i % 4] for i in range(n)], msgs)[0])

    def verify_keys_n(n):
        kidx, msgs, sigs = big[n]
        assert impl.batch_verify_keys_status(kidx, msgs, sigs) == [0] * n

    # prefetch: N fresh 32-byte roots per call, straight through the C call (no per-root Python work in the clock)
    pf_offs = {n: (ctypes.c_uint64 * (n + 1))(*range(0, 32 * n + 1, 32)) for n in set(PREFETCH_SIZES + BESIDE_SIZES)}

    def prefetch_n(n, want_hashed=True):
        h, p = ctypes.c_uint64(), ctypes.c_uint64()
        rc = impl.lib.hipbls_hcache_prefetch(os.urandom(32 * n), pf_offs[n], n, ctypes.byref(h), ctypes.byref(p))
        assert rc == 0 and (not want_hashed or (h.value, p.value) == (n, 0)), (rc, h.value, p.value)

    def prefetched(ks):  # an empty cache, then the duties' roots hashed ahead of their first Verify
        cache(65536)
        assert impl.hcache_prefetch([duties[k][2] for k in ks]) == (len(ks), 0)

    # the collision rows: a thread that prefetches fresh roots back to back while the shape's calls are clocked
    beside = {"stop": None, "thread": None, "ms": []}

    def beside_start(n, capacity, pause_s=0.0):
        cache(capacity)
        verify_keys(1)  # the clocked root is warm
        beside["stop"] = threading.Event()
        beside["ms"] = []

        def loop():
            while not beside["stop"].is_set():
                t0 = time.perf_counter()
                prefetch_n(n)
                beside["ms"].append((time.perf_counter() - t0) * 1e3)
                if pause_s:
                    time.sleep(pause_s)

        beside["thread"] = threading.Thread(target=loop)
        beside["thread"].start()

    def beside_stop():
        beside["stop"].set()
        beside["thread"].join()
        return _stats(beside["ms"]) if beside["ms"] else {"calls": 0}

    shapes = [("verify_1", lambda: verify(d710)), ("fav_1x4", lambda: fav(fav4)), ("fav_1x12", lambda: fav(fav12)),
              ("sigagg_4of6", lambda: sigagg(d46)), ("sigagg_7of10", lambda: sigagg(d710)),
              ("tagg_7of10", lambda: tagg(d710)), ("chain_verify_sigagg_x2", chain),
              ("sigagg_keys_4of6", lambda: sigagg_keys(0)), ("sigagg_keys_7of10", lambda: sigagg_keys(1)),
              ("sigagg_keys_7of10_nocache", lambda: sigagg_keys(1)), ("chain_verify_sigagg_keys_x2", chain_keys),
              ("verify_keys_1_cold", lambda: verify_keys(1)), ("verify_keys_1_warm", lambda: verify_keys(1)),
              ("verify_keys_1_nocache", lambda: verify_keys(1)),
              ("queued_verify_keyed_cold", lambda: verify_queued(1)),
              ("queued_verify_keyed_warm", lambda: verify_queued(1)),
              ("chain_verify_keys_sigagg_keys_x2", chain_keys_all)]
    for size in favs:
        tag = "1x%d" % size if isinstance(size, int) else size
        if size not in (4, 12):
            shapes.append(("fav_" + tag, lambda size=size: fav(favs[size])))
        shapes.append(("fav_keys_%s_warm" % tag if isinstance(size, int) else "fav_keys_" + tag,
                       lambda size=size: fav_keys(size)))
        if isinstance(size, int):
            shapes.append(("fav_keys_%s_nocache" % tag, lambda size=size: fav_keys(size)))
    for n in SIZES:
        shapes.append(("verify_keys_n%d" % n, lambda n=n: verify_keys_n(n)))
        shapes.append(("verify_keys_n%d_warm" % n, lambda n=n: verify_keys_n(n)))
    for n in PREFETCH_SIZES:
        shapes.append(("prefetch_%d" % n, lambda n=n: prefetch_n(n)))
    shapes += [("verify_keys_1_prefetched", lambda: verify_keys(1)),
               ("queued_verify_keyed_prefetched", lambda: verify_queued(1)),
               ("chain_verify_keys_sigagg_keys_x2_prefetched", chain_keys_all)]
    for n in BESIDE_SIZES:
        shapes.append(("verify_keys_1_warm_beside_prefetch_%d" % n, lambda: verify_keys(1)))
        shapes.append(("verify_keys_1_warm_beside_paced_prefetch_%d" % n, lambda: verify_keys(1)))
    if a.shapes:
        shapes = [s for s in shapes if s[0].startswith(tuple(a.shapes.split(",")))]
    # the cache state each shape runs in (set before its warm-up and again before its clocked and timed passes)
    setup = {"sigagg_keys_4of6": lambda: cache(65536, (0,)), "sigagg_keys_7of10": lambda: cache(65536, (1,)),
             "sigagg_keys_7of10_nocache": lambda: cache(0), "chain_verify_sigagg_keys_x2": lambda: cache(65536, (1, 2)),
             "verify_keys_1_warm": lambda: cache(65536), "verify_keys_1_nocache": lambda: cache(0),
             "queued_verify_keyed_warm": lambda: cache(65536)}
    for size in favs:
        if isinstance(size, int):
            setup["fav_keys_1x%d_warm" % size] = lambda size=size: fav_warm(size)
            setup["fav_keys_1x%d_nocache" % size] = lambda: cache(0)
        else:
            setup["fav_keys_" + size] = lambda size=size: fav_warm(size)
    for n in SIZES:
        setup["verify_keys_n%d" % n] = lambda: cache(0)
        setup["verify_keys_n%d_warm" % n] = lambda: cache(65536)
    # run before every call of the shape, outside the clock: an empty cache, so every root is seen for the first time
    before = {"verify_keys_1_cold": lambda: cache(65536), "queued_verify_keyed_cold": lambda: cache(65536),
              "chain_verify_keys_sigagg_keys_x2": lambda: cache(65536)}
    for n in PREFETCH_SIZES:
        before["prefetch_%d" % n] = lambda: cache(65536)
    before["verify_keys_1_prefetched"] = before["queued_verify_keyed_prefetched"] = lambda: prefetched((1,))
    before["chain_verify_keys_sigagg_keys_x2_prefetched"] = lambda: prefetched((1, 2))
    # the other thread's roots must not push the clocked root out of the ring within a pass: 4,096 per call need room
    after = {}
    for n in BESIDE_SIZES:
        setup["verify_keys_1_warm_beside_prefetch_%d" % n] = lambda n=n: beside_start(n, 65536 if n == 1 else 1 << 22)
        after["verify_keys_1_warm_beside_prefetch_%d" % n] = beside_stop
        setup["verify_keys_1_warm_beside_paced_prefetch_%d" % n] = \
            lambda n=n: beside_start(n, 65536 if n == 1 else 1 << 22, PACED_PAUSE_S)
        after["verify_keys_1_warm_beside_paced_prefetch_%d" % n] = beside_stop
    for name, fn in shapes:
        setup.get(name, lambda: None)()
        for _ in range(a.warmup):
            before.get(name, lambda: None)()
            fn()
        after.get(name, lambda: None)()
    out = {"lib": os.environ.get("HIPBLS_LIB") or "in-tree", "build_id": tbls.build_id().get("src", "")[:16],
           "calls": a.calls, "warmup": a.warmup, "shapes": {}, "kernels_ms": {}}
    for name, fn in shapes:
        setup.get(name, lambda: None)()
        ms = []
        wall0 = time.perf_counter()
        for _ in range(a.calls):
            before.get(name, lambda: None)()
            t0 = time.perf_counter()
            fn()
            ms.append((time.perf_counter() - t0) * 1e3)
        wall = (time.perf_counter() - wall0) * 1e3
        out["shapes"][name] = _stats(ms)
        if name in after:
            out["shapes"][name]["max_ms"] = round(max(ms), 4)
            out["shapes"][name]["prefetch_beside"] = after[name]()
            out["shapes"][name]["pass_wall_ms"] = round(wall, 1)
            h, m, _ = impl.hcache_stats()
            out["shapes"][name]["verify_hits_misses"] = [h, m]
    # per-kernel averages, in a pass of their own: the event pairs around each launch are not in the clocked calls
    impl.lib.hipbls_kernel_timing_reset()
    impl.lib.hipbls_set_timing(1)
    try:
        for name, fn in shapes:
            if name.startswith("chain_") or name in after:
                continue
            setup.get(name, lambda: None)()
            impl.lib.hipbls_kernel_timing_reset()
            for _ in range(a.timing_calls):
                before.get(name, lambda: None)()
                fn()
            per = {}
            for st in STAGES:
                avg, cnt = ctypes.c_double(), ctypes.c_uint64()
                impl.lib.hipbls_kernel_timing(st.encode(), ctypes.byref(avg), ctypes.byref(cnt))
                if cnt.value:
                    per[st] = round(avg.value, 4)
            out["kernels_ms"][name] = per
    finally:
        impl.lib.hipbls_set_timing(0)
        impl.hcache_config(0)
    # the lock shape with the split key sum off: HIPBLS_FAV_SUM_SPLIT is read at init, so another process
    nosplit = "fav_keys_%s_nosplit" % lock_name
    if lock_name in favs and selected(nosplit) and os.environ.get("HIPBLS_FAV_SUM_SPLIT") is None:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--calls", str(a.calls), "--warmup", str(a.warmup),
                            "--timing-calls", str(a.timing_calls), "--lock-keys", str(a.lock_keys), "--shapes",
                            "fav_keys_" + lock_name], env=dict(os.environ, HIPBLS_FAV_SUM_SPLIT="0"),
                           capture_output=True, text=True, check=True)
        child = json.loads(r.stdout.strip().splitlines()[-1])
        out["shapes"][nosplit] = child["shapes"]["fav_keys_" + lock_name]
        out["kernels_ms"][nosplit] = child["kernels_ms"]["fav_keys_" + lock_name]
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
