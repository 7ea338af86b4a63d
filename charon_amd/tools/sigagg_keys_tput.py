"""Throughput of sigagg by resident key index against the wire-format call.

The C3 shape of `bench.py --full` (--groups validators, 7-of-10, one signing root each) through the synchronous host
API, the way charon's sigagg goroutines reach it: one call in flight, and two host threads with a call each (the
library overlaps the second call's phase A with the first call's checks).  Forms:

    unkeyed             hipbls_threshold_aggregate_verify_batch: 48-byte root keys, every group's message hashed
    keyed_warm          ..._keys: keys from the resident table, every root already in the H(m) cache (one keyed RLC
                        BatchVerify over the roots ran first)
    keyed_cache_off     ..._keys with cache capacity 0: the call hashes each distinct root itself
    *_64roots           the same three with 64 roots shared over the groups (an attester duty: one root per committee)

    HIPBLS_LIB=<another build> python3 charon_amd/tools/sigagg_keys_tput.py [--groups 10000] [--calls 3]
    ... --unkeyed-only      the unkeyed forms alone (a library without the keyed entry points)

Prints one JSON object: aggregates/s per form and thread count, and the per-kernel averages of a timed pass.
"""
import argparse
import ctypes
import json
import os
import random
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

STAGES = ("tv_phase_a", "tv_phase_a_keys", "tagg_sum", "tv_check_unscale", "tv_prep_pk", "tagg_scale")


def make(impl, bench, G, n_roots, t=7, n=10):
    """bench.make_c3's validators with validator v signing root v % n_roots."""
    part_sks, part_msgs, part_ids, offs, secrets_, roots = [], [], [], [0], [], []
    for v in range(G):
        secret = bench._scalar("c3", "sk", v)
        poly = [secret] + [bench._scalar("c3", "poly", v, k) - 1 for k in range(t - 1)]
        ids = sorted(random.Random(bench._hi("c3", "ids", v)).sample(range(1, n + 1), t))
        root = bench._hb("c3", "root", v % n_roots)
        secrets_.append(secret.to_bytes(32, "big"))
        roots.append(root)
        for i in ids:
            acc = 0
            for c in reversed(poly):
                acc = (acc * i + c) % bench.R_ORDER
            part_sks.append(acc.to_bytes(32, "big"))
            part_msgs.append(root)
            part_ids.append(i)
        offs.append(len(part_ids))
    psigs, st = impl.sign_batch(part_sks, part_msgs)
    assert set(st) <= {0}
    dv_pks, st = impl.secret_to_public_key_batch(secrets_)
    assert set(st) <= {0}
    want, st = impl.sign_batch(secrets_, roots)
    assert set(st) <= {0}
    return dict(G=G, psig=b"".join(psigs), ids=(ctypes.c_int64 * len(part_ids))(*part_ids),
                offs=(ctypes.c_uint64 * (G + 1))(*offs), dv_pks=dv_pks, roots=roots, want=b"".join(want),
                want_sigs=want)


class Call:
    """One caller's buffers for a form; run() is one synchronous call, checked."""

    def __init__(self, impl, d, keyed):
        self.lib, self.d, self.keyed = impl.lib, d, keyed
        G = d["G"]
        self.out = ctypes.create_string_buffer(96 * G)
        self.ast, self.vst = (ctypes.c_int32 * G)(), (ctypes.c_int32 * G)()
        if keyed:
            distinct = list(dict.fromkeys(d["roots"]))
            pos = {r: j for j, r in enumerate(distinct)}
            self.kidx = (ctypes.c_uint32 * G)(*range(G))
            self.midx = (ctypes.c_uint32 * G)(*[pos[r] for r in d["roots"]])
            self.blob = b"".join(distinct)
            self.n_msgs = len(distinct)
            self.moffs = (ctypes.c_uint64 * (self.n_msgs + 1))(*range(0, 32 * (self.n_msgs + 1), 32))
        else:
            self.pks = b"".join(d["dv_pks"])
            self.blob = b"".join(d["roots"])
            self.moffs = (ctypes.c_uint64 * (G + 1))(*range(0, 32 * (G + 1), 32))

    def run(self):
        d = self.d
        if self.keyed:
            rc = self.lib.hipbls_threshold_aggregate_verify_batch_keys(
                d["psig"], d["ids"], d["offs"], d["G"], self.kidx, self.midx, self.blob, self.moffs, self.n_msgs,
                self.out, self.ast, self.vst)
        else:
            rc = self.lib.hipbls_threshold_aggregate_verify_batch(
                d["psig"], d["ids"], d["offs"], d["G"], self.pks, self.blob, self.moffs, self.out, self.ast, self.vst)
        assert rc == 0, self.lib.hipbls_last_error()

    def check(self):
        assert set(self.ast) == {0} and set(self.vst) == {0}
        assert self.out.raw == self.d["want"]


def rate(calls, n_calls):
    """Aggregates/s of len(calls) host threads doing n_calls calls each."""
    def worker(c):
        for _ in range(n_calls):
            c.run()

    for c in calls:  # warm-up, one call each
        c.run()
    th = [threading.Thread(target=worker, args=(c,)) for c in calls[1:]]
    t0 = time.perf_counter()
    for x in th:
        x.start()
    worker(calls[0])
    for x in th:
        x.join()
    el = time.perf_counter() - t0
    for c in calls:
        c.check()
    return round(len(calls) * n_calls * calls[0].d["G"] / el, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=10000)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--unkeyed-only", action="store_true")
    a = ap.parse_args()
    import bench
    from charon_amd import tbls
    impl = tbls.HipBLS()
    data = {"": make(impl, bench, a.groups, a.groups), "_64roots": make(impl, bench, a.groups, 64)}
    out = {"lib": os.environ.get("HIPBLS_LIB") or "in-tree", "build_id": tbls.build_id().get("src", "")[:16],
           "groups": a.groups, "calls": a.calls, "aggregates_per_s": {}, "kernels_ms": {}, "hcache": {}}

    def stage_pass(name, call):
        impl.lib.hipbls_kernel_timing_reset()
        impl.lib.hipbls_set_timing(1)
        try:
            call.run()
            call.run()
        finally:
            impl.lib.hipbls_set_timing(0)
        per = {}
        for st in STAGES:
            avg, cnt = ctypes.c_double(), ctypes.c_uint64()
            impl.lib.hipbls_kernel_timing(st.encode(), ctypes.byref(avg), ctypes.byref(cnt))
            if cnt.value:
                per[st] = round(avg.value, 4)
        out["kernels_ms"][name] = per

    for suffix, d in data.items():
        forms = [("unkeyed" + suffix, False, None)]
        if not a.unkeyed_only:
            forms += [("keyed_warm" + suffix, True, 65536), ("keyed_cache_off" + suffix, True, 0)]
            assert set(impl.load_pubshares(d["dv_pks"])) == {0}
        for name, keyed, cap in forms:
            if keyed:
                impl.hcache_config(cap)
                if cap:  # what the RLC BatchVerify of the roots' partials leaves behind: every root cached
                    st = impl.batch_verify_rlc_keys_status(list(range(d["G"])), d["roots"], d["want_sigs"])
                    assert set(st) == {0}
            calls = [Call(impl, d, keyed), Call(impl, d, keyed)]
            out["aggregates_per_s"][name] = {"one_call": rate(calls[:1], a.calls), "two_threads": rate(calls, a.calls)}
            stage_pass(name, calls[0])
            if keyed:
                h, m, e = impl.hcache_stats()
                out["hcache"][name] = {"hits": h, "misses": m, "entries": e}
        if not a.unkeyed_only:
            impl.hcache_config(0)
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
