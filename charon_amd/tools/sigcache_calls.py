"""sigagg against the signature cache: the C3 shape, cache off and warm, alone and inside the flow.

    python3 charon_amd/tools/sigcache_calls.py [--groups 10000] [--repeats 3] [--slots 262144]
        [--out profiles/sigcache_<tag>]

The shape is bench.py's C3: `groups` validators of 7-of-10, one 32-byte root each, so 7 x groups partials.  The
partials are first verified as core/parsigex does -- one hipbls_batch_verify_rlc_keys call per peer, each over that
peer's partial of every validator -- and then aggregated and verified as core/sigagg does, wire format
(hipbls_threshold_aggregate_verify_batch) and keyed with the H(m) cache warm (..._batch_keys).  Rows, `repeats` runs
each, cache off and warm alternating:

  sigagg        the sigagg call alone; for the warm rows the Verify calls ran just before, outside the clock
  flow          the seven Verify calls and the sigagg call inside the clock: the producers' cost is in the number

Every call is a host-buffer call on pre-packed arguments between two time.perf_counter readings (the calls return
after their stream has drained).  The off rows launch the kernels the library launched before the cache existed
(tests/test_gpu_sigcache.py test_routing_by_launch_counts; their resources are unchanged, tests/test_sigcache_host.py),
so their run-to-run spread is the yardstick for the warm rows' gain.  Prints one JSON object per row and writes them,
with a summary of means and run-to-run spreads, to <out>/sigcache_calls.json.
"""
import argparse
import ctypes
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

R_ORDER = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
IDS = (1, 2, 4, 5, 7, 9, 10)  # the seven peers whose partials arrive, of ten


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=10000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--slots", type=int, default=262144)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from charon_amd import build as hb
    from charon_amd.tbls import HipBLS
    hb.verify()
    torch.zeros(1, device="cuda")
    impl = HipBLS(device=0)
    lib = impl.lib
    has_cache = True
    G, t = args.groups, len(IDS)
    rng = random.Random(4014)

    # shares by the polynomial on the host, everything else on the device
    secrets_, share_sks, roots = [], [], [rng.randbytes(32) for _ in range(G)]
    for _ in range(G):
        poly = [rng.randrange(1, R_ORDER) for _ in range(t)]
        secrets_.append(poly[0].to_bytes(32, "big"))
        for i in IDS:
            acc = 0
            for c in reversed(poly):
                acc = (acc * i + c) % R_ORDER
            share_sks.append(acc.to_bytes(32, "big"))
    root_pks, st = impl.secret_to_public_key_batch(secrets_)
    assert set(st) == {0}
    pubshares, st = impl.secret_to_public_key_batch(share_sks)
    assert set(st) == {0}
    partials, st = impl.sign_batch(share_sks, [roots[k // t] for k in range(G * t)])
    assert set(st) == {0}
    table = list(root_pks) + list(pubshares)  # root key of validator g at g, pubshare of partial k at G + k
    assert set(impl.load_pubshares(table)) == {0}
    impl.hcache_config(2 * G)

    # pre-packed arguments
    u32, u64, i32, i64 = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int32, ctypes.c_int64
    msg_blob = b"".join(roots)
    msg_offs = (u64 * (G + 1))(*[32 * g for g in range(G + 1)])
    seed = bytes(range(32))
    peers = []
    for j in range(t):  # peer j sends its partial of every validator
        items = [g * t + j for g in range(G)]
        peers.append(((u32 * G)(*[G + k for k in items]), b"".join(partials[k] for k in items),
                      (u32 * G)(*range(G)), (i32 * G)()))
    sig_blob = b"".join(partials)
    ids = (i64 * (G * t))(*[IDS[k % t] for k in range(G * t)])
    goffs = (u64 * (G + 1))(*[t * g for g in range(G + 1)])
    dv_blob = b"".join(root_pks)
    kidx, midx = (u32 * G)(*range(G)), (u32 * G)(*range(G))
    out = ctypes.create_string_buffer(96 * G)
    ast, vst = (i32 * G)(), (i32 * G)()

    def verify_all():
        for kid, sigs, mid, stv in peers:
            rc = lib.hipbls_batch_verify_rlc_keys(kid, sigs, mid, G, msg_blob, msg_offs, G, seed, stv)
            assert rc == 0 and not any(stv), "a valid partial failed"

    def sigagg(keyed):
        if keyed:
            rc = lib.hipbls_threshold_aggregate_verify_batch_keys(sig_blob, ids, goffs, G, kidx, midx, msg_blob,
                                                                  msg_offs, G, out, ast, vst)
        else:
            rc = lib.hipbls_threshold_aggregate_verify_batch(sig_blob, ids, goffs, G, dv_blob, msg_blob, msg_offs, out,
                                                             ast, vst)
        assert rc == 0 and not any(ast) and not any(vst), "a valid group failed"
        return out.raw

    def clock(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    def config(slots):
        if has_cache:
            impl.sigcache_config(slots)

    config(0)
    verify_all()  # buffers grown, the key table and the H(m) cache warm
    want = {k: sigagg(k) for k in (False, True)}
    rows = []
    states = ["off", "warm"] if has_cache else ["off"]
    for keyed in (False, True):
        ms = {(row, s): [] for row in ("sigagg", "flow") for s in states}
        stats = []
        for _ in range(args.repeats):
            for s in states:  # alternating
                config(args.slots if s == "warm" else 0)
                if s == "warm":
                    verify_all()
                ms[("sigagg", s)].append(clock(lambda: sigagg(keyed)))
                assert out.raw == want[keyed]
                if s == "warm":
                    stats.append(impl.sigcache_stats())
                config(args.slots if s == "warm" else 0)
                ms[("flow", s)].append(clock(lambda: (verify_all(), sigagg(keyed))))
                assert out.raw == want[keyed]
        for (row, s), v in ms.items():
            rows.append({"row": row, "keyed": keyed, "cache": s, "groups": G, "partials": G * t,
                         "ms": [round(x, 3) for x in v], "mean_ms": round(sum(v) / len(v), 3),
                         "spread_ms": round(max(v) - min(v), 3),
                         "groups_per_s": round(G / (sum(v) / len(v) / 1e3))})
            print(json.dumps(rows[-1]), flush=True)
        if stats:
            rows.append({"row": "stats", "keyed": keyed, "hits_misses_inserts_rollovers": stats})
            print(json.dumps(rows[-1]), flush=True)
    config(0)
    summary = {"tool": "sigcache_calls", "lib": os.environ.get("HIPBLS_LIB") or "in-tree", "has_cache": has_cache,
               "slots": args.slots, "repeats": args.repeats, "rows": rows}
    print(json.dumps(summary))
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "sigcache_calls.json"), "w") as f:
            json.dump(summary, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
