"""Single wire-format Verify calls against the root cache: the cold call and mixed calls.

    [HIPBLS_ROOTCACHE_PARTITION=0] python3 charon_amd/tools/rootcache_calls.py [--n 65536,131072]
        [--warm 0,50,90,100] [--repeats 3] [--slots 1048576] [--lines on,off,hwarm]

Every row is one hipbls_verify_batch_device call of n valid items over n distinct 32-byte roots between two HIP events
on the call's stream.  Before each clocked call the root cache is emptied (hipbls_rootcache_config, outside the clock)
and one unclocked call over the roots that are to be warm fills it; warm roots are spread evenly over the batch
(i * pct // 100 steps), so that in the items' own order every wave mixes hits and misses.  warm = 0 is the cold call;
the "off" row is the same call with the cache off.  The key cache is warm throughout.  HIPBLS_ROOTCACHE_PARTITION is
read at init, so partition on and off are two processes.  --lines names the line-block states to run, each a row of
its own: "on" (the default pool, half the slots: warm roots replay, new ones record), "off" (no pool) and "hwarm" (a
pool of one block, so that the warm roots have H(m) cached and no lines: the state a full pool leaves).  Prints one
JSON object per row, then a summary object.
"""
import argparse
import ctypes
import json
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

R_ORDER = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="65536,131072")
    ap.add_argument("--warm", default="0,50,90,100")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--slots", type=int, default=1 << 20)
    ap.add_argument("--keys", type=int, default=4096)
    ap.add_argument("--lines", default="on,off,hwarm")
    args = ap.parse_args()
    import torch
    from charon_amd import build as hb
    from charon_amd.tbls import PAIR_SINGLE, HipBLS
    hb.verify()
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    impl = HipBLS(device=0)
    impl.set_pair_mode(PAIR_SINGLE)
    lib = impl.lib
    stream = torch.cuda.Stream(dev)
    sp = ctypes.c_void_p(stream.cuda_stream)
    partition = os.environ.get("HIPBLS_ROOTCACHE_PARTITION", "1") != "0"

    sizes = [int(x) for x in args.n.split(",")]
    n_max = max(sizes)
    rng = random.Random(14)
    sks = [rng.randrange(1, R_ORDER).to_bytes(32, "big") for _ in range(args.keys)]
    keys, st = impl.secret_to_public_key_batch(sks)
    assert set(st) == {0}
    owner = [i % args.keys for i in range(n_max)]
    roots = [rng.randbytes(32) for _ in range(n_max)]
    sigs, st = impl.sign_batch([sks[o] for o in owner], roots)
    assert set(st) == {0}

    def u8(blobs):
        return torch.frombuffer(bytearray(b"".join(blobs)), dtype=torch.uint8).to(dev)

    def call(idx, clocked):
        """One device call over the items idx; returns (ms or None)."""
        n = len(idx)
        d_pk, d_sig, d_msg = u8([keys[owner[i]] for i in idx]), u8([sigs[i] for i in idx]), u8([roots[i] for i in idx])
        d_off = torch.arange(0, 32 * (n + 1), 32, dtype=torch.int64).to(dev)
        d_st = torch.full((n,), -7, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record(stream)
            rc = lib.hipbls_verify_batch_device(d_pk.data_ptr(), d_msg.data_ptr(), d_off.data_ptr(), d_sig.data_ptr(), n,
                                                d_st.data_ptr(), sp)
            e1.record(stream)
        assert rc == 0, rc
        torch.cuda.synchronize(dev)
        assert int((d_st != 0).sum().item()) == 0, "a valid item failed"
        return e0.elapsed_time(e1) if clocked else None

    def kernel_ms(name):
        avg, launches = ctypes.c_double(), ctypes.c_uint64()
        lib.hipbls_kernel_timing(name, ctypes.byref(avg), ctypes.byref(launches))
        return avg.value

    lib.hipbls_set_timing(1)  # per-kernel HIP events, as bench.py runs
    impl.rootcache_config(0)
    call(list(range(n_max)), False)  # the key cache warm, buffers grown
    rows = []
    for n in sizes:
        everything = list(range(n))
        off = []
        for _ in range(args.repeats):
            impl.rootcache_config(0)
            off.append(call(everything, True))
        rows.append({"n": n, "warm_pct": None, "cache": "off", "ms": [round(x, 3) for x in off]})
        print(json.dumps(rows[-1]), flush=True)
        for pct, lines in [(int(x), m) for x in args.warm.split(",") for m in args.lines.split(",")]:
            warm = [i for i in everything if (i + 1) * pct // 100 != i * pct // 100]
            if lines == "hwarm" and not warm:
                continue  # nothing is warm: the "on" row
            ms, hits, inserts, fused_ms, lookup_ms, line_hits, published = [], [], [], [], [], [], []
            for _ in range(args.repeats):
                impl.rootcache_config(args.slots)
                impl.rootcache_lines_config({"on": None, "off": 0, "hwarm": 1}[lines])
                if warm:
                    call(warm, False)
                s0, l0 = impl.rootcache_stats(), impl.rootcache_lines_stats()
                lib.hipbls_kernel_timing_reset()
                ms.append(call(everything, True))
                s1, l1 = impl.rootcache_stats(), impl.rootcache_lines_stats()
                hits.append(s1[0] - s0[0])
                inserts.append(s1[2] - s0[2])
                line_hits.append(l1[0] - l0[0])
                published.append(l1[1] - l0[1])
                assert l1[3] == 0, l1
                fused_ms.append(round(kernel_ms(b"verify"), 3))
                lookup_ms.append(round(kernel_ms(b"root_lookup"), 3))
            rows.append({"n": n, "warm_pct": pct, "cache": "on", "lines": lines, "partition": partition,
                         "warm_roots": len(warm), "hits": hits, "inserts": inserts, "line_hits": line_hits,
                         "blocks_published": published, "ms": [round(x, 3) for x in ms],
                         "k_verify_fused_ms": fused_ms, "k_root_lookup_ms": lookup_ms})
            print(json.dumps(rows[-1]), flush=True)
    impl.rootcache_lines_config(None)
    print(json.dumps({"tool": "rootcache_calls", "partition": partition, "slots": args.slots, "repeats": args.repeats,
                      "rows": rows}))


if __name__ == "__main__":
    main()
