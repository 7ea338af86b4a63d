"""Timing of the batched PublicKeyShare / PublicKeyRecover calls; the sibling of deal_timing.py.

    python3 charon_amd/tools/vss_timing.py [--out profiles/r20/vss_timing.json]

Shape: 1,024 validators, 7-of-10, 9 dealers.  Host buffers, wall clock around calls that return after their stream has
drained, `warmup` + `rounds` rounds, medians with min and max.  Rows:

  share_batched        ONE hipbls_public_key_share_batch call: 64,512 commitments, ids 0..10.
  share_per_validator  the same work as 1,024 one-validator calls.  The two alternate in one process and their bytes are
                       compared every round.
  recover_batched      ONE hipbls_public_key_recover_batch call of 1,024 x 4 groups of seven pubshares: verify_pubshares
                       for every validator (ids 1..7 for the key, shifted by 8, 9, 10 for the other three pubshares).
  host_port            the same two batched calls on the host build of vss.h (tests/native/vss_host.cpp --time) on 16
                       threads: kind "port" -- the device code compiled for the CPU, not a tuned CPU library.

Then, in rounds of their own with the library's per-launch events on, the mean time of each kernel of the two batched
calls.  No number is fixed in advance: the ratio of the first two rows and the decode's share are findings.
"""
import argparse
import ctypes
import hashlib
import json
import os
import random
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

R_ORDER = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
N_VAL, N_DEALERS, THRESHOLD, TOTAL = 1024, 9, 7, 10
IDS = list(range(TOTAL + 1))
HOST_THREADS = 16


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "calls_ms": [round(x, 3) for x in ms]}


def host_port(rounds):
    """Build the host program and run its timing mode: (share stats, recover stats)."""
    src = os.path.join(ROOT, "tests", "native", "vss_host.cpp")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "vss_host")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-o", exe, src])
        out = subprocess.run([exe, "--time", str(HOST_THREADS), str(rounds)], capture_output=True, text=True,
                             check=True).stdout
    rows = re.findall(r"round \d+ share_ms ([0-9.]+) recover_ms ([0-9.]+) verified (\d+)", out)
    assert len(rows) == rounds and all(int(r[2]) == N_VAL for r in rows), out
    return [float(r[0]) for r in rows], [float(r[1]) for r in rows]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20", "vss_timing.json"))
    args = ap.parse_args()
    import torch
    from charon_amd import build as hb
    from charon_amd.tbls import HipBLS
    src = hb.verify()
    impl = HipBLS(device=0)
    lib = impl.lib
    rng = random.Random(1024)
    per = N_DEALERS * THRESHOLD
    keys, st = impl.secret_to_public_key_batch([rng.randrange(1, R_ORDER).to_bytes(32, "big")
                                                for _ in range(N_VAL * per)])
    assert not any(st)
    com = b"".join(keys)
    m = len(IDS)
    ids = (ctypes.c_int64 * m)(*IDS)

    def share_batched():
        out = ctypes.create_string_buffer(48 * N_VAL * m)
        sst = (ctypes.c_int32 * N_VAL)()
        assert lib.hipbls_public_key_share_batch(com, N_VAL, N_DEALERS, THRESHOLD, ids, m, out, sst) == 0
        assert not any(sst)
        return out.raw

    def share_per_validator():
        out = ctypes.create_string_buffer(48 * m)
        sst = (ctypes.c_int32 * 1)()
        rows = []
        for v in range(N_VAL):
            one = com[48 * per * v:48 * per * (v + 1)]
            assert lib.hipbls_public_key_share_batch(one, 1, N_DEALERS, THRESHOLD, ids, m, out, sst) == 0 and sst[0] == 0
            rows.append(out.raw)
        return b"".join(rows)

    pubs = share_batched()

    def pub(v, k):
        return pubs[48 * (m * v + k):48 * (m * v + k) + 48]

    base = list(range(1, THRESHOLD + 1))
    others = list(range(THRESHOLD + 1, TOTAL + 1))
    n_groups = N_VAL * (1 + len(others))
    g_shares = b"".join(b"".join(pub(v, k) for k in base) * (1 + len(others)) for v in range(N_VAL))
    g_ids = (ctypes.c_int64 * (n_groups * THRESHOLD))(*([k - q for q in [0] + others for k in base] * N_VAL))
    g_offs = (ctypes.c_uint64 * (n_groups + 1))(*range(0, THRESHOLD * (n_groups + 1), THRESHOLD))
    g_want = b"".join(pub(v, q) for v in range(N_VAL) for q in [0] + others)

    def recover_batched():
        out = ctypes.create_string_buffer(48 * n_groups)
        rst = (ctypes.c_int32 * n_groups)()
        assert lib.hipbls_public_key_recover_batch(g_shares, g_ids, g_offs, n_groups, out, rst) == 0
        assert not any(rst)
        return out.raw

    assert recover_batched() == g_want  # every pubshare lies on its validator's polynomial
    ways = {"share_batched": (share_batched, pubs), "share_per_validator": (share_per_validator, pubs),
            "recover_batched": (recover_batched, g_want)}
    times = {k: [] for k in ways}
    for it in range(args.warmup + args.rounds):
        for k, (fn, want) in ways.items():
            t0 = time.perf_counter()
            got = fn()
            dt = (time.perf_counter() - t0) * 1e3
            assert got == want, k
            if it >= args.warmup:
                times[k].append(dt)
            print(json.dumps({"round": it, "way": k, "ms": round(dt, 3)}), flush=True)
    # the kernels, by the library's own events, in rounds of their own
    lib.hipbls_set_timing(1)
    lib.hipbls_kernel_timing_reset()
    for _ in range(args.rounds):
        share_batched()
        recover_batched()
    kernels = {}
    for name in ("g1_decode", "vss_dealer_sum", "vss_eval", "vss_scale", "vss_sum"):
        avg, launches = ctypes.c_double(), ctypes.c_uint64()
        assert lib.hipbls_kernel_timing(name.encode(), ctypes.byref(avg), ctypes.byref(launches)) == 0
        kernels[name] = {"mean_ms": round(avg.value, 4), "launches": launches.value}
    lib.hipbls_set_timing(0)
    host_share, host_recover = host_port(args.warmup + args.rounds)
    rows = {k: dict(stats(v), kind="product") for k, v in times.items()}
    rows["host_port_share"] = dict(stats(host_share[args.warmup:]), kind="port", threads=HOST_THREADS)
    rows["host_port_recover"] = dict(stats(host_recover[args.warmup:]), kind="port", threads=HOST_THREADS)
    share_k = kernels["g1_decode"]["mean_ms"] + kernels["vss_dealer_sum"]["mean_ms"] + kernels["vss_eval"]["mean_ms"]
    result = {"tool": "vss_timing", "build": src[:16], "device": torch.cuda.get_device_name(0),
              "shape": {"validators": N_VAL, "dealers": N_DEALERS, "threshold": THRESHOLD, "total": TOTAL,
                        "ids": IDS, "recover_groups": n_groups},
              "rounds": args.rounds, "warmup": args.warmup, "rows": rows, "kernels": kernels,
              "per_validator_over_batched": round(rows["share_per_validator"]["median_ms"] /
                                                  rows["share_batched"]["median_ms"], 3),
              "decode_share_of_share_kernels": round(kernels["g1_decode"]["mean_ms"] / share_k, 4),
              "outputs_sha256": hashlib.sha256(pubs + g_want).hexdigest()}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in result.items() if k != "rows"}), flush=True)
    print(json.dumps({k: {x: v[x] for x in ("median_ms", "min_ms", "max_ms", "kind")} for k, v in rows.items()}),
          flush=True)


if __name__ == "__main__":
    main()
