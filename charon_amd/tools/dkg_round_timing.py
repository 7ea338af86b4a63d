"""Timing of the three calls of a joint-Feldman dealing round; the sibling of vss_timing.py.

    python3 charon_amd/tools/dkg_round_timing.py [--out profiles/r22/dkg_round_timing.json]

Shape: 1,024 validators, 7-of-10, 9 dealers.  Host buffers, wall clock around calls that return after their stream has
drained, `warmup` + `rounds` rounds, medians with min and max.  Each new call is timed against the way the same work
was done before it existed, in the same process, the ways alternating, their bytes (or verdicts) compared every round:

  deal_commit            ONE hipbls_deal_commit_batch_ct call: 10,240 shares and 7,168 commitments.
  deal_then_keys         hipbls_threshold_split_batch_ct without public keys, then hipbls_secret_to_public_key_batch_ct
                         on the 7,168 coefficients (256 doublings each).
  check_batched          ONE hipbls_verify_secret_shares_batch_ct call: 9,216 shares against 64,512 commitments at id 3.
  check_two_calls        the same 9,216 checks as hipbls_secret_to_public_key_batch_ct + hipbls_public_key_share_batch
                         (each (v, d) a one-dealer validator) and a host compare: verify_secret_shares' composition,
                         batched over the whole ceremony by hand.
  check_per_validator    HipBLS.verify_secret_shares once per validator (1,024 x those two calls, 9 dealers each).
  combine                ONE hipbls_combine_shares_batch_ct call with pubshares.
  host_sum_then_keys     the sums with Python integers, then hipbls_secret_to_public_key_batch_ct on the 1,024 sums.

Then, in rounds of their own with the library's per-launch events on, the mean time of each kernel of the three new
calls and of k_sk_to_pk_ct.  No number is fixed in advance: the ratios are findings.
"""
import argparse
import ctypes
import hashlib
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

R_ORDER = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
N_VAL, N_DEALERS, THRESHOLD, TOTAL, MY_ID = 1024, 9, 7, 10, 3


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "calls_ms": [round(x, 3) for x in ms]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22", "dkg_round_timing.json"))
    args = ap.parse_args()
    import torch
    from charon_amd import build as hb
    from charon_amd.tbls import HipBLS
    src = hb.verify()
    impl = HipBLS(device=0)
    lib = impl.lib
    rng = random.Random(1024)

    def scalars(n):
        return [rng.randrange(1, R_ORDER).to_bytes(32, "big") for _ in range(n)]

    # ---- round 1 of one dealer: 1,024 polynomials
    secrets, tails = scalars(N_VAL), [scalars(THRESHOLD - 1) for _ in range(N_VAL)]
    sec_b, tail_b = b"".join(secrets), b"".join(b"".join(t) for t in tails)
    coef_b = b"".join(secrets[v] + b"".join(tails[v]) for v in range(N_VAL))  # coefficient order: v, then j
    n_sh, n_com = N_VAL * TOTAL, N_VAL * THRESHOLD

    def deal_commit():
        out, com = ctypes.create_string_buffer(32 * n_sh), ctypes.create_string_buffer(48 * n_com)
        st, cst = (ctypes.c_int32 * N_VAL)(), (ctypes.c_int32 * n_com)()
        assert lib.hipbls_deal_commit_batch_ct(sec_b, tail_b, N_VAL, TOTAL, THRESHOLD, out, st, com, cst) == 0
        assert not any(st) and not any(cst)
        return out.raw + com.raw

    def deal_then_keys():
        out, com = ctypes.create_string_buffer(32 * n_sh), ctypes.create_string_buffer(48 * n_com)
        st, cst = (ctypes.c_int32 * N_VAL)(), (ctypes.c_int32 * n_com)()
        assert lib.hipbls_threshold_split_batch_ct(sec_b, tail_b, N_VAL, TOTAL, THRESHOLD, out, st, None, None) == 0
        assert lib.hipbls_secret_to_public_key_batch_ct(coef_b, n_com, com, cst) == 0
        assert not any(st) and not any(cst)
        return out.raw + com.raw

    dealt = deal_commit()

    # ---- round 2 of one receiver: 9 dealers' shares at MY_ID, 9 commitment lists, per validator
    n_chk = N_VAL * N_DEALERS
    polys = [[[rng.randrange(1, R_ORDER) for _ in range(THRESHOLD)] for _ in range(N_DEALERS)] for _ in range(N_VAL)]
    flat_coef = b"".join(c.to_bytes(32, "big") for val in polys for p in val for c in p)
    com_all = ctypes.create_string_buffer(48 * n_chk * THRESHOLD)
    cst = (ctypes.c_int32 * (n_chk * THRESHOLD))()
    assert lib.hipbls_secret_to_public_key_batch(flat_coef, n_chk * THRESHOLD, com_all, cst) == 0 and not any(cst)
    com_b = com_all.raw
    share_int = [[sum(c * pow(MY_ID, j, R_ORDER) for j, c in enumerate(p)) % R_ORDER for p in val] for val in polys]
    forged = {(5, 2), (N_VAL // 2, 0), (N_VAL - 1, N_DEALERS - 1)}
    for v, d in forged:
        share_int[v][d] = (share_int[v][d] + 1) % R_ORDER
    shares = [[x.to_bytes(32, "big") for x in row] for row in share_int]
    share_b = b"".join(s for row in shares for s in row)
    verdict_want = bytes(0 if (v, d) not in forged else 3 for v in range(N_VAL) for d in range(N_DEALERS))
    my_id = (ctypes.c_int64 * 1)(MY_ID)

    def check_batched():
        st = (ctypes.c_int32 * n_chk)()
        assert lib.hipbls_verify_secret_shares_batch_ct(share_b, com_b, N_VAL, N_DEALERS, THRESHOLD, MY_ID, st) == 0
        return bytes(list(st))

    def check_two_calls():
        got, want = ctypes.create_string_buffer(48 * n_chk), ctypes.create_string_buffer(48 * n_chk)
        st, wst = (ctypes.c_int32 * n_chk)(), (ctypes.c_int32 * n_chk)()
        assert lib.hipbls_secret_to_public_key_batch_ct(share_b, n_chk, got, st) == 0
        assert lib.hipbls_public_key_share_batch(com_b, n_chk, 1, THRESHOLD, my_id, 1, want, wst) == 0
        g, w = got.raw, want.raw
        return bytes(0 if st[i] == 0 and wst[i] == 0 and g[48 * i:48 * i + 48] == w[48 * i:48 * i + 48] else 3
                     for i in range(n_chk))

    com_lists = [[[com_b[48 * ((v * N_DEALERS + d) * THRESHOLD + j):48 * ((v * N_DEALERS + d) * THRESHOLD + j) + 48]
                   for j in range(THRESHOLD)] for d in range(N_DEALERS)] for v in range(N_VAL)]

    def check_per_validator():
        out = bytearray()
        for v in range(N_VAL):
            out += bytes(0 if ok else 3 for ok in impl.verify_secret_shares(shares[v], com_lists[v], MY_ID))
        return bytes(out)

    # ---- the last step: the qualified dealers' shares summed
    include = [[(v, d) not in forged for d in range(N_DEALERS)] for v in range(N_VAL)]
    inc_b = bytes(1 if f else 0 for row in include for f in row)

    def combine():
        out, pubs = ctypes.create_string_buffer(32 * N_VAL), ctypes.create_string_buffer(48 * N_VAL)
        st, pst = (ctypes.c_int32 * N_VAL)(), (ctypes.c_int32 * N_VAL)()
        assert lib.hipbls_combine_shares_batch_ct(share_b, inc_b, N_VAL, N_DEALERS, out, st, pubs, pst) == 0
        assert not any(st) and not any(pst)
        return out.raw + pubs.raw

    def host_sum_then_keys():
        sums = b"".join((sum(int.from_bytes(s, "big") for s, f in zip(shares[v], include[v]) if f) % R_ORDER)
                        .to_bytes(32, "big") for v in range(N_VAL))
        pubs, pst = ctypes.create_string_buffer(48 * N_VAL), (ctypes.c_int32 * N_VAL)()
        assert lib.hipbls_secret_to_public_key_batch_ct(sums, N_VAL, pubs, pst) == 0 and not any(pst)
        return sums + pubs.raw

    combined = combine()
    ways = {"deal_commit": (deal_commit, dealt), "deal_then_keys": (deal_then_keys, dealt),
            "check_batched": (check_batched, verdict_want), "check_two_calls": (check_two_calls, verdict_want),
            "check_per_validator": (check_per_validator, verdict_want),
            "combine": (combine, combined), "host_sum_then_keys": (host_sum_then_keys, combined)}
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
        deal_commit()
        check_batched()
        combine()
        host_sum_then_keys()
    kernels = {}
    for name in ("deal_ct", "commit_ct", "g1_decode", "vss_eval", "share_check_ct", "share_sum_ct", "sk_to_pk_ct"):
        avg, launches = ctypes.c_double(), ctypes.c_uint64()
        assert lib.hipbls_kernel_timing(name.encode(), ctypes.byref(avg), ctypes.byref(launches)) == 0
        kernels[name] = {"mean_ms": round(avg.value, 4), "launches": launches.value}
    lib.hipbls_set_timing(0)
    rows = {k: stats(v) for k, v in times.items()}

    def ratio(a, b):
        return round(rows[a]["median_ms"] / rows[b]["median_ms"], 3)

    result = {"tool": "dkg_round_timing", "build": src[:16], "device": torch.cuda.get_device_name(0),
              "shape": {"validators": N_VAL, "dealers": N_DEALERS, "threshold": THRESHOLD, "total": TOTAL,
                        "my_id": MY_ID, "forged": len(forged)},
              "rounds": args.rounds, "warmup": args.warmup, "rows": rows, "kernels": kernels,
              "note_sk_to_pk_ct": "the 1,024-key launches of host_sum_then_keys",
              "deal_then_keys_over_deal_commit": ratio("deal_then_keys", "deal_commit"),
              "check_two_calls_over_check_batched": ratio("check_two_calls", "check_batched"),
              "check_per_validator_over_check_batched": ratio("check_per_validator", "check_batched"),
              "host_sum_then_keys_over_combine": ratio("host_sum_then_keys", "combine"),
              "outputs_sha256": hashlib.sha256(dealt + verdict_want + combined).hexdigest()}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in result.items() if k != "rows"}), flush=True)
    print(json.dumps({k: {x: v[x] for x in ("median_ms", "min_ms", "max_ms")} for k, v in rows.items()}), flush=True)


if __name__ == "__main__":
    main()
