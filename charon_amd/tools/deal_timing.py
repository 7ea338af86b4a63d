"""Timing of the batched split / recover kernels; the sibling of sign_timing.py.

    python3 charon_amd/tools/deal_timing.py fills      [--out profiles/r16/deal_timing.json]
    python3 charon_amd/tools/deal_timing.py throughput [--old-lib LIB] [--out profiles/r16/deal_throughput.json]

fills: does the run time of deal_ct / recover_ct depend on the secrets?  One process, kernel timing on, the *_device
calls on device buffers, `warmup` + `launches` launches per fill, each kernel by the library's own per-launch events.
deal_ct: 2,048 validators x (7 + 1) lanes = 16,384 lanes, threshold 5; recover_ct: 16,384 groups of three shares at
ids 1, 2, 3.  The fills are sign_timing.py's: every secret value (root secret and tail coefficients, or shares) 1;
every one r - 1; seeded random; alternating 1 and r - 1 (by validator for the deal, whose lanes share a polynomial; by
group for the recovery), and, recorded only, one random polynomial / group in every lane.  The random fill runs three
times (first, middle, last); the criterion is sign_timing.py's: the largest difference between the four fills' means
at most 3 x the spread of those three.  sk_to_pk_ct over 16,384 random secrets is timed in the same run, for the
comparison of the comb with the 4-bit window.  HIPBLS_LIB names another build of the same sources (the comb A/B ran
this command on a build whose g1_pub_ct called sign_ct.h's g1_mul_ct).

throughput: 1,024 validators x 7-of-10 through ONE hipbls_threshold_split_batch_ct call, against the per-validator way
to the same outputs: 1,024 hipbls_threshold_split calls and one hipbls_secret_to_public_key_batch_ct of the 11,264
scalars.  Host buffers, wall clock, alternated in one process, medians.  --old-lib names a library built from the
parent commit (where hipbls_threshold_split is the old one-secret kernel): the process then loads that library alone
and times the per-validator way alone (two copies of the library in one process would share its hardware queues).
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
SPREAD_FACTOR = 3.0
ONE, RM1 = (1).to_bytes(32, "big"), (R_ORDER - 1).to_bytes(32, "big")


def mean(xs):
    return sum(xs) / len(xs)


def unit_fills(n_units, words, seed):
    """{fill: n_units x words 32-byte values}: a unit is a validator's polynomial or a group's shares."""
    rng = random.Random(seed)
    rnd = [[rng.randrange(1, R_ORDER).to_bytes(32, "big") for _ in range(words)] for _ in range(n_units)]
    return {"ones": [[ONE] * words] * n_units, "r_minus_1": [[RM1] * words] * n_units, "random": rnd,
            "alternating": [[ONE if u % 2 == 0 else RM1] * words for u in range(n_units)],
            "same_random": [rnd[0]] * n_units}


def fills_main(args):
    import torch
    from charon_amd import build as hb
    from charon_amd.tbls import HipBLS
    src = hb.verify()
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    impl = HipBLS(device=0)
    lib = impl.lib
    stream = torch.cuda.Stream(dev)
    sp = ctypes.c_void_p(stream.cuda_stream)
    n_val, total, threshold = 2048, 7, 5
    row = total + 1
    lanes = n_val * row
    n_groups, m = lanes, 3

    def dbytes(b):
        return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)

    d_sh = torch.zeros(32 * n_val * total, dtype=torch.uint8, device=dev)
    d_st = torch.full((lanes,), -7, dtype=torch.int32, device=dev)
    d_pub = torch.zeros(48 * lanes, dtype=torch.uint8, device=dev)
    d_pst = torch.full((lanes,), -7, dtype=torch.int32, device=dev)
    d_ids = torch.tensor([1, 2, 3] * n_groups, dtype=torch.int64).to(dev)
    d_off = torch.arange(0, m * (n_groups + 1), m, dtype=torch.int64).to(dev)
    d_sec = torch.zeros(32 * n_groups, dtype=torch.uint8, device=dev)

    def deal(d):
        return lib.hipbls_threshold_split_batch_ct_device(d[0].data_ptr(), d[1].data_ptr(), n_val, total, threshold,
                                                          d_sh.data_ptr(), d_st.data_ptr(), d_pub.data_ptr(),
                                                          d_pst.data_ptr(), sp)

    def recover(d):
        return lib.hipbls_recover_secret_batch_ct_device(d[0].data_ptr(), d_ids.data_ptr(), d_off.data_ptr(), n_groups,
                                                         m * n_groups, d_sec.data_ptr(), d_st.data_ptr(),
                                                         d_pub.data_ptr(), d_pst.data_ptr(), sp)

    def sk_to_pk(d):
        return lib.hipbls_secret_to_public_key_batch_ct_device(d[0].data_ptr(), lanes, d_pub.data_ptr(),
                                                               d_st.data_ptr(), sp)

    def kernel_ms(name):
        avg, launches = ctypes.c_double(), ctypes.c_uint64()
        assert lib.hipbls_kernel_timing(name.encode(), ctypes.byref(avg), ctypes.byref(launches)) == 0
        assert launches.value == 1, (name, launches.value)
        return avg.value

    def run(call, name, d, n_status):
        out = []
        for it in range(args.warmup + args.launches):
            d_st.fill_(-7)
            torch.cuda.synchronize(dev)
            lib.hipbls_kernel_timing_reset()
            with torch.cuda.stream(stream):
                rc = call(d)
            assert rc == 0, rc
            torch.cuda.synchronize(dev)
            assert int((d_st[:n_status] != 0).sum().item()) == 0, "a valid secret was refused"
            if it >= args.warmup:
                out.append(kernel_ms(name))
        return out

    lib.hipbls_set_timing(1)
    deal_data = {}
    for k, v in unit_fills(n_val, threshold, 2048).items():
        deal_data[k] = (dbytes(b"".join(u[0] for u in v)), dbytes(b"".join(b"".join(u[1:]) for u in v)))
    rec_data = {k: (dbytes(b"".join(b"".join(u) for u in v)),) for k, v in unit_fills(n_groups, m, 16384).items()}
    order = ("random", "ones", "r_minus_1", "random", "alternating", "same_random", "random")
    four = ("ones", "r_minus_1", "random", "alternating")
    rows, summary = [], {}
    for path, call, name, data, n_status in (("deal_ct", deal, "deal_ct", deal_data, n_val),
                                             ("recover_ct", recover, "recover_ct", rec_data, n_groups)):
        means, random_means = {}, []
        for fill in order:
            ms = run(call, name, data[fill], n_status)
            mm = mean(ms)
            if fill == "random":
                random_means.append(mm)
                if len(random_means) == 1:
                    means[fill] = mm
            else:
                means[fill] = mm
            rows.append({"path": path, "fill": fill, "run": len(random_means) if fill == "random" else 1,
                         "mean_ms": round(mm, 5), "kernel_ms": [round(x, 4) for x in ms]})
            print(json.dumps(rows[-1]), flush=True)
        spread = max(random_means) - min(random_means)
        diff = max(means[k] for k in four) - min(means[k] for k in four)
        summary[path] = {"fill_mean_ms": {k: round(v, 5) for k, v in means.items()},
                         "random_run_mean_ms": [round(x, 5) for x in random_means], "spread_ms": round(spread, 5),
                         "max_fill_diff_ms": round(diff, 5), "diff_over_spread": round(diff / spread, 3) if spread > 0 else None,
                         "within_3x_spread": bool(diff <= SPREAD_FACTOR * spread)}
    rng = random.Random(7)
    d_sk = (dbytes(b"".join(rng.randrange(1, R_ORDER).to_bytes(32, "big") for _ in range(lanes))),)
    pk_ms = run(sk_to_pk, "sk_to_pk_ct", d_sk, lanes)
    result = {"tool": "deal_timing fills", "build": src[:16], "lib": os.environ.get("HIPBLS_LIB", "product"),
              "device": torch.cuda.get_device_name(0), "lanes": lanes, "deal_shape": [n_val, total, threshold],
              "recover_shape": [n_groups, m], "launches": args.launches, "warmup": args.warmup, "order": order,
              "summary": summary, "sk_to_pk_ct_ms": {"mean": round(mean(pk_ms), 5), "launches": [round(x, 4) for x in pk_ms]},
              "rows": rows}
    write(args.out or os.path.join(ROOT, "profiles", "r16", "deal_timing.json"), result)
    print(json.dumps({k: result[k] for k in ("lib", "summary", "sk_to_pk_ct_ms")}), flush=True)


def write(path, result):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


def throughput_main(args):
    n_val, total, threshold = 1024, 10, 7
    row = total + 1
    rng = random.Random(1024)
    secrets = [rng.randrange(1, R_ORDER).to_bytes(32, "big") for _ in range(n_val)]
    tails = [b"".join(rng.randrange(R_ORDER).to_bytes(32, "big") for _ in range(threshold - 1)) for _ in range(n_val)]
    sec_flat, tail_flat = b"".join(secrets), b"".join(tails)
    u8p, i32p = ctypes.c_char_p, ctypes.POINTER(ctypes.c_int32)
    if args.old_lib:
        lib = ctypes.CDLL(os.path.abspath(args.old_lib))
        lib.hipbls_threshold_split.argtypes = [u8p, u8p, ctypes.c_uint32, ctypes.c_uint32, u8p, i32p]
        lib.hipbls_secret_to_public_key_batch_ct.argtypes = [u8p, ctypes.c_uint64, u8p, i32p]
        assert lib.hipbls_init(0) == 0
        src = "old-lib"
    else:
        from charon_amd import build as hb
        from charon_amd.tbls import HipBLS
        src = hb.verify()
        lib = HipBLS(device=0).lib

    def per_validator():
        """The loop of dkg/keycast.go over the C-ABI: one split call per validator, then every public key at once."""
        out = ctypes.create_string_buffer(32 * total)
        st = (ctypes.c_int32 * 1)()
        shares = []
        for v in range(n_val):
            assert lib.hipbls_threshold_split(secrets[v], tails[v], total, threshold, out, st) == 0 and st[0] == 0
            shares.append(out.raw)
        scalars = b"".join(secrets[v] + shares[v] for v in range(n_val))
        pubs = ctypes.create_string_buffer(48 * n_val * row)
        pst = (ctypes.c_int32 * (n_val * row))()
        assert lib.hipbls_secret_to_public_key_batch_ct(scalars, n_val * row, pubs, pst) == 0
        assert not any(pst)
        return b"".join(shares), pubs.raw

    def batched():
        out = ctypes.create_string_buffer(32 * n_val * total)
        st = (ctypes.c_int32 * n_val)()
        pubs = ctypes.create_string_buffer(48 * n_val * row)
        pst = (ctypes.c_int32 * (n_val * row))()
        assert lib.hipbls_threshold_split_batch_ct(sec_flat, tail_flat, n_val, total, threshold, out, st, pubs, pst) == 0
        assert not any(st) and not any(pst)
        return out.raw, pubs.raw

    ways = {"per_validator": per_validator} if args.old_lib else {"batched": batched, "per_validator": per_validator}
    ref = next(iter(ways.values()))()
    times = {k: [] for k in ways}
    for it in range(args.warmup + args.launches):
        for k, fn in ways.items():
            t0 = time.perf_counter()
            got = fn()
            dt = (time.perf_counter() - t0) * 1e3
            assert got == ref, k  # the same shares and keys either way
            if it >= args.warmup:
                times[k].append(dt)
    res = {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
               "calls_ms": [round(x, 3) for x in v]} for k, v in times.items()}
    result = {"tool": "deal_timing throughput", "build": src[:16], "shape": [n_val, total, threshold],
              "launches": args.launches, "warmup": args.warmup, "ways": res,
              "outputs_sha256": hashlib.sha256(ref[0] + ref[1]).hexdigest()}
    if not args.old_lib:
        result["per_validator_over_batched"] = round(res["per_validator"]["median_ms"] / res["batched"]["median_ms"], 3)
    write(args.out or os.path.join(ROOT, "profiles", "r16", "deal_throughput.json"), result)
    print(json.dumps({k: v for k, v in result.items() if k != "ways"}), flush=True)
    print(json.dumps({k: {x: v[x] for x in ("median_ms", "min_ms", "max_ms")} for k, v in res.items()}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("fills", "throughput"))
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--old-lib", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    {"fills": fills_main, "throughput": throughput_main}[args.mode](args)


if __name__ == "__main__":
    main()
