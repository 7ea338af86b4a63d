"""Does a signing kernel's run time depend on the secrets?  

    python3 charon_amd/tools/sign_timing.py [--n 16384] [--launches 10] [--warmup 2] [--out profiles/r15/sign_timing.json]

One process, kernel timing on.  For the secret-independent kernels (sign_ct_mul, sk_to_pk_ct) and, for contrast, the
existing variable-time paths (sign, sk_to_pk): n items over ONE fixed 32-byte message, `warmup` + `launches` launches of
the *_device call on device buffers, with the secrets filled four ways:

    ones         every sk = 1
    r_minus_1    every sk = r - 1
    random       seeded random secrets
    alternating  sk = 1 and sk = r - 1 lane by lane

and, recorded only, same_random: ONE random secret in every lane.  It separates the two things that can make a fill
slower: lanes that disagree (divergence: absent here, present in `random`) and operands with more bits toggling
(present in both).

The random fill runs three times over (first, in the middle and last, so that drift over the session is part of what
they measure): the spread of those three means is the noise floor of identical work.  For each `_ct` kernel the
largest difference between the four fills' means is to be at most 3 x that spread (three samples understate a
spread).  The variable-time paths' figures are recorded only: they show that the instrument resolves the effect.

Times: the `_ct` kernels' are the library's own per-launch HIP events (hipbls_kernel_timing); every path also has the
whole device call between two events on its stream ("call_ms": for Sign that is hash + multiplication, which is what
the existing k_sign holds in one kernel).  Prints one JSON object per row and writes the whole result to --out.
"""
import argparse
import ctypes
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

R_ORDER = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
SPREAD_FACTOR = 3.0


def fills(n, seed=16384):
    one, rm1 = (1).to_bytes(32, "big"), (R_ORDER - 1).to_bytes(32, "big")
    rng = random.Random(seed)
    rnd = [rng.randrange(1, R_ORDER).to_bytes(32, "big") for _ in range(n)]
    return {"ones": [one] * n, "r_minus_1": [rm1] * n, "random": rnd,
            "alternating": [one if i % 2 == 0 else rm1 for i in range(n)], "same_random": [rnd[0]] * n}


def mean(xs):
    return sum(xs) / len(xs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15", "sign_timing.json"))
    args = ap.parse_args()
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
    n = args.n
    msg = bytes((0xA5 ^ (7 * i)) & 0xFF for i in range(32))
    d_msg = torch.frombuffer(bytearray(msg * n), dtype=torch.uint8).to(dev)
    d_off = torch.arange(0, 32 * (n + 1), 32, dtype=torch.int64).to(dev)
    d_sig = torch.zeros(96 * n, dtype=torch.uint8, device=dev)
    d_pk = torch.zeros(48 * n, dtype=torch.uint8, device=dev)
    d_st = torch.full((n,), -7, dtype=torch.int32, device=dev)

    def kernel_ms(name):
        avg, launches = ctypes.c_double(), ctypes.c_uint64()
        assert lib.hipbls_kernel_timing(name.encode(), ctypes.byref(avg), ctypes.byref(launches)) == 0
        assert launches.value == 1, (name, launches.value)
        return avg.value

    # path -> (the device call, the library's timing names of its kernels)
    paths = {
        "sign_ct": (lambda d_sk: lib.hipbls_sign_batch_ct_device(d_sk.data_ptr(), d_msg.data_ptr(), d_off.data_ptr(), n,
                                                                 d_sig.data_ptr(), d_st.data_ptr(), sp),
                    ("sign_ct_hash", "sign_ct_mul")),
        "sk_to_pk_ct": (lambda d_sk: lib.hipbls_secret_to_public_key_batch_ct_device(d_sk.data_ptr(), n, d_pk.data_ptr(),
                                                                                     d_st.data_ptr(), sp),
                        ("sk_to_pk_ct",)),
        "sign": (lambda d_sk: lib.hipbls_sign_batch_device(d_sk.data_ptr(), d_msg.data_ptr(), d_off.data_ptr(), n,
                                                           d_sig.data_ptr(), d_st.data_ptr(), sp), ()),
        "sk_to_pk": (lambda d_sk: lib.hipbls_secret_to_public_key_batch_device(d_sk.data_ptr(), n, d_pk.data_ptr(),
                                                                               d_st.data_ptr(), sp), ()),
    }
    # the kernel the acceptance criterion reads per `_ct` path
    criterion = {"sign_ct": "sign_ct_mul", "sk_to_pk_ct": "sk_to_pk_ct"}

    def run(path, d_sk):
        call, names = paths[path]
        call_ms, kern = [], {k: [] for k in names}
        for it in range(args.warmup + args.launches):
            d_st.fill_(-7)
            torch.cuda.synchronize(dev)
            lib.hipbls_kernel_timing_reset()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(stream):
                e0.record(stream)
                rc = call(d_sk)
                e1.record(stream)
            assert rc == 0, rc
            torch.cuda.synchronize(dev)
            assert int((d_st != 0).sum().item()) == 0, "a valid secret was refused"
            if it >= args.warmup:
                call_ms.append(e0.elapsed_time(e1))
                for k in names:
                    kern[k].append(kernel_ms(k))
        return call_ms, kern

    lib.hipbls_set_timing(1)
    data = {k: torch.frombuffer(bytearray(b"".join(v)), dtype=torch.uint8).to(dev) for k, v in fills(n).items()}
    order = ("random", "ones", "r_minus_1", "random", "alternating", "same_random", "random")
    four = ("ones", "r_minus_1", "random", "alternating")  # the fills the criterion compares
    rows, summary = [], {}
    for path in paths:
        means, random_means = {}, []
        for fill in order:
            call_ms, kern = run(path, data[fill])
            key = criterion.get(path)
            m = mean(kern[key]) if key else mean(call_ms)
            if fill == "random":
                random_means.append(m)
                if len(random_means) == 1:
                    means[fill] = m
            else:
                means[fill] = m
            rows.append({"path": path, "fill": fill, "run": len(random_means) if fill == "random" else 1,
                         "timed": key or "call", "mean_ms": round(m, 5), "call_ms": [round(x, 4) for x in call_ms],
                         "kernel_ms": {k: [round(x, 4) for x in v] for k, v in kern.items()}})
            print(json.dumps(rows[-1]), flush=True)
        spread = max(random_means) - min(random_means)
        diff = max(means[k] for k in four) - min(means[k] for k in four)
        summary[path] = {"timed": criterion.get(path) or "call", "fill_mean_ms": {k: round(v, 5) for k, v in means.items()},
                         "random_run_mean_ms": [round(x, 5) for x in random_means], "spread_ms": round(spread, 5),
                         "max_fill_diff_ms": round(diff, 5),
                         "diff_over_spread": round(diff / spread, 3) if spread > 0 else None}
        if path in criterion:
            summary[path]["within_3x_spread"] = bool(diff <= SPREAD_FACTOR * spread)
    # the `_ct` / existing ratio on the random fill: whole device calls (Sign: hash + multiplication on both sides)
    call_random = {p: mean([x for r in rows if r["path"] == p and r["fill"] == "random" for x in r["call_ms"]])
                   for p in paths}
    result = {"tool": "sign_timing", "build": src[:16], "device": torch.cuda.get_device_name(0), "n": n,
              "launches": args.launches, "warmup": args.warmup, "order": order, "summary": summary,
              "random_call_ms": {k: round(v, 4) for k, v in call_random.items()},
              "ratio_ct_over_existing": {"sign": round(call_random["sign_ct"] / call_random["sign"], 4),
                                         "sk_to_pk": round(call_random["sk_to_pk_ct"] / call_random["sk_to_pk"], 4)},
              "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({k: result[k] for k in ("summary", "random_call_ms", "ratio_ct_over_existing")}), flush=True)


if __name__ == "__main__":
    main()
