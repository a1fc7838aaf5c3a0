"""Time the fused d = 64 AbbyNormal kernels (asrx_abby64_fwd, asrx_abby64_bwd) against the split path they
replace -- asrx_gemm_wn_router + asrx_abby_fwd_logits2 forward, asrx_abby_bwd2 + the beta = 1 input-gradient GEMM
backward -- at the flagship step's three row counts (tiny config, B = 32 x 30 s: 1 152 384, 576 000 and 49 152
rows of 64 features), forward with and without the kept h_pre (bf16 out, noise on), and backward.

Same process, same inputs; the variants alternate inside every repetition; device-event time, median of --reps
after --warmup.  Outputs are compared (torch.equal) before timing.  GB/s are the bytes each path has to move per
row over its time: forward 400 B fused (x 256, out 128, ys and idx 16) against 680 B split (x twice, logits
written and read), + 256 B with h_pre kept; backward 1296 B fused (g, x, h_pre, ys, idx 784; dx, dh 512) against
2064 B split (the GEMM reads dh and dx and writes dx again).  Prints one JSON line and, with --out, writes it.

usage: python tools/abby64_bench.py [--reps 20] [--warmup 5] [--acc 0] [--out profiles/abby64_micro.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "asr-model_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

ROWS = ((32, 6002, 6), (32, 3000, 6), (32, 256, 6))  # (B, L, H) of the audio self, cross and text-side norms
BYTES = {"fwd_split": 680, "fwd_fused": 400, "fwd_keep_split": 936, "fwd_keep_fused": 656, "bwd_split": 2064,
         "bwd_fused": 1296}


def _time(variants, reps, warmup):
    import torch

    times = {k: [] for k in variants}
    for rep in range(warmup + reps):
        for name, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            fn()
            b.record()
            b.synchronize()
            if rep >= warmup:
                times[name].append(a.elapsed_time(b) * 1e3)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--acc", type=int, default=0, help="backward adds into an existing dx (+256 B per row read)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from asrx import gemm as G
    from asrx import lib

    if not torch.cuda.is_available():
        raise SystemExit("abby64_bench: needs a GPU (a CPU timing says nothing about it)")
    dev = torch.device("cuda:0")
    P, S = lib.ptr, lib.stream
    g = torch.Generator().manual_seed(0)
    W1 = (torch.randn(64, 64, generator=g) / 8).to(dev)
    b1 = (torch.randn(64, generator=g) * 0.2).to(dev)
    W2 = (torch.randn(3, 64, generator=g) * 0.4).to(dev)
    b2 = (torch.randn(3, generator=g) * 0.2).to(dev)
    Wb, Wt = G.weight_bf16(W1, cache=False), G.weight_bf16(W1, trans=True, cache=False)
    res = {"reps": args.reps, "warmup": args.warmup, "acc": args.acc, "cases": {}}
    for B, L, H in ROWS:
        rows = B * L * H
        x = torch.randn(rows, 64, device=dev) * (0.25 + 4.0 * torch.rand(rows, 1, device=dev))
        gy = torch.randn(rows, 64, device=dev)
        E = lambda *s, dt=torch.float32: torch.empty(*s, device=dev, dtype=dt)  # noqa: E731
        logits, hp = E(rows, 3), {"split": E(rows, 64), "fused": E(rows, 64)}
        out = {k: E(rows, 64, dt=torch.bfloat16) for k in ("split", "fused")}
        ys = {k: E(rows, 3) for k in ("split", "fused")}
        idx = {k: E(rows, dt=torch.int32) for k in ("split", "fused")}
        dx = {k: torch.zeros(rows, 64, device=dev) for k in ("split", "fused")}
        dh = {k: E(rows, 64) for k in ("split", "fused")}
        dW2, db2 = torch.zeros(3, 64, device=dev), torch.zeros(3, device=dev)

        def fwd_split(keep):
            lib.call("asrx_gemm_wn_router", P(x), 64, P(Wb), 64, P(b1), P(W2), P(hp["split"]) if keep else None, 64,
                     P(logits), rows, 64, 64, S())
            lib.call("asrx_abby_fwd_logits2", P(x), P(logits), P(b2), P(out["split"]), 1, P(ys["split"]),
                     P(idx["split"]), rows, 64, L, H, 0, 7, 1, None, None, None, S())

        def fwd_fused(keep):
            lib.call("asrx_abby64_fwd", P(x), P(Wb), 64, P(b1), P(W2), P(b2), P(out["fused"]), 1, P(ys["fused"]),
                     P(idx["fused"]), P(hp["fused"]) if keep else None, rows, L, H, 0, 7, 1, S())

        def bwd_split():
            lib.call("asrx_abby_bwd2", P(gy), P(x), P(hp["split"]), P(W2), P(ys["split"]), P(idx["split"]),
                     P(dx["split"]), P(dh["split"]), P(dW2), P(db2), rows, 64, args.acc, S())
            G.gemm_wn(dh["split"], Wt, dx["split"], M=rows, N=64, K=64, lda=64, ldc=64, beta=1.0)

        def bwd_fused():
            lib.call("asrx_abby64_bwd", P(gy), P(x), P(hp["split"]), P(Wt), 64, P(W2), P(ys["split"]), P(idx["split"]),
                     P(dx["fused"]), P(dh["fused"]), P(dW2), P(db2), rows, args.acc, S())

        fwd_split(True), fwd_fused(True), bwd_split(), bwd_fused()
        torch.cuda.synchronize()
        same = all(bool(torch.equal(d["split"], d["fused"])) for d in (out, ys, idx, hp, dx, dh))
        if not same:
            raise SystemExit(f"abby64_bench: the fused kernels differ from the split path at {rows} rows")
        variants = {"fwd_split": lambda: fwd_split(False), "fwd_fused": lambda: fwd_fused(False),
                    "fwd_keep_split": lambda: fwd_split(True), "fwd_keep_fused": lambda: fwd_fused(True),
                    "bwd_split": bwd_split, "bwd_fused": bwd_fused}
        t = {"outputs_equal": same}
        for name, ts in _time(variants, args.reps, args.warmup).items():
            us = statistics.median(ts)
            nbytes = (BYTES[name] + (256 if args.acc and name.startswith("bwd") else 0)) * rows
            t[name] = {"device_us": round(us, 1), "min_max_us": [round(min(ts), 1), round(max(ts), 1)],
                       "bytes_per_row": nbytes // rows, "GBps": round(nbytes / us / 1e3, 0)}
        for k in ("fwd", "fwd_keep", "bwd"):
            t[f"ratio_{k}_split_over_fused"] = round(t[k + "_split"]["device_us"] / t[k + "_fused"]["device_us"], 3)
        res["cases"][str(rows)] = t
        del x, gy, logits, hp, out, ys, idx, dx, dh
        torch.cuda.empty_cache()

    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
