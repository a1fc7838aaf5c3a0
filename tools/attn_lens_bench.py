"""Time attention with per-sample lengths (asrx_lattn_fwd + asrx_lattn_bwd) against the uniform entry points on the
padded batch (asrx_attn_fwd2 + asrx_attn_bwd2), which is all there was before and is the yardstick.

Shape: B = 32, H = 6, hd 64, non-causal, forward + backward, bf16 mode with the storage the model uses when a
backward runs (io = 1: q / k / v stored bf16, o and dO fp32).  Two launches: audio self-attention Lq = Lk = 3001,
and the cross shape Lq = 256 against Lk = 3001.  Three variants, alternating inside every repetition:

  (a) uniform     asrx_attn_fwd2 / asrx_attn_bwd2 on the padded batch
  (b) lens_full   the new entry points with every length at the launch extent: what the table costs
  (c) lens_mixed  the new entry points with the frame counts of the mixed batch of DESIGN section 7 (clip lengths
                  5-30 s uniform, seed 0, as tools/ragged_mel_bench.py draws them) as key lengths, and as query
                  lengths too in the self shape (the cross shape keeps every query row live)

Median of --reps after --warmup, with min-max; device-event time and host enqueue time per variant.  (b) is
compared with (a) bit for bit before timing.  Also printed: the live-work fraction sum(ql kl) / (B Lq Lk) and the
share of workgroups of each kernel that hold a live row (those run; the others store zeros and return).
Prints one JSON line and, with --out, writes it to a file.

usage: python tools/attn_lens_bench.py [--reps 20] [--warmup 5] [--out profiles/attn_lens.json]
"""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "asr-model_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

B, H, HD, L, LQ_CROSS = 32, 6, 64, 3001, 256
IO = 1  # q / k / v stored bf16; o and dO fp32


def _st(t):
    arr = (ctypes.c_int64 * 3)(t.stride(0), t.stride(1), t.stride(2))
    return arr, ctypes.cast(arr, ctypes.c_void_p).value


def _time(variants, reps, warmup):
    import torch

    times = {k: {"device": [], "enqueue": []} for k in variants}
    for rep in range(warmup + reps):
        for name, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a.record()
            fn()
            b.record()
            t1 = time.perf_counter()
            b.synchronize()
            if rep >= warmup:
                times[name]["device"].append(a.elapsed_time(b) * 1e3)
                times[name]["enqueue"].append((t1 - t0) * 1e6)
    out = {}
    for name, kinds in times.items():
        out[name] = {}
        for kind, ts in kinds.items():
            out[name][kind + "_us"] = round(statistics.median(ts), 1)
            out[name][kind + "_min_max_us"] = [round(min(ts), 1), round(max(ts), 1)]
    return out


def _live_blocks(lens, rows):
    """Share of the ceil(extent / rows) blocks per sample that hold a live row, for lens <= extent."""
    return lambda extent: sum(math.ceil(n / rows) for n in lens) / (len(lens) * math.ceil(extent / rows))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    from asrx import lib

    if not torch.cuda.is_available():
        raise SystemExit("attn_lens_bench: needs a GPU (a CPU timing says nothing about it)")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(args.seed)
    samples = rng.integers(5 * 16000, 30 * 16000 + 1, B).tolist()  # ragged_mel_bench's mixed batch
    frames = [int(lib.load().asrx_mel_frames(n)) for n in samples]
    assert max(frames) <= L
    P, S = lib.ptr, lib.stream
    scale = 1.0 / math.sqrt(HD)
    res = {"B": B, "H": H, "hd": HD, "io": IO, "reps": args.reps, "warmup": args.warmup, "seed": args.seed,
           "mixed_frames": {"live": sum(frames), "padded_batch": B * max(frames), "longest": max(frames)}, "cases": {}}

    for case, Lq, q_mixed in (("self_3001", L, frames), ("cross_256x3001", LQ_CROSS, [LQ_CROSS] * B)):
        g = torch.Generator().manual_seed(1)
        q = torch.randn(B, Lq, H, HD, generator=g).bfloat16().to(dev)
        k, v = (torch.randn(B, L, H, HD, generator=g).bfloat16().to(dev) for _ in range(2))
        dO = torch.randn(B, Lq, H, HD, generator=g).to(dev)
        tabs = {"lens_full": torch.tensor([[Lq, L]] * B, dtype=torch.int32, device=dev),
                "lens_mixed": torch.tensor(list(zip(q_mixed, frames)), dtype=torch.int32, device=dev)}

        def buffers():
            return dict(o=torch.empty(B, Lq, H, HD, device=dev), lse=torch.empty(B, H, Lq, device=dev),
                        delta=torch.empty(B, H, Lq, device=dev), dq=torch.empty(B, Lq, H, HD, device=dev),
                        dk=torch.empty(B, L, H, HD, device=dev), dv=torch.empty(B, L, H, HD, device=dev))

        def make(table, w):
            st = {n: _st(t) for n, t in dict(q=q, k=k, v=v, dO=dO, o=w["o"], dq=w["dq"], dk=w["dk"], dv=w["dv"]).items()}
            tab = [] if table is None else [P(table)]
            fwd, bwd = ("asrx_attn_fwd2", "asrx_attn_bwd2") if table is None else ("asrx_lattn_fwd", "asrx_lattn_bwd")

            def run(_keep=st):
                lib.call(fwd, 1, IO & 3, P(q), st["q"][1], P(k), st["k"][1], P(v), st["v"][1], P(w["o"]), st["o"][1],
                         P(w["lse"]), *tab, B, H, Lq, L, HD, 0, scale, S())
                lib.call(bwd, 1, IO, P(q), st["q"][1], P(k), st["k"][1], P(v), st["v"][1], P(w["o"]), st["o"][1],
                         P(dO), st["dO"][1], P(w["lse"]), P(w["delta"]), P(w["dq"]), st["dq"][1], P(w["dk"]),
                         st["dk"][1], P(w["dv"]), st["dv"][1], *tab, B, H, Lq, L, HD, 0, scale, S())
            return run

        bufs = {n: buffers() for n in ("uniform", "lens_full", "lens_mixed")}
        variants = {"uniform": make(None, bufs["uniform"]), "lens_full": make(tabs["lens_full"], bufs["lens_full"]),
                    "lens_mixed": make(tabs["lens_mixed"], bufs["lens_mixed"])}
        for fn in variants.values():
            fn()
        torch.cuda.synchronize()
        for n in ("o", "lse", "dq", "dk", "dv"):
            if not torch.equal(bufs["uniform"][n], bufs["lens_full"][n]):
                raise SystemExit(f"attn_lens_bench: full-length lens differs from the uniform call ({case}, {n})")
            if not bool(torch.isfinite(bufs["lens_mixed"][n]).all()):
                raise SystemExit(f"attn_lens_bench: non-finite output with the mixed lengths ({case}, {n})")
        t = _time(variants, args.reps, args.warmup)
        a = t["uniform"]["device_us"]
        live = sum(x * y for x, y in zip(q_mixed, frames)) / (B * Lq * L)
        t["ratio_lens_full_to_uniform"] = round(t["lens_full"]["device_us"] / a, 4)
        t["ratio_lens_mixed_to_uniform"] = round(t["lens_mixed"]["device_us"] / a, 4)
        t["uniform_spread"] = round(t["uniform"]["device_min_max_us"][1] / t["uniform"]["device_min_max_us"][0], 4)
        t["live_work_fraction"] = round(live, 4)
        # workgroups with a live row: forward and dq over 256 query rows, dkdv over 256 key rows (hd 64)
        t["live_workgroups"] = {"fwd_dq": round(_live_blocks(q_mixed, 256)(Lq), 4),
                                "dkdv": round(_live_blocks(frames, 256)(L), 4)}
        # of the live workgroups' key tiles (64 keys) / query tiles (64 rows), the share that is live work
        t["live_tile_fraction"] = round(sum(math.ceil(a_ / 256) * math.ceil(b_ / 64) for a_, b_ in zip(q_mixed, frames))
                                        / (B * math.ceil(Lq / 256) * math.ceil(L / 64)), 4)
        res["cases"][case] = t

    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
