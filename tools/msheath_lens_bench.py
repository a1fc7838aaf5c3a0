"""Time one MSheath call with per-sample lengths (MSheath.run(lens=), the LENS kernels of csrc/rowops.hip and
csrc/msheath.hip) against the same call on the padded batch, which is all there was before and is the yardstick.

Shape: the bench's (`tiny`, B = 32, L = 3001): MSheath(384, 6, 4), 32 x 3001 x 384, train mode, forward + backward,
bf16 mode.  Three variants, alternating inside every repetition:

  (a) uniform     lens=None on the padded batch
  (b) lens_full   the LENS entry points with every length at 3001, forced past the full-length shortcut: what the
                  table costs
  (c) lens_mixed  lengths drawn uniformly between half and full length (seed 0)

Median of --reps after --warmup, with min-max; device-event time and host enqueue time per variant.  (b) is compared
with (a) bit for bit before timing (output and input gradient).  Only the row, jump and x_new passes skip pad rows,
and the row-list GEMMs all-pad tiles from layer 1 on -- the tail's GEMMs and LayerNorm and layer 0's projection do not.
Prints one JSON line and, with --out, writes it to a file.  Judges nothing.

usage: python tools/msheath_lens_bench.py [--reps 20] [--warmup 5] [--out profiles/msheath_lens.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "asr-model_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

B, L, D, HEAD, LAYER = 32, 3001, 384, 6, 4


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    from asrx import ops, prec
    from asrx.model import MSheath
    from asrx.noise import NoiseCtx

    if not torch.cuda.is_available():
        raise SystemExit("msheath_lens_bench: needs a GPU (a CPU timing says nothing about it)")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(args.seed)
    lens = rng.integers((L + 1) // 2, L + 1, B).tolist()

    class Forced(ops.SeqLens):
        """Never reports a full-length batch: the LENS kernels run whatever the lengths."""

        __slots__ = ()

        def check(self, B_, T_, device):
            super().check(B_, T_, device)
            return False

    torch.manual_seed(0)
    mod = MSheath(D, HEAD, LAYER).to(dev).train()
    noise = NoiseCtx(1, 0, True)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, L, D, generator=g)
    for b, t in enumerate(lens):  # the project's rule: zero pad rows
        x[b, t:] = 0.0
    x = x.to(dev).requires_grad_()
    cot = torch.randn(B, L, D, generator=g).to(dev)
    full = ops.seq_lens([L] * B, device=dev)
    tabs = {"uniform": None, "lens_full": Forced(full.lens, full.table), "lens_mixed": ops.seq_lens(lens, device=dev)}
    last = {}

    def make(name):
        def run():
            x.grad = None
            for p in mod.parameters():
                p.grad = None
            y = mod.run(x, noise, "bench.jump", 0, lens=tabs[name])
            y.backward(cot)
            last[name] = (y.detach(), x.grad)
        return run

    res = {"B": B, "L": L, "D": D, "layers": LAYER, "mode": "bf16", "reps": args.reps, "warmup": args.warmup,
           "seed": args.seed,
           "mixed_rows": {"live": sum(lens), "launch": B * L, "live_fraction_of_launch": round(sum(lens) / (B * L), 4)}}
    with prec.precision("bf16"):
        variants = {k: make(k) for k in tabs}
        for fn in variants.values():
            fn()
        torch.cuda.synchronize()
        for i, what in enumerate(("output", "input gradient")):
            if not torch.equal(last["uniform"][i], last["lens_full"][i]):
                raise SystemExit(f"msheath_lens_bench: full-length lens differs from the uniform call ({what})")
            if not bool(torch.isfinite(last["lens_mixed"][i]).all()):
                raise SystemExit(f"msheath_lens_bench: non-finite {what} with the mixed lengths")
        last.clear()
        t = _time(variants, args.reps, args.warmup)
    a = t["uniform"]["device_us"]
    t["ratio_lens_full_to_uniform"] = round(t["lens_full"]["device_us"] / a, 4)
    t["ratio_lens_mixed_to_uniform"] = round(t["lens_mixed"]["device_us"] / a, 4)
    t["uniform_spread"] = round(t["uniform"]["device_min_max_us"][1] / t["uniform"]["device_min_max_us"][0], 4)
    res["msheath_fwd_bwd"] = t
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
