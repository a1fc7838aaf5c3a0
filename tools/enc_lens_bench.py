"""Time the encoder layers with per-sample lengths (AudioEncoder.layers(lens=), the LENS kernels of csrc/rowops.hip)
against the same layers on the padded batch, which is all there was before and is the yardstick.

Shape: the bench's stream group, 64 x 3001 x 384 (two equal-length streams of 32 clips), 2 layers, train mode,
forward + backward, bf16 mode.  Three variants, alternating inside every repetition:

  (a) uniform     lens=None on the padded batch
  (b) lens_full   the LENS entry points with every length at 3001, forced past the full-length shortcut: what the
                  table costs
  (c) lens_mixed  the frame counts of the mixed batch of DESIGN section 7 (clip lengths 5-30 s uniform, seed 0, as
                  tools/ragged_mel_bench.py draws them), once per stream

Median of --reps after --warmup, with min-max; device-event time and host enqueue time per variant.  (b) is
compared with (a) bit for bit before timing (output and input gradient).  Only the convolutions, the statistics and
the activation passes skip dead rows -- the GEMMs and LayerNorm do not -- so (c) sits well above the live fraction.
Prints one JSON line and, with --out, writes it to a file.

usage: python tools/enc_lens_bench.py [--reps 20] [--warmup 5] [--out profiles/enc_lens.json]
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

B, STREAMS, T, D, LAYERS = 32, 2, 3001, 384, 2


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

    from asrx import lib, ops, prec
    from asrx.model import AudioEncoder
    from asrx.noise import NoiseCtx

    if not torch.cuda.is_available():
        raise SystemExit("enc_lens_bench: needs a GPU (a CPU timing says nothing about it)")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(args.seed)
    samples = rng.integers(5 * 16000, 30 * 16000 + 1, B).tolist()  # ragged_mel_bench's mixed batch
    frames = [int(lib.load().asrx_mel_frames(n)) for n in samples]
    assert max(frames) <= T

    class Forced(ops.SeqLens):
        """Never reports a full-length batch: the LENS kernels run whatever the lengths."""

        __slots__ = ()

        def check(self, B_, T_, device):
            super().check(B_, T_, device)
            return False

    torch.manual_seed(0)
    enc = AudioEncoder(128, D, 6, LAYERS, "gelu", "AbbyNormal").to(dev).train()
    noise = NoiseCtx(1, 0, True)
    g = torch.Generator().manual_seed(1)
    n = B * STREAMS
    x = torch.randn(n, T, D, generator=g).to(dev).requires_grad_()
    cot = torch.randn(n, T, D, generator=g).to(dev)
    full = ops.seq_lens([T] * n, device=dev)
    mixed = ops.seq_lens(frames * STREAMS, device=dev)
    tabs = {"uniform": None, "lens_full": Forced(full.lens, full.table), "lens_mixed": mixed}
    last = {}

    def make(name):
        def run():
            x.grad = None
            y = enc.layers(x, noise, 0, tabs[name])
            y.backward(cot)
            last[name] = (y.detach(), x.grad)
        return run

    res = {"B": n, "T": T, "D": D, "layers": LAYERS, "mode": "bf16", "reps": args.reps, "warmup": args.warmup,
           "seed": args.seed,
           "mixed_frames": {"live": sum(frames), "padded_batch": B * max(frames), "longest": max(frames),
                            "live_fraction_of_launch": round(sum(frames) / (B * T), 4)}}
    with prec.precision("bf16"):
        variants = {k: make(k) for k in tabs}
        for fn in variants.values():
            fn()
        torch.cuda.synchronize()
        for i, what in enumerate(("output", "input gradient")):
            if not torch.equal(last["uniform"][i], last["lens_full"][i]):
                raise SystemExit(f"enc_lens_bench: full-length lens differs from the uniform layers ({what})")
            if not bool(torch.isfinite(last["lens_mixed"][i]).all()):
                raise SystemExit(f"enc_lens_bench: non-finite {what} with the mixed lengths")
        last.clear()
        t = _time(variants, args.reps, args.warmup)
    a = t["uniform"]["device_us"]
    t["ratio_lens_full_to_uniform"] = round(t["lens_full"]["device_us"] / a, 4)
    t["ratio_lens_mixed_to_uniform"] = round(t["lens_mixed"]["device_us"] / a, 4)
    t["uniform_spread"] = round(t["uniform"]["device_min_max_us"][1] / t["uniform"]["device_min_max_us"][0], 4)
    res["layers_fwd_bwd"] = t
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
