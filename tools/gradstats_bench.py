"""Time GradStats.measure() on the real gradient set of a config against the two ways the reference
loop gets the same numbers: torch.nn.utils.clip_grad_norm_(foreach=True) and the per-parameter
``p.grad.norm().item()`` loop of track_grad_norms (essentials.py:778-821).

One forward + backward (B = 2, 1 s clips) produces the gradients; each variant is then timed with
device events, median of --reps after --warmup, the three variants alternating inside every repetition.
Prints one JSON line and, with --out, writes it to a file.

usage: python tools/gradstats_bench.py [--config tiny] [--reps 20] [--warmup 5] [--out profiles/gradstats_tiny.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="tiny")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from asrx import prec
    from asrx.config import CONFIGS
    from asrx.model import Model
    from asrx.optim import GS_CHUNK, GradStats

    if not torch.cuda.is_available():
        raise SystemExit("gradstats_bench: needs a GPU (a CPU timing says nothing about it)")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    cfg = CONFIGS[args.config]
    model = Model(cfg).to(dev).train()
    g = torch.Generator().manual_seed(0)
    B, T, S = 2, 8, 101
    ids = torch.randint(3, cfg.tokens, (B, T), generator=g)
    ids[:, 0] = 1
    labels = torch.cat([ids[:, 1:], torch.full((B, 1), 2)], 1)
    model.set_noise(1, 0)
    with prec.precision("bf16"):
        out = model(labels=labels.to(dev), text_ids=ids.to(dev), spectrogram=torch.randn(B, 128, S, generator=g).to(dev),
                    pitch=(torch.rand(B, 1, S, generator=g) * 200).to(dev),
                    waveform=(torch.randn(B, 1, S - 1, generator=g) * 0.1).to(dev))
        out["loss"].backward()
    params = [p for p in model.parameters() if p.grad is not None]
    elements = sum(p.grad.numel() for p in params)
    stats = GradStats(model.named_parameters(), max_norm=1e9)

    def ours():
        stats.measure()

    def foreach_clip():
        torch.nn.utils.clip_grad_norm_(params, 1e9, foreach=True)  # coefficient clamps to 1: gradients keep their values

    def item_loop():
        return [p.grad.norm().item() for p in params]

    variants = {"measure_us": ours, "clip_grad_norm_foreach_us": foreach_clip, "norm_item_loop_us": item_loop}
    times = {k: [] for k in variants}
    for rep in range(args.warmup + args.reps):
        for name, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            fn()
            b.record()
            b.synchronize()
            if rep >= args.warmup:
                times[name].append(a.elapsed_time(b) * 1e3)
    want = torch.stack([p.grad.double().square().sum() for p in params]).sum().sqrt().item()
    res = {"config": args.config, "gradients": len(params), "elements": elements, "chunk": GS_CHUNK,
           "chunks": stats._nitems, "launches_per_measure": 2, "reps": args.reps, "warmup": args.warmup,
           "total_norm": float(stats.total_norm), "total_norm_float64": want}
    for name, ts in times.items():
        res[name] = round(statistics.median(ts), 2)
        res[name.replace("_us", "_min_max_us")] = [round(min(ts), 2), round(max(ts), 2)]
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
