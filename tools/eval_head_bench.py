"""Time the logits-free head (ops.logits_head: asrx_gemm_wn_head + asrx_head_merge) against the path
evaluation had before it: ops.LogitsCE's forward under no_grad (the fp32 logits written) + torch.argmax (the
logits read back) -- essentials.py:893-920.

Head alone at the config's (V, D), rows = 8192 (tiny, B = 32, T = 256) and rows = 32 (one greedy step of
B = 32; there the head is also timed in its decode form, without labels), then the whole teacher-forced
evaluation step at --batch clips of 30 s: Model.forward + argmax against Model.evaluate, eval mode.  Same
process, same inputs; device events, median of --reps after --warmup, the variants alternating inside every
repetition.  Outputs are compared before timing.  Prints one JSON line and, with --out, writes it to a file.

usage: python tools/eval_head_bench.py [--config tiny] [--batch 32] [--reps 20] [--warmup 5]
                                       [--out profiles/eval_head_tiny.json]
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


def _time(variants, reps, warmup):
    """{name: [us]}: every variant once per repetition, in turn, each between device events."""
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


def _summary(times):
    out = {}
    for name, ts in times.items():
        out[name + "_us"] = round(statistics.median(ts), 2)
        out[name + "_min_max_us"] = [round(min(ts), 2), round(max(ts), 2)]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="tiny")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--text-len", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--step-reps", type=int, default=8)
    ap.add_argument("--step-warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from asrx import gemm as G
    from asrx import ops, prec, synth
    from asrx.config import CONFIGS
    from asrx.mel import logmel
    from asrx.model import Model

    if not torch.cuda.is_available():
        raise SystemExit("eval_head_bench: needs a GPU (a CPU timing says nothing about it)")
    dev = torch.device("cuda:0")
    prec.set_precision("bf16")
    cfg = CONFIGS[args.config]
    V, D = cfg.tokens, cfg.dims
    res = {"config": args.config, "V": V, "D": D, "reps": args.reps, "warmup": args.warmup, "head": {}}
    g = torch.Generator().manual_seed(0)
    W = (torch.randn(V, D, generator=g) * 0.05).to(dev)

    with torch.no_grad():
        for rows in (args.batch * args.text_len, args.batch):
            h = (torch.randn(rows, D, generator=g) * 0.5).to(torch.bfloat16).to(dev)
            labels = torch.randint(3, V, (rows,), generator=g)
            labels[::7] = 0
            labels = labels.to(dev)

            def parent():
                logits, loss = ops.LogitsCE.apply(h, W, labels, None, False)
                return torch.argmax(logits, -1), loss

            def head():
                return ops.logits_head(h, W, labels)

            def head_decode():
                return ops.logits_head(h, W)

            p0, l0 = parent()
            o = head()
            same = bool(torch.equal(p0, o["pred"]))
            lerr = abs(float(l0) - float(o["loss"])) / abs(float(l0))
            if not same or lerr > 1e-5:
                raise SystemExit(f"eval_head_bench: the head differs from the stored logits at rows = {rows} "
                                 f"(pred equal {same}, loss rel err {lerr:.2e})")
            variants = {"logits_ce_argmax": parent, "logits_head": head}
            if rows == args.batch:
                variants["logits_head_decode"] = head_decode
            t = _summary(_time(variants, args.reps, args.warmup))
            nj = G._nj(rows, V)
            t.update(rows=rows, nj=nj, pred_equal=same, loss_rel_err=lerr,
                     ratio_parent_over_head=round(t["logits_ce_argmax_us"] / t["logits_head_us"], 3),
                     logits_bytes_not_written_and_reread=2 * rows * V * 4,
                     partial_bytes=12 * rows * ((V + 128 * nj - 1) // (128 * nj)))
            res["head"][str(rows)] = t
            del h, labels

        # the whole teacher-forced evaluation step (bench.py's synthetic clips, features made once)
        torch.manual_seed(0)
        model = Model(cfg).to(dev).eval()
        B = args.batch
        wav = synth.waveform(B, 30.0, first_seed=1000).to(dev)
        pitch = synth.pitch(B, frames=3001, first_seed=1000, mask_seed=2000).to(dev)
        ids, labels = synth.text(B, args.text_len, V, seed=7)
        ids, labels = ids.to(dev), labels.to(dev)
        spec, wfeat = logmel(wav, layout="BFM", pool=True)
        feats = {"spectrogram": spec.transpose(1, 2), "pitch": pitch, "waveform": wfeat.unsqueeze(1)}

        def step_parent():
            model.set_noise(0, 0)
            out = model(labels=labels, text_ids=ids, **feats)
            return torch.argmax(out["logits"], -1), out["loss"]

        def step_evaluate():
            model.set_noise(0, 0)
            out = model.evaluate(labels=labels, text_ids=ids, **feats)
            return out["predictions"], out["loss"]

        p0, l0 = step_parent()
        p1, l1 = step_evaluate()
        same = bool(torch.equal(p0, p1))
        lerr = abs(float(l0) - float(l1)) / abs(float(l0))
        peaks = {}
        for name, fn in (("forward_argmax", step_parent), ("evaluate", step_evaluate)):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            fn()
            torch.cuda.synchronize()
            peaks[name + "_peak_bytes"] = torch.cuda.max_memory_allocated() - base
        t = _summary(_time({"forward_argmax": step_parent, "evaluate": step_evaluate}, args.step_reps,
                           args.step_warmup))
        t.update(batch=B, text_len=args.text_len, reps=args.step_reps, warmup=args.step_warmup, pred_equal=same,
                 loss_rel_err=lerr, ratio_parent_over_evaluate=round(t["forward_argmax_us"] / t["evaluate_us"], 3),
                 **peaks)
        res["eval_step"] = t

    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
