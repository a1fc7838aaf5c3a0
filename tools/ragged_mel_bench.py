"""Time the ragged-batch feature call (mel.logmel_ragged: asrx_logmel_ragged + asrx_wave_pool_ragged, the
collated batch written directly) against the path extract_features_batch had before it: one mel.logmel (and,
when 160 does not divide n, one mel.wave_pool) per clip, then DataCollator's pad and stack.

Two batches of --batch clips, already on the device as load_batch leaves them (row stride = the longest
clip): lengths drawn once (fixed seed) uniformly from 5-30 s, and all clips 30 s.  Where that stride is no
multiple of 4 every tile is staged element-wise, so the mixed batch is also run from rows padded to a
multiple of 4 (the LDS-DMA staging path).  At 30 s the ragged
call is also timed against the equal-length mel.logmel(pool=True) on the same buffer, and the C entry points
alone (table uploaded and outputs allocated beforehand) against asrx_logmel alone: what raggedness costs
where it is not needed, with and without the host work of the call.  Same
process, same inputs; the variants alternate inside every repetition; median of --reps after --warmup.
Three times per variant: device-event time, the host time to enqueue the work, and host wall time to the end
of the device work (the per-clip loop is host-bound, so the three differ).  Outputs are compared
(torch.equal) before timing.  Prints one JSON line and, with --out, writes it to a file.

usage: python tools/ragged_mel_bench.py [--batch 32] [--reps 20] [--warmup 5] [--out profiles/ragged_mel.json]
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


def _time(variants, reps, warmup):
    """{name: {"device": [us], "enqueue": [us], "wall": [us]}}: every variant once per repetition, in turn."""
    import torch

    times = {k: {"device": [], "enqueue": [], "wall": []} for k in variants}
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
            t2 = time.perf_counter()
            if rep >= warmup:
                times[name]["device"].append(a.elapsed_time(b) * 1e3)
                times[name]["enqueue"].append((t1 - t0) * 1e6)
                times[name]["wall"].append((t2 - t0) * 1e6)
    return times


def _summary(times):
    out = {}
    for name, kinds in times.items():
        out[name] = {}
        for kind, ts in kinds.items():
            out[name][kind + "_us"] = round(statistics.median(ts), 1)
            out[name][kind + "_min_max_us"] = [round(min(ts), 1), round(max(ts), 1)]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    from asrx import lib, mel, synth
    from asrx.features import DataCollator

    if not torch.cuda.is_available():
        raise SystemExit("ragged_mel_bench: needs a GPU (a CPU timing says nothing about it)")
    dev = torch.device("cuda:0")
    B = args.batch
    full = synth.waveform(B, 30.0, first_seed=1000)  # (B, 480000)
    nmax = full.shape[1]
    rng = np.random.default_rng(args.seed)
    mixed = rng.integers(5 * 16000, nmax + 1, B).tolist()
    collator = DataCollator(None)
    res = {"batch": B, "reps": args.reps, "warmup": args.warmup, "seed": args.seed, "cases": {}}

    for case, lengths in (("mixed_5_30s", mixed), ("uniform_30s", [nmax] * B)):
        nmx = max(lengths)
        host = torch.zeros(B, 1, nmx)
        for b, n in enumerate(lengths):
            host[b, 0, :n] = full[b, :n]
        wave = host.to(dev)  # (B, 1, Nmax), zero past each clip: load_batch's result
        wav2 = wave[:, 0]
        plan = mel.ragged_plan(lengths)

        def per_clip_loop():
            """extract_features_batch before the ragged call, then the collator."""
            feats = []
            for i, n in enumerate(lengths):
                audio = wave[i, 0, :n].contiguous()
                s = mel.logmel(audio.unsqueeze(0), layout="BMF")[0]
                target = int((n / 16000) * (16000 // 160))
                if n == target * 160:
                    _, w = mel.logmel(audio.unsqueeze(0), layout="BMF", pool=True)
                else:
                    w = mel.wave_pool(audio.unsqueeze(0), target)
                feats.append({"spectrogram": s, "waveform": w, "labels": []})
            return collator(feats)

        def ragged():
            rm = mel.logmel_ragged(wav2, lengths, layout="BMF", pool=True)
            return {"spectrogram": rm.mel, "waveform": rm.pool.unsqueeze(1)}

        ref, got = per_clip_loop(), ragged()
        same = all(bool(torch.equal(ref[k], got[k])) for k in ("spectrogram", "waveform"))
        if not same:
            raise SystemExit(f"ragged_mel_bench: the ragged batch differs from the per-clip path ({case})")
        variants = {"per_clip_loop_collate": per_clip_loop, "ragged": ragged}
        if nmx % 4:
            padded = torch.nn.functional.pad(host[:, 0], (0, -nmx % 4)).to(dev)[:, :nmx]  # row stride 4-aligned
            variants["ragged_aligned_rows"] = lambda: mel.logmel_ragged(padded, lengths, layout="BMF", pool=True)
        if case == "uniform_30s":
            variants["logmel_equal_length"] = lambda: mel.logmel(wav2, layout="BMF", pool=True)
            # the entry points alone: nothing allocated, planned or uploaded inside the timed window
            consts, fbw, fbs = mel.device_consts(dev)
            clips = plan.table().to(dev)
            o = torch.empty(B, 128, plan.Fmax, device=dev)
            pl = torch.empty(B, plan.Tmax, device=dev)
            ws = torch.empty(lib.load().asrx_logmel_ws_bytes(B, nmx) // 4, device=dev)
            ld = wav2.stride(0)

            def ragged_entry():
                lib.call("asrx_logmel_ragged", lib.ptr(wav2), B, nmx, ld, lib.ptr(clips), lib.ptr(consts),
                         lib.ptr(fbw), lib.ptr(fbs), lib.ptr(o), 1, plan.Fmax * 128, plan.Fmax, lib.ptr(ws),
                         lib.ptr(pl), plan.Tmax, lib.stream())

            def equal_entry():
                lib.call("asrx_logmel", lib.ptr(wav2), B, nmx, ld, lib.ptr(consts), lib.ptr(fbw), lib.ptr(fbs),
                         lib.ptr(o), 1, plan.Fmax * 128, lib.ptr(ws), lib.ptr(pl), plan.Tmax, lib.stream())

            variants["ragged_entry_only"] = ragged_entry
            variants["logmel_entry_only"] = equal_entry
        t = _summary(_time(variants, args.reps, args.warmup))
        n_fused = sum(plan.fused)
        general_pool = not (n_fused == B and min(plan.T) == plan.Tmax)  # as logmel_ragged decides
        t.update(lengths=lengths, outputs_equal=same, frames=sum(plan.F), padded_frames=B * plan.Fmax,
                 live_tiles=sum((f + 15) // 16 for f in plan.F), grid_tiles=B * ((plan.Fmax + 15) // 16),
                 parent_launches=3 * B + n_fused, ragged_launches=3 if general_pool else 2,
                 algorithmic_bytes=sum(mel.algorithmic_bytes(1, n, True) for n in lengths))
        for kind in ("device", "enqueue", "wall"):
            t[f"ratio_{kind}_parent_over_ragged"] = round(
                t["per_clip_loop_collate"][kind + "_us"] / t["ragged"][kind + "_us"], 2)
        if case == "uniform_30s":
            t["ratio_device_ragged_over_equal_length"] = round(
                t["ragged"]["device_us"] / t["logmel_equal_length"]["device_us"], 3)
            t["ratio_device_ragged_entry_over_logmel_entry"] = round(
                t["ragged_entry_only"]["device_us"] / t["logmel_entry_only"]["device_us"], 3)
        res["cases"][case] = t
        del wave, wav2

    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
