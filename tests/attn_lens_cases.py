"""Ragged attention cases shared by test_attn_lens_ref.py (CPU) and test_gpu_attn_lens.py (GPU): a launch with
extents (Lq, Lk) whose samples have their own (q_len, k_len).  The ground truth of sample b is what already exists:
attn_ref.Case(mode, 1, H, q_len, k_len, hd, causal, family, io, layout), its make_inputs() and reference().

The lengths sit on the kernels' edges: the forward block of 256 query rows, the 32-row wave, the 64-key tile, the
backward blocks of 256 (hd 64) and 128 (hd 128) rows, the 64-row tiles of the fp32 kernels, and length 1.
Nothing here touches the GPU.
"""
import functools
from dataclasses import dataclass

import attn_ref as R

H = 2

# name -> (causal, (Lq, Lk) of the launch, per-sample (q_len, k_len))
LAUNCHES = {
    # full extent; one forward block exactly and one past a key tile; one past a wave and one key tile exactly; 1
    "cross": (False, (300, 321), ((300, 321), (256, 257), (33, 64), (1, 1))),
    "causal": (True, (321, 321), ((321, 321), (256, 256), (65, 65), (1, 1))),
    "causal300": (True, (300, 300), ((70, 300), (300, 70))),
    "cross257": (False, (257, 256), ((257, 65), (31, 256))),
}
LARGE = ("cross", "causal")


@dataclass(frozen=True)
class Ragged:
    launch: str
    mode: str  # "perf" or "parity"
    hd: int
    family: str = "unit"
    io: int = 0
    layout: str = "contig"
    variant: int = 1  # forward kernel at hd 64 (asrx_set_attn_variant)

    @property
    def causal(self):
        return LAUNCHES[self.launch][0]

    @property
    def extents(self):
        return LAUNCHES[self.launch][1]

    @property
    def lens(self):
        return LAUNCHES[self.launch][2]

    @property
    def samples(self):
        """The uniform B = 1 case of every sample."""
        return tuple(R.Case(self.mode, 1, H, ql, kl, self.hd, self.causal, self.family, self.io, self.layout)
                     for ql, kl in self.lens)

    @property
    def id(self):
        s = f"{self.launch}-{self.mode}-hd{self.hd}-{self.family}-io{self.io}-{self.layout}"
        return s + ("" if self.variant == 1 else f"-v{self.variant}")


def _ragged():
    out = []
    for la in LAUNCHES:
        for mode in ("perf", "parity"):
            for hd in (64, 128):
                out.append(Ragged(la, mode, hd))
    for la in LARGE:
        for hd in (64, 128):
            out.append(Ragged(la, "perf", hd, "flat", 7))  # every operand stored bf16
            for io in (0, 7):
                out.append(Ragged(la, "perf", hd, "unit", io, "kvpad"))
        out.append(Ragged(la, "perf", 64, variant=0))
    assert len({r.id for r in out}) == len(out)
    return out


RAGGED = _ragged()
# every distinct per-sample case (the forward variant gives the same numbers)
SAMPLES = sorted({c for r in RAGGED for c in r.samples}, key=lambda c: c.id)


@functools.lru_cache(maxsize=None)
def sample(case):
    """-> (raw, vis, reference) of one per-sample case; computed once and shared, never modified."""
    raw, vis = R.make_inputs(case)
    return raw, vis, R.reference_for(case, vis)
