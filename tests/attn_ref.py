"""Float64 reference of softmax attention (forward and backward) with COMPONENTWISE error bounds, a float64 model
of the roundings the kernels document, and the list of cases both test_attn_ref.py (CPU: the bounds hold for the
rounding model, and a mutated model breaks them) and test_gpu_attn_ref.py (the kernels of csrc/attn.hip and
csrc/attn_mf.hip against the reference) run.  Nothing here touches the GPU.

q, k, v, dO are float64 (B, L, H, hd) and already hold the values the kernel computes with: bf16-representable in
the perf mode (a fp32-stored operand is rounded by the kernel on its way into the MFMA, make_inputs() applies the
same rounding), fp32-representable in the parity mode.  With S = scale q k^T (top-left causal mask), P = softmax(S),
O = P V, Delta_i = sum_d dO_id O_id, dP = dO V^T, dS = P (dP - Delta), dV = P^T dO, dQ = scale dS K, dK = scale dS^T Q:

    bO_id    = u_i sum_j P_ij |V_jd|                          P carries a relative error u before P V
    bDelta_i = sum_d |dO_id| (bO_id + [u |O_id|])             Delta is taken from the kernel's own O; [..] when dO is
                                                              rounded in the Delta pass (RD) or o is stored bf16
    eS_ij    = P_ij (u_i |dP_ij - Delta_i| + bDelta_i) + u_i |dS_ij|
                                                              P's error, Delta's error, dS rounded before its products
    bV_jd    = 2 sum_i u_i P_ij |dO_id|                       P's error and P rounded before P^T dO
    bQ_id    = scale sum_j eS_ij |K_jd|,   bK_jd = scale sum_i eS_ij |Q_id|
    bO of an o stored bf16 gains u |O_id| (the final rounding of the stored value, 2^-9 |O| at most).

u_i = u + 2^-22 max_j |S_ij|: the exponent S c - m c is one fp32 fma of numbers as large as the largest score, so
P's relative error grows with the scores (2^-24 per rounding of the product and of the sum, x ln 2 ... < 2^-22
|S|); at unit-scale inputs the term is 1e-6 and vanishes beside u, at the peaked inputs (|S| of 1e2 .. 1e3) it is
what keeps the parity bound honest.  It is applied to every case, not only to the peaked ones.

Score accumulation (a term the first derivation missed; found on the CPU, where torch float32 left the parity
bound by 1.2 .. 2.4 once |S| passed 1e2): S_ij is itself an fp32 dot product of hd terms, in the MFMA too (the bf16
products are exact, the hd accumulations round), so |S~_ij - S_ij| <= a_ij = hd 2^-24 scale sum_d |q_id k_jd|, and
an ABSOLUTE error of S is a RELATIVE error of P = exp(S - lse), in lse as the P-weighted mean of the row.  Where u
stands for P's own error above (bO, the first term of eS, one of the two u of bV) it is therefore
u_i + a_ij + sum_j P_ij a_ij.  At unit-scale inputs a_ij is 2e-5 (0.5 % of the perf u, the size of the parity u);
at the peaked inputs it reaches 1e-3.  It is the worst case of hd roundings; the observed error is nearer its root.

Underflow floor (a term the first derivation missed; found on the CPU, where the rounding model of a near one-hot
row left the bound by 1 / 2u = 128): a P_ij or dS_ij below the smallest normal number, 2^-126 in fp32 and in bf16
alike, is flushed to zero or rounded on the denormal grid, an ABSOLUTE error of up to 2^-126 that no relative u
covers.  Every unmasked (i, j) therefore adds 2^-126 to P's error: 2^-126 sum_j |V_jd| to bO, 2^-126 sum_i |dO_id|
to bV, 2^-126 (|dP_ij - Delta_i| + 1) to eS.  These are 1e-38 and change nothing a test can see except that
exactly underflowed elements stay inside.  Masked elements get no floor: their gradients must be exact zeros.

Perf mode (attn_mf.hip): u = 2^-8.  bf16 keeps 8 significant bits, so 2^-8 is the largest relative error of ONE
round-to-nearest (the spacing of bf16 numbers is 2^-7): bO is the exact worst case of rounding P, reached only when
one key carries the whole error of a row, and the rounding model lands at up to 0.87 of it (two comparable keys),
0.2 at most for dQ / dK and 0.5 for dV, where a second u stands for the second rounding.  What is left over is all
there is for fp32 accumulation, the hardware exp2 / log2 and the up-to-256 unnormalised P of the lazy rescale, all
orders of magnitude smaller than u.  u is not a knob: a ratio above 1 is a bug or a missing TERM, to be added above
with its reason.
Parity mode (attn.hip): u = (Lk + hd + 8) 2^-24, the gamma_n of an fp32 dot product in any summation order.

Not claimed: a single row rounded a couple of percent wrong sits inside a worst-case bf16 bound (the model lands
at 0.02 .. 0.87 of it) and passes.  What fails is anything structural: a key or a tile dropped or counted twice, a
mask off by one, a missing scale, a stride or a tail handled wrongly, rows that must be exactly zero and are not
(their bound IS zero), an unrounded Delta where the cancellation needs the rounded one.

The fp8 forward (attn_f8.hip) is not covered; reference() takes any u, so a bound for it can be added later.
"""
import math
from dataclasses import dataclass

import torch

U_BF16 = 2.0 ** -8
TINY = 2.0 ** -126  # smallest normal fp32 / bf16: the absolute underflow floor of P and dS
OUTPUTS = ("O", "dQ", "dK", "dV")

# multiplier of q[..., :8] of the second peaked family.  Chosen on the CPU: of PEAK2_CANDIDATES (max |S| of 30 to
# 1100; 1024 would leave the 1e2 .. 1e3 the model produces) the largest at which the rounding model stays under 1 on
# every peaked2 case.  All of them do (worst ratios 0.837, 0.817, 0.818, 0.786, 0.684, 0.549), so it is the last;
# test_attn_ref.py test_peaked_level checks the choice.
PEAK2_CANDIDATES = (16.0, 32.0, 64.0, 128.0, 256.0, 512.0)
PEAK2 = 512.0


def parity_u(Lk, hd):
    return (Lk + hd + 8) * 2.0 ** -24


def bf16r(x):
    """Round to bf16 (nearest even), returned in float64."""
    return x.float().bfloat16().double()


@dataclass(frozen=True)
class Case:
    mode: str  # "perf" (attn_mf.hip, bf16 MFMA) or "parity" (attn.hip, fp32)
    B: int
    H: int
    Lq: int
    Lk: int
    hd: int
    causal: bool
    family: str = "unit"  # unit, peaked6, peaked2 (PEAK2), flat
    io: int = 0  # bit 0 q / k / v stored bf16, bit 1 o stored bf16, bit 2 dO stored bf16
    layout: str = "contig"  # contig, kvpad (k, v halves of one buffer, q rows padded), headmajor ((B, H, L, hd))
    variant: int = 1  # forward kernel at hd 64 (asrx_set_attn_variant)

    @property
    def id(self):
        s = f"{self.mode}-{self.B}x{self.H}-{self.Lq}x{self.Lk}-hd{self.hd}-{'c' if self.causal else 'n'}-{self.family}"
        s += f"-io{self.io}-{self.layout}"
        return s + ("" if self.variant == 1 else f"-v{self.variant}")

    @property
    def u(self):
        return U_BF16 if self.mode == "perf" else parity_u(self.Lk, self.hd)

    @property
    def rd(self):
        """The Delta pass rounds a fp32-stored dO to bf16 (perf mode)."""
        return self.mode == "perf" and not self.io & 4

    @property
    def o_term(self):
        return self.rd or bool(self.io & 2)

    @property
    def scale(self):
        return 1.0 / math.sqrt(self.hd)


NONCAUSAL = [(1, 1), (33, 63), (32, 64), (31, 65), (255, 128), (256, 129), (257, 192), (513, 193), (64, 257)]
CAUSAL = [(1, 1), (64, 64), (65, 65), (129, 129), (257, 257), (300, 70), (70, 300), (257, 513), (513, 257)]


def _cases():
    out = []
    shapes = [(lq, lk, False) for lq, lk in NONCAUSAL] + [(lq, lk, True) for lq, lk in CAUSAL]
    for i, (lq, lk, c) in enumerate(shapes):
        b, h = ((1, 1), (2, 3))[i % 2]
        b2, h2 = ((2, 3), (1, 1))[i % 2]
        out.append(Case("perf", b, h, lq, lk, 64, c))
        out.append(Case("perf", b2, h2, lq, lk, 128, c))
        out.append(Case("parity", b, h, lq, lk, (64, 128)[i % 2], c))
    # the round-4 forward kernel (variant 0) at hd 64: every tile count, both grids
    for lq, lk, c in [(31, 65, False), (257, 192, False), (513, 193, False), (129, 129, True), (70, 300, True),
                      (513, 257, True)]:
        out.append(Case("perf", 2, 3, lq, lk, 64, c, variant=0))
    # input families
    for lq, lk, c in [(257, 192, False), (129, 129, True), (70, 300, True), (513, 257, True)]:
        for fam in ("peaked6", "peaked2", "flat"):
            for hd in (64, 128):
                out.append(Case("perf", 2, 3, lq, lk, hd, c, fam))
            out.append(Case("parity", 1, 2, lq, lk, 64 if c else 128, c, fam))
    # storage: every (q/k/v, o, dO) combination; the forward sees io & 3, the backward all three bits
    for lq, lk, c in [(257, 192, False), (300, 70, True)]:
        for io in range(1, 8):
            for hd in (64, 128):
                out.append(Case("perf", 2, 3, lq, lk, hd, c, "flat" if io & 2 else "unit", io))
    # strides
    for lay in ("kvpad", "headmajor"):
        for lq, lk, c in [(257, 192, False), (70, 300, True)]:
            for hd in (64, 128):
                for io in (0, 7):
                    out.append(Case("perf", 2, 3, lq, lk, hd, c, "unit", io, lay))
            out.append(Case("parity", 2, 3, lq, lk, 128 if c else 64, c, "unit", 0, lay))
    # the Delta kernel's grid-stride loop: 8192 blocks of 4 rows, so B H Lq = 33300 is two passes, the second ragged
    for hd in (64, 128):
        for io in (0, 6):
            out.append(Case("perf", 3, 3, 3700, 8, hd, False, "flat", io))
    out.append(Case("parity", 3, 3, 3700, 8, 64, False))
    assert len({c.id for c in out}) == len(out)
    return out


CASES = _cases()


def make_inputs(case):
    """-> (raw, vis): raw the tensors handed to the kernel (fp32, or bf16 where io says so), vis the float64 values
    the kernel computes with (a fp32-stored perf-mode operand is NOT bf16-representable: the kernel rounds it, and
    the Delta pass rounds dO, which is what RD is about).  Deterministic per case."""
    c = case
    fam = ("unit", "peaked6", "peaked2", "flat").index(c.family)
    seed = ((((c.B * 7 + c.H) * 4099 + c.Lq) * 4099 + c.Lk) * 3 + c.hd // 64) * 8 + 2 * fam + int(c.causal)
    g = torch.Generator().manual_seed(seed)
    q, k, v, dO = (torch.randn(c.B, L, c.H, c.hd, generator=g) for L in (c.Lq, c.Lk, c.Lk, c.Lq))
    if c.family == "peaked6":
        q[..., :8] *= 6.0
    elif c.family == "peaked2":
        q[..., :8] *= PEAK2
    elif c.family == "flat":  # values nearly constant over the keys: dP - Delta cancels (model.py on bf16 o, RD)
        v = torch.randn(c.B, 1, c.H, c.hd, generator=g) + 2.0 ** -6 * v
    elif c.family != "unit":
        raise ValueError(c.family)
    raw, vis = {}, {}
    for name, t, bit in (("q", q, 1), ("k", k, 1), ("v", v, 1), ("dO", dO, 4)):
        if c.mode == "perf" and c.io & bit:
            raw[name] = t.bfloat16()
            vis[name] = raw[name].double()
        else:
            raw[name] = t
            vis[name] = bf16r(t) if c.mode == "perf" else t.double()
    return raw, vis


def _heads(*ts):
    return tuple(t.permute(0, 2, 1, 3) for t in ts)  # (B, H, L, hd)


def _back(t):
    return t.permute(0, 2, 1, 3).contiguous()


def reference(q, k, v, dO, causal, scale, u, o_term=False, o_stored=False):
    """Float64 attention and its bounds (module docstring).  -> dict: O, dQ, dK, dV (B, L, H, hd), lse, Delta,
    bDelta (B, H, Lq), bound: {O, dQ, dK, dV}, smax: max_j |S_ij| per row, P."""
    qh, kh, vh, gh = _heads(q, k, v, dO)
    Lq, Lk = qh.shape[2], kh.shape[2]
    S = qh @ kh.transpose(-1, -2) * scale
    hidden = torch.ones(Lq, Lk, dtype=torch.bool).triu(1) if causal else torch.zeros(Lq, Lk, dtype=torch.bool)
    smax = S.masked_fill(hidden, 0.0).abs().amax(-1)
    S = S.masked_fill(hidden, float("-inf"))
    lse = torch.logsumexp(S, -1)
    P = torch.exp(S - lse[..., None])
    O = P @ vh
    Delta = (gh * O).sum(-1)
    dP = gh @ vh.transpose(-1, -2)
    dS = P * (dP - Delta[..., None])
    dV = P.transpose(-1, -2) @ gh
    dQ = scale * (dS @ kh)
    dK = scale * (dS.transpose(-1, -2) @ qh)

    ur = (u + 2.0 ** -22 * smax)[..., None]  # one rounding (of P before P V, of dS) on row i
    # S is an fp32 dot product over hd: |dS_ij| <= hd 2^-24 scale sum_d |q_id k_jd|, and P = exp(S - lse) turns it,
    # and its P-weighted row mean in lse, into a relative error of P
    a = (qh.abs() @ kh.abs().transpose(-1, -2)).masked_fill(hidden, 0.0) * (scale * qh.shape[-1] * 2.0 ** -24)
    uP = ur + a + (P * a).sum(-1, keepdim=True)  # relative error of P_ij
    seen = (~hidden).double() * TINY  # the underflow floor of every P the kernel forms
    bO = (P * uP) @ vh.abs() + seen @ vh.abs()
    bDelta = (gh.abs() * (bO + (U_BF16 * O.abs() if o_term else 0.0))).sum(-1)
    eS = P * (uP * (dP - Delta[..., None]).abs() + bDelta[..., None]) + ur * dS.abs()
    eS = eS + seen * ((dP - Delta[..., None]).abs() + 1.0)
    bV = (P * (uP + ur)).transpose(-1, -2) @ gh.abs() + seen.transpose(-1, -2) @ gh.abs()
    bQ = scale * (eS @ kh.abs())
    bK = scale * (eS.transpose(-1, -2) @ qh.abs())
    if o_stored:
        bO = bO + U_BF16 * O.abs()
    return {"O": _back(O), "dQ": _back(dQ), "dK": _back(dK), "dV": _back(dV), "lse": lse, "Delta": Delta,
            "bDelta": bDelta, "smax": smax, "P": P,
            "bound": {"O": _back(bO), "dQ": _back(bQ), "dK": _back(bK), "dV": _back(bV)}}


def reference_for(case, vis):
    return reference(vis["q"], vis["k"], vis["v"], vis["dO"], case.causal, case.scale, case.u, case.o_term,
                     bool(case.io & 2))


MUTATIONS = ("causal+1", "drop64", "droptail", "noscale_dk", "delta_nord", "ghost_dkdv")


def mutation_applies(case, m):
    c = case
    if m == "causal+1":
        return c.causal and c.Lk > 1
    if m == "drop64":  # key 64 exists and some query sees it
        return c.Lk > 64 and (not c.causal or c.Lq > 64)
    if m == "droptail":  # a partial last tile that is not the only one, seen by some query
        t0 = c.Lk // 64 * 64
        return c.Lk % 64 != 0 and t0 > 0 and (not c.causal or c.Lq > t0)
    if m == "delta_nord":
        return c.rd
    if m == "ghost_dkdv":
        return c.causal and c.Lk > c.Lq
    return m == "noscale_dk" and c.Lk > 1  # one key: dS = P (dP - Delta) is exactly zero


def rounding_model(q, k, v, dO, causal, scale, o_bf16=False, rnd=bf16r, mutate=None, dO_raw=None):
    """Float64 model of the perf kernels' documented roundings: the unnormalised exp(S - m) rounded to bf16 before
    P V and divided by the unrounded l; o stored bf16 where the variant says so; Delta from that O; P and dS
    rounded to bf16 before the three gradient products.  rnd = identity and float32 tensors give the parity
    arithmetic.  mutate: one of MUTATIONS (dO_raw: the unrounded dO, for "delta_nord")."""
    qh, kh, vh, gh = _heads(q, k, v, dO)
    Lq, Lk = qh.shape[2], kh.shape[2]
    S = qh @ kh.transpose(-1, -2) * scale
    hidden = torch.zeros(Lq, Lk, dtype=torch.bool)
    if causal:
        hidden = torch.ones(Lq, Lk, dtype=torch.bool).triu(2 if mutate == "causal+1" else 1)
    if mutate == "drop64":
        hidden = hidden.clone()
        hidden[:, 64] = True
    if mutate == "droptail":
        hidden = hidden.clone()
        hidden[:, Lk // 64 * 64:] = True
    S = S.masked_fill(hidden, float("-inf"))
    m = S.amax(-1, keepdim=True)
    e = torch.exp(S - m)
    l = e.sum(-1, keepdim=True)
    O = (rnd(e) @ vh) / l
    lse = (m + torch.log(l))[..., 0]
    if o_bf16:
        O = rnd(O)
    gD = _heads(dO_raw)[0] if mutate == "delta_nord" else gh
    Delta = (gD * O).sum(-1)
    P = torch.exp(S - lse[..., None])
    dS = P * (gh @ vh.transpose(-1, -2) - Delta[..., None])
    Pb, dSb = rnd(P), rnd(dS)
    dV = Pb.transpose(-1, -2) @ gh
    dQ = scale * (dSb @ kh)
    dK = (1.0 if mutate == "noscale_dk" else scale) * (dSb.transpose(-1, -2) @ qh)
    if mutate == "ghost_dkdv":  # keys no query sees must get exact zeros
        dK, dV = dK.clone(), dV.clone()
        dK[:, :, Lq:] += 2.0 ** -20
        dV[:, :, Lq:] += 2.0 ** -20
    return {"O": _back(O), "dQ": _back(dQ), "dK": _back(dK), "dV": _back(dV), "lse": lse, "Delta": Delta}


def ratio(got, ref, bound):
    """max over elements of |got - ref| / bound and its index; a zero bound admits only an exact match (the ratio
    is then 0 or inf), and a non-finite value is inf."""
    err = (got.double() - ref).abs()
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, math.inf, 0.0).to(err.dtype))
    r = torch.where(torch.isfinite(got.double()), r, torch.full_like(r, math.inf))
    i = int(r.argmax())
    return float(r.flatten()[i]), tuple(int(x) for x in torch.unravel_index(torch.tensor(i), r.shape))


def ratios(got, ref):
    """{output: (worst ratio, index)} of a result dict against reference()'s."""
    return {n: ratio(got[n], ref[n], ref["bound"][n]) for n in OUTPUTS}


def where(case, name, idx):
    """Human-readable location of a worst element: (b, row, h, d) and the tiles it falls in."""
    b, row, h, d = idx
    if name in ("dK", "dV"):
        blk = 256 if case.hd == 64 else 128
        t = f"key tile {row // 64} (last tile holds {(case.Lk - 1) % 64 + 1} keys), dkdv block {row // blk}"
    else:
        blk = 256 if name == "O" or case.hd == 64 else 128
        t = f"query block {row // blk}, wave rows {row % blk // 32 * 32}.., parity tile {row // 64}"
    return f"{name}[b={b}, row={row}, h={h}, d={d}]: {t}"


def lse32_error(vis, causal, scale, ref_lse):
    """Error of an fp32 CPU evaluation of (m c + log2 l) ln 2, c = scale log2 e, against the float64 lse."""
    qh, kh = _heads(vis["q"].float(), vis["k"].float())
    c = torch.tensor(scale * 1.4426950408889634, dtype=torch.float32)
    S = qh @ kh.transpose(-1, -2)
    if causal:
        S = S.masked_fill(torch.ones(S.shape[-2], S.shape[-1], dtype=torch.bool).triu(1), float("-inf"))
    m = S.amax(-1)
    l = torch.exp2(S * c - (m * c)[..., None]).sum(-1)
    lse = (m * c + torch.log2(l)) * torch.tensor(0.6931471805599453, dtype=torch.float32)
    return float((lse.double() - ref_lse).abs().max())


def lse_tolerance(case, vis, ref_lse):
    """1e-3 absolute at unit-scale scores (the bound test_attention_bf16 has always used); for the peaked families
    the larger of that and 8 x the error of the fp32 CPU evaluation on the same inputs."""
    if not case.family.startswith("peaked"):
        return 1e-3
    return max(1e-3, 8.0 * lse32_error(vis, case.causal, case.scale, ref_lse))
