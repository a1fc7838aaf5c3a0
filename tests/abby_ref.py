"""Float64 reference of the AbbyNormal row kernels (csrc/abby.hip: abby_fwd_kernel<E>, abby_bwd_kernel<E>,
abby_fwd64_kernel, abby_bwd64_kernel), the inputs, the metric and the mutations of tests/test_abby_ref.py (CPU) and
tests/test_gpu_abby_ref.py (GPU).

Reference.  forward() is the header comment of abby.hip and oracle/model.py:abby_normal in plain torch, in the dtype
of x (float64; the same code in float32 is the yardstick e32).  d, the window W = odd(max(3, int(0.05 d))) and the
padding W // 2 come from window(), not from the kernel's constants.  res is added after the normalisation.  tc =
out @ tw.T + tb is taken on the output BEFORE the residual is added.  The kernel's `ov` has the residual added
first -- the opposite order -- but no entry point passes both (asrx_abby_fwd_res hands the kernel no tw, the
entries that take tw no res), so the order cannot be observed through the C ABI; only the CPU test evaluates the
two together.  backward() is torch autograd on float64 leaves x, hpre, W2, b2 with the straight-through dec =
onehot(idx) - ys.detach() + ys; hpre is an independent leaf (the kernel's dx excludes dh_pre @ W1, which the host
adds).  F.max_pool1d routes the gradient of a tied maximum to its first position (tests/test_abby_ref.py checks
it), the order abby_wmax documents.  A constant row (the all-zero row) has std 0 and, as in the kernel (csd = 0),
no gradient through it.

Inputs (deterministic from the case, every value fp32-representable, returned as float64):
  mixed  row scale a_r log-uniform in [0.5, 200], x = a_r sign (0.7 + 0.6 u), per row c in {0, 0.3, 1} and each
         feature times 4 with probability c / W; row 1 all zero, row 2 the legacy 3 randn (rows >= 3).
  ties   magnitudes from {33, 51, 69, 93}, random signs: squares are odd and W is odd, so W max != 2 sum and
         `cond` cannot tie; window sums stay below 2^24 (exact in fp32); many windows hold a tied maximum.
  modes  logits = t_r - b2 + 0.3 n with t_r = onehot(r % 3) (ties tier: mode 2 on every row) and n a standard
         normal draw clamped to [-1, 1]: the two largest z of a row are then at least 0.4 apart, so every row's
         mode is known (an unclamped draw would leave a near-tie somewhere among 32 773 rows) and ys is far
         from saturation.  The backward puts the same targets on top of the hpre / W2 logits through `gumbel`.
         The hpre entry without noise lets the modes fall as they may (hpre = randn, W2 = 0.4 randn).

Metric.  Per row max_f |got - ref| / max_f |ref| (absolute where the reference row is zero), maximum over the
checked rows; ys absolute; dW2 / db2 relative to their largest entry.  Bound = max(floor, 20 e32), e32 the same
metric of the float32 evaluation of this reference against float64 -- never the kernel; floors FWD_TRANS (out,
ys, nrm, tc) and BWD_TRANS (dx, dhpre, dhpre0, dW2, db2) of ref_check.py.  `edge` is the same per-row metric on the
first and last W // 2 features alone: the only place where an average over the in-range count differs.
  Dead rows.  dz_k = y_k (dd_k - sum_j y_j dd_j), and where `cond` is false on every feature of a row -- no feature
  takes its window's maximum -- dd0 = dd1 = dd2, so dz, the row of dhpre and the row's share of dW2 / db2 are exactly
  0.  Autograd leaves float64 rounding noise there and a kernel fp32 noise, whose ratio says nothing.  backward()
  therefore sets dz and dhpre of these rows to the exact 0 (a condition on the reference's own `cond`), and they
  are measured absolutely, as the all-zero row is, under a name of their own (`dhpre0`), so that their noise does
  not enter the e32 of the other rows; the float32 yardstick keeps its own noise there (exact_dead = False).
  Every other row of dhpre is measured per row as above, with no floor under its scale -- a row whose dz nearly
  cancels raises e32, and with it the bound, by itself; dW2 / db2 are ref_check.rel, relative to their largest
  entry (absolute if the reference is all 0: a case whose every row is dead).

Exclusions (conditions on the float64 reference, never measurements): a mode-2 row with a feature whose cmargin =
|max - 2 avg| / max is below 1e-4 is left out of out (cmargin counts as 1 where max = 0: both arms give div = 0);
on the hpre entry a row whose two largest z are less than 1e-3 apart is left out too.  The backward evaluates
mode 2 on every row (dd1), so there any row with such a feature is left out and its gy is zeroed, which also keeps
it out of the dW2 / db2 sums.  idx must equal the reference on every other row.  At most 3 % of a case's rows
may be left out (CAP); the ties tier leaves out nothing and has cmargin >= 1e-5 everywhere.

Mutations (keyword `mut`; each breaks the bound in tests/test_abby_ref.py, which names the case): window (W - 2),
avg_shift (the avg window one feature to the right), avg_count (avg over the in-range count; caught by `edge`),
thr22 (max > 2.2 avg), mode2_avg (mode 2 takes avg everywhere), last_argmax (dx, ties tier), nrm_nosqrt,
tc_after_res, dx_no_pool (no gradient through the pools), dW2_hpre (dW2 from hpre instead of SiLU(hpre)).
NOT detectable: biased_std (the biased std in cv).  cv is added to all three z alike and cancels in the softmax, and
d cv = sum_k dz_k = 0 in the backward: the mutation moves ys, out and dx by float64 roundings only, and the CPU
test asserts that it stays inside every bound instead of listing it as covered.
"""
import functools
import math
import types

import torch
import torch.nn.functional as F

from ref_check import BWD_TRANS, FWD_TRANS, f32, gen, rel

DS = (64, 128, 256, 384, 512, 768, 1024)
SMALL_ROWS = (1, 3, 4, 5, 74)
CMARGIN_MIN = 1e-4
ZGAP_MIN = 1e-3
CAP = 0.03  # largest share of a case's rows that the exclusions may take
MUTATIONS = ("window", "avg_shift", "avg_count", "thr22", "mode2_avg", "last_argmax", "nrm_nosqrt", "tc_after_res",
             "dx_no_pool", "dW2_hpre")
NULL_MUTATIONS = ("biased_std",)

# grid caps of the host entry points (abby.hip): workgroups of 4 waves, one row per wave and sweep (d >= 128),
# four rows per wave at d = 64
FWD_SWEEP = 4096 * 4
BWD_SWEEP = 1024 * 4
BWD64_SWEEP = 1024 * 4 * 4
FWD_WRAP = ((128, FWD_SWEEP + 3), (128, 2 * FWD_SWEEP + 5), (384, FWD_SWEEP + 3))
BWD_WRAP = ((128, BWD_SWEEP + 3), (128, 2 * BWD_SWEEP + 5), (384, BWD_SWEEP + 3), (384, 2 * BWD_SWEEP + 5),
            (768, BWD_SWEEP + 3), (1024, BWD_SWEEP + 3), (64, BWD64_SWEEP + 5))


def window(d):
    W = max(3, int(0.05 * d))
    if W % 2 == 0:
        W += 1
    return W, W // 2


# ------------------------------------------------------------------------------------------------- reference
def _pools(sq, W, mut):
    rows = sq.unsqueeze(1)
    if mut == "last_argmax":  # the pools are symmetric: on the reversed row the first argmax is the last
        rows = rows.flip(-1)
    if mut == "window":
        W -= 2
    pad = W // 2
    mx = F.max_pool1d(rows, W, 1, pad)
    if mut == "avg_shift":
        avg = F.avg_pool1d(F.pad(rows, (pad - 1, pad + 1)), W, 1, 0)
    else:
        avg = F.avg_pool1d(rows, W, 1, pad, count_include_pad=mut != "avg_count")
    if mut == "last_argmax":
        mx, avg = mx.flip(-1), avg.flip(-1)
    return avg.squeeze(1), mx.squeeze(1)


def forward(x, *, logits=None, hpre=None, W2=None, b2, gumbel=None, res=None, tw=None, tb=None, idx=None, mut=None):
    """x (rows, d); router logits (rows, 3, without b2) or hpre (rows, d) / W2 (3, d); gumbel (rows, 3) or None;
    idx: the modes to use instead of the argmax of ys (the backward's input)."""
    rows, d = x.shape
    W, pad = window(d)
    lin = logits + b2 if logits is not None else F.linear(F.silu(hpre), W2, b2)
    const = (x == x[:, :1]).all(-1, keepdim=True)
    ramp = torch.arange(d, dtype=x.dtype).expand(rows, d)
    sd = torch.where(const, torch.zeros((), dtype=x.dtype),
                     torch.where(const, ramp, x).std(-1, keepdim=True, unbiased=mut != "biased_std"))
    cv = sd / (x.abs().mean(-1, keepdim=True) + 1e-6)
    z = lin + cv
    if gumbel is not None:
        z = z + gumbel
    ys = torch.softmax(z, -1)
    own = ys.argmax(-1)
    use = own if idx is None else idx.long()
    hard = torch.zeros_like(ys).scatter_(-1, use.unsqueeze(-1), 1.0)
    dec = hard - ys.detach() + ys
    xs = x.detach() if mut == "dx_no_pool" else x
    avg, mx = _pools(xs * xs, W, mut)
    cond = mx > (2.2 if mut == "thr22" else 2.0) * avg
    if mut == "mode2_avg":
        cond = torch.zeros_like(cond)
    c = cond.to(x.dtype)
    m2 = c * mx + (1 - c) * avg
    div = dec[:, 0:1] * avg + dec[:, 1:2] * m2 + dec[:, 2:3] * avg
    base = div * 1e-4 + 1.0
    norm = x / base.pow(0.75)
    out = norm if res is None else norm + res
    ss = (x * x).sum(-1)
    top = z.detach().topk(2, -1).values
    mxd, avgd = mx.detach(), avg.detach()
    cmargin = torch.where(mxd > 0, (mxd - 2.0 * avgd).abs() / mxd.clamp_min(1e-300), torch.ones_like(mxd))
    tc = None
    if tw is not None:
        tc = F.linear(out if mut == "tc_after_res" else norm, tw, tb)
    return types.SimpleNamespace(out=out, ys=ys, idx=own, used=use, nrm=ss if mut == "nrm_nosqrt" else ss.sqrt(),
                                 tc=tc, cond=cond, zgap=top[:, 0] - top[:, 1], cmargin=cmargin, z=z,
                                 avg=avgd, m2=m2.detach(), base=base.detach(), W=W, pad=pad)


def backward(x, hpre, W2, b2, gumbel, gy, idx, *, mut=None, exact_dead=True):
    """Returns dx, dhpre, dW2, db2, the ys it used, and `dead` (rows,), see the module docstring.  exact_dead =
    False leaves autograd's rounding noise on the dead rows: the float32 yardstick's own."""
    lx, lh, lW, lb = (t.detach().clone().requires_grad_(True) for t in (x, hpre, W2, b2))
    f = forward(lx, hpre=lh, W2=lW, b2=lb, gumbel=gumbel, idx=idx, mut=mut)
    f.z.retain_grad()
    f.out.backward(gy)
    with torch.no_grad():
        dead = ~f.cond.any(-1, keepdim=True)  # dd0 = dd1 = dd2: the exact dz is 0 (module docstring)
        zero = dead & exact_dead
        dz = torch.where(zero, torch.zeros_like(f.z.grad), f.z.grad)
        dhpre = torch.where(zero, torch.zeros_like(lh.grad), lh.grad)
        dW2 = dz.t() @ (hpre if mut == "dW2_hpre" else F.silu(hpre))
        db2 = dz.sum(0)
    return types.SimpleNamespace(dx=lx.grad, dhpre=dhpre, dW2=dW2, db2=db2, ys=f.ys.detach(), dead=dead.squeeze(-1),
                                 cond=f.cond, cmargin=f.cmargin)


# ---------------------------------------------------------------------------------------------------- inputs
def _seed(tier, d, rows):
    return 100003 * d + 7 * rows + (0 if tier == "mixed" else 3)


def x_mixed(g, rows, d):
    W, _ = window(d)
    lo, hi = math.log(0.5), math.log(200.0)
    a = torch.exp(lo + (hi - lo) * torch.rand(rows, 1, generator=g, dtype=torch.float64))
    sign = torch.where(torch.rand(rows, d, generator=g) < 0.5, -1.0, 1.0).double()
    x = a * sign * (0.7 + 0.6 * torch.rand(rows, d, generator=g, dtype=torch.float64))
    c = torch.tensor([0.0, 0.3, 1.0])[torch.randint(0, 3, (rows, 1), generator=g)]
    x = torch.where(torch.rand(rows, d, generator=g) < c / W, 4.0 * x, x)
    legacy = 3.0 * torch.randn(d, generator=g, dtype=torch.float64)
    if rows >= 3:
        x[1] = 0.0
        x[2] = legacy
    return f32(x)


def x_ties(g, rows, d):
    mag = torch.tensor([33.0, 51.0, 69.0, 93.0], dtype=torch.float64)[torch.randint(0, 4, (rows, d), generator=g)]
    return mag * torch.where(torch.rand(rows, d, generator=g) < 0.5, -1.0, 1.0).double()


@functools.lru_cache(maxsize=3)
def data(tier, d, rows):
    """Every operand of a case, float64 holding fp32 values."""
    g = gen(_seed(tier, d, rows))
    x = x_mixed(g, rows, d) if tier == "mixed" else x_ties(g, rows, d)

    def rn(*shape):
        return torch.randn(*shape, generator=g, dtype=torch.float32).double()

    t = types.SimpleNamespace(tier=tier, d=d, rows=rows, x=x)
    t.b2 = f32(0.2 * rn(3))
    t.modes = torch.arange(rows) % 3 if tier == "mixed" else torch.ones(rows, dtype=torch.long)
    target = F.one_hot(t.modes, 3).double() + 0.3 * rn(rows, 3).clamp(-1.0, 1.0)
    t.logits = f32(target - t.b2)
    t.hpre = rn(rows, d)
    t.W2 = f32(0.4 * rn(3, d))
    t.gumbel = f32(target - F.linear(F.silu(t.hpre), t.W2, t.b2))  # z = target + cv on the hpre / W2 logits
    t.res = rn(rows, d)
    t.tw = f32(rn(3, d) / math.sqrt(d))
    t.tb = f32(0.2 * rn(3))
    t.gy = rn(rows, d)
    t.old = rn(rows, d)
    return t


def cast32(v):
    return v.float() if torch.is_tensor(v) and v.dtype == torch.float64 else v


def fwd_pair(t, form, **kw):
    """(float64, float32) forward of a case; form 'logits' (controlled modes) or 'hpre' (modes as they fall)."""
    a = dict(b2=t.b2, **kw)
    if form == "logits":
        a["logits"] = t.logits
    else:
        a.update(hpre=t.hpre, W2=t.W2)
    r64 = forward(t.x, **a)
    with torch.no_grad():
        r32 = forward(t.x.float(), idx=r64.idx, **{k: cast32(v) for k, v in a.items()})
    return r64, r32


def keep_fwd(r64, form, tier="mixed"):
    """Rows whose out is compared (and whose idx must match); the ties tier leaves out nothing."""
    if tier == "ties":
        return torch.ones(r64.idx.shape[0], dtype=torch.bool)
    keep = ~((r64.idx == 1) & (r64.cmargin < CMARGIN_MIN).any(-1))
    if form != "logits":
        keep &= r64.zgap >= ZGAP_MIN
    return keep


def bwd_pair(t, mut=None):
    """(float64, float32, keep, gy) backward of a case: modes as in `t.modes`, gy zeroed on the rows left out."""
    with torch.no_grad():
        f = forward(t.x, hpre=t.hpre, W2=t.W2, b2=t.b2, gumbel=t.gumbel)
    keep = ~(f.cmargin < CMARGIN_MIN).any(-1) | (t.tier == "ties")
    gy = t.gy * keep.unsqueeze(-1)
    r64 = backward(t.x, t.hpre, t.W2, t.b2, t.gumbel, gy, f.idx, mut=mut)
    r32 = backward(*(v.float() for v in (t.x, t.hpre, t.W2, t.b2, t.gumbel, gy)), f.idx, exact_dead=False)
    r64.idx = f.idx
    return r64, r32, keep, gy


# ---------------------------------------------------------------------------------------------------- metric
def _rows2(v):
    v = v.detach().double().cpu()
    return v.unsqueeze(-1) if v.dim() == 1 else v


def row_err(got, ref, keep=None, cols=None, absolute=False):
    """max over the kept rows of max_f |got - ref| / max_f |ref| (cols: the features that count in the numerator)."""
    got, ref = _rows2(got), _rows2(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    den = ref.abs().amax(-1)
    den = torch.where(den == 0, torch.ones_like(den), den)
    if absolute:
        den = torch.ones_like(den)
    diff = (got - ref).abs()
    if cols is not None:
        diff = diff[:, cols]
    e = diff.amax(-1) / den
    if keep is not None:
        e = e[keep]
    return float(e.max()) if e.numel() else 0.0


def all_err(got, ref):
    """ref_check.rel: relative to the largest entry of the reference; absolute if the reference is all 0."""
    ref = ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return rel(got, ref) if float(ref.abs().max()) > 0 else float(got.detach().double().cpu().abs().max())


def edge_cols(d):
    _, pad = window(d)
    return list(range(pad)) + list(range(d - pad, d))


def fwd_errors(got, r64, keep, d):
    """got: anything with out / ys / nrm / tc (None or missing: not compared) -> {name: error}."""
    e = {}
    if getattr(got, "out", None) is not None:
        e["out"] = row_err(got.out, r64.out, keep)
        e["edge"] = row_err(got.out, r64.out, keep, cols=edge_cols(d))
    if getattr(got, "ys", None) is not None:
        e["ys"] = row_err(got.ys, r64.ys, keep, absolute=True)
    if getattr(got, "nrm", None) is not None:
        e["nrm"] = row_err(got.nrm, r64.nrm, None)
    if getattr(got, "tc", None) is not None and r64.tc is not None:
        e["tc"] = row_err(got.tc, r64.tc, keep)
    return e


def bwd_errors(got, r64, keep, old=None):
    """got: anything with dx / dhpre / dW2 / db2; old: what dx held before an acc = 1 call."""
    dx = r64.dx if old is None else r64.dx + old
    return {"dx": row_err(got.dx, dx, keep),
            "dhpre": row_err(got.dhpre, r64.dhpre, keep & ~r64.dead),
            "dhpre0": row_err(got.dhpre, r64.dhpre, keep & r64.dead, absolute=True),
            "dW2": all_err(got.dW2, r64.dW2), "db2": all_err(got.db2, r64.db2)}


FLOORS = dict(out=FWD_TRANS, edge=FWD_TRANS, ys=FWD_TRANS, nrm=FWD_TRANS, tc=FWD_TRANS, dx=BWD_TRANS, dhpre=BWD_TRANS,
              dhpre0=BWD_TRANS, dW2=BWD_TRANS, db2=BWD_TRANS)


def bounds(e32):
    return {k: max(FLOORS[k], 20.0 * v) for k, v in e32.items()}


def check(label, e, e32):
    """Prints e, e32 and the bound of every output, then asserts e <= bound for all.  Returns the rows."""
    b = bounds(e32)
    rows = [(f"{label}.{k}", e[k], e32[k], b[k]) for k in e]
    for name, a, c, bd in rows:
        print(f"ABBYREF {name:<52s} e={a:.2e} e32={c:.2e} bound={bd:.2e}")
    bad = [r for r in rows if not r[1] <= r[3]]
    assert not bad, bad
    return rows
