"""Attention with per-sample query and key lengths on the GPU: asrx_lattn_fwd / asrx_lattn_bwd (the LENS
instantiations of the kernels of csrc/attn_mf.hip and csrc/attn.hip), ops.attention(lens=) and attention.run(lens=).

The C-ABI is called directly on the ragged cases of attn_lens_cases.py, in buffers built as in
test_gpu_attn_ref.py (inputs NaN outside each sample's live rows, outputs a sentinel, spare rows, the kvpad gaps):

- bit identity: sample b's live O, lse, dQ, dK, dV are torch.equal to asrx_attn_fwd2 / asrx_attn_bwd2 run at B = 1,
  Lq = q_len, Lk = k_len on views of the same input buffers (no float atomics in these kernels);
- bounds: the same live values pass attn_ref's elementwise err / bound <= 1 and its lse tolerance per sample
  (proven for these inputs on the CPU by test_attn_lens_ref.py);
- dead regions: O, lse, dQ rows in [q_len, Lq) and dK, dV rows in [k_len, Lk) are zero and finite, although every
  dead input row holds NaN; spare rows, gaps and the words past B*H*Lq of lse and delta_ws keep the sentinel;
- zero and out-of-range lengths: the table {(70, 130), (0, 130), (70, 0), (999, -5)} at a (70, 130) launch.  The
  last entry clamps to (70, 0).  Every address these rows can form lies inside the buffers of the test.

Then the ops.attention plumbing and attention.run's pad invariance (see those tests).
"""
import faulthandler
import math

import pytest
import torch

import attn_lens_cases as L
import attn_ref as R
import test_gpu_attn_ref as G

pytestmark = pytest.mark.gpu

SENTINEL = G.SENTINEL


@pytest.fixture(autouse=True)
def _time_limit():
    """Each case has its own limit: a hung kernel ends the run instead of holding the GPU."""
    faulthandler.dump_traceback_later(60, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _inputs(lay, B, Lq, Lk, H, hd, dtypes, dev):
    """q, k, v, dO batch views (B, L, H, hd), NaN everywhere."""
    nan = float("nan")
    ins, kvbuf = {}, None
    for name, n in (("q", Lq), ("k", Lk), ("v", Lk), ("dO", Lq)):
        if lay == "kvpad" and name in ("k", "v"):
            if kvbuf is None:
                kvbuf = G._alloc(lay, B, n, H, hd, dtypes[name], nan, dev, pair=True)
            ins[name] = G._view(kvbuf, lay, n, H, hd, half=("k", "v").index(name))
        else:
            ins[name] = G._view(G._alloc(lay, B, n, H, hd, dtypes[name], nan, dev), lay, n, H, hd)
    return ins


class _Outputs:
    """o, dq, dk, dv in sentinel-filled buffers of the layout, lse and delta_ws with 8 spare words."""

    def __init__(self, lay, B, Lq, Lk, H, hd, odt, dev):
        self.obuf = G._alloc(lay, B, Lq, H, hd, odt, SENTINEL, dev)
        self.dqbuf = G._alloc(lay, B, Lq, H, hd, torch.float32, SENTINEL, dev)
        if lay == "kvpad":
            self.dkbuf = self.dvbuf = G._alloc(lay, B, Lk, H, hd, torch.float32, SENTINEL, dev, pair=True)
            self.mk_dk = lambda b: G._view(b, lay, Lk, H, hd, half=0)
            self.mk_dv = lambda b: G._view(b, lay, Lk, H, hd, half=1)
        else:
            self.dkbuf = G._alloc(lay, B, Lk, H, hd, torch.float32, SENTINEL, dev)
            self.dvbuf = G._alloc(lay, B, Lk, H, hd, torch.float32, SENTINEL, dev)
            self.mk_dk = self.mk_dv = lambda b: G._view(b, lay, Lk, H, hd)
        self.mk_q = lambda b: G._view(b, lay, Lq, H, hd)
        self.o, self.dq = self.mk_q(self.obuf), self.mk_q(self.dqbuf)
        self.dk, self.dv = self.mk_dk(self.dkbuf), self.mk_dv(self.dvbuf)
        self.rows = B * H * Lq
        self.lse = torch.full((self.rows + 8,), SENTINEL, device=dev)
        self.delta = torch.full((self.rows + 8,), SENTINEL, device=dev)

    def problems(self):
        out = []
        for name, buf, views in (("o", self.obuf, [self.mk_q]), ("dq", self.dqbuf, [self.mk_q]),
                                 ("dk/dv", self.dkbuf, [self.mk_dk, self.mk_dv]),
                                 ("dv", self.dvbuf, [self.mk_dk, self.mk_dv])):
            if not G._gaps_untouched(buf, views):
                out.append(f"{name}: written outside the logical rows")
        for name, t in (("lse", self.lse), ("delta_ws", self.delta)):
            if not bool((t[self.rows:] == SENTINEL).all()):
                out.append(f"{name}: written past B*H*Lq")
        return out


def _fwd_bwd(entry, prec, io, ins, out, lse, delta, table, B, H, Lq, Lk, hd, causal):
    """asrx_attn_fwd2 + asrx_attn_bwd2 (table None) or asrx_lattn_fwd + asrx_lattn_bwd on (B, L, H, hd) views."""
    from asrx import lib

    P = lib.ptr
    o, dq, dk, dv = out
    st = {n: G._st(t) for n, t in dict(ins, o=o, dq=dq, dk=dk, dv=dv).items()}
    tab = [] if table is None else [P(table)]
    scale = 1.0 / math.sqrt(hd)
    lib.call(entry[0], prec, io & 3, P(ins["q"]), st["q"][1], P(ins["k"]), st["k"][1], P(ins["v"]), st["v"][1], P(o),
             st["o"][1], P(lse), *tab, B, H, Lq, Lk, hd, int(causal), scale, lib.stream())
    lib.call(entry[1], prec, io, P(ins["q"]), st["q"][1], P(ins["k"]), st["k"][1], P(ins["v"]), st["v"][1], P(o),
             st["o"][1], P(ins["dO"]), st["dO"][1], P(lse), P(delta), P(dq), st["dq"][1], P(dk), st["dk"][1], P(dv),
             st["dv"][1], *tab, B, H, Lq, Lk, hd, int(causal), scale, lib.stream())


UNIFORM = ("asrx_attn_fwd2", "asrx_attn_bwd2")
LENS = ("asrx_lattn_fwd", "asrx_lattn_bwd")


def _run(mode, hd, io, lay, variant, causal, Lq, Lk, table, raws, live, dev):
    """One launch with the lengths `table` (the device values) and, for every sample b with live[b] = (ql, kl) not
    None, the uniform B = 1 launch on views of the same inputs.  raws[b]: make_inputs' tensors of sample b or None.
    -> (outputs of the lens call, outputs the uniform calls wrote into, problems)"""
    from asrx import lib

    B, H = len(table), L.H
    prec = 1 if mode == "perf" else 0
    some = next(r for r in raws if r is not None)
    ins = _inputs(lay, B, Lq, Lk, H, hd, {n: t.dtype for n, t in some.items()}, dev)
    for b, raw in enumerate(raws):
        if raw is not None:
            ql, kl = live[b]
            for name, n in (("q", ql), ("k", kl), ("v", kl), ("dO", ql)):
                ins[name][b, :n].copy_(raw[name][0].to(dev))
    odt = torch.bfloat16 if io & 2 else torch.float32
    got = _Outputs(lay, B, Lq, Lk, H, hd, odt, dev)
    uni = _Outputs(lay, B, Lq, Lk, H, hd, odt, dev)
    tab = torch.tensor(table, dtype=torch.int32, device=dev)
    assert tab.shape == (B, 2) and tab.is_contiguous()
    old = lib.load().asrx_set_attn_variant(variant)
    try:
        _fwd_bwd(LENS, prec, io, ins, (got.o, got.dq, got.dk, got.dv), got.lse, got.delta, tab, B, H, Lq, Lk, hd,
                 causal)
        for b in range(B):
            if live[b] is None:
                continue
            ql, kl = live[b]
            one = {n: t[b:b + 1, :(ql if n in ("q", "dO") else kl)] for n, t in ins.items()}
            outs = (uni.o[b:b + 1, :ql], uni.dq[b:b + 1, :ql], uni.dk[b:b + 1, :kl], uni.dv[b:b + 1, :kl])
            _fwd_bwd(UNIFORM, prec, io, one, outs, uni.lse[b * H * Lq:], uni.delta[b * H * Lq:], None, 1, H, ql, kl, hd,
                     causal)
        torch.cuda.synchronize()
    finally:
        lib.load().asrx_set_attn_variant(old)
    return got, uni, got.problems()


def _check_sample(tag, b, got, uni, ql, kl, Lq, Lk, H, problems):
    """Bit identity of sample b's live region with its uniform call; zeros on its dead rows."""
    lse = got.lse[:got.rows].view(-1, H, Lq)[b]
    pairs = [("O", got.o[b], uni.o[b], ql), ("dQ", got.dq[b], uni.dq[b], ql), ("dK", got.dk[b], uni.dk[b], kl),
             ("dV", got.dv[b], uni.dv[b], kl)]
    for name, g, u, n in pairs:
        if not torch.equal(g[:n], u[:n]):
            bad = int((g[:n] != u[:n]).any(-1).any(-1).nonzero()[0]) if n else -1
            problems.append(f"{tag} sample {b}: live {name} differs from the uniform call (first at row {bad})")
        dead = g[n:]
        if not (bool(torch.isfinite(dead.float()).all()) and bool((dead == 0).all())):
            problems.append(f"{tag} sample {b}: dead {name} rows [{n}, ..) are not zero")
    ulse = uni.lse[b * H * Lq:b * H * Lq + H * ql].view(H, ql)
    if not torch.equal(lse[:, :ql], ulse):
        problems.append(f"{tag} sample {b}: live lse differs from the uniform call")
    if not (bool(torch.isfinite(lse[:, ql:]).all()) and bool((lse[:, ql:] == 0).all())):
        problems.append(f"{tag} sample {b}: dead lse rows are not zero")


@pytest.mark.parametrize("rag", L.RAGGED, ids=[r.id for r in L.RAGGED])
def test_lens_kernels(cuda, rag):
    """Measured worst err / bound of the live values: the uniform kernels' own figures (the values are theirs, bit
    for bit); DESIGN.md, attention section."""
    (Lq, Lk), lens = rag.extents, rag.lens
    samples = [L.sample(c) for c in rag.samples]
    got, uni, problems = _run(rag.mode, rag.hd, rag.io, rag.layout, rag.variant, rag.causal, Lq, Lk,
                              [list(x) for x in lens], [s[0] for s in samples], list(lens), cuda)
    for b, ((ql, kl), case, (raw, vis, ref)) in enumerate(zip(lens, rag.samples, samples)):
        _check_sample(rag.id, b, got, uni, ql, kl, Lq, Lk, L.H, problems)
        mine = {"O": got.o[b:b + 1, :ql], "dQ": got.dq[b:b + 1, :ql], "dK": got.dk[b:b + 1, :kl],
                "dV": got.dv[b:b + 1, :kl]}
        mine = {n: t.detach().double().cpu() for n, t in mine.items()}
        for name, (r, idx) in R.ratios(mine, ref).items():
            print(f"{rag.id} sample {b} ({ql}, {kl}) {name} {r:.3f}")
            if not r <= 1.0:
                problems.append(f"sample {b}: err / bound {r:.3g} at {R.where(case, name, idx)}")
        lse = got.lse[:got.rows].view(-1, L.H, Lq)[b:b + 1, :, :ql].double().cpu()
        tol = R.lse_tolerance(case, vis, ref["lse"])
        e = (lse - ref["lse"]).abs()
        worst = float(e.max()) if bool(torch.isfinite(e).all()) else math.inf
        print(f"{rag.id} sample {b} ({ql}, {kl}) lse {worst:.3g} (tolerance {tol:.3g})")
        if not worst < tol:
            problems.append(f"sample {b}: lse off by {worst:.3g} (tolerance {tol:.3g})")
    assert not problems, rag.id + ": " + "; ".join(problems)


@pytest.mark.parametrize("mode,hd", [("perf", 64), ("parity", 128)])
def test_zero_and_clamped_lengths(cuda, mode, hd):
    """Lengths of zero, above the extent and below zero: sample 0 matches its uniform call, every output of the
    other samples is zero and finite (their inputs are NaN throughout), nothing outside the logical rows is
    written."""
    Lq, Lk = 70, 130
    table = [[70, 130], [0, 130], [70, 0], [999, -5]]
    case = R.Case(mode, 1, L.H, Lq, Lk, hd, False)
    raw, vis, ref = L.sample(case)
    got, uni, problems = _run(mode, hd, 0, "contig", 1, False, Lq, Lk, table, [raw, None, None, None],
                              [(Lq, Lk), None, None, None], cuda)
    _check_sample("zero", 0, got, uni, Lq, Lk, Lq, Lk, L.H, problems)
    mine = {"O": got.o[:1], "dQ": got.dq[:1], "dK": got.dk[:1], "dV": got.dv[:1]}
    for name, (r, idx) in R.ratios({n: t.double().cpu() for n, t in mine.items()}, ref).items():
        print(f"zero lengths {mode} hd {hd} sample 0 {name} {r:.3f}")
        if not r <= 1.0:
            problems.append(f"sample 0: err / bound {r:.3g} at {R.where(case, name, idx)}")
    lse = got.lse[:got.rows].view(-1, L.H, Lq)
    for b in (1, 2, 3):
        for name, t in (("O", got.o[b]), ("dQ", got.dq[b]), ("dK", got.dk[b]), ("dV", got.dv[b]), ("lse", lse[b])):
            if not (bool(torch.isfinite(t).all()) and bool((t == 0).all())):
                problems.append(f"sample {b} {table[b]}: {name} is not all zero")
    assert not problems, "; ".join(problems)


# ---------------------------------------------------------------------------------------------- ops.attention

@pytest.mark.parametrize("stored", [False, True])
def test_ops_attention_lens(cuda, stored):
    """ops.attention(lens=) in the perf mode on test_ops_attention_plumbing's two configurations (k and v the halves
    of one kv buffer; the output stored bf16 with its gradient through the output's sink and a forked q) against a
    per-sample loop of ops.attention on slices: live forward rows and live rows of the q / k / v gradients are
    torch.equal, dead gradient rows are zero, NaN in the dead rows of the incoming gradient changes nothing, and a
    full-length lens is torch.equal to lens=None."""
    from asrx import ops, prec

    c = R.Case("perf", 2, 3, 257, 192, 64, False, "flat", 2) if stored else R.Case("perf", 2, 3, 257, 192, 64, False,
                                                                                    "unit", 0, "kvpad")
    raw, _ = R.make_inputs(c)
    q_lens, k_lens = (100, 257), (192, 65)
    D = c.H * c.hd
    dO = raw["dO"].to(cuda).reshape(c.B, c.Lq, D)
    dO_nan = dO.clone()
    for b in range(c.B):
        dO_nan[b, q_lens[b]:] = float("nan")

    def run(lens, gO, rows=None):
        """-> (y, q.grad, kv.grad); rows: None the whole batch, or (b, ql, kl) one sample's slices"""
        q = raw["q"].to(cuda).requires_grad_(True)
        kv = torch.stack([raw["k"], raw["v"]], 2).to(cuda).requires_grad_(True)  # (B, Lk, 2, H, hd)
        ys = []
        for b, ql, kl in ([(slice(None), c.Lq, c.Lk)] if rows is None else rows):
            b = b if isinstance(b, slice) else slice(b, b + 1)
            qs = q[b, :ql]
            qf = ops.fork(qs) if stored else qs
            y = ops.attention(qf, kv[b, :kl, 0], kv[b, :kl, 1], False, out_bf16=stored, merge_heads=True, lens=lens)
            assert y.dtype == (torch.bfloat16 if stored else torch.float32)
            if stored:
                buf, acc = ops.sink_of(y).target(y)
                assert acc == 0
                buf.copy_(gO[b, :ql])
                y.backward(torch.zeros_like(y))
            else:
                y.backward(gO[b, :ql].contiguous())
            ys.append(y.detach())
        torch.cuda.synchronize()
        return ys, q.grad, kv.grad

    with prec.precision("bf16"):
        lens = ops.attn_lens(q_lens, k_lens)
        assert lens.table.dtype == torch.int32 and lens.table.tolist() == [[100, 192], [257, 65]]
        (y,), gq, gkv = run(lens, dO)
        (y2,), gq2, gkv2 = run(lens, dO_nan)
        ys, lq, lkv = run(None, dO, [(b, q_lens[b], k_lens[b]) for b in range(c.B)])
        (yf,), fq, fkv = run(ops.attn_lens((257, 257), (192, 192)), dO)
        (yn,), nq, nkv = run(None, dO)
    assert torch.equal(y, y2) and torch.equal(gq, gq2) and torch.equal(gkv, gkv2)  # NaN in dead dO rows
    assert torch.equal(yf, yn) and torch.equal(fq, nq) and torch.equal(fkv, nkv)  # full length: the uniform path
    for b in range(c.B):
        ql, kl = q_lens[b], k_lens[b]
        assert torch.equal(y[b, :ql], ys[b][0]), f"forward, sample {b}"
        assert torch.equal(gq[b, :ql], lq[b, :ql]), f"q.grad, sample {b}"
        assert torch.equal(gkv[b, :kl], lkv[b, :kl]), f"k.grad / v.grad, sample {b}"
        assert not gq[b, ql:].any() and not gkv[b, kl:].any() and not y[b, ql:].any(), f"dead rows, sample {b}"
        assert not lq[b, ql:].any() and not lkv[b, kl:].any()
    assert bool(torch.isfinite(gq).all()) and bool(torch.isfinite(gkv).all()) and bool(torch.isfinite(y.float()).all())
    assert not torch.equal(y[1], yn[1])  # the lengths do something: sample 1 sees 65 of 192 keys


def test_attn_lens_arguments(cuda):
    from asrx import ops

    with pytest.raises(TypeError):
        ops.attn_lens(torch.tensor([3, 4], device=cuda))
    with pytest.raises(TypeError):
        ops.attn_lens([3, 4], torch.tensor([3, 4], device=cuda))
    with pytest.raises(TypeError):
        ops.attn_lens([3.5, 4])
    for bad in ([3, 0], [-1, 2], []):
        with pytest.raises(ValueError):
            ops.attn_lens(bad)
    with pytest.raises(ValueError):
        ops.attn_lens([3, 4], [5])
    s = ops.attn_lens(torch.tensor([3, 4]))
    assert s.q_lens == s.k_lens == (3, 4) and s.B == 2 and s.table.tolist() == [[3, 3], [4, 4]]
    x = ops.attn_lens((3, 4), [5, 6])
    assert x.k_lens == (5, 6) and x.table.device.type == "cuda" and x.pairs() == 39
    q = torch.zeros(2, 4, 2, 64, device=cuda)
    k = torch.zeros(2, 6, 2, 64, device=cuda)
    for lens, kk in ((ops.attn_lens([3, 4, 4], [5, 6, 6]), k), (ops.attn_lens([3, 5], [5, 6]), k),
                     (ops.attn_lens([3, 4], [5, 7]), k), (x, k[:, :5])):
        with pytest.raises(ValueError):
            ops.attention(q, kk, kk, False, lens=lens)


# ---------------------------------------------------------------------------------------------- attention.run

def _pad_runs(att, noise, mode, call, x_shape, x_len, xa_shape, xa_len, lens, dev):
    """The call with the pad rows of x (and xa) holding zeros, then N(0, 10^2) noise -> [(live out, x.grad live,
    xa.grad live)] of the two runs; the loss is a fixed weighting of the live output rows only."""
    from asrx import prec

    g = torch.Generator().manual_seed(11)
    x0 = torch.randn(x_shape, generator=g)
    xa0 = torch.randn(xa_shape, generator=g) if xa_shape else None
    w = torch.randn(x_shape, generator=g).to(dev)
    pad_x, pad_xa = 10.0 * torch.randn(x_shape, generator=g), (10.0 * torch.randn(xa_shape, generator=g)
                                                               if xa_shape else None)
    live = (torch.arange(x_shape[1])[None, :] < torch.tensor(x_len)[:, None]).to(dev)
    live_a = (torch.arange(xa_shape[1])[None, :] < torch.tensor(xa_len)[:, None]).to(dev) if xa_shape else None
    out = []
    for noisy in (False, True):
        x = torch.where(live[..., None], x0.to(dev), pad_x.to(dev) if noisy else torch.zeros((), device=dev))
        x.requires_grad_(True)
        xa = None
        if xa_shape:
            xa = torch.where(live_a[..., None], xa0.to(dev), pad_xa.to(dev) if noisy else torch.zeros((), device=dev))
            xa.requires_grad_(True)
        with prec.precision(mode):
            y = call(att, x, xa, noise, lens)
            (y * w * live[..., None]).sum().backward()
        torch.cuda.synchronize()
        out.append((y.detach()[live], x.grad[live], xa.grad[live_a] if xa_shape else None))
    return out


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_attention_run_pad_invariance(cuda, mode):
    """attention.run on a zero-padded batch: with lens, the live output rows and the live rows of the data gradients
    do not depend on what the pad rows hold (torch.equal; data gradients carry no atomics); without lens they do,
    which shows the test sees what it is for.  The causal self call is the exception to the second half: a live
    causal query sees no pad key, and the pad queries carry a zero output gradient (the loss is over live rows), so
    there the pad rows cannot show with or without lens, and only the first half is asserted.  Parameter gradients
    sum with atomics and are not compared."""
    from asrx import ops
    from asrx.model import attention
    from asrx.noise import NoiseCtx

    torch.manual_seed(0)
    att = attention(128, 2, 4, n_type="AbbyNormal").to(cuda).train()
    noise = NoiseCtx(3, 1, True)

    def self_call(masked):
        return lambda a, x, xa, nz, lens: a.run(x, None, nz, "t.sa", 0, masked, lens=lens)

    def cross_call(a, x, xa, nz, lens):
        return a.run(x, a.project_kv(xa, nz, "t.ca", 0, False), nz, "t.ca", 0, False, lens=lens)

    for what, call, xs, xl, xas, xal in (("self", self_call(False), (2, 70, 128), (70, 33), None, None),
                                         ("causal self", self_call(True), (2, 70, 128), (70, 33), None, None),
                                         ("cross", cross_call, (2, 9, 128), (9, 4), (2, 70, 128), (70, 33))):
        lens = ops.attn_lens(xl, xal)
        a, b = _pad_runs(att, noise, mode, call, xs, xl, xas, xal, lens, cuda)
        for name, s, t in zip(("output", "x.grad", "xa.grad"), a, b):
            if s is not None:
                assert bool(torch.isfinite(s.float()).all()), (what, name)
                assert torch.equal(s, t), f"{mode} {what}: live {name} depends on the pad rows"
        a, b = _pad_runs(att, noise, mode, call, xs, xl, xas, xal, None, cuda)
        if what != "causal self":  # a causal query sees no pad key: only the non-causal calls must differ
            assert not torch.equal(a[0], b[0]), f"{mode} {what}: without lens the pad rows should show"
        assert not torch.equal(a[1], b[1]) or what == "causal self"
