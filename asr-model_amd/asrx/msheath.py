"""MSheath.forward (model.py:429-507) as ONE autograd node with a hand-written backward.

Composed from per-op autograd Functions, a MSheath call leaves autograd to sum the gradient of every
activation with several consumers -- each layer's input feeds v_gate, the LayerNorm, the x + g*ion*out
update and the jump select, the original input feeds every layer's jump and the policy pooling -- which
cost ~30 full-size add kernels per call in the backward (~14 ms of the tiny
step).  MSheathFn runs the forward below, then walks the layers backwards with every contribution to a
layer input landing in one buffer: written by its first producer (the jump-select pass-through of
inactive samples, the x_new backward of active ones), accumulated by the rest (the fused row backward,
v_gate's input GEMM with beta = 1), and the original input's jump gradient kept apart until one final
pass.  Parameter gradients go straight into p.grad (asrx.ops direct-gradient convention).  Batch-1
semantics per sample exactly as asrx.model.MSheath.run_composed (masked per-sample trajectories, no
host syncs).

Per layer the forward is 6-8 launches instead of the composed path's 17: v_gate's two projections as
one GEMM against [normalize(mkey); mlp[0].weight] (asrx_vgate_weights builds it and its bf16 copy),
one row pass for LayerNorm + |x| + gate + v_gate (asrx_msheath_row_fwd), the adapter GEMM (even
layers), x_new with the per-sample mem mean in the same pass (asrx_axpy_row2_colsum), the control step
with mem_gate inside it (asrx_msheath_ctrl_fwd3) and the jump select.  The backward mirrors it
(asrx_msheath_row_bwd, asrx_msheath_ctrl_bwd3, one dgrad GEMM against the same combined weight).
"""
from __future__ import annotations

import ctypes
import math

import torch

from . import gemm as G
from . import decisions, lib, ops, prec

_E = torch.empty
_P = lib.ptr
_S = lib.stream
SIG = G.ACT["sigmoid"]
SILU = G.ACT["silu"]

_REC = None

ROW_DIMS = (128, 256, 384, 512, 768, 1024)  # the fused row kernels' register-resident widths

# The backward's per-sample jump sums (dalpha, dbeta, dgam) as ordered partial sums instead of float
# atomics: with it no float atomic feeds the data gradient, so a whole backward is bit-reproducible
# (tests/test_gpu_fusions.py).  False: the atomic form (kept for A/B diagnostics).
DETERMINISTIC = True
# A layer without adapter (its update is px itself) forms x_new and the per-chunk column sums in its row pass
# (asrx_msheath_row_fwd3) instead of a separate asrx_axpy_row2_colsum launch.  False: the two-launch form.
ROW_COLSUM = __import__("os").environ.get("ASRX_ROW_COLSUM", "1") != "0"
# The layer backward with fewer layer-sized passes: the jump backward stores no dxn = alpha g (the x_new backward takes
# g and alpha, asrx_axpy_row2_bwd_acc2); on a layer without adapter the row backward forms g' = alpha g + g_mem / L
# itself and does the x_new backward on a recomputed px (asrx_msheath_row_bwd2 mode 2: no asrx_axpy_row2_bwd_acc launch,
# and the forward stores no px there); v_gate's two weight gradients are one launch (gemm.wgrad_cols2).  False: the
# six-step form.
BWD_FUSED = __import__("os").environ.get("ASRX_MSHEATH_BWD_FUSED", "1") != "0"
# Measurement only (DESIGN.md §7 measures BWD_FUSED's weight-gradient part apart with it; nothing else sets it).
WGRAD_MERGED = __import__("os").environ.get("ASRX_MSHEATH_WGRAD_MERGED", "1") != "0"


def _rec_bytes():
    global _REC
    if _REC is None:
        _REC = int(lib.load().asrx_msheath_rec_bytes())
    return _REC


def supported(mod, D):
    """The fused path covers these widths (msheath_row_* kernels); others run MSheath.run_composed."""
    return D in ROW_DIMS and all(lay["v_gate"].mkey.shape[0] <= 64 for lay in mod.layers)


def _params(mod):
    """Every parameter MSheathFn reads, in a fixed order (tx is a frozen buffer-like parameter)."""
    ps = [mod.pnet.net[0].weight, mod.pnet.net[0].bias, mod.pnet.net[2].weight, mod.pnet.net[2].bias, mod.mem_w,
          mod.mem_gate[0].weight, mod.mem_gate[0].bias, mod.jump_s, mod.mlp_gate[0].weight, mod.mlp_gate[0].bias,
          mod.mlp_ln.weight, mod.mlp_ln.bias, mod.mlp[0].weight, mod.mlp[0].bias, mod.mlp[2].weight, mod.mlp[2].bias]
    for i, lay in enumerate(mod.layers):
        vg = lay["v_gate"]
        ps += [lay["ln"].weight, lay["ln"].bias, lay["gate"][0].weight, lay["gate"][0].bias, vg.mkey, vg.mval,
               vg.mlp[0].weight, vg.mlp[0].bias, vg.mlp[2].weight, vg.mlp[2].bias, vg.concat.weight, vg.concat.bias]
        if lay["adapter"] is not None:
            ps += [lay["adapter"].weight, lay["adapter"].bias]
    return ps


ACT_SOFTMAX = 16  # csrc/common.h


def _live_lens(lens, x):
    """lens of a MSheath call on x (B, L, D) -> None when absent or every sample is full length (today's calls and
    kernels, untouched), else lens after the checks of the LENS path: a call it cannot take is an error, never a
    fall-back to kernels that would ignore the lengths."""
    if lens is None:
        return None
    if not isinstance(lens, ops.SeqLens):
        raise TypeError(f"msheath: lens must come from ops.seq_lens, got {type(lens).__name__}")
    if x.dim() != 3:
        raise ValueError(f"msheath: lens needs a (B, L, D) tensor, got {tuple(x.shape)}")
    if lens.check(x.shape[0], x.shape[1], x.device):  # wrong count, a length above L: ValueError
        return None
    if not DETERMINISTIC:
        raise ValueError("msheath: lens needs the ordered jump sums (msheath.DETERMINISTIC is False)")
    if decisions.active():
        raise ValueError("msheath: lens with an active asrx.decisions recorder is not supported")
    if x.shape[-1] not in ROW_DIMS:
        raise ValueError(f"msheath: lens needs a width in {ROW_DIMS}, got {x.shape[-1]}")
    return lens


def forward(mod, x0, gpol, save, tag=None, lens=None, vetted=False):
    """MSheath forward on (B, L, D) x0 with policy noise gpol (B, layers, 3).  Returns (out, saved).
    tag: (noise site key, sid_base) of the call, for asrx.decisions.
    lens (ops.SeqLens; None or all-full: the calls below unchanged): sample b's rows [0, T_b) come out as for
    x0[b:b+1, :T_b] alone, the pooled, mem and ion means taken over them; rows at or past T_b are not read (those of
    x0 must be finite: the GEMMs pass over them) and are zeros in everything stored."""
    if not vetted:  # (msheath() and MSheathFn hand over what _live_lens returned)
        lens = _live_lens(lens, x0)
    lt = lens.table if lens is not None else None
    B, L, D = x0.shape
    rows = B * L
    dev = x0.device
    st = _S()
    sv = {} if save else None
    # policy = softmax(MPNet(mean_l x))            model.py:432-435, 375-385
    nchunk = int(lib.load().asrx_mem_chunks(L))
    part = _E(len(mod.layers) + 1, B, nchunk, D, device=dev)  # row-chunk column sums (deterministic means)
    pooled = _E(B, D, device=dev)
    if lt is not None:
        lib.call("asrx_seg_colsum_lens_det", _P(x0), _P(part[-1]), _P(pooled), _P(lt), B, L, D, st)
    else:
        lib.call("asrx_seg_colsum_det", _P(x0), _P(part[-1]), _P(pooled), B, L, D, 1.0 / L, st)
    net = mod.pnet.net
    zp = _E(B, net[0].weight.shape[0], device=dev) if save else None
    hp = G.linear_fwd(pooled, net[0].weight, net[0].bias, act="silu", preact=zp)
    policy = _E(B, 3, device=dev)  # softmax(net[2](hp)) in one launch (act 16: the row softmax)
    lib.call("asrx_small_linear_fwd", _P(hp), _P(net[2].weight), _P(net[2].bias), _P(policy), B, hp.shape[1], 3,
             ACT_SOFTMAX, st)
    nl = len(mod.layers)
    wide = G.use_wide(D)
    mg = mod.mem_gate[0]
    mem_w, ld_mw = mod.mem_w, 0
    next_i = None
    x = x0
    rec_bytes = _rec_bytes()
    # the layers' small per-row / per-sample outputs live in four per-call workspaces, handed to the kernels as
    # addresses (the kernels take raw pointers): ~16 tensor allocations per layer were ~10 % of the host's issue
    # time on the host-bound small config (tools/host_prof.py)
    wsr = _E(nl, 7, rows, device=dev)                       # mean, rstd, nx, g, ion, kv, m2
    wsb = _E(nl, 5, B, device=dev)                          # alpha, beta, active, next_out, mem_v
    wsd = _E(nl, 3, B, D, device=dev)                       # gam, mwo, mem
    wsc = _E(nl, B * rec_bytes, dtype=torch.uint8, device=dev)  # control records
    a_r, a_b, a_d, a_c = wsr.data_ptr(), wsb.data_ptr(), wsd.data_ptr(), wsc.data_ptr()
    if save:
        sv["ws"] = (wsr, wsb, wsd, wsc)
        sv["bwd_fused"] = BWD_FUSED  # the backward follows what this forward stored
        sv["lens"] = lens
    inv_sqrt_d = 1.0 / math.sqrt(D)
    layers = []
    for i, lay in enumerate(mod.layers):
        vg = lay["v_gate"]
        Dh = vg.mlp[0].weight.shape[0]
        M = vg.mkey.shape[0]
        N = M + Dh
        # SH = [x normalize(mkey)^T | mlp[0](x)]     model.py:346-349

        def build(vg=vg, M=M, Dh=Dh, N=N):
            Wc, bc, mkn = _E(N, D, device=dev), _E(N, device=dev), _E(M, device=dev)
            wb = _E(N, D, dtype=torch.int16, device=dev) if wide else None
            lib.call("asrx_vgate_weights", _P(vg.mkey), _P(vg.mlp[0].weight), _P(vg.mlp[0].bias), _P(Wc), _P(bc),
                     _P(mkn), _P(wb), M, Dh, D, st)
            return Wc, bc, mkn, wb

        Wc, bc, mkn, wb = G.derived(("vgate", bool(wide)), build, (vg.mkey, vg.mlp[0].weight, vg.mlp[0].bias))
        # rows of samples not at this layer (next_i[b] != i; the reference never runs them) are skipped:
        # by whole 128-row tiles in the GEMMs, by row in the row kernels
        # (with lens: by 128-row tiles holding no live row too; layer 0 keeps the plain GEMM, as the sample alone)
        mt = G.row_tiles(next_i, i, L, rows, dev, lens=lt) if (wide and next_i is not None) else None
        SH = G.linear_fwd(x, Wc, bc, wbf=wb, mtiles=mt)
        # px = LayerNorm(x), |x|, g = sigmoid(gate(px)), ion = v_gate(x)   (346-351, 452-460)
        ln, gt = lay["ln"], lay["gate"][0]
        ad = lay["adapter"]
        # px feeds only the adapter GEMM on even layers (bf16-stored); on odd layers it is the update itself
        pxb = int(ad is not None and wide and prec.bf16_storage())
        # (not stored at all where the fused backward recomputes it: x_new is stored and px has no other reader)
        no_px = save and BWD_FUSED and ad is None and ROW_COLSUM
        px = None if no_px else _E(B, L, D, device=dev, dtype=torch.bfloat16 if pxb else torch.float32)
        mean, rstd, nx, gv, ion, kv, m2 = (a_r + 4 * rows * (7 * i + j) for j in range(7))
        # x_new = x + g * ion * out; mem = mean_l x_new   (461-463).  Without a backward x_new is not
        # materialised: the column sums are taken and the jump step below recomputes it
        x_new = _E(B, L, D, device=dev) if save else None
        if lt is not None:  # the same launches from the LENS entry points
            if ad is None and ROW_COLSUM:
                lib.call("asrx_msheath_row_lens_fwd3", _P(x), _P(ln.weight), _P(ln.bias), _P(gt.weight), _P(gt.bias),
                         _P(SH), N, _P(vg.mval), _P(vg.mlp[2].weight), _P(vg.mlp[2].bias), _P(vg.concat.weight),
                         _P(vg.concat.bias), _P(vg.tx), _P(px), _P(mean), _P(rstd), _P(nx), _P(gv), _P(ion), _P(kv),
                         _P(m2), _P(x_new), _P(part[i]), _P(lt), rows, D, M, Dh, float(ln.eps), inv_sqrt_d, _P(next_i),
                         i, L, st)
                out = px
            else:
                lib.call("asrx_msheath_row_lens_fwd2", _P(x), _P(ln.weight), _P(ln.bias), _P(gt.weight), _P(gt.bias),
                         _P(SH), N, _P(vg.mval), _P(vg.mlp[2].weight), _P(vg.mlp[2].bias), _P(vg.concat.weight),
                         _P(vg.concat.bias), _P(vg.tx), _P(px), pxb, _P(mean), _P(rstd), _P(nx), _P(gv), _P(ion),
                         _P(kv), _P(m2), _P(lt), rows, D, M, Dh, float(ln.eps), inv_sqrt_d, _P(next_i), i, L, st)
                out = G.linear_fwd(px, ad.weight, ad.bias, mtiles=mt) if ad is not None else px
                lib.call("asrx_axpy_row2_lens_colsum", _P(x), _P(gv), _P(ion), _P(out), _P(x_new), _P(part[i]), _P(lt),
                         B, L, D, _P(next_i), i, st)
        elif ad is None and ROW_COLSUM:  # out = px: the row pass forms x_new and its column sums itself
            lib.call("asrx_msheath_row_fwd3", _P(x), _P(ln.weight), _P(ln.bias), _P(gt.weight), _P(gt.bias), _P(SH),
                     N, _P(vg.mval), _P(vg.mlp[2].weight), _P(vg.mlp[2].bias), _P(vg.concat.weight),
                     _P(vg.concat.bias), _P(vg.tx), _P(px), _P(mean), _P(rstd), _P(nx), _P(gv), _P(ion), _P(kv), _P(m2),
                     _P(x_new), _P(part[i]), rows, D, M, Dh, float(ln.eps), inv_sqrt_d, _P(next_i), i, L, st)
            out = px
        else:
            lib.call("asrx_msheath_row_fwd2", _P(x), _P(ln.weight), _P(ln.bias), _P(gt.weight), _P(gt.bias), _P(SH),
                     N, _P(vg.mval), _P(vg.mlp[2].weight), _P(vg.mlp[2].bias), _P(vg.concat.weight),
                     _P(vg.concat.bias), _P(vg.tx), _P(px), pxb, _P(mean), _P(rstd), _P(nx), _P(gv), _P(ion), _P(kv),
                     _P(m2), rows, D, M, Dh, float(ln.eps), inv_sqrt_d, _P(next_i), i, L, st)
            out = G.linear_fwd(px, ad.weight, ad.bias, mtiles=mt) if ad is not None else px
            lib.call("asrx_axpy_row2_colsum", _P(x), _P(gv), _P(ion), _P(out), _P(x_new), _P(part[i]), B, L, D,
                     _P(next_i), i, st)
        # mem_v = sigmoid(mem_gate(mem)); control; jump select   (464-501)
        alpha, beta, active, next_out, mem_v = (a_b + 4 * B * (5 * i + j) for j in range(5))
        gam, mwo, mem = (a_d + 4 * B * D * (3 * i + j) for j in range(3))
        rec = a_c + B * rec_bytes * i
        gp = gpol[:, i]
        if lt is not None:
            lib.call("asrx_msheath_ctrl_lens_fwd3", _P(policy), _P(gp), gp.stride(0), _P(ion), _P(mg.weight),
                     _P(mg.bias), _P(mem_v), _P(mem_w), ld_mw, _P(part[i]), _P(mem), _P(mod.jump_s), _P(next_i), i, nl,
                     _P(lt), B, L, D, _P(alpha), _P(beta), _P(gam), _P(mwo), _P(active), _P(next_out), _P(rec), st)
        else:
            lib.call("asrx_msheath_ctrl_fwd3", _P(policy), _P(gp), gp.stride(0), _P(ion), _P(mg.weight), _P(mg.bias),
                     _P(mem_v), _P(mem_w), ld_mw, _P(part[i]), _P(mem), _P(mod.jump_s), _P(next_i), i, nl, B, L, D,
                     _P(alpha), _P(beta), _P(gam), _P(mwo), _P(active), _P(next_out), _P(rec), st)
        if tag is not None and decisions.active():
            decisions.msheath_layer(tag[0], tag[1], i, wsr[i, 4].view(B, L), wsc[i].view(torch.float32).view(B, -1))
        if save:
            x_out = _E(B, L, D, device=dev)
            if lt is not None:
                lib.call("asrx_jump_lens_select4", _P(x_new), _P(x0), _P(x), _P(active), _P(alpha), _P(beta), _P(gam),
                         _P(x_out), _P(lt), B, L, D, st)
            else:
                lib.call("asrx_jump_select4", _P(x_new), _P(x0), _P(x), _P(active), _P(alpha), _P(beta), _P(gam),
                         _P(x_out), B, L, D, st)
        else:  # one pass, in place from layer 1 on (samples not at the layer keep their rows untouched)
            x_out = _E(B, L, D, device=dev) if i == 0 else x
            if lt is not None:  # (layer 0, out of place, stores the zero pad rows; in place they stay)
                lib.call("asrx_jump_lens_axpy_inplace", _P(x), _P(x_out), _P(gv), _P(ion), _P(out), _P(x0), _P(active),
                         _P(alpha), _P(beta), _P(gam), _P(lt), B, L, D, st)
            else:
                lib.call("asrx_jump_axpy_inplace", _P(x), _P(x_out), _P(gv), _P(ion), _P(out), _P(x0), _P(active),
                         _P(alpha), _P(beta), _P(gam), B, L, D, st)
        if save:
            layers.append(dict(x=x, Wc=Wc, mkn=mkn, SH=SH, nx=nx, kv=kv, m2=m2, px=px, mean=mean, rstd=rstd,
                               out=out, g=gv, ion=ion, x_new=x_new, mem=mem, mem_v=mem_v, mem_w=mem_w, ld_mw=ld_mw,
                               rec=rec, active=active, alpha=alpha, beta=beta, next_i=next_i, mt=mt))
        mem_w, ld_mw, next_i = mwo, D, next_out
        x = x_out
    # x + sigmoid(mlp_gate(x)) * mlp(mlp_ln(x))   (503-506): the gate from the LayerNorm's row pass
    gate = _E(rows, device=dev)
    hb = int(wide and prec.bf16_storage())  # hln only feeds mlp[0]
    hln = _E(B, L, D, device=dev, dtype=torch.bfloat16 if hb else torch.float32)
    mean2, rstd2 = _E(rows, device=dev), _E(rows, device=dev)
    lib.call("asrx_layernorm_fwd3", _P(x), _P(mod.mlp_ln.weight), _P(mod.mlp_ln.bias), _P(hln), hb, _P(mean2),
             _P(rstd2), None, _P(mod.mlp_gate[0].weight), _P(mod.mlp_gate[0].bias), _P(gate), 1, rows, D,
             float(mod.mlp_ln.eps), st)
    # perf mode: the backward's GEMM recomputes mlp[0]'s pre-activation (gemm_wn_gact) -- no z1 store
    rec1 = save and G.can_recompute_act(hln, mod.mlp[0].weight, "silu")
    z1 = _E(B, L, mod.mlp[0].weight.shape[0], device=dev) if save and not rec1 else None
    a1 = G.linear_fwd(hln, mod.mlp[0].weight, mod.mlp[0].bias, act="silu", preact=z1,
                      out_bf16=prec.bf16_storage())
    hh = G.linear_fwd(a1, mod.mlp[2].weight, mod.mlp[2].bias)
    y = _E(B, L, D, device=dev)
    if lt is not None:  # pad rows of y are zeros (the tail's LayerNorm and GEMMs ran over zero rows)
        lib.call("asrx_axpy_lens_row", _P(x), _P(gate), _P(hh), _P(y), _P(lt), B, L, D, st)
    else:
        lib.call("asrx_axpy_row", _P(x), _P(gate), _P(hh), _P(y), rows, D, st)
    if save:
        sv.update(x0=x0, pooled=pooled, zp=zp, hp=hp, policy=policy, layers=layers, x=x, gate=gate, hln=hln,
                  mean2=mean2, rstd2=rstd2, z1=z1, a1=a1, hh=hh)
    return y, sv


class MSheathFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x0, gpol, mod, tag, lens, *params):
        x0 = x0 if x0.is_contiguous() else x0.contiguous()
        y, sv = forward(mod, x0, gpol, save=True, tag=tag, lens=lens, vetted=True)
        ctx.mod, ctx.sv = mod, sv
        return y

    @staticmethod
    def backward(ctx, gy):
        mod, sv = ctx.mod, ctx.sv
        ctx.sv = None
        gy = gy if gy.is_contiguous() else gy.contiguous()
        x0 = sv["x0"]
        B, L, D = x0.shape
        rows = B * L
        dev = x0.device
        st = _S()
        touched = []
        # per-sample lengths: the LENS entry points below.  g_mem / T_b and dpooled / T_b go to live rows only, every
        # sum takes live rows only, pad rows of gy are not read, and each gradient buffer's first writer stores zeros
        # in its pad rows (the tail's GEMMs, LayerNorm and weight gradients then see zero rows)
        lt = sv["lens"].table if sv["lens"] is not None else None

        def gb(p):  # accumulation target p.grad (created zeroed on first use)
            touched.append(p)
            return ops._gbuf(p, True)

        # ---- tail: y = x + gate * hh, hh = mlp2(silu(mlp0(LN(x)))), gate = sigmoid(mlp_gate(x))
        x = sv["x"]
        dx = _E(B, L, D, device=dev)
        dhh = _E(B, L, D, device=dev)
        dgate = _E(rows, device=dev)
        if lt is not None:
            lib.call("asrx_axpy_lens_row_bwd2", _P(gy), _P(sv["gate"]), _P(sv["hh"]), _P(dhh), _P(dgate), _P(dx), _P(lt),
                     B, L, D, st)
        else:
            lib.call("asrx_axpy_row_bwd2", _P(gy), _P(sv["gate"]), _P(sv["hh"]), _P(dhh), _P(dgate), _P(dx), rows, D, st)
        mg = mod.mlp_gate[0]
        lib.call("asrx_small_linear_bwd", _P(dgate), _P(sv["gate"]), _P(x), _P(mg.weight), _P(dx), _P(gb(mg.weight)),
                 _P(gb(mg.bias)), rows, D, 1, SIG, 1.0, st)
        m0, m2l = mod.mlp[0], mod.mlp[2]
        da1 = G.linear_dgrad(dhh, m2l.weight)
        G.linear_wgrad(dhh, sv["a1"], out=gb(m2l.weight), accumulate=True, db=gb(m2l.bias))
        H1 = da1.shape[-1]
        if sv["z1"] is None:  # pre-activation recomputed: gz = bf16(da1 * silu'(hln W0^T + b0)), db0 summed
            ga1 = _E(da1.shape, dtype=torch.bfloat16, device=dev)
            G.linear_gact(sv["hln"], m0.weight, m0.bias, da1, ga1, "silu", db=gb(m0.bias))
            da1 = ga1
        elif prec.get() == prec.PREC_BF16 and H1 % 8 == 0 and G.use_wide(H1):
            # perf mode: silu' applied, the gradient stored bf16 for both GEMMs, mlp[0]'s bias gradient
            # summed in the same pass
            ga1 = _E(da1.shape, dtype=torch.bfloat16, device=dev)
            lib.call("asrx_act_bwd_bias", _P(da1), _P(sv["z1"]), _P(ga1), _P(gb(m0.bias)), rows, H1, SILU, st)
            da1 = ga1
        else:
            lib.call("asrx_act_bwd", _P(da1), _P(sv["z1"]), _P(da1), da1.numel(), SILU, st)
            ops.colsum(da1.view(rows, -1), out=gb(m0.bias))
        dhln = G.linear_dgrad(da1, m0.weight)
        G.linear_wgrad(da1, sv["hln"], out=gb(m0.weight), accumulate=True)
        lib.call("asrx_layernorm_bwd_acc", _P(dhln), _P(x), _P(mod.mlp_ln.weight), _P(sv["mean2"]), _P(sv["rstd2"]),
                 _P(dx), _P(gb(mod.mlp_ln.weight)), _P(gb(mod.mlp_ln.bias)), rows, D, 1, st)
        del dhh, da1, dhln
        # ---- layers, last to first
        nl = len(mod.layers)
        g_policy = _E(B, 3, device=dev)
        has_orig = _E(B, dtype=torch.int32, device=dev)
        lib.call("asrx_zero", _P(has_orig), B * 4, st)
        dorig = _E(B, L, D, device=dev)  # written by the first jumping layer of each sample (has_orig)
        g_mwo = None
        mg_w, mg_b = mod.mem_gate[0].weight, mod.mem_gate[0].bias
        inv_sqrt_d = 1.0 / math.sqrt(D)
        fused = sv["bwd_fused"]
        for i in range(nl - 1, -1, -1):
            s = sv["layers"][i]
            lay = mod.layers[i]
            vg = lay["v_gate"]
            M, Dh = vg.mkey.shape[0], vg.mlp[0].weight.shape[0]
            N = M + Dh
            xi = s["x"]
            dxi = _E(B, L, D, device=dev)
            dxn = None if fused else _E(B, L, D, device=dev)  # fused: alpha g is formed by its consumers
            g_mem_w, g_mem = _E(B, D, device=dev), _E(B, D, device=dev)
            if lt is not None:  # (the forward refused lengths without DETERMINISTIC)
                part = _E(int(lib.load().asrx_jump_bwd_part_floats(B, L, D)), device=dev)
                lib.call("asrx_jump_lens_select4_bwd_part2", _P(dx), _P(s["x_new"]), _P(x0), _P(s["active"]),
                         _P(s["alpha"]), _P(s["beta"]), _P(has_orig), _P(dxn), _P(dorig), _P(dxi), _P(part), _P(lt),
                         B, L, D, st)
                lib.call("asrx_msheath_ctrl_lens_bwd4", _P(part), _P(lt), L, _P(g_mwo), _P(s["mem_v"]), _P(s["mem_w"]),
                         s["ld_mw"], _P(s["mem"]), _P(mod.jump_s), _P(s["rec"]), i, nl, B, D, _P(g_policy),
                         int(i != nl - 1), _P(g_mem_w), _P(g_mem), _P(gb(mod.jump_s)), _P(has_orig), _P(mg_w),
                         _P(gb(mg_w)), _P(gb(mg_b)), st)
            elif DETERMINISTIC:  # per-chunk partials summed in order by the control backward
                part = _E(int(lib.load().asrx_jump_bwd_part_floats(B, L, D)), device=dev)
                lib.call("asrx_jump_select4_bwd_part2" if fused else "asrx_jump_select4_bwd_part",
                         _P(dx), _P(s["x_new"]), _P(x0), _P(s["active"]), _P(s["alpha"]), _P(s["beta"]), _P(has_orig),
                         _P(dxn), _P(dorig), _P(dxi), _P(part), B, L, D, st)
                lib.call("asrx_msheath_ctrl_bwd4", _P(part), L, _P(g_mwo), _P(s["mem_v"]), _P(s["mem_w"]),
                         s["ld_mw"], _P(s["mem"]), _P(mod.jump_s), _P(s["rec"]), i, nl, B, D, _P(g_policy),
                         int(i != nl - 1), _P(g_mem_w), _P(g_mem), _P(gb(mod.jump_s)), _P(has_orig), _P(mg_w),
                         _P(gb(mg_w)), _P(gb(mg_b)), st)
            else:
                dctl = _E(B * (2 + D), device=dev)  # [dalpha | dbeta | dgam]: zeroed by one memset
                dalpha, dbeta, dgam = dctl[:B], dctl[B:2 * B], dctl[2 * B:]
                lib.call("asrx_jump_select4_bwd_acc2" if fused else "asrx_jump_select4_bwd_acc",
                         _P(dx), _P(s["x_new"]), _P(x0), _P(s["active"]), _P(s["alpha"]), _P(s["beta"]), _P(has_orig),
                         _P(dxn), _P(dorig), _P(dxi), _P(dalpha), _P(dbeta), _P(dgam), B, L, D, st)
                lib.call("asrx_msheath_ctrl_bwd3", _P(dalpha), _P(dbeta), _P(dgam), _P(g_mwo), _P(s["mem_v"]),
                         _P(s["mem_w"]), s["ld_mw"], _P(s["mem"]), _P(mod.jump_s), _P(s["rec"]), i, nl, B, D,
                         _P(g_policy), int(i != nl - 1), _P(g_mem_w), _P(g_mem), _P(gb(mod.jump_s)), _P(has_orig),
                         _P(mg_w), _P(gb(mg_w)), _P(gb(mg_b)), st)
            ad = lay["adapter"]
            mode = 2 if fused and ad is None else 0  # asrx_msheath_row_bwd2's mode
            dout = dgv = dion = None
            if lt is not None and (not fused or ad is not None):  # one entry point, alpha when g arrives unscaled
                dout = _E(B, L, D, device=dev)
                dgv, dion = _E(rows, device=dev), _E(rows, device=dev)
                lib.call("asrx_axpy_row2_lens_bwd_acc2", _P(dx if fused else dxn), _P(s["alpha"]) if fused else None,
                         _P(g_mem), _P(s["active"]), _P(s["g"]), _P(s["ion"]), _P(s["out"]), _P(dout), _P(dgv),
                         _P(dion), _P(dxi), _P(lt), B, L, D, st)
            elif lt is not None:
                pass
            elif not fused:
                dout = _E(B, L, D, device=dev)
                dgv, dion = _E(rows, device=dev), _E(rows, device=dev)
                lib.call("asrx_axpy_row2_bwd_acc", _P(dxn), _P(g_mem), 1.0 / L, _P(s["active"]), _P(s["g"]),
                         _P(s["ion"]), _P(s["out"]), _P(dout), _P(dgv), _P(dion), _P(dxi), B, L, D, st)
            elif ad is not None:  # the same from (g, alpha) instead of dxn
                dout = _E(B, L, D, device=dev)
                dgv, dion = _E(rows, device=dev), _E(rows, device=dev)
                lib.call("asrx_axpy_row2_bwd_acc2", _P(dx), _P(s["alpha"]), _P(g_mem), 1.0 / L, _P(s["active"]),
                         _P(s["g"]), _P(s["ion"]), _P(s["out"]), _P(dout), _P(dgv), _P(dion), _P(dxi), B, L, D, st)
            del dxn
            if ad is not None:
                dpx = G.linear_dgrad(dout, ad.weight, mtiles=s["mt"])  # rows off the layer: not read below
                G.linear_wgrad(dout, s["px"], out=gb(ad.weight), accumulate=True, db=gb(ad.bias))
            else:
                dpx = dout
            # LayerNorm + gate + |x| + v_gate backward in one row pass; dSH = [dS | dh]
            ln, gt = lay["ln"], lay["gate"][0]
            dSH = _E(rows, N, device=dev)
            row_args = (_P(dpx), _P(xi), _P(ln.weight), _P(ln.bias), _P(s["mean"]), _P(s["rstd"]), _P(dgv), _P(s["g"]),
                        _P(gt.weight), _P(dion), _P(s["SH"]), N, _P(s["nx"]), _P(vg.mval), _P(vg.mlp[2].weight),
                        _P(vg.concat.weight), _P(s["kv"]), _P(s["m2"]), _P(dxi), _P(gb(ln.weight)), _P(gb(ln.bias)),
                        _P(gb(gt.weight)), _P(gb(gt.bias)), _P(dSH), _P(gb(vg.mval)), _P(gb(vg.mlp[2].weight)),
                        _P(gb(vg.mlp[2].bias)), _P(gb(vg.concat.weight)), _P(gb(vg.concat.bias)),
                        _P(gb(vg.mlp[0].bias)), rows, D, M, Dh, inv_sqrt_d, _P(s["next_i"]), i, L, st)
            if lt is not None:  # both modes from one entry point; 1 / T_b is formed on the device
                lib.call("asrx_msheath_row_lens_bwd2", mode, _P(dx) if mode else None,
                         _P(s["alpha"]) if mode else None, _P(g_mem) if mode else None,
                         _P(s["ion"]) if mode else None, *row_args[:-9], _P(lt), *row_args[-9:])
            elif mode:
                # no adapter (dpx, dgv, dion are None): dxi's base g' formed from (dx, alpha, g_mem / L) in the row
                # pass, which is dxi's first writer for samples at the layer, and the x_new backward done there on px
                # recomputed from x, mean and rstd
                lib.call("asrx_msheath_row_bwd2", mode, _P(dx), _P(s["alpha"]), _P(g_mem),
                         1.0 / L, _P(s["ion"]), *row_args)
            else:
                lib.call("asrx_msheath_row_bwd", *row_args)
            del dout, dpx
            # x's gradient through both projections: one GEMM against [normalize(mkey); mlp[0].weight]
            G.linear_dgrad(dSH, s["Wc"], out=dxi, beta=1.0, mtiles=s["mt"])
            x2 = xi.view(rows, D)
            dmk = _E(M, D, device=dev)
            lib.call("asrx_zero", _P(dmk), dmk.numel() * 4, st)
            if fused and WGRAD_MERGED:  # both column blocks of dSH^T x in one pass over dSH and x
                G.wgrad_cols2(dSH, M, dmk, gb(vg.mlp[0].weight), x2)
                lib.call("asrx_row_normalize_bwd", _P(dmk), _P(s["Wc"]), _P(s["mkn"]), _P(gb(vg.mkey)), M, D, 1, st)
            else:
                G.wgrad_cols(dSH, 0, M, x2, dmk)
                lib.call("asrx_row_normalize_bwd", _P(dmk), _P(s["Wc"]), _P(s["mkn"]), _P(gb(vg.mkey)), M, D, 1, st)
                G.wgrad_cols(dSH, M, Dh, x2, gb(vg.mlp[0].weight))
            del dSH, dmk
            g_mwo = g_mem_w
            dx = dxi
        # layer 0's mem_w is the (1, 1, D) parameter broadcast over the samples
        lib.call("asrx_colsum", _P(g_mwo), _P(gb(mod.mem_w)), B, D, st)
        # policy = softmax(MPNet(pooled)) backward, then the pooled-mean broadcast and orig's jump grads
        net = mod.pnet.net
        g_pl = _E(B, 3, device=dev)
        lib.call("asrx_softmax_small_bwd", _P(g_policy), _P(sv["policy"]), _P(g_pl), B, 3, st)
        dhp = _E(sv["hp"].shape, device=dev)
        lib.call("asrx_small_linear_bwd", _P(g_pl), None, _P(sv["hp"]), _P(net[2].weight), _P(dhp),
                 _P(gb(net[2].weight)), _P(gb(net[2].bias)), B, dhp.shape[1], 3, 0, 0.0, st)
        lib.call("asrx_act_bwd", _P(dhp), _P(sv["zp"]), _P(dhp), dhp.numel(), SILU, st)
        dpooled = G.linear_dgrad(dhp, net[0].weight)
        G.linear_wgrad(dhp, sv["pooled"], out=gb(net[0].weight), accumulate=True)
        ops.colsum(dhp, out=gb(net[0].bias))
        if lt is not None:  # u = dpooled / T_b formed in the pass, pad rows of dx stored as zeros
            lib.call("asrx_msheath_lens_dx_final", _P(dx), _P(dorig), _P(has_orig), _P(dpooled), _P(lt), B, L, D, st)
        else:
            u = _E(B, D, device=dev)
            lib.call("asrx_lincomb", _P(dpooled), None, None, 1.0 / L, 0.0, 0.0, _P(u), B * D, st)
            lib.call("asrx_msheath_dx_final", _P(dx), _P(dorig), _P(has_orig), _P(u), B, L, D, st)
        # announce each parameter's accumulated gradient once (asrx.dist.GradSync counts events)
        seen = set()
        for p in touched:
            if id(p) not in seen:
                seen.add(id(p))
                ops._gret(p, p.grad, True)
        return (dx, None, None, None, None) + (None,) * len(ctx.needs_input_grad[5:])


# ------------------------------------------------------------------------------------------------ no-save composite
# forward(save=False) -- the reference's dead blocks, eval and decoding -- as ONE C-ABI call (asrx_msheath_fwd,
# csrc/msheath_plan.cpp) that enqueues the same launches from C++: the per-layer Python around ~7 launches cost
# ~30 us of host time each (profiles/r06_host_vs_gpu.txt).  The per-module constants travel as an
# asrx_msheath_plan, built once per step and stream (the v_gate projections and bf16 weight copies it points at
# are per-step values).  False: the Python loop above (same kernels, bit-identical results).
COMPOSITE = True


class _Layer(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in ("ln_w", "ln_b", "gate_w", "gate_b", "mval", "vw2", "vb2", "cw", "cb",
                                                "tx", "bc", "wcb", "ad_wb", "ad_b")] + \
               [("M", ctypes.c_int64), ("Dh", ctypes.c_int64), ("ln_eps", ctypes.c_float), ("px_bf16", ctypes.c_int32)]


class _Plan(ctypes.Structure):
    _fields_ = [("p0_wb", ctypes.c_void_p), ("p0_b", ctypes.c_void_p), ("p2_w", ctypes.c_void_p),
                ("p2_b", ctypes.c_void_p), ("p_hidden", ctypes.c_int64), ("mem_w", ctypes.c_void_p),
                ("mg_w", ctypes.c_void_p), ("mg_b", ctypes.c_void_p), ("jump_s", ctypes.c_void_p),
                ("mln_w", ctypes.c_void_p), ("mln_b", ctypes.c_void_p), ("mln_eps", ctypes.c_float),
                ("hln_bf16", ctypes.c_int32), ("mgate_w", ctypes.c_void_p), ("mgate_b", ctypes.c_void_p),
                ("m0_wb", ctypes.c_void_p), ("m0_b", ctypes.c_void_p), ("m2_wb", ctypes.c_void_p),
                ("m2_b", ctypes.c_void_p), ("H1", ctypes.c_int64), ("a1_bf16", ctypes.c_int32),
                ("n_layers", ctypes.c_int32), ("layers", ctypes.c_void_p)]


def _composite_ok(mod, x, gpol, tag):
    from . import probe
    D = x.shape[-1]
    H1 = mod.mlp[0].weight.shape[0]
    return (COMPOSITE and ROW_COLSUM and prec.get() == prec.PREC_BF16 and G.use_wide(D) and G.use_wide(H1) and H1 % 4 == 0
            and G._nj_override is None and not probe.active() and not (tag is not None and decisions.active())
            and x.is_cuda and gpol.is_contiguous() and gpol.dtype == torch.float32 and x.dtype == torch.float32)


def _build_plan(mod, D):
    dev = mod.mem_w.device
    st = _S()
    wide = True
    store = prec.bf16_storage()
    keep = []  # every tensor the plan points at (bf16 copies, derived weights): alive while the plan is

    def a(t):
        if t is None:
            return None
        keep.append(t)
        return t.data_ptr()

    layers = (_Layer * len(mod.layers))()
    for i, lay in enumerate(mod.layers):
        vg = lay["v_gate"]
        Dh, M = vg.mlp[0].weight.shape[0], vg.mkey.shape[0]
        N = M + Dh

        def build(vg=vg, M=M, Dh=Dh, N=N):  # the same derived entry as forward()
            Wc, bc, mkn = _E(N, D, device=dev), _E(N, device=dev), _E(M, device=dev)
            wb = _E(N, D, dtype=torch.int16, device=dev) if wide else None
            lib.call("asrx_vgate_weights", _P(vg.mkey), _P(vg.mlp[0].weight), _P(vg.mlp[0].bias), _P(Wc), _P(bc),
                     _P(mkn), _P(wb), M, Dh, D, st)
            return Wc, bc, mkn, wb

        Wc, bc, mkn, wb = G.derived(("vgate", bool(wide)), build, (vg.mkey, vg.mlp[0].weight, vg.mlp[0].bias))
        ad = lay["adapter"]
        ln, gt = lay["ln"], lay["gate"][0]
        layers[i] = _Layer(a(ln.weight), a(ln.bias), a(gt.weight), a(gt.bias), a(vg.mval), a(vg.mlp[2].weight),
                           a(vg.mlp[2].bias), a(vg.concat.weight), a(vg.concat.bias), a(vg.tx), a(bc), a(wb),
                           a(G.weight_bf16(ad.weight)) if ad is not None else None,
                           a(ad.bias) if ad is not None else None, M, Dh, float(ln.eps),
                           int(ad is not None and store))
    net = mod.pnet.net
    H1 = mod.mlp[0].weight.shape[0]
    plan = _Plan(a(G.weight_bf16(net[0].weight)), a(net[0].bias), a(net[2].weight), a(net[2].bias),
                 net[0].weight.shape[0], a(mod.mem_w), a(mod.mem_gate[0].weight), a(mod.mem_gate[0].bias),
                 a(mod.jump_s), a(mod.mlp_ln.weight), a(mod.mlp_ln.bias), float(mod.mlp_ln.eps), int(store),
                 a(mod.mlp_gate[0].weight), a(mod.mlp_gate[0].bias), a(G.weight_bf16(mod.mlp[0].weight)),
                 a(mod.mlp[0].bias), a(G.weight_bf16(mod.mlp[2].weight)), a(mod.mlp[2].bias), H1,
                 int(store and H1 % 4 == 0), len(mod.layers), ctypes.addressof(layers))
    return {"plan": plan, "layers": layers, "keep": keep, "ws": {}}


def _forward_composite(mod, x0, gpol):
    B, L, D = x0.shape
    pl = G.derived(("msheath_plan", id(mod), prec.bf16_storage()), lambda: _build_plan(mod, D), (mod.jump_s,))
    L_ = lib.load()
    nb = pl["ws"].get((B, L))
    if nb is None:
        nb = pl["ws"][(B, L)] = int(L_.asrx_msheath_fwd_ws_bytes(ctypes.byref(pl["plan"]), B, L, D))
    ws = _E(nb, dtype=torch.uint8, device=x0.device)
    y = _E(B, L, D, device=x0.device)
    lib.call("asrx_msheath_fwd", ctypes.addressof(pl["plan"]), _P(x0), _P(gpol), gpol.stride(0), _P(y), _P(ws), nb,
             B, L, D, _S())
    return y


def msheath(mod, x, gpol, tag=None, lens=None):
    """Fused MSheath call.  Without autograd (the reference's dead blocks, eval, decoding) the forward
    runs without saving anything for a backward -- from C++ in one call where it can (_forward_composite).
    tag: (noise site key, sid_base) for asrx.decisions.
    lens (ops.seq_lens): per-sample row counts of a zero-padded batch (forward()); None or all-full changes nothing.
    With live lengths the no-grad forward is the Python loop (the composite call does not take lengths)."""
    lens = _live_lens(lens, x)
    if not torch.is_grad_enabled():
        x = x if x.is_contiguous() else x.contiguous()
        if lens is None and _composite_ok(mod, x, gpol, tag):
            return _forward_composite(mod, x, gpol)
        return forward(mod, x, gpol, save=False, tag=tag, lens=lens, vetted=True)[0]
    # the parameter list (~60 nn.Module attribute walks) is made once per module: the module tree is fixed
    params = mod.__dict__.get("_asrx_params")
    if params is None or params[4] is not mod.mem_w or params[7] is not mod.jump_s:  # (replaced parameters)
        params = _params(mod)
        mod.__dict__["_asrx_params"] = params
    if not (x.requires_grad or any(p.requires_grad for p in params)):
        x = x if x.is_contiguous() else x.contiguous()
        if lens is None and _composite_ok(mod, x, gpol, tag):
            return _forward_composite(mod, x, gpol)
        return forward(mod, x, gpol, save=False, tag=tag, lens=lens, vetted=True)[0]
    return MSheathFn.apply(x, gpol, mod, tag, lens, *params)
