"""Float64 reference of MSheath on a padded batch with per-sample lengths (in the style of tests/enc_lens_ref.py): the
oracle's per-sample loop (oracle/model.py msheath) run on the whole padded sample x[b] (L rows, of which T_b are live),
with the points where a pad row could reach a live one named, so that each can be switched off:

  pooled     the policy's pooled mean over rows [0, T_b)
  mem        the mem mean over rows [0, T_b)
  potential  the ion mean over rows [0, T_b)
  xzero      zero pad rows of x_new and of the jump output (what the next layer and the tail read)
  yzero      zero pad rows of the module output y

Every mask is a select (torch.where), so what a pad row holds -- a sentinel in x, NaN in the cotangent -- reaches
nothing, and the gradient sent back to a pad row is an exact zero.
"""
import torch
import torch.nn.functional as F

from oracle import model as om

POINTS = ("pooled", "mem", "potential", "xzero", "yzero")


def _mean(v, live, on):
    """mean over the rows (dim 1) of v (1, L, C): the live ones when the mask point is on."""
    if not on:
        return v.mean(dim=1)
    return torch.where(live.view(1, -1, 1), v, torch.zeros_like(v)).sum(dim=1) / int(live.sum())


def msheath_lens(P, pre, x, layer, g_pol, lens, points=POINTS):
    """-> (y, xs): the module output (B, L, D) and the last jump output, for the pad-row checks."""
    outs, lasts = [], []
    D = x.shape[-1]
    L = x.shape[1]
    for s in range(x.shape[0]):
        live = torch.arange(L) < int(lens[s])
        lv = live.view(1, L, 1)

        def zero_pad(v, on):
            return torch.where(lv, v, torch.zeros_like(v)) if on else v

        xs = x[s:s + 1]
        orig_x = xs
        mem_w = P[pre + ".mem_w"].expand(1, -1, -1)
        pooled = _mean(xs, live, "pooled" in points)
        policy = torch.softmax(om._lin(P, pre + ".pnet.net.2", F.silu(om._lin(P, pre + ".pnet.net.0", pooled))), -1)
        i = 0
        while i < layer:
            lp = f"{pre}.layers.{i}"
            ion, _ = om.v_gate(P, lp + ".v_gate", xs)
            px = om._ln(P, lp + ".ln", xs)
            out = om._lin(P, lp + ".adapter", px) if i % 2 == 0 else px
            g_val = torch.sigmoid(om._lin(P, lp + ".gate.0", px))
            xs = zero_pad(xs + g_val * (out * ion.expand(-1, L, D)), "xzero" in points)
            mem = _mean(xs, live, "mem" in points).unsqueeze(1)
            mem_v = torch.sigmoid(om._lin(P, pre + ".mem_gate.0", mem))
            mem_w = mem_v * mem_w + (1 - mem_v) * mem
            potential = _mean(ion, live, "potential" in points).reshape(())
            jump_g = 1.0
            if bool(potential < 0.1) and i < layer - 1:
                action = 1
            elif i < layer - 1:
                ys = torch.softmax(policy + g_pol[s:s + 1, i], dim=-1)
                idx = ys.argmax(dim=-1, keepdim=True)
                jump = torch.zeros_like(ys).scatter_(-1, idx, 1.0) - ys.detach() + ys
                action = int(jump.argmax(dim=-1).item())
                jump_g = jump[0, action]
            else:
                action = 0
            if action > 0:
                jump_w = P[pre + ".jump_s"][min(action - 1, 2)]
                xs = xs + (jump_w * orig_x + (1 - jump_w) * mem_w.expand(-1, L, -1)) * jump_g
                i = min(i + action + 1, layer)
            else:
                xs = xs * jump_g
                i += 1
            xs = zero_pad(xs, "xzero" in points)
        gate = torch.sigmoid(om._lin(P, pre + ".mlp_gate.0", xs))
        h = om._lin(P, pre + ".mlp.2", F.silu(om._lin(P, pre + ".mlp.0", om._ln(P, pre + ".mlp_ln", xs))))
        outs.append(zero_pad(xs + gate * h, "yzero" in points))
        lasts.append(xs)
    return torch.cat(outs), torch.cat(lasts)
