"""Plain torch references of the row, elementwise and MSheath step kernels (csrc/rowops.hip,
csrc/msheath.hip), one function per operation, definitions taken from the comment above each kernel.

Every function computes in the dtype of the tensors it is given: float64 inputs give the reference,
float32 inputs give the same formulas with float32 rounding (the yardstick e32 of the GPU tests).
Backward formulas are written out where the kernel's backward is hand-written, so that each output of a
kernel (ds, dalpha, dgam, mean, rstd, nrm, gate, ...) can be compared on its own, without autograd;
tests/test_rowops_ref.py checks them against autograd of the forward.  Nothing here imports asrx.
"""
import math

import torch

ACTS = ("none", "gelu", "silu", "sigmoid", "relu")


# ------------------------------------------------------------------------------------------ elementwise
def lincomb(x, y, z, a, b, c):
    """out = a*x + b*y (+ c*z); y and z may be None."""
    v = a * x
    if y is not None:
        v = v + b * y
    if z is not None:
        v = v + c * z
    return v


def act_fwd(x, name):
    """none / exact (erf) GELU / SiLU / sigmoid / ReLU."""
    if name == "none":
        return x.clone()
    if name == "gelu":
        return 0.5 * x * (1.0 + torch.erf(x * math.sqrt(0.5)))
    if name == "silu":
        return x / (1.0 + torch.exp(-x))
    if name == "sigmoid":
        return 1.0 / (1.0 + torch.exp(-x))
    if name == "relu":
        return torch.where(x > 0, x, torch.zeros_like(x))
    raise ValueError(name)


def act_deriv(x, name):
    """d act(x) / dx, elementwise (ReLU: 1 for x > 0, else 0)."""
    if name == "none":
        return torch.ones_like(x)
    if name == "gelu":
        cdf = 0.5 * (1.0 + torch.erf(x * math.sqrt(0.5)))
        pdf = torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
        return cdf + x * pdf
    if name == "silu":
        s = 1.0 / (1.0 + torch.exp(-x))
        return s * (1.0 + x * (1.0 - s))
    if name == "sigmoid":
        s = 1.0 / (1.0 + torch.exp(-x))
        return s * (1.0 - s)
    if name == "relu":
        return (x > 0).to(x.dtype)
    raise ValueError(name)


def act_bwd(g, x, name):
    """dx = g * act'(x)."""
    return g * act_deriv(x, name)


def act_dropout_fwd(z, keep, p, act, act2):
    """y = act2(act(z) * keep / (1 - p)); keep is the 0/1 mask."""
    return act_fwd(act_fwd(z, act) * keep * (1.0 / (1.0 - p)), act2)


def act_dropout_bwd(g, z, keep, p, act, act2):
    """dz = g * act2'(act(z) * keep / (1 - p)) * keep / (1 - p) * act'(z)."""
    sc = 1.0 / (1.0 - p)
    return g * act_deriv(act_fwd(z, act) * keep * sc, act2) * keep * sc * act_deriv(z, act)


def glu_fwd(x):
    """rows of 2C: out = a * sigmoid(b), a = x[..., :C], b = x[..., C:]."""
    C = x.shape[-1] // 2
    return x[..., :C] / (1.0 + torch.exp(-x[..., C:]))


def glu_bwd(g, x):
    """da = g * s, db = g * a * s * (1 - s), s = sigmoid(b); returned as rows of 2C."""
    C = x.shape[-1] // 2
    a = x[..., :C]
    s = 1.0 / (1.0 + torch.exp(-x[..., C:]))
    return torch.cat([g * s, g * a * s * (1.0 - s)], -1)


# ------------------------------------------------------------------------------------------ row-indexed
def add_rows(x, t, u, B, L, d):
    """out[b, l, :] = x[b, l, :] + t[l, :] + u[b, :]; each of x, t (>= L rows), u may be None."""
    ref = next(v for v in (x, t, u) if v is not None)
    out = torch.zeros(B, L, d, dtype=ref.dtype, device=ref.device)
    if x is not None:
        out = out + x.reshape(B, L, d)
    if t is not None:
        out = out + t[:L].reshape(1, L, d)
    if u is not None:
        out = out + u.reshape(B, 1, d)
    return out


def axpy_row(x, s, y):
    """out = x + s[r] * y on (rows, d); s None means 1."""
    return x + y if s is None else x + s[:, None] * y


def axpy_row_bwd(g, s, y):
    """dy = s[r] * g, ds[r] = sum_j g[r, j] y[r, j], dx = g."""
    return s[:, None] * g, (g * y).sum(-1), g.clone()


def axpy_row2(x, s1, s2, y):
    """out = x + s1[r] * s2[r] * y; s2 None means 1."""
    sc = s1 if s2 is None else s1 * s2
    return x + sc[:, None] * y


def axpy_row2_bwd(g, s1, s2, y):
    """dy = s1 s2 g; t = sum_j g y; ds1 = s2 t; ds2 = s1 t (s2 None: ds1 = t, no ds2)."""
    t = (g * y).sum(-1)
    if s2 is None:
        return s1[:, None] * g, t, None
    return (s1 * s2)[:, None] * g, s2 * t, s1 * t


def seg_sum(x, scale):
    """out[b, :] = scale * sum_l x[b, l, :] (scale = 1 / L: the mean over dim 1)."""
    return x.sum(1) * scale


def seg_mean_bwd(g, L):
    """dx[b, l, :] = g[b, :] / L."""
    return (g * (1.0 / L))[:, None, :].expand(g.shape[0], L, g.shape[1]).contiguous()


def colsum(x, out0):
    """out[c] = out0[c] + sum_r x[r, c]."""
    return out0 + x.sum(0)


def embed_fwd(ids, E):
    """y[r] = E[ids[r]]."""
    return E[ids]


def embed_bwd(ids, g, dE0):
    """dE = dE0 with g[r] added to row ids[r] (repeated ids add up; other rows keep dE0)."""
    return dE0.index_add(0, ids.reshape(-1), g.reshape(-1, g.shape[-1]))


def stem1_fwd(x, W, b):
    """Conv1d(1, D, 3, padding=1) on (B, T), channels-last: y[b, t, o] = b[o] + sum_k W[o, k] x[b, t + k - 1]."""
    B, T = x.shape
    xp = torch.zeros(B, T + 2, dtype=x.dtype, device=x.device)
    xp[:, 1:T + 1] = x
    y = b.reshape(1, 1, -1).expand(B, T, -1).clone()
    for k in range(3):
        y = y + xp[:, k:k + T, None] * W[:, k].reshape(1, 1, -1)
    return y


def stem1_bwd(g, x, dW0, db0):
    """dW[o, k] = dW0 + sum_{b, t} g[b, t, o] x[b, t + k - 1]; db[o] = db0 + sum_{b, t} g[b, t, o]."""
    B, T = x.shape
    xp = torch.zeros(B, T + 2, dtype=x.dtype, device=x.device)
    xp[:, 1:T + 1] = x
    dW = torch.stack([(g * xp[:, k:k + T, None]).sum((0, 1)) for k in range(3)], 1)
    return dW0 + dW, db0 + g.sum((0, 1))


# ------------------------------------------------------------------------------------------ LayerNorm
def layernorm_fwd(x, w, b, eps):
    """y = (x - mean) * rstd * w + b with the biased variance; returns (y, mean, rstd) per row."""
    mean = x.mean(-1)
    xc = x - mean[:, None]
    rstd = 1.0 / torch.sqrt((xc * xc).mean(-1) + eps)
    return xc * rstd[:, None] * w + b, mean, rstd


def layernorm_row_outputs(x, y, gw, gb, gate_on_x):
    """nrm[r] = |x_r|_2; gate[r] = sigmoid((x_r if gate_on_x else y_r) . gw + gb)."""
    nrm = torch.sqrt((x * x).sum(-1))
    q = ((x if gate_on_x else y) * gw).sum(-1) + gb
    return nrm, 1.0 / (1.0 + torch.exp(-q))


def layernorm_bwd(dy, x, w, mean, rstd, dx0, dw0, db0):
    """xh = (x - mean) rstd; g = dy w; dx = dx0 + rstd (g - mean_j g - xh mean_j (g xh));
    dw = dw0 + sum_r dy xh; db = db0 + sum_r dy.  dx0 None: dx is overwritten."""
    xh = (x - mean[:, None]) * rstd[:, None]
    g = dy * w
    dx = rstd[:, None] * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
    if dx0 is not None:
        dx = dx0 + dx
    return dx, dw0 + (dy * xh).sum(0), db0 + dy.sum(0)


# ------------------------------------------------------------------------------------------ MSheath steps
def jump_select(xn, orig, xold, act, alpha, beta, gam):
    """out[b] = act[b] != 0 ? alpha[b] xn[b] + beta[b] orig[b] + gam[b, :] : xold[b]; tensors (B, L, d)."""
    on = (act != 0)[:, None, None]
    v = alpha[:, None, None] * xn + beta[:, None, None] * orig + gam[:, None, :]
    return torch.where(on, v, xold)


def jump_select_bwd(g, xn, orig, act, alpha, beta):
    """Active samples: dxn = alpha g, dorig = beta g, dxold = 0, dalpha = sum g xn, dbeta = sum g orig,
    dgam = sum_l g.  Inactive samples: dxold = g and everything else is zero.
    Returns (dxn, dorig, dxold, dalpha, dbeta, dgam)."""
    on = (act != 0).to(g.dtype)
    o3 = on[:, None, None]
    return (o3 * alpha[:, None, None] * g, o3 * beta[:, None, None] * g, (1.0 - o3) * g,
            on * (g * xn).sum((1, 2)), on * (g * orig).sum((1, 2)), on[:, None] * g.sum(1))


def jump_axpy(xin, s1, s2, y, orig, act, alpha, beta, gam):
    """Samples at the layer: alpha (xin + s1 s2 y) + beta orig + gam; the others keep xin."""
    B, L, d = xin.shape
    xn = axpy_row2(xin.reshape(B * L, d), s1.reshape(-1), s2.reshape(-1), y.reshape(B * L, d)).reshape(B, L, d)
    return jump_select(xn, orig, xin, act, alpha, beta, gam)
