"""Float64 restatement of one MaxFactor parameter step INCLUDING the ``clip`` / ``cap`` branch
(optimizerc.py:55-130; the direction, cap and apply lines are :113-130).  Test infrastructure only:
oracle/maxfactor.py stops before the cap, and tests/test_gradstats_host.py pins this restatement to it
with ``clip=False``.  Shared by test_gradstats_host.py (CPU) and test_gpu_optim_seam.py (GPU)."""
import torch

# the shapes / parameter groups and hyper-parameters of tests/test_gpu_optim.py, restated
SHAPES = [((37, 53), 0), ((16, 4, 3), 0), ((29,), 0), ((), 0), ((384, 1, 1), 0), ((300, 40), 0),
          ((1, 1, 384), 1), ((8, 20), 1), ((5,), 1), ((6, 2, 10), 1),
          ((48, 40, 3), 1), ((7, 5, 15), 0), ((33, 17), 0), ((9, 7, 2), 1)]
HP = dict(lr=2.5e-3, b_decay=-0.8, eps=(1e-8, 1e-8), d=1.0, decay=1e-2, gamma=0.99, max=False, bias=1,
          min_lr=1e-9, clip=False, cap=0.0)


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))


def make_params(seed=0):
    torch.manual_seed(seed)
    return [torch.randn(s, dtype=torch.float32) for s, _ in SHAPES]


def make_grads(gen):
    return [torch.randn(s, generator=gen) * (0.1 + 3 * i) for i, (s, _) in enumerate(SHAPES)]


def group_of(i, **over):
    return dict(HP, bias=1.0 if SHAPES[i][1] == 0 else 2.0, **over)


def step_param(p, grad, st, g):
    """One parameter, in place, float64.  Returns update_rms / max_allowed_step (None without clip): the cap
    binds when it is > 1."""
    eps1, eps2 = g["eps"]
    if g["max"]:
        grad = -grad
    st["step"] += 1
    t = st["step"]
    beta = t ** g["b_decay"]
    rho = max(g["min_lr"], min(g["lr"], 1.0 / (t ** 0.5)))
    alpha = max(eps2, float(p.norm(2)) / (p.numel() ** 0.5)) * rho
    if g["decay"] != 0:
        p.mul_(1 - g["lr"] * g["decay"])
    if grad.dim() > 1:
        st["row_var"].lerp_(grad.square().sum(-1, keepdim=True) / (grad.size(-1) + 1e-8), beta)
        st["col_var"].lerp_(grad.square().sum(-2, keepdim=True) / (grad.size(-2) + 1e-8), beta)
        var_est = (st["row_var"] @ st["col_var"]) / st["row_var"].max(dim=-2, keepdim=True)[0].clamp(min=eps1)
    else:
        st["v"].mul_(g["gamma"]).add_(grad ** 2, alpha=1 - g["gamma"])
        var_est = st["v"]  # the reference's in-place ops below run on state["v"] itself
    update = var_est.clamp_(min=eps1 * eps1).rsqrt_().mul_(grad)
    inf_norm = update.abs().max()
    if inf_norm > 0:
        update.div_(inf_norm.clamp(min=eps1))
    denom = max(1.0, float(update.norm(2)) / ((update.numel() ** 0.5) * g["d"]))
    # ---- optimizerc.py:113-130
    if p.dim() < 3 or g["bias"] == 1:
        scale = update.abs().max(dim=-1, keepdim=True)[0]
    else:
        scale = torch.median(update.abs(), dim=-1, keepdim=True)[0]
    final_direction = update.sign() * scale
    step_size = alpha / denom
    ratio = None
    if g["clip"]:
        param_rms = float(torch.norm(p)) / (p.numel() ** 0.5)  # after the decay multiply above
        max_allowed_step = param_rms * g["cap"]
        update_rms = float(torch.norm(final_direction * step_size)) / (final_direction.numel() ** 0.5)
        ratio = update_rms / max_allowed_step if max_allowed_step > 0 else float("inf")
        if update_rms > max_allowed_step:
            step_size = step_size * (max_allowed_step / (update_rms + 1e-8))
    p.add_(final_direction, alpha=-step_size)
    return ratio
