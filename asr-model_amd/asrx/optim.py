"""MaxFactor optimizer and FAMScheduler2 (optimizerc.py:6-147, 770-795) with the same constructor
signatures, parameter-group semantics and state names, so the reference's setup (model.py:772-791:
group 1 = every parameter, 'bias': 1.0; group 2 = names containing jump / pnet / micro_filter,
'bias': 2.0) drops in unchanged.

The step itself is one native call (``asrx_maxfactor_step``, csrc/maxfactor.hip) over every
parameter that has a gradient: eight kernel launches for the whole model, no per-parameter host
sync.  The reference reads four scalars back per parameter (.item()); here the only host work is
updating the cached parameter table (step counts, beta_t / rho_t, lr) and one asynchronous H2D copy.
Deliberate difference: ``state["RMS"]`` (written by the reference, never read) is not kept.
``clip=True`` (optimizerc.py:121-128, off in the reference configuration) caps each parameter's update
RMS at ``cap`` times the parameter's RMS inside the same call.

The seam between backward and the step (essentials.py:778-821: per-parameter gradient norms, the
global norm, ``GradScaler.unscale_``'s inf/NaN check, ``clip_grad_norm_``, the skipped step) stays on
the device: ``GradStats.measure()`` is one native call (``asrx_grad_stats``, csrc/gradstats.hip) that
leaves the norms and a control word (gradient scale, skip flag) in device memory, and
``MaxFactor.step(grad_ctl=stats)`` (``asrx_maxfactor_step_ex``) scales every gradient read by it or
skips the whole step, without a host sync.  A skipped step does not count: its flag reaches the host
by an asynchronous copy that the next ``step()`` reads, and the step counts are then taken back.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import lib


# one parameter record, byte-compatible with MFParam in csrc/maxfactor.hip (144 bytes)
_REC = np.dtype([("p", "u8"), ("g", "u8"), ("rv", "u8"), ("cv", "u8"), ("v", "u8"), ("n", "i8"), ("mats", "i4"),
                 ("rows", "i4"), ("cols", "i4"), ("mode", "i4"), ("beta", "f4"), ("rho", "f4"), ("lr", "f4"),
                 ("decay", "f4"), ("gamma", "f4"), ("d", "f4"), ("eps1", "f4"), ("eps2", "f4"), ("row0", "i8"),
                 ("cc0", "i8"), ("col0", "i8"), ("mat0", "i8"), ("item0", "i8"), ("gsz", "i4"),
                 ("cap", "f4")])
_CLIP = 4  # mode flag MF_CLIP: the record's cap applies

# one gradient record of asrx_grad_stats (GSParam in csrc/gradstats.hip)
_GREC = np.dtype([("g", "u8"), ("n", "i8"), ("item0", "i8")])
GS_CHUNK = 4096  # elements per chunk of the gradient-statistics kernel (GS_CHUNK), one wave each
GS_MAX_TENSORS = 4096  # gradients per call (GS_MAXP)


_CHUNK = 256  # rows per column-sum work item (MF_CHUNK)


def _group(length: int) -> int:
    """Lanes per row in the row kernels: the power of two >= the row length, at most a wave (64)."""
    g = 1
    while g < min(length, 64):
        g *= 2
    return g


def _geometry(p: torch.Tensor):
    """(mats, rows, cols) of the reference's factored view: rows reduce over the last dim, columns
    over dim -2, leading dims are independent matrices (row_var (..., R, 1), col_var (..., 1, C))."""
    if p.dim() <= 1:  # vectors and 0-d scalars (e.g. blend / threshold parameters)
        return 1, 1, p.numel()
    rows, cols = p.shape[-2], p.shape[-1]
    return p.numel() // (rows * cols), rows, cols


class MaxFactor(torch.optim.Optimizer):
    __version__ = "1.0"

    def __init__(self, params, lr=0.025, b_decay=-0.8, eps=(1e-8, 1e-8), d=1.0, decay=0.01, gamma=0.99, max=False,
                 bias=1, min_lr=1e-9, clip=False, cap=0.0):
        defaults = dict(lr=lr, b_decay=b_decay, eps=eps, d=d, decay=decay, gamma=gamma, max=max, bias=bias,
                        min_lr=min_lr, clip=clip, cap=cap)
        if clip and not cap >= 0.0:
            raise ValueError(f"MaxFactor(clip=True) needs cap >= 0 (got {cap})")
        super().__init__(params=params, defaults=defaults)
        self._ws = None
        self._skipped = 0
        self._flag = None  # (pinned copy of the last step's skip flag, event behind the copy), while unread

    def _settle_skip(self):
        """Read the skip flag of the last ``step(grad_ctl=...)`` (its copy is a forward and a backward old by
        the next step) and, if that step was skipped on the device, take it off the step counts: beta_t and
        rho_t come from them, and a skipped step did not happen (GradScaler semantics)."""
        if self._flag is None:
            return
        host, event = self._flag
        self._flag = None
        event.synchronize()
        if float(host[0]) != 0.0:
            c = self._cache
            torch._foreach_sub_(c["step_tensors"], 1.0)
            c["steps"] -= 1.0
            self._skipped += 1

    def sync_skips(self) -> int:
        """Wait for the last step's skip flag, settle the step counts, and return the number of steps skipped
        so far."""
        self._settle_skip()
        return self._skipped

    def state_dict(self):
        self.sync_skips()
        return super().state_dict()

    @torch.no_grad()
    def step(self, closure=None, *, grad_ctl=None):
        """``grad_ctl``: a ``GradStats`` (or any object with a device float32 tensor ``.ctl`` of at least two
        elements) measured on this step's gradients: ctl[0] scales every gradient read, ctl[1] != 0 skips
        the step on the device."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._settle_skip()
        live = []  # (group, p, grad)
        for group in self.param_groups:
            if group["clip"] and not group["cap"] >= 0.0:
                raise ValueError(f"MaxFactor: clip needs cap >= 0 (got {group['cap']})")
            for p in group["params"]:
                if p.grad is None:
                    continue
                lib.require_gpu(p, p.grad)
                if p.dtype != torch.float32 or not p.is_contiguous():
                    raise ValueError("MaxFactor expects contiguous float32 parameters")
                grad = p.grad if p.grad.dtype == torch.float32 and p.grad.is_contiguous() else p.grad.float().contiguous()
                if group["max"]:
                    grad = -grad
                live.append((group, p, grad))
        if not live:
            return loss
        key = tuple((id(g), p.data_ptr(), gr.data_ptr(), bool(g["clip"])) for g, p, gr in live)
        if getattr(self, "_key", None) != key:
            self._build(live)
            self._key = key
        c = self._cache
        # per-step scalars, vectorised over the table (steps advance together for every live param)
        torch._foreach_add_(c["step_tensors"], 1.0)
        c["steps"] += 1.0
        tab = c["tab"]
        tab["lr"] = np.array([g["lr"] for g, _, _ in live], dtype=np.float32)
        tab["beta"] = c["steps"] ** c["b_decay"]
        tab["rho"] = np.maximum(c["min_lr"], np.minimum(tab["lr"], 1.0 / np.sqrt(c["steps"])))
        if c["clip_any"]:
            tab["cap"] = np.array([g["cap"] for g, _, _ in live], dtype=np.float32)
        # asynchronous H2D of the table from two alternating pinned buffers: a buffer is rewritten
        # only after the copy that read it two steps ago has completed
        k = c["flip"] = c["flip"] ^ 1
        c["done"][k].synchronize()
        c["pinned"][k].numpy()[:] = tab.view(np.uint8)
        c["dev_tab"][k].copy_(c["pinned"][k], non_blocking=True)
        c["done"][k].record()
        if grad_ctl is None and not c["clip_any"]:
            lib.call("asrx_maxfactor_step", c["dev_tab"][k].data_ptr(), len(live), c["nrows"], c["ncols"], c["ncc"],
                     c["nmats"], c["nitems"], c["ws"].data_ptr(), lib.stream())
        else:
            ctl = None
            if grad_ctl is not None:
                ctl = grad_ctl.ctl
                lib.require_gpu(ctl)
                if ctl.dtype != torch.float32 or ctl.numel() < 2 or not ctl.is_contiguous():
                    raise ValueError("MaxFactor.step: grad_ctl.ctl is a contiguous float32 tensor [coef, found_inf, ...]")
            lib.call("asrx_maxfactor_step_ex", c["dev_tab"][k].data_ptr(), len(live), c["nrows"], c["ncols"],
                     c["ncc"], c["nmats"], c["nitems"], c["ws"].data_ptr(), lib.ptr(ctl), int(c["clip_any"]),
                     lib.stream())
            if ctl is not None:  # the flag follows the step to the host; the next step() reads it
                c["flag_host"].copy_(ctl[1:2], non_blocking=True)
                c["flag_done"].record()
                self._flag = (c["flag_host"], c["flag_done"])
        self._keep = [gr for _, _, gr in live]  # asynchronous call: keep converted gradients alive
        return loss

    def _build(self, live):
        lib_ = lib.load()
        if _REC.itemsize != lib_.asrx_maxfactor_param_bytes():
            raise RuntimeError("MaxFactor record layout does not match libasrx")
        tab = np.zeros(len(live), dtype=_REC)
        nrows = ncols = ncc = nmats = nitems = 0
        steps, b_decay, min_lr, step_tensors = [], [], [], []
        for i, (group, p, grad) in enumerate(live):
            eps1, eps2 = group["eps"]
            if eps1 is None:
                eps1 = torch.finfo(torch.float32).eps
            state = self.state[p]
            if len(state) == 0:  # optimizerc.py:39-46
                state["step"] = torch.tensor(0.0, dtype=torch.float32)
                if p.dim() > 1:
                    rs, cs = list(p.shape), list(p.shape)
                    rs[-1], cs[-2] = 1, 1
                    state["row_var"], state["col_var"] = p.new_zeros(rs), p.new_zeros(cs)
                state["v"] = torch.zeros_like(p)
            mats, rows, cols = _geometry(p)
            mode = 0 if p.dim() <= 1 else (1 if (p.dim() < 3 or group["bias"] == 1) else 2)
            clip = _CLIP if group["clip"] else 0
            gsz = _group(p.numel() if mode == 0 else cols)
            tab[i] = (p.data_ptr(), grad.data_ptr(), lib.ptr(state.get("row_var")) or 0,
                      lib.ptr(state.get("col_var")) or 0, state["v"].data_ptr(), p.numel(), mats, rows, cols,
                      mode | clip, 0.0, 0.0, group["lr"], group["decay"], group["gamma"], group["d"], eps1, eps2, nrows,
                      ncc, ncols, nmats, nitems, gsz, group["cap"] if clip else 0.0)
            nitems += -(-(1 if mode == 0 else mats * rows) // (64 // gsz))
            if mode == 0:
                nrows += 1
            else:
                nrows += mats * rows
                ncols += mats * cols
                ncc += mats * cols * ((rows + _CHUNK - 1) // _CHUNK)
                nmats += mats
            steps.append(float(state["step"]))
            b_decay.append(group["b_decay"])
            min_lr.append(group["min_lr"])
            step_tensors.append(state["step"])
        device = live[0][1].device
        self._cache = dict(tab=tab, nrows=nrows, ncols=ncols, ncc=ncc, nmats=nmats, nitems=nitems, device=device,
                           steps=np.array(steps, dtype=np.float64), b_decay=np.array(b_decay, dtype=np.float64),
                           min_lr=np.array(min_lr, dtype=np.float64), step_tensors=step_tensors,
                           clip_any=any(g["clip"] for g, _, _ in live),
                           ws=torch.empty(4 * len(live) + 5 * nrows + ncols + nmats, device=device,
                                          dtype=torch.float32),
                           flag_host=torch.zeros(1, dtype=torch.float32).pin_memory(), flag_done=torch.cuda.Event(),
                           pinned=[torch.empty(tab.nbytes, dtype=torch.uint8).pin_memory() for _ in range(2)],
                           dev_tab=[torch.empty(tab.nbytes, dtype=torch.uint8, device=device) for _ in range(2)],
                           done=[torch.cuda.Event(), torch.cuda.Event()], flip=0)


class GradStats:
    """Gradient statistics of a whole model in one native call (``asrx_grad_stats``), kept on the device.

    ``named_params``: an iterable of ``(name, parameter)`` (``model.named_parameters()``) or of parameters
    (named by their index).  ``measure(inv_scale)`` reads every gradient once and leaves, as device views that
    never sync: ``sumsq`` (per-parameter sum of squares of ``inv_scale * grad``), ``total_norm``,
    ``found_inf`` (0 / 1: a NaN or inf element, or a norm that is not finite), ``coef`` (what the optimizer
    multiplies gradients by: ``inv_scale * min(1, max_norm / (total_norm + eps))``, ``inv_scale`` when
    ``max_norm <= 0``, 0 when ``found_inf``) and ``ctl = [coef, found_inf, total_norm, non-finite count]``, the
    control word ``MaxFactor.step(grad_ctl=...)`` takes.  ``norms()`` is the one host read: every
    per-parameter L2 norm with a single device-to-host copy (the reference's track_grad_norms syncs once per
    parameter).  Parameters without a gradient are left out.
    """

    def __init__(self, named_params, max_norm=0.0, eps=1e-6):
        self._params = []
        for i, item in enumerate(named_params):
            name, p = item if isinstance(item, (tuple, list)) else (str(i), item)
            self._params.append((name, p))
        self.max_norm = float(max_norm)
        self.eps = float(eps)
        self._key = None
        self._stats = None
        self._names = []

    def measure(self, inv_scale=1.0):
        live = []  # (name, fp32 contiguous gradient)
        for name, p in self._params:
            if p.grad is None:
                continue
            lib.require_gpu(p.grad)
            g = p.grad
            live.append((name, g if g.dtype == torch.float32 and g.is_contiguous() else g.float().contiguous()))
        if not live:
            raise ValueError("GradStats.measure: no parameter has a gradient")
        key = tuple((g.data_ptr(), g.numel()) for _, g in live)
        if self._key != key:
            self._build(live)
            self._key = key
        lib.call("asrx_grad_stats", self._dev_tab.data_ptr(), len(live), self._nitems, float(inv_scale), self.max_norm,
                 self.eps, self._stats.data_ptr(), self._ws.data_ptr(), lib.stream())
        self._keep = [g for _, g in live]  # asynchronous call: keep converted gradients alive
        return self

    def _build(self, live):
        if len(live) > GS_MAX_TENSORS:
            raise ValueError(f"GradStats: at most {GS_MAX_TENSORS} gradients per call (got {len(live)})")
        if _GREC.itemsize != lib.load().asrx_grad_stats_param_bytes():
            raise RuntimeError("GradStats record layout does not match libasrx")
        tab = np.zeros(len(live), dtype=_GREC)
        nitems = 0
        for i, (_, g) in enumerate(live):
            tab[i] = (g.data_ptr(), g.numel(), nitems)
            nitems += -(-g.numel() // GS_CHUNK)
        device = live[0][1].device
        self._names = [name for name, _ in live]
        self._nitems = nitems
        self._pinned = torch.from_numpy(tab.view(np.uint8).copy()).pin_memory()
        self._dev_tab = torch.empty(tab.nbytes, dtype=torch.uint8, device=device)
        self._dev_tab.copy_(self._pinned, non_blocking=True)
        self._stats = torch.zeros(len(live) + 4, dtype=torch.float32, device=device)
        self._ws = torch.empty(max(2 * nitems, 2), dtype=torch.float32, device=device)

    def _view(self, lo, hi=None):
        if self._stats is None:
            raise RuntimeError("GradStats: call measure() first")
        return self._stats[lo] if hi is None else self._stats[lo:hi]

    @property
    def names(self):
        return list(self._names)

    @property
    def sumsq(self):
        return self._view(0, len(self._names))

    @property
    def ctl(self):
        return self._view(len(self._names), len(self._names) + 4)

    @property
    def coef(self):
        return self._view(len(self._names))

    @property
    def found_inf(self):
        return self._view(len(self._names) + 1)

    @property
    def total_norm(self):
        return self._view(len(self._names) + 2)

    def norms(self) -> dict:
        """{name: L2 norm of inv_scale * grad} for every parameter that had a gradient; one device-to-host copy."""
        host = self.sumsq.cpu().double().sqrt().tolist()
        return dict(zip(self._names, host))


class FAMScheduler2(torch.optim.lr_scheduler.LRScheduler):
    """optimizerc.py:770-795: linear warmup from warmup_start, hold until decay_start, then cosine to
    eta_min (+1e-8)."""

    def __init__(self, optimizer, warmup_steps=1000, total_steps=100000, decay_start=10, warmup_start=1e-6,
                 eta_min=1e-6, last_epoch=-1):
        self.warmup_steps = warmup_steps
        self.total_steps = total_steps
        self.decay_start_step = decay_start if decay_start is not None else warmup_steps
        self.warmup_start_lr = warmup_start
        self.eta_min = eta_min
        super().__init__(optimizer, last_epoch)

    def get_lr(self):
        if self.last_epoch < self.warmup_steps:
            a = self.last_epoch / self.warmup_steps
            return [self.warmup_start_lr + (b - self.warmup_start_lr) * a for b in self.base_lrs]
        if self.last_epoch < self.decay_start_step:
            return list(self.base_lrs)
        frac = (self.last_epoch - self.decay_start_step) / (self.total_steps - self.decay_start_step)
        return [self.eta_min + (b - self.eta_min) * (1 + math.cos(math.pi * frac)) / 2 + 1e-8 for b in self.base_lrs]


def reference_param_groups(model: torch.nn.Module):
    """model.py:772-781: the two MaxFactor groups of the reference training script."""
    main, jump = [], []
    for name, p in model.named_parameters():
        if not p.requires_grad:
            continue
        (jump if ("jump" in name or "pnet" in name or "micro_filter" in name) else main).append(p)
    return [{"params": main, "bias": 1.0}, {"params": jump, "bias": 2.0}]
