"""Float64 restatement of one padded train-mode encoder pass with per-sample lengths: the semantics the LENS
kernels of asr-model_amd/csrc/rowops.hip follow (test_enc_lens_ref.py proves them against oracle.model.encode_stream
run on every sample alone; test_gpu_enc_lens.py holds the kernels to the same rule).

It is oracle.model.encode_stream on a zero-padded (B, C, T) batch plus exactly five mask points, each a select
(torch.where), never a multiply:

  gelu0  zeros in the pad rows after layer 0's leading GELU (the input of the first k3 GEMM conv);
  k15    the k15 depthwise conv reads zeros at and past T_b (its row limit);
  bn     the BatchNorm statistics of sample b run over its rows [0, T_b);
  k3     the k3 depthwise conv reads zeros at and past T_b;
  tail   zeros in the pad rows after the layer's tail dropout (the input of the next layer's k3 GEMM conv, whose
         leading GELU maps 0 to 0, and of the positional table at the end).

Everything else (the k3 GEMM convs, LayerNorm, the 1x1 convs, GLU, SiLU, the dropouts) is row-local or reads what a
mask point has zeroed, and computes the pad rows like any other.  `skip` leaves mask points out, to show that each
is needed.
"""
import torch
import torch.nn.functional as F

from oracle import model as om

POINTS = ("gelu0", "k15", "bn", "k3", "tail")


def params(mels, D, layers, seed=0):
    """Random float64 encoder parameters under the oracle's names, leaves with requires_grad."""
    g = torch.Generator().manual_seed(seed)

    def r(*shape, scale=1.0, shift=0.0):
        return (torch.randn(*shape, generator=g, dtype=torch.float64) * scale + shift).requires_grad_()

    P = {"enc.conv1.0.weight": r(D, mels, 3, scale=0.4), "enc.conv1.0.bias": r(D, scale=0.3)}
    for l in range(layers):
        p = f"enc.encoder.{l}"
        P[p + ".1.parametrizations.weight.original0"] = r(D, 1, 1, scale=0.2, shift=1.0)
        P[p + ".1.parametrizations.weight.original1"] = r(D, D, 3, scale=0.4)
        P[p + ".1.bias"] = r(D, scale=0.3)
        P[p + ".2.gamma"] = r(D, scale=0.2, shift=1.0)
        P[p + ".2.beta"] = r(D, scale=0.3)
        P[p + ".3.point1.weight"] = r(2 * D, D, 1, scale=0.4)
        P[p + ".3.point1.bias"] = r(2 * D, scale=0.3)
        P[p + ".3.depth.weight"] = r(D, 1, 15, scale=0.3)
        P[p + ".3.depth.bias"] = r(D, scale=0.3)
        P[p + ".3.bn.weight"] = r(D, scale=0.2, shift=1.0)
        P[p + ".3.bn.bias"] = r(D, scale=0.3)
        P[p + ".3.point2.weight"] = r(D, D, 1, scale=0.4)
        P[p + ".3.point2.bias"] = r(D, scale=0.3)
        P[p + ".5.weight"] = r(D, 1, 3, scale=0.5)
        P[p + ".5.bias"] = r(D, scale=0.3)
    return P


def stem(P, x):
    """The mel stem of encode_stream: (B, mels, T) -> (B, D, T)."""
    return F.conv1d(x, P["enc.conv1.0.weight"], P["enc.conv1.0.bias"], padding=1)


def layers_padded(P, h, lens, layers, noise, sids, skip=(), site="enc"):
    """The encoder layers of encode_stream (train mode) on the padded stem output h (B, D, T) with the mask points
    above.  -> (encodings (B, T, D), {name: masked tensor (B, D, T)}): every tensor a mask point wrote."""
    B, D, T = h.shape
    live = torch.arange(T)[None, None, :] < torch.as_tensor(lens)[:, None, None]
    masked = {}

    def Z(t, point, name):
        if point in skip:
            return t
        masked[name] = torch.where(live, t, torch.zeros((), dtype=t.dtype))
        return masked[name]

    x = h
    for l in range(layers):
        pre = f"enc.encoder.{l}"
        x = F.gelu(x)
        if l == 0:
            x = Z(x, "gelu0", "gelu0")
        W = om._weight_norm(P[pre + ".1.parametrizations.weight.original0"],
                            P[pre + ".1.parametrizations.weight.original1"])
        x = F.conv1d(x, W, P[pre + ".1.bias"], padding=1)
        x = om.channel_layer_norm(P, pre + ".2", x)
        res = x
        y = F.conv1d(x, P[pre + ".3.point1.weight"], P[pre + ".3.point1.bias"])
        y = Z(F.glu(y, dim=1), "k15", f"L{l}.k15")
        y = F.conv1d(y, P[pre + ".3.depth.weight"], P[pre + ".3.depth.bias"], padding=7, groups=D)
        w, b = P[pre + ".3.bn.weight"], P[pre + ".3.bn.bias"]
        out = []
        for s in range(B):  # batch-1 statistics over the sample's live rows
            n = T if "bn" in skip else int(lens[s])
            mean = y[s:s + 1, :, :n].mean(dim=(0, 2), keepdim=True)
            var = y[s:s + 1, :, :n].var(dim=(0, 2), unbiased=False, keepdim=True)
            out.append((y[s:s + 1] - mean) / torch.sqrt(var + 1e-5) * w[None, :, None] + b[None, :, None])
        y = F.silu(torch.cat(out))
        y = F.conv1d(y, P[pre + ".3.point2.weight"], P[pre + ".3.point2.bias"])
        y = y * noise.keep(f"{site}.L{l}.cl", sids, D, T, 0.1)
        x = Z(F.gelu(res + y), "k3", f"L{l}.k3")
        x = F.conv1d(x, P[pre + ".5.weight"], P[pre + ".5.bias"], padding=1, groups=D)
        x = F.gelu(x) * noise.keep(f"{site}.L{l}.dr", sids, D, T, 0.1)
        x = Z(x, "tail", f"L{l}.tail")
    x = x.permute(0, 2, 1).contiguous()
    return x + om.sinusoids(T, D, x.dtype), masked
