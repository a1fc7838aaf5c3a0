"""The encoder's per-sample-length entry points (asrx_*_lens_*, csrc/rowops.hip and csrc/stepops.hip) reject bad
calls before any launch, like the uniform entry points they mirror:

- every refusal of the uniform twin is given by the new entry point too, with code 2 and the same text (each twin
  is called with the same bad arguments here, so the texts cannot drift apart);
- what only the twin's non-float4 fall-back kernels would take (C % 4 != 0, a misaligned tensor, 2^31 elements or
  more, an untiled K) is refused, as the LENS kernels exist in the float4 form only;
- a null `lens` and a `lens` that is not 4-byte aligned are refused after the tensor checks, in that order;
- the early return for an empty batch stands ahead of all of them, where the twin has it.

Host code with made-up pointers: runs only without a GPU, like test_attn_lens_args.py (a call that passed every
check would try to launch and fail for want of a device, which one control per entry point shows).
"""
import os
import re

import pytest
import torch

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="made-up pointers: host validation only, no device")


def _addr(i):
    return 0x7F0000000000 + i * 0x10000000  # distinct, 16-byte aligned


# name -> (argument order, uniform twin, the twin's argument order or None when its sizes differ)
ENTRY = {
    "asrx_act_lens_fwd": ("x y lens B T C act stream", None, None),
    "asrx_act_lens_bwd": ("g x dx lens B T C act stream", None, None),
    "asrx_act_dropout_lens_fwd": ("z res y lens B T C sid key p act act2 stream", "asrx_act_dropout_fwd",
                                  "z res y B T C sid key p act act2 stream"),
    "asrx_act_dropout_lens_bwd": ("g z dz lens B T C sid key p act act2 stream", "asrx_act_dropout_bwd",
                                  "g z dz B T C sid key p act act2 stream"),
    "asrx_dwconv_lens_fwd": ("x w b y lens B T C K stream", "asrx_dwconv_fwd", "x w b y B T C K stream"),
    "asrx_dwconv_pre_lens_bwd": ("g x z w dz dw db lens B T C K pre stream", "asrx_dwconv_pre_bwd",
                                 "g x z w dz dw db B T C K pre stream"),
    "asrx_bn_silu_lens_fwd": ("x w b y mean rstd lens B T C eps ubs stream", "asrx_bn_silu_fwd",
                              "x w b y mean rstd B T C eps ubs stream"),
    "asrx_bn_silu_lens_bwd": ("g x mean rstd w b sg sgx dx dw db lens B T C stream", "asrx_bn_silu_bwd",
                              "g x mean rstd w b sg sgx dx dw db B T C stream"),
    "asrx_bn_running_lens": ("mean rstd rm rv nbt lens B C T eps mom stream", "asrx_bn_running",
                             "mean rstd rm rv nbt B C T eps mom stream"),
}
POINTERS = "x y g dx z res dz w b dw db mean rstd sg sgx rm rv nbt lens".split()
GOOD = dict({n: _addr(i + 1) for i, n in enumerate(POINTERS)}, B=2, T=40, C=8, K=15, pre=1, act=1, act2=0, sid=0,
            key=5, p=0.1, eps=1e-5, ubs=1, mom=0.1, stream=None)
OK = None  # the early return: code 0

AD = "act_dropout: needs C % 4 == 0 and 16-byte aligned tensors"
DWK = "dwconv: K must be odd and <= 15"
DWL = ("asrx_dwconv_lens_fwd: K of 3, 5, 7 or 15 with C % 4 == 0, 16-byte aligned tensors and fewer than "
       "2^31 elements")
PRE = ("asrx_dwconv_pre_bwd: GLU -> k15 or GELU -> k3 with C % 4 == 0, 16-byte aligned tensors and fewer than 2^31 "
       "elements")
BNF = "asrx_bn_silu_fwd: needs C % 4 == 0, 16-byte aligned tensors and B*T*C < 2^31"
BNB = "asrx_bn_silu_bwd: needs C % 4 == 0, 16-byte aligned tensors and B*T*C < 2^31"
BNT = "asrx_bn_silu_lens_fwd: train-mode statistics only"
ACF = "asrx_act_lens_fwd: needs C % 4 == 0, 16-byte aligned tensors and B*T*C < 2^31"
ACB = "asrx_act_lens_bwd: needs C % 4 == 0, 16-byte aligned tensors and B*T*C < 2^31"
BIG = dict(B=1 << 11, T=1 << 10, C=1 << 10)  # 2^31 elements


def _lnull(n):
    return f"{n}: per-sample lengths: null table"


def _lalign(n):
    return f"{n}: per-sample lengths: table must be 4-byte aligned"


def _mis(names, text):
    return [(f"{p} + 8", {p: GOOD[p] + 8}, text, True) for p in names.split()]


# name -> [(what, change, text, shared with the twin)]
REFUSALS = {
    "asrx_act_lens_fwd": [("C = 6", dict(C=6), ACF, False), ("2^31 elements", BIG, ACF, False)]
    + [(w, c, t, False) for w, c, t, _ in _mis("x y", ACF)],
    "asrx_act_lens_bwd": [("C = 6", dict(C=6), ACB, False), ("2^31 elements", BIG, ACB, False)]
    + [(w, c, t, False) for w, c, t, _ in _mis("g x dx", ACB)],
    "asrx_act_dropout_lens_fwd": [("C = 6", dict(C=6), AD, True)] + _mis("z res y", AD),
    "asrx_act_dropout_lens_bwd": [("C = 6", dict(C=6), AD, True)] + _mis("g z dz", AD),
    "asrx_dwconv_lens_fwd": [("K = 4", dict(K=4), DWK, True), ("K = 17", dict(K=17), DWK, True),
                             ("K = 4 before the early return", dict(K=4, B=0), DWK, True),
                             ("K = 9: not tiled", dict(K=9), DWL, False), ("C = 6", dict(C=6), DWL, False),
                             ("2^31 elements", BIG, DWL, False)]
    + [(w, c, t, False) for w, c, t, _ in _mis("x y b", DWL)],
    "asrx_dwconv_pre_lens_bwd": [("C = 6", dict(C=6), PRE, True), ("glu with K = 3", dict(K=3), PRE, True),
                                 ("gelu with K = 15", dict(pre=2), PRE, True), ("pre = 0", dict(pre=0), PRE, True),
                                 ("2^31 elements (2C wide)", dict(B=1 << 10, T=1 << 10, C=1 << 10), PRE, True)]
    + _mis("g x z dz", PRE),
    "asrx_bn_silu_lens_fwd": [("C = 6", dict(C=6), BNF, True), ("2^31 elements", BIG, BNF, True),
                              ("running statistics", dict(ubs=0), BNT, False),
                              ("alignment before running statistics", dict(ubs=0, x=GOOD["x"] + 8), BNF, False)]
    + _mis("x w b y mean rstd", BNF),
    "asrx_bn_silu_lens_bwd": [("C = 6", dict(C=6), BNB, True), ("2^31 elements", BIG, BNB, True)]
    + _mis("g x mean rstd w b sg sgx dx", BNB),
    "asrx_bn_running_lens": [],
}
EMPTY = {n: [dict(B=0), dict(T=0)] for n in ENTRY}
EMPTY["asrx_act_lens_fwd"] = EMPTY["asrx_act_lens_bwd"] = [dict(B=0), dict(T=0), dict(C=0)]
EMPTY["asrx_act_dropout_lens_fwd"] = EMPTY["asrx_act_dropout_lens_bwd"] = [dict(B=0), dict(T=0), dict(C=0)]
EMPTY["asrx_bn_running_lens"] = [dict(C=0)]

CASES = []
for n in ENTRY:
    CASES += [(n, w, c, t, tw) for w, c, t, tw in REFUSALS[n]]
    first = REFUSALS[n][0] if REFUSALS[n] else None
    CASES += [
        (n, "lens null", dict(lens=None), _lnull(n), False),
        (n, "lens + 2", dict(lens=GOOD["lens"] + 2), _lalign(n), False),
        (n, "lens + 1", dict(lens=GOOD["lens"] + 1), _lalign(n), False),
    ]
    if first is not None:  # the tensor checks answer before the table's
        CASES += [(n, f"{first[0]} before lens null", dict(first[1], lens=None), first[2], False),
                  (n, f"{first[0]} before lens alignment", dict(first[1], lens=GOOD["lens"] + 2), first[2], False)]
    for e in EMPTY[n]:  # the early return stands ahead of every check but asrx_dwconv_fwd's K
        k = "".join(f"{a} = {b}" for a, b in e.items())
        CASES += [(n, f"{k}: early return", e, OK, True),
                  (n, f"{k}: early return before lens null", dict(e, lens=None), OK, False),
                  (n, f"{k}: early return before lens alignment", dict(e, lens=GOOD["lens"] + 2), OK, False)]
        if first is not None and n != "asrx_dwconv_lens_fwd" and not set(e) & set(first[1]):
            CASES.append((n, f"{k}: early return before {first[0]}", dict(first[1], **e), OK, True))
IDS = [f"{c[0][5:]}-{c[1]}".replace(" ", "_") for c in CASES]


def _call(name, order, change):
    from asrx import lib

    unknown = set(change) - set(GOOD)
    assert not unknown, unknown
    v = dict(GOOD, **change)
    lib.call(name, *[v[k] for k in order.split()])


def _text(name, order, change):
    """None for code 0, else the text of the refusal."""
    try:
        _call(name, order, change)
    except RuntimeError as e:
        m = re.fullmatch(re.escape(name) + r" failed \(code (\d+)\): (.*)", str(e), re.S)
        assert m and m.group(1) == "2", str(e)
        return m.group(2)
    return None


def test_header_declares_these_entry_points():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "asrx.h")).read()
    assert set(re.findall(r"\b(asrx_[a-z0-9_]*_lens(?:_fwd|_bwd)?)\s*\(", hdr)) == set(ENTRY)
    assert len({(c[0], c[1]) for c in CASES}) == len(CASES)
    # every refusal text of the new entry points is pinned here
    src = ""
    for f in ("rowops.hip", "stepops.hip"):
        src += open(os.path.join(root, "asr-model_amd", "csrc", f)).read()
    for n in ENTRY:
        body = src[src.index(f"int {n}("):]
        body = body[:body.index("\n}\n")]
        for t in re.findall(r'ASRX_REQUIRE\((?:[^"]|\n)*?((?:"[^"]*"\s*)+)\)', body):
            t = "".join(re.findall(r'"([^"]*)"', t)).replace("%%", "%")
            assert any(c[0] == n and c[3] == t for c in CASES), (n, t)


@pytest.mark.parametrize("name,what,change,text,twin", CASES, ids=IDS)
def test_rejected(name, what, change, text, twin):
    order, uniform, uorder = ENTRY[name]
    assert _text(name, order, change) == text
    if twin and uniform is not None:  # the uniform entry point answers the same call in the same words
        assert _text(uniform, uorder, change) == text


@pytest.mark.parametrize("name", sorted(ENTRY))
def test_a_good_call_passes_every_check(name):
    """Control: with nothing wrong the call gets as far as the launch, which fails for want of a device."""
    with pytest.raises(RuntimeError) as e:
        _call(name, ENTRY[name][0], {})
    assert "(code 2)" not in str(e.value), str(e.value)
