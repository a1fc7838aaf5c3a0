"""MSheath's per-sample-length entry points (asrx_*_lens_*, csrc/rowops.hip, csrc/msheath.hip and
csrc/gemm_wn.hip) reject bad calls before any launch, like the uniform entry points they mirror:

- every refusal of the uniform twin is given by the new entry point too, with code 2 and the same text (the twin is
  called with the same bad arguments here, so the texts cannot drift apart);
- a null `lens` and a `lens` that is not 4-byte aligned are refused after the tensor checks, in that order and in
  ASRX_REQUIRE_LENS's words;
- the early return for an empty batch stands where the twin has it, ahead of the table's checks.

Host code with made-up pointers: runs only without a GPU, like test_enc_lens_args.py (a call that passed every check
would try to launch and fail for want of a device, which one control per entry point shows).
"""
import os
import re

import pytest
import torch

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="made-up pointers: host validation only, no device")

ROW_F = "x lnw lnb gw gb SH ldsh mval w2 b2 cw cb tx"
ROW_T = "rows D M Dh eps isd next_i layer L stream"
ROW_B = ("dpx x lnw lnb mean rstd dg g gw dion SH ldsh nx mval w2 cw kv m2 dx dlnw dlnb dgw dgb dSH dmval dw2 db2 dcw dcb "
         "db1")
ROW_BT = "rows D M Dh isd next_i layer L stream"
CTRL_F = "policy gpol ldg ion mgw mgb memv memw ldmw mpart mem jumps next_i layer layers"
CTRL_T = "alpha beta gam mwo act nout rec stream"
CTRL_B = "gmwo memv memw ldmw mem jumps rec layer layers B D gpolicy accp gmemw gmem gjumps has_orig mgw gmgw gmgb stream"

# name -> (argument order, uniform twin, the twin's argument order)
ENTRY = {
    "asrx_seg_colsum_lens_det": ("x part out lens B L D stream", "asrx_seg_colsum_det", "x part out B L D scale stream"),
    "asrx_msheath_row_lens_fwd2": (f"{ROW_F} px pxb mean rstd nx g ion kv m2 lens {ROW_T}", "asrx_msheath_row_fwd2",
                                   f"{ROW_F} px pxb mean rstd nx g ion kv m2 {ROW_T}"),
    "asrx_msheath_row_lens_fwd3": (f"{ROW_F} px mean rstd nx g ion kv m2 xnew part lens {ROW_T}",
                                   "asrx_msheath_row_fwd3", f"{ROW_F} px mean rstd nx g ion kv m2 xnew part {ROW_T}"),
    "asrx_msheath_row_lens_bwd2": (f"mode gj alpha gm ion {ROW_B} lens {ROW_BT}", "asrx_msheath_row_bwd2",
                                   f"mode gj alpha gm scale ion {ROW_B} {ROW_BT}"),
    "asrx_axpy_lens_row": ("x s1 y out lens B L D stream", None, None),
    "asrx_axpy_lens_row_bwd2": ("g s1 y dy ds1 dx lens B L D stream", None, None),
    "asrx_axpy_row2_lens_colsum": ("x s1 s2 y out part lens B L D next_i layer stream", "asrx_axpy_row2_colsum",
                                   "x s1 s2 y out part B L D next_i layer stream"),
    "asrx_msheath_ctrl_lens_fwd3": (f"{CTRL_F} lens B L D {CTRL_T}", "asrx_msheath_ctrl_fwd3",
                                    f"{CTRL_F} B L D {CTRL_T}"),
    "asrx_jump_lens_select4": ("xn orig xold act alpha beta gam out lens B L D stream", "asrx_jump_select4",
                               "xn orig xold act alpha beta gam out B L D stream"),
    "asrx_jump_lens_axpy_inplace": ("x out s1 s2 y orig act alpha beta gam lens B L D stream",
                                    "asrx_jump_axpy_inplace", "x out s1 s2 y orig act alpha beta gam B L D stream"),
    "asrx_jump_lens_select4_bwd_part2": ("g xn orig act alpha beta has_orig dxn dorig dx part lens B L D stream",
                                         "asrx_jump_select4_bwd_part2",
                                         "g xn orig act alpha beta has_orig dxn dorig dx part B L D stream"),
    "asrx_msheath_ctrl_lens_bwd4": (f"part lens L {CTRL_B}", "asrx_msheath_ctrl_bwd4", f"part L {CTRL_B}"),
    "asrx_axpy_row2_lens_bwd_acc2": ("g alpha gm act s1 s2 y dy ds1 ds2 dx lens B L D stream",
                                     "asrx_axpy_row2_bwd_acc2", "g alpha gm scale act s1 s2 y dy ds1 ds2 dx B L D stream"),
    "asrx_msheath_lens_dx_final": ("dx dorig has_orig gm lens B L D stream", "asrx_msheath_dx_final",
                                   "dx dorig has_orig gm B L D stream"),
    "asrx_row_lens_tiles": ("next_i layer lens L Mrows mtiles nm stream", "asrx_row_tiles",
                            "next_i layer L Mrows mtiles nm stream"),
}
NAMES = sorted({a for o in ENTRY.values() for a in (o[0] + " " + (o[2] or "")).split()})
INTS = dict(B=2, L=40, D=128, rows=80, M=8, Dh=64, ldsh=72, layer=1, layers=4, ldg=12, ldmw=128, pxb=0, mode=2, accp=1,
            Mrows=80)
FLOATS = dict(eps=1e-5, isd=0.0884, scale=0.025)
GOOD = {n: 0x7F0000000000 + (i + 1) * 0x10000000 for i, n in enumerate(NAMES)}  # distinct, 16-byte aligned
GOOD.update(INTS)
GOOD.update(FLOATS)
GOOD["stream"] = None

# name -> [(what, change)]: refusals the twin gives too (the same text is asserted by calling both)
SHARED = {
    "asrx_seg_colsum_lens_det": [],
    "asrx_msheath_row_lens_fwd2": [("M = 65", dict(M=65, ldsh=200)), ("ldsh short", dict(ldsh=70)),
                                   ("Dh = 65", dict(Dh=65, ldsh=200)), ("x + 4", dict(x=GOOD["x"] + 4)),
                                   ("L = 0 with next_i", dict(L=0))],
    "asrx_msheath_row_lens_fwd3": [("M = 65", dict(M=65, ldsh=200)), ("Dh = 65", dict(Dh=65, ldsh=200)),
                                   ("part + 4", dict(part=GOOD["part"] + 4)), ("part null", dict(part=None)),
                                   ("rows not B L", dict(rows=81)), ("px and xnew null", dict(px=None, xnew=None))],
    "asrx_msheath_row_lens_bwd2": [("mode 1", dict(mode=1)), ("mode 2, M = 65", dict(M=65, ldsh=200)),
                                   ("mode 0, M = 65", dict(mode=0, M=65, ldsh=200)),
                                   ("mode 0, dx + 4", dict(mode=0, dx=GOOD["dx"] + 4)),
                                   ("mode 2, gj null", dict(gj=None)), ("mode 2, ion null", dict(ion=None)),
                                   ("mode 2, gm + 4", dict(gm=GOOD["gm"] + 4))],
    "asrx_axpy_lens_row": [],
    "asrx_axpy_lens_row_bwd2": [],
    "asrx_axpy_row2_lens_colsum": [("D = 6", dict(D=6)), ("D = 2048", dict(D=2048)), ("s2 null", dict(s2=None))],
    "asrx_msheath_ctrl_lens_fwd3": [],
    "asrx_jump_lens_select4": [("D = 6", dict(D=6)), ("D = 2048", dict(D=2048))],
    "asrx_jump_lens_axpy_inplace": [("D = 6", dict(D=6)), ("xout is orig", dict(out=GOOD["orig"])),
                                    ("D = 2048", dict(D=2048))],
    "asrx_jump_lens_select4_bwd_part2": [("D = 6", dict(D=6))],
    "asrx_msheath_ctrl_lens_bwd4": [("D = 6", dict(D=6))],
    "asrx_axpy_row2_lens_bwd_acc2": [("D = 6", dict(D=6))],
    "asrx_msheath_lens_dx_final": [("D = 6", dict(D=6))],
    "asrx_row_lens_tiles": [("L = 0", dict(L=0)), ("M = 0", dict(Mrows=0))],
}
# refusals of the new entry points alone, with their text
OWN = {
    "asrx_axpy_lens_row": [("D = 6", dict(D=6)), ("x + 8", dict(x=GOOD["x"] + 8))],
    "asrx_axpy_row2_lens_bwd_acc2": [("dx null", dict(dx=None))],
    "asrx_msheath_row_lens_fwd2": [("rows not B L", dict(rows=81))],
}
OWN_TEXT = {
    "asrx_axpy_lens_row": "asrx_axpy_lens_row: needs d % 4 == 0, 16-byte aligned tensors and B*L*d/4 < 2^31",
    "asrx_axpy_row2_lens_bwd_acc2": "asrx_axpy_row2_lens_bwd_acc2: dx required",
    "asrx_msheath_row_lens_fwd2": "asrx_msheath_row_lens_fwd2: rows = B L < 2^31 required",
}
EMPTY = {n: [dict(B=0)] for n in ENTRY}
for n in ("asrx_msheath_row_lens_fwd2", "asrx_msheath_row_lens_fwd3", "asrx_msheath_row_lens_bwd2"):
    EMPTY[n] = [dict(rows=0)]
for n in ("asrx_axpy_lens_row", "asrx_axpy_lens_row_bwd2", "asrx_axpy_row2_lens_colsum", "asrx_jump_lens_select4",
          "asrx_jump_lens_axpy_inplace", "asrx_jump_lens_select4_bwd_part2", "asrx_axpy_row2_lens_bwd_acc2",
          "asrx_msheath_lens_dx_final"):
    EMPTY[n] = [dict(B=0), dict(L=0)]
EMPTY["asrx_row_lens_tiles"] = []  # the twin has no early return


def _call(name, order, change):
    from asrx import lib

    unknown = set(change) - set(GOOD)
    assert not unknown, unknown
    v = dict(GOOD, **change)
    lib.call(name, *[v[k] for k in order.split()])


def _text(name, order, change):
    """None for code 0, else the text of the refusal (code 2)."""
    try:
        _call(name, order, change)
    except RuntimeError as e:
        m = re.fullmatch(re.escape(name) + r" failed \(code (\d+)\): (.*)", str(e), re.S)
        assert m and m.group(1) == "2", str(e)
        return m.group(2)
    return None


def _twin_change(name, change):
    return {k: v for k, v in change.items() if k != "lens"}


CASES = []
for n in ENTRY:
    CASES += [(n, w, c, "twin") for w, c in SHARED[n]]
    CASES += [(n, w, c, OWN_TEXT[n]) for w, c in OWN.get(n, [])]
    CASES += [(n, "lens null", dict(lens=None), f"{n}: per-sample lengths: null table"),
              (n, "lens + 2", dict(lens=GOOD["lens"] + 2), f"{n}: per-sample lengths: table must be 4-byte aligned"),
              (n, "lens + 1", dict(lens=GOOD["lens"] + 1), f"{n}: per-sample lengths: table must be 4-byte aligned")]
    if SHARED[n]:  # the tensor checks answer before the table's
        w, c = SHARED[n][0]
        CASES += [(n, f"{w} before lens null", dict(c, lens=None), "twin"),
                  (n, f"{w} before lens alignment", dict(c, lens=GOOD["lens"] + 2), "twin")]
    for e in EMPTY[n]:
        k = "".join(f"{a} = {b}" for a, b in e.items())
        CASES += [(n, f"{k}: early return", e, None),
                  (n, f"{k}: early return before lens null", dict(e, lens=None), None),
                  (n, f"{k}: early return before lens alignment", dict(e, lens=GOOD["lens"] + 2), None)]
IDS = [f"{c[0][5:]}-{c[1]}".replace(" ", "_") for c in CASES]


def test_header_declares_these_entry_points():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "asrx.h")).read()
    assert set(ENTRY) <= set(re.findall(r"\b(asrx_[a-z0-9_]+)\s*\(", hdr))
    assert len({(c[0], c[1]) for c in CASES}) == len(CASES)


@pytest.mark.parametrize("name,what,change,text", CASES, ids=IDS)
def test_rejected(name, what, change, text):
    order, uniform, uorder = ENTRY[name]
    got = _text(name, order, change)
    if text == "twin":  # the uniform entry point answers the same call in the same words
        want = _text(uniform, uorder, _twin_change(name, change))
        assert want is not None and got == want, (got, want)
    else:
        assert got == text
        if text is None and uniform is not None and "lens" not in change:
            assert _text(uniform, uorder, change) is None


@pytest.mark.parametrize("name", sorted(ENTRY))
def test_a_good_call_passes_every_check(name):
    """Control: with nothing wrong the call gets as far as the launch, which fails for want of a device."""
    with pytest.raises(RuntimeError) as e:
        _call(name, ENTRY[name][0], {})
    assert "(code 2)" not in str(e.value), str(e.value)


def test_bwd_acc_without_alpha_answers_in_its_own_twins_words():
    """asrx_axpy_row2_lens_bwd_acc2 with a null alpha is asrx_axpy_row2_bwd_acc's form and gives that twin's text."""
    order = ENTRY["asrx_axpy_row2_lens_bwd_acc2"][0]
    got = _text("asrx_axpy_row2_lens_bwd_acc2", order, dict(alpha=None, D=6))
    want = _text("asrx_axpy_row2_bwd_acc", "g gm scale act s1 s2 y dy ds1 ds2 dx B L D stream", dict(D=6))
    assert want is not None and got == want and got.startswith("asrx_axpy_row2_bwd_acc:")


def test_row_bwd2_refuses_a_sample_of_2_31_rows():
    order = ENTRY["asrx_axpy_lens_row_bwd2"][0]
    assert _text("asrx_axpy_lens_row_bwd2", order, dict(B=1, L=1 << 31)) == \
        "asrx_axpy_lens_row_bwd2: L < 2^31 required"
