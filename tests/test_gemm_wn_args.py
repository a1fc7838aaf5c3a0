"""The wide-GEMM entry points (csrc/gemm_wn.hip) reject bad calls before any launch: return code 2 and a fixed
asrx_last_error() text, checked here for every argument check of every entry point, and for which check
answers when several fail.

Validation is host code, so this runs without a GPU -- and only without one: the pointers are made-up integers
with the alignment a case needs, nothing reads them here, but a case that wrongly passed validation on a machine
with a device would launch a kernel on them.
"""
import re

import pytest
import torch

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="made-up pointers: host validation only, no device")

GELU, RELU = 1, 4  # common.h enum Act


def _addr(i):
    return 0x7F0000000000 + i * 0x10000000  # distinct, 16-byte aligned


# argument order of each entry point (include/asrx.h) and a call that passes every check
ORDER = {
    "asrx_gemm_wn": "A lda conv convF convC W ldw C ldc bias Z M N K alpha beta act nj stream",
    "asrx_gemm_wn_ex": "A a_bf16 lda conv convF convC W ldw C c_bf16 ldc bias Z M N K alpha beta act nj mtiles "
    "n_mtiles stream",
    "asrx_gemm_wn_ce": "A lda W ldw Zb ldc part M N K nj stream",
    "asrx_gemm_wn_ce_f32": "A lda W ldw Zf ldc part M N K nj stream",
    "asrx_gemm_wn_head": "A lda W ldw part labels zlab M N K nj stream",
    "asrx_gemm_wn_res": "A lda W ldw C ldc bias R ldr M N K nj stream",
    "asrx_gemm_wn_rot": "A a_bf16 lda W ldw C Z ldc bias m tab L hd scale M N K nj stream",
    "asrx_gemm_wn_gact": "A a_bf16 lda W ldw bias G ldg gz ldc db M N K act nj stream",
    "asrx_gemm_wn_rows": "A lda W ldw C ldc bias Z M N K alpha beta act nj mtiles n_mtiles stream",
    "asrx_gemm_wn_router": "A lda W1 ldw b1 W2 hpre ldc logits M N K stream",
}
POINTERS = ["A", "W", "W1", "C", "bias", "Z", "Zb", "Zf", "part", "labels", "zlab", "R", "m", "tab", "G", "gz", "db",
            "mtiles", "n_mtiles", "b1", "W2", "hpre", "logits"]
GOOD = dict({n: _addr(i + 1) for i, n in enumerate(POINTERS)}, lda=64, ldw=64, ldc=384, ldr=384, ldg=384, M=256,
            N=384, K=64, conv=0, convF=0, convC=0, a_bf16=0, c_bf16=0, alpha=1.0, beta=0.0, act=0, nj=3, L=128, hd=64,
            scale=1.0, stream=None)
GOOD_FOR = {
    "asrx_gemm_wn_ex": dict(mtiles=None, n_mtiles=None),
    "asrx_gemm_wn_gact": dict(act=GELU),
}

EMPTY = "empty problem"
ALIGN = "A/W must be 16-byte aligned"
SPAN = "operand spans >= 2^31 elements"
BIG = dict(M=1 << 20, lda=2048)  # M * lda = 2^31
BIG_W = dict(N=1 << 20, ldw=2048, ldc=1 << 20, ldr=1 << 20, ldg=1 << 20, hd=64)


def _shared(name, align, strides, fp32=True, bf16=False, bf16_only=False, w="W"):
    """One case per shared check of an entry point; align / strides: its wording of the second and third."""
    on = dict(a_bf16=1) if bf16 else {}
    c = [
        (name, "M = 0", dict(M=0), EMPTY),
        (name, "N = 0", dict(N=0), EMPTY),
        (name, "K = 0", dict(K=0), EMPTY),
        (name, "A misaligned", dict(A=GOOD["A"] + 8), align),
        (name, "W misaligned", {w: GOOD[w] + 8}, align),
        (name, "K % 8", dict(K=68, lda=68 + 4 * bf16_only, ldw=72), strides),
        (name, "ldw % 8", dict(ldw=68), strides),
        (name, "A spans 2^31", BIG, SPAN),
    ]
    if fp32:
        c.append((name, "lda % 4, fp32 A", dict(lda=66), strides))
    if bf16 or bf16_only:
        c.append((name, "lda % 8, bf16 A", dict(on, lda=68), strides))
    if name != "asrx_gemm_wn_router":  # the router's one-column weight has no span check
        c.append((name, "W spans 2^31", BIG_W, SPAN))
    return c


CASES = []

n = "asrx_gemm_wn"
CASES += _shared(n, ALIGN, "K%8, lda%4, ldw%8 required")
CASES += [
    (n, "conv without F", dict(conv=1, convF=0, convC=64), "conv needs F > 0 and C % 4 == 0"),
    (n, "conv C % 4", dict(conv=1, convF=10, convC=6), "conv needs F > 0 and C % 4 == 0"),
    (n, "misaligned before K % 8", dict(A=GOOD["A"] + 4, K=68), ALIGN),
    (n, "empty before misaligned", dict(M=0, A=GOOD["A"] + 4), EMPTY),
]

n = "asrx_gemm_wn_ex"
S = "K%8, lda%4 (fp32) / lda%8 (bf16), ldw%8 required"
CASES += _shared(n, ALIGN, S, bf16=True)
CASES += [
    (n, "conv without F", dict(conv=1, convF=0, convC=64), "conv needs F > 0 and C % 4 (8 for bf16)"),
    (n, "conv C % 4", dict(conv=1, convF=10, convC=6), "conv needs F > 0 and C % 4 (8 for bf16)"),
    (n, "conv C % 8, bf16 A", dict(a_bf16=1, conv=1, convF=10, convC=12), "conv needs F > 0 and C % 4 (8 for bf16)"),
    (n, "bf16 C with beta", dict(c_bf16=1, beta=1.0), "a bf16 output takes beta = 0"),
    (n, "conv with tile list", dict(conv=1, convF=10, convC=64, mtiles=GOOD["mtiles"]), "tile lists are for plain GEMMs"),
    (n, "strides before span", dict(BIG, ldw=68), S),
    (n, "span before conv", dict(BIG, conv=1), SPAN),
    (n, "conv before bf16 C", dict(conv=1, c_bf16=1, beta=1.0), "conv needs F > 0 and C % 4 (8 for bf16)"),
]

for n, z, A in (("asrx_gemm_wn_ce", "Zb", "A/W 16-byte, Zb/part 8-byte aligned"),
                ("asrx_gemm_wn_ce_f32", "Zf", "A/W 16-byte, Zf 16-byte, part 8-byte aligned")):
    S = "K, lda, ldw % 8 and N, ldc % 4 required"
    CASES += _shared(n, A, S, fp32=False, bf16_only=True)
    CASES += [
        (n, "logits misaligned", {z: GOOD[z] + 4}, A),
        (n, "part misaligned", dict(part=GOOD["part"] + 4), A),
        (n, "N % 4", dict(N=386), S),
        (n, "ldc % 4", dict(ldc=386), S),
        (n, "nj 0", dict(nj=0), "nj in 1..3"),
        (n, "nj 4", dict(nj=4), "nj in 1..3"),
        (n, "span before nj", dict(BIG, nj=4), SPAN),
    ]
CASES.append(("asrx_gemm_wn_ce_f32", "fp32 logits 8-byte aligned only", dict(Zf=GOOD["Zf"] + 8),
              "A/W 16-byte, Zf 16-byte, part 8-byte aligned"))

n = "asrx_gemm_wn_head"
A, S = "A/W 16-byte, part 8-byte aligned", "K, lda, ldw % 8, N % 4 and lda >= K required"
CASES += _shared(n, A, S, fp32=False, bf16_only=True)
CASES += [
    (n, "part misaligned", dict(part=GOOD["part"] + 4), A),
    (n, "N % 4", dict(N=386), S),
    (n, "lda < K", dict(lda=32), S),
    (n, "nj 0", dict(nj=0), "nj in 1..3"),
    (n, "nj 4", dict(nj=4), "nj in 1..3"),
    (n, "labels without zlab", dict(zlab=None), "labels need zlab"),
    (n, "nj before labels", dict(nj=4, zlab=None), "nj in 1..3"),
]

n = "asrx_gemm_wn_res"
A, S = "A/W/C/R must be 16-byte aligned", "K, ldw % 8; lda, N, ldc, ldr % 4"
CASES += _shared(n, A, S)
CASES += [
    (n, "C misaligned", dict(C=GOOD["C"] + 8), A),
    (n, "R misaligned", dict(R=GOOD["R"] + 8), A),
    (n, "N % 4", dict(N=386), S),
    (n, "ldc % 4", dict(ldc=386), S),
    (n, "ldr % 4", dict(ldr=386), S),
    (n, "no residual", dict(R=None), "a residual input distinct from C is required"),
    (n, "residual aliases C", dict(R=GOOD["C"]), "a residual input distinct from C is required"),
    (n, "nj 2", dict(nj=2), "nj 1 or 3"),
    (n, "residual before nj", dict(R=None, nj=2), "a residual input distinct from C is required"),
]

n = "asrx_gemm_wn_rot"
A, S, H = "A/W/C/Z/tab must be 16-byte aligned", "K, ldw % 8; lda % 4 (8 bf16); N, ldc % 4", "head dim % 4, N % hd"
CASES += _shared(n, A, S, bf16=True)
CASES += [
    (n, "L = 0", dict(L=0), EMPTY),
    (n, "C misaligned", dict(C=GOOD["C"] + 8), A),
    (n, "Z misaligned", dict(Z=GOOD["Z"] + 8), A),
    (n, "tab misaligned", dict(tab=GOOD["tab"] + 8), A),
    (n, "N % 4", dict(N=386), S),
    (n, "ldc % 4", dict(ldc=386), S),
    (n, "hd 0", dict(hd=0), H),
    (n, "hd 2", dict(hd=2), H),
    (n, "hd % 4", dict(hd=6), H),
    (n, "N % hd", dict(hd=256), H),
    (n, "no row norms", dict(m=None), "row norms and angle table required"),
    (n, "no angle table", dict(tab=None), "row norms and angle table required"),
    (n, "nj 2", dict(nj=2), "nj 1 or 3"),
    (n, "strides before head dim", dict(hd=6, ldc=386), S),
    (n, "head dim before span", dict(BIG, hd=6), H),
    (n, "span before table", dict(BIG, m=None), SPAN),
    (n, "table before nj", dict(m=None, nj=2), "row norms and angle table required"),
]

n = "asrx_gemm_wn_gact"
A, S = "A/W/G 16-byte, gz 8-byte aligned", "K, ldw % 8; lda % 4 (8 bf16); N, ldc, ldg % 4"
CASES += _shared(n, A, S, bf16=True)
CASES += [
    (n, "nj 1", dict(nj=1), "nj 3 only"),
    (n, "nj 2", dict(nj=2), "nj 3 only"),
    (n, "no activation", dict(act=0), "gelu/silu/sigmoid only"),
    (n, "relu", dict(act=RELU), "gelu/silu/sigmoid only"),
    (n, "G misaligned", dict(G=GOOD["G"] + 8), A),
    (n, "gz misaligned", dict(gz=GOOD["gz"] + 4), A),
    (n, "N % 4", dict(N=386), S),
    (n, "ldc % 4", dict(ldc=386), S),
    (n, "ldg % 4", dict(ldg=386), S),
    (n, "empty before nj", dict(M=0, nj=1), EMPTY),
    (n, "nj before activation", dict(nj=1, act=0), "nj 3 only"),
    (n, "activation before misaligned", dict(act=RELU, A=GOOD["A"] + 8), "gelu/silu/sigmoid only"),
    (n, "nj before span", dict(BIG, nj=2), "nj 3 only"),
]

n = "asrx_gemm_wn_rows"
CASES += _shared(n, ALIGN, "K%8, lda%4, ldw%8 required")
CASES += [
    (n, "no tile list", dict(mtiles=None), "tile list required"),
    (n, "no tile count", dict(n_mtiles=None), "tile list required"),
    (n, "span before tile list", dict(BIG, mtiles=None), SPAN),
]

n = "asrx_gemm_wn_router"
CASES += _shared(n, ALIGN, "K%8, lda%4, ldw%8 required", w="W1")
CASES += [
    (n, "N > 384", dict(N=388), "N must be <= 384 (one tile column)"),
    (n, "empty before N", dict(M=0, N=388), EMPTY),
    (n, "N before misaligned", dict(N=388, A=GOOD["A"] + 8), "N must be <= 384 (one tile column)"),
]


def test_table_covers_every_entry_point():
    """Every asrx_gemm_wn* entry point of the header has its cases, each with the shared checks."""
    import os

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "asrx.h")).read()
    names = set(re.findall(r"\b(asrx_gemm_wn[a-z0-9_]*)\s*\(", hdr))
    assert names == set(ORDER)
    for name in names:
        texts = {c[3] for c in CASES if c[0] == name}
        assert {EMPTY, SPAN} <= texts and len(texts) >= 4, name
    assert len({(c[0], c[1]) for c in CASES}) == len(CASES)


@pytest.mark.parametrize("name,what,change,text", CASES, ids=[f"{c[0][5:]}-{c[1]}".replace(" ", "_") for c in CASES])
def test_rejected(name, what, change, text):
    from asrx import lib

    unknown = set(change) - set(GOOD)
    assert not unknown, unknown
    v = dict(GOOD, **GOOD_FOR.get(name, {}))
    v.update(change)
    args = [v[k] for k in ORDER[name].split()]
    with pytest.raises(RuntimeError) as e:
        lib.call(name, *args)
    assert str(e.value) == f"{name} failed (code 2): {name}: {text}"
