"""Helpers of the float64 reference tests (tests/test_gpu_rowops_ref.py, tests/test_gpu_msheath_steps_ref.py).

Tier A (exact): small-integer inputs make every product and sum exact in fp32 in any order, so the kernel
output must EQUAL the float64 reference on every element.  Tier B (real inputs): the error against the
float64 reference, relative to its largest entry, is bounded by max(floor, 20 x e32), where e32 is the
same reference function evaluated in float32 on the CPU -- the reference measured against itself, never
the kernel -- and the floor counts fp32 roundings.  Tier C (path equivalence): torch.equal of two paths.

Outputs are filled with SENTINEL before every call.  In tier A an element whose reference is itself 7.0 cannot be
told from an unwritten one; tiers B and C fill their outputs the same way on real-valued data, where no reference
element is 7.0, so an unwritten element shows there as an error of order one.
"""
import torch

SENTINEL = 7.0
EPS = 2.0 ** -24  # half an ulp at 1: the relative error of one fp32 rounding
FWD_TRANS = 1e-5  # the project's forward / gradient floors for kernels using __expf, erff or v_rcp
BWD_TRANS = 1e-4


def gen(seed):
    return torch.Generator().manual_seed(seed)


def ints(g, *shape, lo=-3, hi=3):
    """Integer-valued float64 data in [lo, hi]."""
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def randn(g, *shape):
    """Normal draws that fp32 holds exactly, as float64: the kernel and the reference see the same numbers."""
    return torch.randn(*shape, generator=g, dtype=torch.float32).double()


def f32(t):
    """Round to values fp32 holds exactly (after scaling or shifting randn data), still float64."""
    return t.float().double()


def dev(t):
    """fp32 (or the integer tensor itself) on the device, freshly allocated: 16-byte aligned."""
    if t is None:
        return None
    t = t.float() if t.is_floating_point() else t
    out = t.contiguous().cuda()
    assert out.data_ptr() % 16 == 0
    return out


def dev_offset(t):
    """The same values in a contiguous view that starts one float into its buffer (address % 16 == 4):
    what forces the scalar form of a float4 kernel."""
    if t is None:
        return None
    buf = torch.empty(t.numel() + 1, device="cuda")
    v = buf[1:].view(t.shape)
    v.copy_(t.float())
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def sentinel(*shape, offset=False):
    """An output buffer pre-filled with the sentinel (optionally one float into its allocation)."""
    n = 1
    for s in shape:
        n *= s
    if offset:
        buf = torch.full((n + 1,), SENTINEL, device="cuda")
        v = buf[1:].view(shape)
        assert v.data_ptr() % 16 == 4
        return v
    return torch.full(shape, SENTINEL, device="cuda")


def call(name, *args):
    """lib.call on the current stream; tensors are passed as themselves and stay alive until the launch is
    queued (a temporary's block must not be handed to the next allocation before that)."""
    from asrx import lib

    lib.call(name, *[a.data_ptr() if torch.is_tensor(a) else a for a in args], lib.stream())


def exact(name, got, ref64):
    """Tier A: every element equals the float64 reference; the reference stays below 2^24, where fp32
    holds every integer."""
    assert float(ref64.abs().max()) < 2 ** 24, name
    want = ref64.float()
    got = got.detach().cpu()
    assert got.shape == want.shape, (name, got.shape, want.shape)
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        i = tuple(int(v) for v in bad[0])
        raise AssertionError(f"{name}: {len(bad)} of {want.numel()} elements differ; first at {i}: "
                             f"got {float(got[i])}, want {float(want[i])}")


def rel(got, ref64):
    got = got.detach().double().cpu()
    return float((got - ref64).abs().max() / ref64.abs().max().clamp_min(1e-300))


def _cast32(a):
    if torch.is_tensor(a) and a.dtype == torch.float64:
        return a.float()
    return a


def tier_b(name, gots, fn, args, floors, names=None):
    """gots: the kernel's outputs, one per output of fn(*args) (args: CPU float64 tensors and plain values).
    Prints e, e32 and the bound of every output, then asserts e <= bound = max(floor, 20 e32) for all.
    Returns the rows (name, e, e32, bound)."""
    ref = fn(*args)
    r32 = fn(*[_cast32(a) for a in args])
    if torch.is_tensor(ref):
        ref, r32, gots = (ref,), (r32,), (gots,)
    if not isinstance(floors, (tuple, list)):
        floors = (floors,) * len(ref)
    rows = []
    for k, (g, r, r3, fl) in enumerate(zip(gots, ref, r32, floors)):
        if g is None:
            continue
        assert g.shape == r.shape, (name, k, g.shape, r.shape)
        assert bool(torch.isfinite(g).all()), (name, k)
        e, e32 = rel(g, r), rel(r3, r)
        bound = max(fl, 20 * e32)
        label = f"{name}.{names[k] if names else k}"
        print(f"TIERB {label:<44s} e={e:.2e} e32={e32:.2e} bound={bound:.2e}")
        rows.append((label, e, e32, bound))
    bad = [r for r in rows if not r[1] <= r[3]]
    assert not bad, bad
    return rows


def ops_floor(k):
    """(k + 1) 2^-24 for k dependent fp32 operations per element."""
    return (k + 1) * EPS
