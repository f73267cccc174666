"""dosx_grad_accumulate / _f64 (csrc/grad_accumulate.hip) on a real MI355X, through ``ops.grad_accumulate`` / ``grad_accumulate64``:
bit for bit ``torch.add`` on the device (the copy form: the operand's own bits) at every size where the kernel takes another path
- below, at and above one 16-byte vector, one workgroup's span and the capped grid's sweep (sizes from the header's constants) -
in all four forms (copy, dst apart, dst == a, dst == b), with the scalar triple absent, copying and adding; NaN, +-inf, -0.0 and
denormals among the elements; a guard band on both sides of dst bitwise untouched; two runs bitwise equal.

The NaNs stand where the other operand is finite (and the infinities never meet their opposite): which of two NaN payloads an
add returns is the instruction's business, not this kernel's."""
import pytest
import torch

from dostransformer_amd import _abi
from tests.gpu_util import DEV

pytestmark = pytest.mark.gpu

DTYPES = {"fp32": torch.float32, "float64": torch.float64}
BAND = 64                                          # guard elements on each side of dst (a multiple of 16 bytes: dst stays aligned)
FORMS = ("copy", "apart", "dst_is_a", "dst_is_b")
SCALARS = ("none", "copy", "add")


def _sizes(dtype):
    per = 16 // torch.empty(0, dtype=dtype).element_size()
    span = _abi.DOSX_ACCUM_THREADS * per
    sweep = _abi.DOSX_ACCUM_MAX_BLOCKS * span
    # sweep + 1: one more than the capped grid covers in one trip (its tail); sweep + per + 1: one more VECTOR than that, so that
    # the stride loop goes round a second time, and a tail behind it
    return sorted({1, per - 1, per, per + 1, span - 1, span, span + 1, sweep + 1, sweep + per + 1} - {0})


CASES = [(dn, n) for dn, dt in DTYPES.items() for n in _sizes(dt)]


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _same_bits(x, y):
    return x.shape == y.shape and torch.equal(_bits(x), _bits(y))


def _operands(n, dtype, seed):
    """a, b of n elements with the special values at fixed places (wrapped into short buffers), b finite wherever a is NaN and
    the reverse; infinities of one sign only per index."""
    gen = torch.Generator().manual_seed(seed)
    a = torch.randn(n, generator=gen, dtype=torch.float64).to(dtype)
    b = (torch.randn(n, generator=gen, dtype=torch.float64) * 1e-3).to(dtype)
    tiny = torch.finfo(dtype).tiny
    nan, inf = float("nan"), float("inf")
    special = [(nan, 1.5), (0.25, nan), (inf, 2.0), (-inf, -inf), (3.0, -inf), (inf, inf), (-0.0, -0.0), (-0.0, 0.0), (0.0, -0.0),
               (tiny / 4, tiny / 8), (tiny / 2, -tiny / 2), (tiny, -tiny / 4), (-tiny / 16, 0.0)]
    for k, (x, y) in enumerate(special):
        for base in (0, n // 2, n - len(special)):                  # head, middle, and the tail elements behind the last vector
            i = (base + k) % n
            a[i], b[i] = x, y
    return a.to(DEV), b.to(DEV)


def _banded(t, fill):
    """t inside a larger buffer: [BAND | t | BAND], the bands filled with ``fill`` - (buffer, view of the middle)"""
    buf = torch.full((t.numel() + 2 * BAND,), fill, dtype=t.dtype, device=t.device)
    buf[BAND:BAND + t.numel()] = t
    return buf, buf[BAND:BAND + t.numel()]


def _run(fn, form, scalar, a0, b0, s0):
    """one launch in the given form on fresh copies -> (dst buffer with its bands, the scalar's [3] buffer)"""
    n, dt = a0.numel(), a0.dtype
    sent = -7.25
    abuf, a = _banded(a0, sent)
    bbuf, b = _banded(b0, sent)
    if form in ("copy", "apart"):
        dbuf, dst = _banded(torch.full((n,), float("nan"), dtype=dt, device=DEV), sent)      # a stale NaN must not leak
    elif form == "dst_is_a":
        dbuf, dst = abuf, a
    else:
        dbuf, dst = bbuf, b
    s = s0.clone()                                  # [sdst, sa, sb]
    kw = {} if scalar == "none" else {"sdst": s[0:1], "sa": s[1:2], "sb": s[2:3] if scalar == "add" else None}
    fn(dst, a, None if form == "copy" else b, n, **kw)
    return dbuf, s


@pytest.mark.parametrize("dtn,n", CASES, ids=[f"{d}-{n}" for d, n in CASES])
def test_bitwise_torch_add_in_every_form(dtn, n):
    from dostransformer_amd import ops
    dt = DTYPES[dtn]
    fn = ops.grad_accumulate if dt == torch.float32 else ops.grad_accumulate64
    a0, b0 = _operands(n, dt, seed=n % 9973)
    want_add = torch.add(a0, b0)                   # the reference, once for all forms of this size
    assert bool(torch.isnan(want_add).any()) and bool(torch.isinf(want_add).any()) or n < 8
    s0 = torch.tensor([float("nan"), 0.1, -0.0], dtype=dt, device=DEV)
    s_add = torch.add(s0[1:2], s0[2:3])
    band = torch.full((BAND,), -7.25, dtype=dt, device=DEV)
    for form in FORMS:
        want = a0 if form == "copy" else want_add
        for scalar in SCALARS:
            dbuf, s = _run(fn, form, scalar, a0, b0, s0)
            tag = (dtn, n, form, scalar)
            assert _same_bits(dbuf[BAND:BAND + n], want), tag
            assert _same_bits(dbuf[:BAND], band) and _same_bits(dbuf[BAND + n:], band), tag + ("guard band",)
            assert _same_bits(s[1:], s0[1:]), tag + ("sa, sb are only read",)
            if scalar == "none":
                assert _same_bits(s[:1], s0[:1]), tag
            else:
                assert _same_bits(s[:1], s0[1:2] if scalar == "copy" else s_add), tag
        again, _ = _run(fn, form, "add", a0, b0, s0)
        assert _same_bits(again, dbuf), (dtn, n, form, "two runs")


@pytest.mark.parametrize("dtn", list(DTYPES))
def test_scalar_in_place_and_the_window_order(dtn):
    """sdst == sa (how a window carries its loss) and the three launches of a window of three: copy, acc += g, g = acc + g -
    ((g1 + g2) + g3) bit for bit, the accumulator's stale NaNs never read."""
    from dostransformer_amd import ops
    dt = DTYPES[dtn]
    fn = ops.grad_accumulate if dt == torch.float32 else ops.grad_accumulate64
    n = 16 // torch.empty(0, dtype=dt).element_size() * 37 + 1
    gen = torch.Generator().manual_seed(3)
    gs = [torch.randn(n, generator=gen, dtype=torch.float64).to(dt).to(DEV) * 10.0 ** k for k in (0, -3, 2)]
    ls = [torch.randn(1, generator=gen, dtype=torch.float64).to(dt).to(DEV) for _ in gs]
    acc = torch.full((n + 5,), float("nan"), dtype=dt, device=DEV)
    total = torch.full((1,), float("nan"), dtype=dt, device=DEV)
    grad = gs[0].clone()
    fn(acc, grad, None, n, sdst=total, sa=ls[0])
    grad.copy_(gs[1])
    fn(acc, acc, grad, n, sdst=total, sa=total, sb=ls[1])
    grad.copy_(gs[2])
    fn(grad, acc, grad, n, sdst=total, sa=total, sb=ls[2])
    assert _same_bits(grad, (gs[0] + gs[1]) + gs[2])
    assert _same_bits(acc[:n], gs[0] + gs[1]) and bool(torch.isnan(acc[n:]).all())
    assert _same_bits(total, (ls[0] + ls[1]) + ls[2])
    assert not _same_bits(grad, gs[0] + (gs[1] + gs[2]))               # (the order is visible at these magnitudes)


def test_python_side_refusals():
    from dostransformer_amd import ops
    from dostransformer_amd._lib import DosxError
    x, y = torch.zeros(64, device=DEV), torch.ones(64, device=DEV)
    with pytest.raises(TypeError):
        ops.grad_accumulate(x, y.double())
    with pytest.raises(TypeError):
        ops.grad_accumulate64(x, y)
    with pytest.raises(TypeError):
        ops.grad_accumulate(x.view(8, 8)[:, :4], y)
    with pytest.raises(ValueError):
        ops.grad_accumulate(x, y, None, 65)
    with pytest.raises(ValueError):
        ops.grad_accumulate(x, y, sdst=x[:1])
    with pytest.raises(DosxError, match="dosx_grad_accumulate: dst overlaps a"):
        ops.grad_accumulate(x[4:], x, None, 32)
    with pytest.raises(DosxError, match="16-byte"):
        ops.grad_accumulate(x[1:], y, None, 32)
    ops.grad_accumulate(x, y)                                           # default n: all of it; no scalar
    assert torch.equal(x, y)
