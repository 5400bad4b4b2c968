"""Shared pieces of the kernel-level float64 parity tests (test_fusion_kernels_gpu.py, test_optim_kernels_gpu.py,
test_nms_kernels_gpu.py): the reduction-mode fixture, the bar that is derived from the reference's own rounding, and
small input builders.  Not a test module and not a conftest: every test file imports what it needs by name.

The bar.  For a quantity computed in floating point the same formula is evaluated on the CPU once in float64 (``r64``)
and once in float32 (``r32``), both from inputs already rounded to the kernel's storage dtype.  With
``e_ref = max|r32 - r64|`` and ``s = max|r64|`` the kernel has to satisfy

    max|gpu - r64| <= 8 * e_ref + u * s,        u = half an ulp of the OUTPUT dtype (2^-24 f32, 2^-11 f16, 2^-8 bf16).

The 8 pays for a summation order other than torch's (wave shuffles, workgroup partials, atomics in arrival order) and
for fast intrinsics; it is a margin over the reference's rounding, never over the code under test.  Every element is
compared: there is no mask and no "all but k %".

Long sums.  torch's CPU sum is a cascade (error ~ log n), so ``e_ref`` says nothing about a sum in which one f32 accumulator
takes k terms in sequence: there the textbook bound is  |error| <= k * 2^-24 * sum|terms|  (Higham, Accuracy and Stability of
Numerical Algorithms, section 4.2: k = the largest number of additions any term passes through).  Tests of such sums pass this
as ``extra = sum_bound(k, sum|terms|)`` with k taken from the kernel's documented geometry; it grows with the shape only, so
the small shapes keep the plain bar.
"""
import pytest
import torch

DEV = "cuda"
HALF_ULP = {torch.float32: 2.0 ** -24, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
FACTOR = 8.0


def ops():
    from sy11 import ops as o
    return o


def lib():
    from sy11 import _lib
    return _lib


@pytest.fixture(params=["ordered", "atomic"])
def reduction_mode(request):
    """Runs the test once with the ordered reductions of csrc/det.h and once with the atomic ones (what bench.py times);
    the library option is restored afterwards (the session default comes from tests/conftest.py)."""
    _lib = lib()
    prev = _lib.get_option("deterministic")
    _lib.set_option("deterministic", 1 if request.param == "ordered" else 0)
    yield request.param
    _lib.set_option("deterministic", prev)


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g, dtype=torch.float64) * 2 - 1).float() * scale


def rounded(t, dtype):
    """CPU f32 tensor rounded through the kernel's storage dtype."""
    return t.to(dtype).float()


def same_bits(a, b):
    """Bit-for-bit equality of two f32 tensors (+0 / -0 and NaN payloads count)."""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))


def sum_bound(depth, abs_sum):
    """Worst-case rounding error of an f32 sum in which a term passes through at most `depth` additions."""
    return float(depth) * 2.0 ** -24 * float(abs_sum)


class Bars:
    """Collects ``gpu_err, e_ref, ratio`` per quantity, prints each line, and fails once with all of them."""

    def __init__(self, what):
        self.what, self.lines, self.bad = what, [], []

    def add(self, name, gpu, r64, r32, out_dtype=torch.float32, factor=FACTOR, extra=0.0):
        gpu = gpu.detach().cpu().double()
        r64 = r64.detach().double()
        r32 = r32.detach().double()
        assert gpu.shape == r64.shape == r32.shape, (name, tuple(gpu.shape), tuple(r64.shape), tuple(r32.shape))
        assert bool(torch.isfinite(r64).all()) and bool(torch.isfinite(r32).all()), f"{name}: the reference is not finite"
        if gpu.numel() == 0:
            return
        e_ref = (r32 - r64).abs().max().item()
        s = r64.abs().max().item()
        diff = (gpu - r64).abs()
        err = diff.max().item() if bool(torch.isfinite(gpu).all()) else float("inf")
        bar = factor * e_ref + HALF_ULP[out_dtype] * s + extra
        ratio = err / bar if bar > 0 else (0.0 if err == 0 else float("inf"))
        line = f"[parity] {self.what} {name}: gpu_err {err:.3e} e_ref {e_ref:.3e} scale {s:.3e} bar {bar:.3e} ratio {ratio:.3f} err/e_ref {err / e_ref if e_ref > 0 else float('nan'):.2f}"
        print(line)
        self.lines.append(line)
        if not err <= bar:
            self.bad.append(line)

    def check(self):
        assert not self.bad, "over the bar (8 * e_ref + u * scale):\n" + "\n".join(self.bad) + "\nall quantities:\n" + "\n".join(self.lines)


def nhwc_view(x_cpu_nhwc, dtype, strided, fill=1.0e3):
    """(B,H,W,C) cpu f32 -> device tensor of ``dtype``: contiguous, or the channel slice [vec : vec + C] of a buffer that is two
    16-byte vectors wider (ld > C, the slice starts 16 bytes in) and is filled with ``fill`` elsewhere, so that a read with the
    wrong stride or offset cannot go unnoticed.  Returns (view, whole buffer)."""
    B, H, W, Cn = x_cpu_nhwc.shape
    if not strided:
        v = x_cpu_nhwc.to(DEV, dtype).contiguous()
        return v, v
    vec = 16 // torch.empty((), dtype=dtype).element_size()
    buf = torch.full((B, H, W, Cn + 2 * vec), fill, dtype=dtype, device=DEV)
    v = buf[..., vec:vec + Cn]
    v.copy_(x_cpu_nhwc.to(DEV, dtype))
    return v, buf


def outside_untouched(buf, Cn, fill=1.0e3):
    """The pad columns of a buffer made by nhwc_view(strided=True) still hold ``fill``."""
    if buf.shape[-1] == Cn:
        return True
    vec = (buf.shape[-1] - Cn) // 2
    pad = torch.cat((buf[..., :vec], buf[..., vec + Cn:]), -1).float()
    return bool((pad == fill).all())
