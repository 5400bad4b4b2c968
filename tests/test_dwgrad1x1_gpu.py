"""The fused input + filter gradient of a dense 1x1 layer (sy11_conv2d_dgrad_wgrad_1x1, csrc/dwgrad1x1.hip) against float64:
dx = dy * W^T and dW = dy^T * x computed on the CPU from the same 16-bit inputs, with proof that the fused kernel is what ran
("wgrad_last_cfg" == 101 before anything is compared).

Bar: on the same inputs the existing pair conv2d_dgrad + conv2d_wgrad is run too; the fused result's largest error against
float64 may be at most TWICE the pair's (per output, per case).  The factor 2 allows for a different summation order over at most
256 terms (dx) and for partial sums that meet in dW through a few more f32 atomics; it is derived from the pair, never from the
fused output.  Both errors are printed.

Cases (the smallest shapes at which this kernel can still go wrong):
  pixels    M = 126 (one 128-pixel tile with a tail), M = 130 (a second, nearly empty tile; two workgroups),
            M = 128 * 5 + 3 on a grid forced to two workgroups (runs of three and of three tiles, the last one a tail)
  channels  (C, N) = (16, 16), (48, 32), (96, 128), (128, 64), (256, 256): sizes that are no multiple of the 32-wide MFMA block or
            of the 64 / 128 / 256 tile widths, C != N both ways, and the largest filter (two column blocks)
  layouts   contiguous tensors, and dy / x / dx as channel slices of wider tensors whose other channels hold a sentinel
  every case with `accumulate` off and on (dx pre-filled: pre-fill + result), dW pre-filled non-zero (the kernel adds), f16 and bf16.
Ordered mode and the engine's dispatch: the tests at the end.
"""
import functools

import pytest
import torch

from tests.test_conv_variants_gpu import DEV, SENTINEL, lib, ops, options

pytestmark = pytest.mark.gpu

FUSED_CFG = 101
PIXELS = {"m126": (2, 7, 9, 0), "m130": (2, 5, 13, 0), "m643_2wg": (1, 1, 128 * 5 + 3, 2)}       # B, H, W, forced workgroups
CHANNELS = [(16, 16), (48, 32), (96, 128), (128, 64), (256, 256)]
MARGIN = 2.0


@functools.lru_cache(maxsize=None)
def reference(pix, C, N, dtype):
    """16-bit operands (uniform in [-1, 1), a seed per case) and the float64 results, computed once; callers do not write into them."""
    B, H, W, _ = PIXELS[pix]
    gen = torch.Generator().manual_seed(1000 * C + N + len(pix))
    u = lambda *s: (torch.rand(*s, generator=gen) * 2 - 1).to(dtype)
    r = {"dy": u(B, H, W, N), "x": u(B, H, W, C), "w": (u(N, C).float() / N ** 0.5).to(dtype), "dx0": u(B, H, W, C), "dw0": u(N, C).float()}
    dy, x, w = (r[k].double().reshape(-1, r[k].shape[-1]) for k in ("dy", "x", "w"))
    r["dx"] = (dy @ w).reshape(B, H, W, C)
    r["dw"] = dy.t() @ x
    return r


def sliced(t, dtype, on):
    """Device copy of NHWC `t`: contiguous, or channels 8 .. 8 + C of a buffer 24 channels wider that holds the sentinel elsewhere."""
    Cn = t.shape[-1]
    buf = torch.full(tuple(t.shape[:-1]) + (Cn + (24 if on else 0),), SENTINEL, dtype=dtype, device=DEV)
    v = buf[..., 8:8 + Cn] if on else buf
    v.copy_(t.to(DEV, dtype))
    return buf, v


def untouched(buf, Cn, on, what):
    if on:
        assert (buf[..., :8] == SENTINEL).all() and (buf[..., 8 + Cn:] == SENTINEL).all(), f"{what}: wrote outside its channel slice"


def worst(got, ref):
    return (got.double().cpu() - ref).abs().max().item()


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("layout", ["contiguous", "slices"])
@pytest.mark.parametrize("cn", CHANNELS, ids=lambda cn: f"c{cn[0]}n{cn[1]}")
@pytest.mark.parametrize("pix", list(PIXELS))
def test_fused_against_float64_and_the_pair(pix, cn, layout, dtype):
    o, (C, N), on = ops(), cn, layout == "slices"
    B, H, W, forced = PIXELS[pix]
    r = reference(pix, C, N, dtype)
    dyb, dy = sliced(r["dy"], dtype, on)
    xb, x = sliced(r["x"], dtype, on)
    w = r["w"].to(DEV).reshape(N, 1, 1, C).contiguous()
    wt = o.weight_transpose(w)
    for accumulate in (False, True):
        what = f"{pix} {C}->{N} {layout} {str(dtype)[6:]} accumulate={accumulate}"
        want_dx = r["dx"] + (r["dx0"].double() if accumulate else 0)
        want_dw = r["dw0"].double() + r["dw"]
        got = {}
        for name in ("pair", "fused"):
            dxb, dx = sliced(r["dx0"], dtype, on)
            dw = r["dw0"].to(DEV).reshape(N, 1, 1, C).clone()
            with options(tune=0, deterministic=0, dwgrad_wg=forced):
                if name == "pair":
                    o.conv2d_dgrad(dy, wt, dx, (B, H, W, N), 1, 1, 0, 1, 1, accumulate=accumulate)
                    o.conv2d_wgrad(x, dy, dw, 1, 1, 0, 1)
                    assert lib().get_option("wgrad_last_cfg") != FUSED_CFG
                else:
                    o.conv2d_dgrad_wgrad_1x1(dy, x, wt, dx, dw, accumulate=accumulate)
                    assert lib().get_option("wgrad_last_cfg") == FUSED_CFG, "the fused kernel did not run"
            torch.cuda.synchronize()
            untouched(dxb, C, on, f"{what} {name} dx")
            got[name] = (worst(dx, want_dx), worst(dw.reshape(N, C), want_dw))
        untouched(dyb, N, on, f"{what} dy")
        untouched(xb, C, on, f"{what} x")
        print(f"\nDWGRAD1X1 {what}: max |err| dx pair {got['pair'][0]:.3e} fused {got['fused'][0]:.3e}; dW pair {got['pair'][1]:.3e} fused {got['fused'][1]:.3e}")
        assert got["pair"][0] > 0 and got["pair"][1] > 0, f"{what}: the pair is exact here, it gives no bar"
        assert got["fused"][0] <= MARGIN * got["pair"][0], f"{what}: dx error {got['fused'][0]:.3e} above {MARGIN} x the pair's {got['pair'][0]:.3e}"
        assert got["fused"][1] <= MARGIN * got["pair"][1], f"{what}: dW error {got['fused'][1]:.3e} above {MARGIN} x the pair's {got['pair'][1]:.3e}"


def test_refusals_launch_nothing():
    o, E = ops(), lib().Sy11Error
    r = reference("m126", 48, 32, torch.float16)
    dy, x = r["dy"].to(DEV), r["x"].to(DEV)
    wt = o.weight_transpose(r["w"].to(DEV).reshape(32, 1, 1, 48).contiguous())
    dx, dw = torch.zeros_like(x), torch.zeros(32, 1, 1, 48, device=DEV)
    with options(deterministic=1), pytest.raises(E):                      # ordered mode: the pair's job
        o.conv2d_dgrad_wgrad_1x1(dy, x, wt, dx, dw)
    with options(deterministic=0):
        with pytest.raises(E):                                            # f32
            o.conv2d_dgrad_wgrad_1x1(dy.float(), x.float(), wt.float(), dx.float(), dw)
        with pytest.raises(E):                                            # N = 24: no multiple of 16
            o.conv2d_dgrad_wgrad_1x1(dy[..., :24], x, wt[..., :24].contiguous(), dx, torch.zeros(24, 1, 1, 48, device=DEV))
    torch.cuda.synchronize()
    assert (dx == 0).all() and (dw == 0).all()


# ------------------------------------------------------------------------------------------------------------ engine
def _c3k2_backward(dtype, fused, det, monkeypatch, threshold=512):
    """One C3k2 block at 2 x 16 x 16 (M = 512), forward and backward: (input gradient, parameter gradients by name, names of the C-ABI calls)."""
    from sy11.nn.modules import conv as conv_mod
    from sy11.nn.modules.block import C3k2
    monkeypatch.setattr(conv_mod, "_DWGRAD_FUSED_MIN_PIXELS", threshold)
    torch.manual_seed(11)
    m = C3k2(32, 32, 1)                                  # cv1: 32 -> 32 and cv2: 48 -> 32 are the dense 1x1 layers
    m._sy11_dtype = dtype
    m = m.to(DEV).train()
    gen = torch.Generator().manual_seed(12)
    x = torch.randn(2, 32, 16, 16, generator=gen).to(DEV).requires_grad_(True)
    gy = torch.randn(2, 32, 16, 16, generator=gen).to(DEV)
    L = lib()
    with options(tune=0, deterministic=det, dwgrad_fused=fused):
        L.PROFILE = []
        try:
            (m(x).float() * gy).sum().backward()
            torch.cuda.synchronize()
            names = [rec[0] for rec in L.PROFILE]
        finally:
            L.PROFILE = None
    return x.grad.detach().clone(), {n: p.grad.detach().clone() for n, p in m.named_parameters()}, names


def test_engine_c3k2_fused_against_the_pair(monkeypatch):
    """Bar: as above, with the f32 engine standing where float64 stood — the f16 block's gradients with the switch off (the pair) and
    on, each against the same block run in f32; the fused run's largest error per tensor at most twice the pair's."""
    gx32, g32, n32 = _c3k2_backward(torch.float32, 1, 0, monkeypatch)
    assert "sy11_conv2d_dgrad_wgrad_1x1" not in n32                       # f32 stays on the pair
    gx0, g0, n0 = _c3k2_backward(torch.float16, 0, 0, monkeypatch)
    gx1, g1, n1 = _c3k2_backward(torch.float16, 1, 0, monkeypatch)
    assert n0.count("sy11_conv2d_dgrad_wgrad_1x1") == 0
    assert n1.count("sy11_conv2d_dgrad_wgrad_1x1") == 2, "cv1 and cv2 must take the fused call"
    assert n0.count("sy11_conv2d_dgrad") - n1.count("sy11_conv2d_dgrad") == 2
    _, _, above = _c3k2_backward(torch.float16, 1, 0, monkeypatch, threshold=513)
    assert above.count("sy11_conv2d_dgrad_wgrad_1x1") == 0, "M = 512 is below a threshold of 513"
    for name, ref, a, b in [("input", gx32, gx0, gx1)] + [(n, g32[n], g0[n], g1[n]) for n in g32]:
        e0, e1 = worst(a, ref.double().cpu()), worst(b, ref.double().cpu())
        print(f"\nDWGRAD1X1 engine {name}: max |err| against f32 pair {e0:.3e} fused {e1:.3e}")
        assert float(ref.abs().max()) > 0 and e0 > 0
        assert e1 <= MARGIN * e0, f"{name}: fused error {e1:.3e} above {MARGIN} x the pair's {e0:.3e}"


def test_engine_ordered_mode_takes_the_pair(monkeypatch):
    gx0, g0, n0 = _c3k2_backward(torch.float16, 0, 1, monkeypatch)
    gx1, g1, n1 = _c3k2_backward(torch.float16, 1, 1, monkeypatch)
    assert "sy11_conv2d_dgrad_wgrad_1x1" not in n1 and n1 == n0, "ordered mode must run the pair's launches"
    assert torch.equal(gx0.view(torch.int32), gx1.view(torch.int32))
    for n in g0:
        assert torch.equal(g0[n].view(torch.int32), g1[n].view(torch.int32)), f"ordered mode: {n} differs with the switch on"
