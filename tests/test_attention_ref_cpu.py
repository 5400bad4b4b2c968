"""CPU: the attention reference of tests/_attention_ref.py is right, and the bar built from it bites.

1. The float64 reference equals float64 autograd of softmax((q^T k) kd^-0.5) / v @ attn^T, written as tests/test_kernels_gpu.py
   writes it, to 1e-12 of each quantity's largest value; the two forms of the softmax row sum agree to 1e-12.
2. expected_path returns the documented kernel family on each side of every dispatch boundary.
3. Mutants.  A float32 evaluation of the formulas stands in for a kernel.  Unmutated, with the MFMA path's documented roundings modelled
   (P and dS rounded to 16 bit before their products, the row sums taken from a 16-bit o), it has to stay UNDER the bar of
   tests/_kernel_ref.Bars with the extras of _attention_ref.extras; with any one of six deliberate mistakes it has to land OVER the bar for
   at least one of P, o, dq, dk, dv — for every input regime of tests/test_attention_kernels_gpu.py, at N = 36 and 132, in f32 (bar of the
   VALU paths) and in f16 / bf16 (the widest bar: MFMA with the row sums from o).
"""
import pytest
import torch

from tests import _attention_ref as R
from tests._kernel_ref import Bars, rnd

F32, F16, BF16, F64 = torch.float32, torch.float16, torch.bfloat16, torch.float64


# ------------------------------------------------------------------------------------------------ 1. against autograd
@pytest.mark.parametrize("regime", ["flat", "peaked"])
@pytest.mark.parametrize("kd,hd", [(32, 64), (5, 7)])
def test_reference_equals_float64_autograd(kd, hd, regime):
    B, heads, H, W = 2, 2, 3, 5
    N, hc = H * W, 2 * kd + hd
    qkv_nhwc, dO_nhwc = R.inputs(B, heads, N, kd, hd, F32, regime)
    qkv = qkv_nhwc.reshape(B, H, W, heads * hc).permute(0, 3, 1, 2).contiguous().double().requires_grad_(True)      # NCHW, as the model's graph
    do = dO_nhwc.reshape(B, H, W, heads * hd).permute(0, 3, 1, 2).contiguous().double()
    qh, kh, vh = qkv.view(B, heads, hc, N).split([kd, kd, hd], 2)
    attn = ((qh.transpose(-2, -1) @ kh) * kd ** -0.5).softmax(-1)
    oref = (vh @ attn.transpose(-2, -1)).view(B, heads * hd, H, W)
    (oref * do).sum().backward()

    scale = kd ** -0.5
    q, k, v = R.split_heads(qkv_nhwc, heads, kd, hd)
    dO = R.split_o(dO_nhwc, heads, hd)
    fw = R.forward(q, k, v, scale, F64)
    bw = R.backward(q, k, v, dO, fw["P"], scale, F64)

    def same(name, got, want):
        err, s = (got - want).abs().max().item(), want.abs().max().item()
        assert err <= 1e-12 * s, (name, err, s)

    same("P", fw["P"], attn.detach())
    same("o", R.merge_o(fw["o"]).reshape(B, H, W, heads * hd).permute(0, 3, 1, 2), oref.detach())
    want = qkv.grad.permute(0, 2, 3, 1).reshape(B, N, heads * hc)
    wq, wk, wv = R.split_heads(want, heads, kd, hd)
    same("dq", bw["dq"], wq)
    same("dk", bw["dk"], wk)
    same("dv", bw["dv"], wv)
    same("merge_heads", R.merge_heads(bw["dq"], bw["dk"], bw["dv"]), want)
    same("delta", R.delta_from_o(dO, fw["o"], F64), R.delta_from_P(bw["dP"], fw["P"], F64))
    same("delta (backward(o=...))", R.backward(q, k, v, dO, fw["P"], scale, F64, o=fw["o"])["dq"], bw["dq"])


def test_layout_helpers_invert():
    x = rnd(2, 6, 2 * (2 * 5 + 7), seed=3)
    assert torch.equal(R.merge_heads(*R.split_heads(x, 2, 5, 7)), x)
    y = rnd(2, 6, 2 * 7, seed=4)
    assert torch.equal(R.merge_o(R.split_o(y, 2, 7)), y)
    q, k, v = R.split_heads(x, 2, 5, 7)
    assert torch.equal(q[1, 1, 4], x[1, 4, 17:22]) and torch.equal(k[1, 1, 4], x[1, 4, 22:27]) and torch.equal(v[1, 0, 2], x[1, 2, 10:17])


def test_kernel_scale_is_the_f32_value():
    assert R.kernel_scale(16) == 0.25 and R.kernel_scale(64) == 0.125
    assert R.kernel_scale(32) == float(torch.tensor(1.0) / torch.tensor(32.0).sqrt())
    assert abs(R.kernel_scale(5) - 5 ** -0.5) <= 2.0 ** -24


# ------------------------------------------------------------------------------------------------ 2. dispatch
def _path(dtype, N, kd=32, hd=64, heads=2, have_o=True, **kw):
    hc = heads * (2 * kd + hd)
    lds = dict(qkv=hc, o=heads * hd, do=heads * hd, dqkv=hc)
    lds.update({n[:-3]: v for n, v in kw.items() if n.endswith("_ld")})
    offs = {n[:-4]: v for n, v in kw.items() if n.endswith("_off")}
    return tuple(R.expected_path(dtype, N, kd, hd, lds, offs, have_o))


def test_expected_path_at_every_boundary():
    for dt in (F16, BF16):
        assert _path(dt, 32) == ("mma", "mma", True)
        assert _path(dt, 32, have_o=False) == ("mma", "mma", False)
        for N in (36, 68, 132, 260):
            assert _path(dt, N) == ("mma", "mma", True), N
        for N in (9, 28, 31, 33, 65, 66, 130):                        # N < 32 or N % 4 != 0
            assert _path(dt, N) == ("fast", "fast", False), N
        # the fallbacks at N = 68
        assert _path(dt, 68, qkv_off=8) == ("fast", "fast", False)
        assert _path(dt, 68, qkv_ld=256 + 4) == ("fast", "fast", False)
        assert _path(dt, 68, dqkv_ld=256 + 4) == ("mma", "fast", False)
        assert _path(dt, 68, dqkv_off=8) == ("mma", "fast", False)
        assert _path(dt, 68, do_ld=128 + 4) == ("mma", "fast", False)
        assert _path(dt, 68, o_ld=128 + 4) == ("fast", "mma", False)   # the forward writes o, the backward only drops the row sums from o
        assert _path(dt, 68, o_off=8) == ("fast", "mma", False)
        assert _path(dt, 68, p_off=4) == ("fast", "fast", False)
        assert _path(dt, 68, qkv_ld=256 + 16, o_ld=128 + 16, do_ld=128 + 16, dqkv_ld=256 + 16) == ("mma", "mma", True)
        # other head sizes never take MFMA
        assert _path(dt, 36, kd=16, hd=32) == ("generic", "generic", False)
        assert _path(dt, 36, kd=64, hd=64) == ("generic", "generic", False)
    assert _path(F32, 36) == ("fast", "fast", False)
    # score rows against 160 KB of LDS: forward 32 N + 5120 floats, backward 32 N + 6208 floats
    assert _path(F32, 1086) == ("fast", "fast", False)
    assert _path(F32, 1087) == ("fast", "gs", False)
    assert _path(F32, 1120) == ("fast", "gs", False)
    assert _path(F32, 1121) == ("gs", "gs", False)
    assert _path(F32, 1125) == ("gs", "gs", False)
    assert _path(F16, 1125) == ("gs", "gs", False)
    assert _path(F32, 65, kd=16, hd=32) == ("generic", "generic", False)
    assert _path(F32, 1400, kd=16, hd=32) == ("gs", "gs", False)
    # the 16-bit backward stages all of K: 64 bytes per key of ceil(N / 32) tiles, up to 150 KB
    assert _path(BF16, 2400) == ("mma", "mma", True)
    assert _path(BF16, 2404) == ("mma", "gs", False)
    assert R.supported(24, 104) and R.supported(64, 64) and R.supported(5, 7) and R.supported(16, 32)
    assert not R.supported(64, 128) and not R.supported(65, 8) and not R.supported(8, 129)


# ------------------------------------------------------------------------------------------------ 3. mutants
MUTANTS = ("drop_last_key", "swap_keys_3_4_in_pv", "scale_twice_on_dq", "delta_omitted", "head1_k_v_offsets_exchanged", "dk_without_scale")
SWAP_TILE = {36: 0, 132: 2}          # the 32-key tile whose keys 3 and 4 are exchanged in P v


def _stand_in(ref, qkv, heads, kd, hd, dtype, model_mma, have_o, mutant=None):
    """A float32 evaluation of the formulas in the role of the kernels: forward from q, k, v; backward from the reference P and o, as the
    GPU tests feed it.  -> dict P (f32), o, dq, dk, dv (values of ``dtype``)."""
    rd = (lambda t: t.to(dtype).to(F32)) if model_mma else (lambda t: t)
    q, k, v, scale = ref.q.to(F32), ref.k.to(F32), ref.v.to(F32), ref.scale
    if mutant == "head1_k_v_offsets_exchanged":        # head 1 reads k at the v offset and v at the k offset
        x = qkv.reshape(qkv.shape[0], -1, heads, 2 * kd + hd)[:, :, 1]
        k, v = k.clone(), v.clone()
        k[:, 1], v[:, 1] = x[..., 2 * kd:3 * kd], x[..., kd:kd + hd]
    N = q.shape[-2]
    s = R.scores(q, k, scale, F32)
    if mutant == "drop_last_key":
        P = torch.cat((R.softmax_rows(s[..., :-1]), torch.zeros_like(s[..., -1:])), -1)
    else:
        P = R.softmax_rows(s)
    vo = v
    if mutant == "swap_keys_3_4_in_pv":
        j = SWAP_TILE[N] * 32 + 3
        vo = v.clone()
        vo[..., [j, j + 1], :] = v[..., [j + 1, j], :]
    o = R.out(rd(P), vo, F32)
    # backward, from the reference's P and o
    P_in = ref.P_in
    if mutant == "drop_last_key":
        P_in = torch.cat((P_in[..., :-1], torch.zeros_like(P_in[..., -1:])), -1)
    dP = R.dP(ref.dO, v, F32)
    delta = R.delta_from_o(ref.dO, ref.o_in, F32) if have_o else R.delta_from_P(dP, P_in, F32)
    if mutant == "delta_omitted":
        delta = torch.zeros_like(delta)
    dS = rd(R.dS(P_in, dP, delta, F32))
    dq = R.dq(dS, k, scale * scale if mutant == "scale_twice_on_dq" else scale, F32)
    dk = R.dk(dS, q, 1.0 if mutant == "dk_without_scale" else scale, F32)
    dv = R.dv(rd(P_in), ref.dO, F32)
    st = lambda t: t.to(dtype).to(F32)                 # noqa: E731
    return dict(P=P, o=st(o), dq=st(dq), dk=st(dk), dv=st(dv))


def _bars(what, ref, got, dtype, path, have_o):
    ex = R.extras(path, dtype, ref.f64, ref.b64,ref.q, ref.k, ref.v, ref.dO, ref.scale, o_in=ref.o_in)
    b = Bars(what)
    b.add("P", got["P"], ref.f64["P"], ref.f32["P"], F32, extra=ex.get("P", 0.0))
    b.add("o", got["o"], ref.f64["o"], ref.f32["o"], dtype, extra=ex.get("o", 0.0))
    for n in ("dq", "dk", "dv"):
        b.add(n, got[n], ref.b64[n], ref.b32[n], dtype, extra=ex.get(n, 0.0))
    return b


@pytest.fixture(scope="module")
def refs():
    cache = {}

    def get(dtype, N, regime):
        key = (dtype, N, regime)
        if key not in cache:
            qkv, dO = R.inputs(2, 2, N, 32, 64, dtype, regime)
            cache[key] = (qkv, R.reference(qkv, dO, 2, 32, 64, dtype))
        return cache[key]
    return get


def _lds():
    return dict(qkv=256, o=128, do=128, dqkv=256)


@pytest.mark.parametrize("regime", R.REGIMES)
@pytest.mark.parametrize("N", [36, 132])
@pytest.mark.parametrize("dtype", [F32, F16, BF16], ids=["f32", "f16", "bf16"])
def test_modelled_roundings_stay_under_the_bar(refs, dtype, N, regime):
    qkv, ref = refs(dtype, N, regime)
    for have_o in ((False, True) if dtype != F32 else (False,)):
        path = R.expected_path(dtype, N, 32, 64, _lds(), {}, have_o)
        assert path.fwd == path.bwd == ("fast" if dtype == F32 else "mma") and path.delta_from_o == have_o
        got = _stand_in(ref, qkv, 2, 32, 64, dtype, model_mma=dtype != F32, have_o=have_o)
        _bars(f"model[{str(dtype)[6:]} N{N} {regime} have_o={int(have_o)}]", ref, got, dtype, path, have_o).check()


@pytest.mark.parametrize("mutant", MUTANTS)
@pytest.mark.parametrize("regime", R.REGIMES)
@pytest.mark.parametrize("N", [36, 132])
@pytest.mark.parametrize("dtype", [F32, F16, BF16], ids=["f32", "f16", "bf16"])
def test_every_mutant_lands_over_the_bar(refs, dtype, N, regime, mutant):
    qkv, ref = refs(dtype, N, regime)
    have_o = dtype != F32                                # the widest bar a 16-bit case ever gets
    path = R.expected_path(dtype, N, 32, 64, _lds(), {}, have_o)
    got = _stand_in(ref, qkv, 2, 32, 64, dtype, model_mma=False, have_o=have_o, mutant=mutant)
    b = _bars(f"mutant {mutant}[{str(dtype)[6:]} N{N} {regime}]", ref, got, dtype, path, have_o)
    assert b.bad, "this mutant passes every bar, so these inputs cannot tell it from a right kernel:\n" + "\n".join(b.lines)
