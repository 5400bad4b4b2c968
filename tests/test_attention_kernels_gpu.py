"""GPU: the nine kernels of csrc/attention.hip, part by part, against the float64 reference of tests/_attention_ref.py with the bar of
tests/_kernel_ref.py (8 * e_ref + u * scale + the documented-rounding extras of _attention_ref.extras; every element, no mask).

Every case prints one ``[parity]`` line each for P, o, dq, dk, dv (dq / dk / dv sliced out of dqkv per head, so each is scaled by its own
maximum) and, where the backward takes the MFMA path, for the row-sum workspace.  The label carries the kernel family
_attention_ref.expected_path names for the case's dtype, sizes, strides and pointers ("mma", "fast", "generic", "gs", per direction);
it selects the extras and nothing else.

* The backward is fed the REFERENCE P (float64 rounded to f32) and the reference o rounded to the dtype, so its error is its own; the
  ``end_to_end`` cases feed it the device's P and o, as the model does.
* o, dqkv, P and the workspace are pre-filled with NaN; every element has to come back finite (the workspace: its row sums).
* Views with a stride keep a fill value in their pad columns, which has to survive.
* Where the backward is MFMA both forms run (row sums from dP P, and from dO o); elsewhere one runs and passing o must change no bit.

Inputs (`_attention_ref.inputs`): flat, peaked (q, k times 6), dominant (one key more than 104 above all others in half of the (image,
head) pairs; last key, and first key for shapes of more than one 32-key tile).  tests/test_attention_ref_cpu.py shows that six
deliberate mistakes each land over the bar on every one of them.

Shapes: see the tables below; B = 2 and heads = 2 (batch and head strides of P and qkv) except for the four shapes whose score rows do
not fit LDS.  Also here: the two `copy2d` calls Attention._run makes around the core (v gather, accumulate of the pe-branch gradient).

Measured ratios (MI355X) are in DESIGN.md section 4, "Attention parity".
"""
import contextlib
import functools

import pytest
import torch

from tests import _attention_ref as R
from tests._kernel_ref import DEV, FACTOR, HALF_ULP, Bars, lib, nhwc_view, ops, outside_untouched, rnd

pytestmark = pytest.mark.gpu
F32, F16, BF16, F64 = torch.float32, torch.float16, torch.bfloat16, torch.float64
NAME = {F32: "f32", F16: "f16", BF16: "bf16"}
FILL = 1.0e3
NAN = float("nan")

# layouts: per tensor (first channel of the view in its buffer, extra channels of the buffer); "slice" = nhwc_view(strided=True)
LAYOUTS = {
    "contig": {},
    "slice": "nhwc_view",                            # every tensor 16 bytes into a buffer two 16-byte vectors wider: aligned, ld > C
    "qkv+8B": {"qkv": (4, 8)},                       # 16-bit: the view starts 8 bytes into its buffer, ld still a multiple of 8
    "qkv_ld": {"qkv": (0, 4)},                       # ld % 8 != 0: every other pixel row is 8 bytes off
    "dqkv_ld": {"dqkv": (0, 4)},
    "o_ld": {"o": (0, 4)},
}
RECT = {36: (6, 6), 68: (4, 17), 132: (11, 12), 260: (13, 20), 9: (3, 3), 33: (3, 11), 65: (5, 13), 130: (10, 13), 64: (8, 8)}


def _hw(N):
    return RECT.get(N, (1, N))


def _regimes(N, tile=32):
    return ("flat", "peaked", "dominant_last") + (("dominant_first",) if N > tile else ())


class _Views:
    """Device views of one case, by layout; remembers the buffers for the pad check."""

    def __init__(self, layout, dtype):
        self.layout, self.dtype, self.bufs = LAYOUTS[layout], dtype, []

    def make(self, name, x_cpu):
        if self.layout == "nhwc_view":
            v, buf = nhwc_view(x_cpu, self.dtype, True, FILL)
            self.bufs.append((name, buf, None, x_cpu.shape[-1]))
            return v
        off, pad = self.layout.get(name, (0, 0))
        B, H, W, Cn = x_cpu.shape
        buf = torch.full((B, H, W, Cn + pad), FILL, dtype=self.dtype, device=DEV)
        v = buf[..., off:off + Cn]
        v.copy_(x_cpu.to(DEV, self.dtype))
        self.bufs.append((name, buf, off, Cn))
        return v

    def nan(self, name, shape):
        v = self.make(name, torch.zeros(shape))
        v.fill_(NAN)
        return v

    def pads_untouched(self):
        for name, buf, off, Cn in self.bufs:
            if off is None:
                assert outside_untouched(buf, Cn, FILL), f"{name}: a pad column of the strided buffer was written"
            else:
                pad = torch.cat((buf[..., :off], buf[..., off + Cn:]), -1).float()
                assert bool((pad == FILL).all()), f"{name}: a pad column of the buffer was written"


def _make_reference(B, heads, N, kd, hd, dtype, regime):
    qkv, dO = R.inputs(B, heads, N, kd, hd, dtype, regime)
    return qkv, dO, R.reference(qkv, dO, heads, kd, hd, dtype)


_cached_reference = functools.lru_cache(maxsize=8)(_make_reference)


def _reference(B, heads, N, kd, hd, dtype, regime):
    """Computed once per case and shared by its layouts; the four shapes past 1 000 tokens (N x N float64 matrices) are not kept."""
    return (_cached_reference if N <= 300 else _make_reference)(B, heads, N, kd, hd, dtype, regime)


def _finite(name, t):
    assert bool(torch.isfinite(t.float()).all()), f"{name}: an element was left unwritten (NaN pre-fill) or is not finite"


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == F32 else torch.int16)


def _bar_of(r64, r32, out_dtype, extra):
    return FACTOR * float((r32.double() - r64).abs().max()) + HALF_ULP[out_dtype] * float(r64.abs().max()) + extra


def _run(dtype, B, heads, N, kd, hd, regime, layout="contig", end_to_end=False):
    o_ = ops()
    H, W = _hw(N)
    hc = 2 * kd + hd
    qkv_c, dO_c, ref = _reference(B, heads, N, kd, hd, dtype, regime)
    vw = _Views(layout, dtype)
    qv = vw.make("qkv", qkv_c.reshape(B, H, W, heads * hc))
    dov = vw.make("do", dO_c.reshape(B, H, W, heads * hd))
    ov = vw.nan("o", (B, H, W, heads * hd))
    p = torch.full((B, heads, N, N), NAN, dtype=F32, device=DEV)
    lds = dict(qkv=o_.view_ld(qv), o=o_.view_ld(ov), do=o_.view_ld(dov), dqkv=0)
    offs = dict(qkv=qv.data_ptr() % 16, o=ov.data_ptr() % 16, do=dov.data_ptr() % 16, p=p.data_ptr() % 16)

    def fresh_dqkv():
        v = vw.nan("dqkv", (B, H, W, heads * hc))
        lds["dqkv"], offs["dqkv"] = o_.view_ld(v), v.data_ptr() % 16
        return v

    dq1 = fresh_dqkv()
    path = R.expected_path(dtype, N, kd, hd, lds, offs, have_o=True)
    two_pass = path._replace(delta_from_o=False)
    tag = f"{NAME[dtype]} B{B} h{heads} N{N} kd{kd} hd{hd} {regime} {layout}{' end_to_end' if end_to_end else ''} fwd={path.fwd} bwd={path.bwd}"
    b = Bars(f"attention[{tag}]")

    # ---- forward
    o_.attention_fwd(qv, heads, kd, hd, ov, p)
    torch.cuda.synchronize()
    _finite("P", p)
    _finite("o", ov)
    ex = R.extras(path, dtype, ref.f64, None, ref.q, ref.k, ref.v, ref.dO, ref.scale)
    b.add("P", p, ref.f64["P"], ref.f32["P"], F32, extra=ex["P"])
    o_gpu = R.split_o(ov.cpu().float().reshape(B, N, heads * hd), heads, hd)
    b.add("o", o_gpu, ref.f64["o"], ref.f32["o"], dtype, extra=ex.get("o", 0.0))

    # ---- backward: from the reference's P and o (end_to_end: from the device's)
    if end_to_end:
        P_dev, P_in, o_in, o_view = p, p.cpu(), o_gpu, ov
        b64 = R.backward(ref.q, ref.k, ref.v, ref.dO, P_in, ref.scale, F64)
        b32 = R.backward(ref.q, ref.k, ref.v, ref.dO, P_in, ref.scale, F32)
        # the device's o is within the forward's bar of the float64 o (checked above): that bound replaces u |o| in the dq / dk extras
        o_err = _bar_of(ref.f64["o"], ref.f32["o"], dtype, ex.get("o", 0.0))
    else:
        P_dev, P_in, o_in = ref.P_in.to(DEV), ref.P_in, ref.o_in
        o_view = vw.make("o", R.merge_o(o_in).reshape(B, H, W, heads * hd))
        b64, b32, o_err = ref.b64, ref.b32, None
    n_delta = B * heads * N

    def backward(dqkv, o_arg):
        ws = torch.full((B * heads * N * N,), NAN, dtype=F32, device=DEV)
        o_.attention_bwd(qv, heads, kd, hd, P_dev, dov, dqkv, ws, o=o_arg)
        torch.cuda.synchronize()
        _finite("dqkv", dqkv)
        return ws[:n_delta].cpu().reshape(B, heads, N)

    def add_grads(suffix, dqkv, pth):
        exb = R.extras(pth, dtype, None, b64, ref.q, ref.k, ref.v, ref.dO, ref.scale, o_in=o_in, o_err=o_err)
        got = R.split_heads(dqkv.cpu().float().reshape(B, N, heads * hc), heads, kd, hd)
        for name, g in zip(("dq", "dk", "dv"), got):
            b.add(name + suffix, g, b64[name], b32[name], dtype, extra=exb.get(name, 0.0))

    d1 = backward(dq1, None)
    add_grads("", dq1, two_pass)
    if path.bwd == "mma":
        _finite("row sums", d1)
        b.add("delta", d1, b64["delta"], b32["delta"], F32)
    dq2 = fresh_dqkv()
    d2 = backward(dq2, o_view)
    if path.delta_from_o:
        add_grads("(o)", dq2, path)
        _finite("row sums (o)", d2)
        b.add("delta(o)", d2, R.delta_from_o(ref.dO, o_in, F64), R.delta_from_o(ref.dO, o_in, F32), F32)
    else:
        assert torch.equal(_bits(dq2), _bits(dq1)), f"{tag}: passing o changed dqkv on a path that has to ignore it"
        if path.bwd == "mma":
            assert torch.equal(_bits(d2), _bits(d1)), f"{tag}: passing an o the MFMA path cannot read changed the row sums"
    vw.pads_untouched()
    b.check()
    return path


def _ids(cases):
    return ["-".join(NAME.get(c, str(c)) for c in case) for case in cases]


# ------------------------------------------------------------------------------------------------ MFMA
MMA_N = (32, 36, 68, 132, 260)      # one full tile | partial 2nd tile, lane half 1 dead | 2nd V chunk of one tile | 2nd workgroup: 1 live wave | LDS double buffer wraps
MMA = [(dt, N, rg) for dt in (F16, BF16) for N in MMA_N for rg in _regimes(N)]


@pytest.mark.parametrize("dtype,N,regime", MMA, ids=_ids(MMA))
def test_mma(dtype, N, regime):
    path = _run(dtype, 2, 2, N, 32, 64, regime)
    assert tuple(path) == ("mma", "mma", True)


SLICE = [(dt, N, rg) for dt in (F16, BF16) for N in (36, 132) for rg in _regimes(N)]


@pytest.mark.parametrize("dtype,N,regime", SLICE, ids=_ids(SLICE))
def test_mma_strided_but_aligned(dtype, N, regime):
    path = _run(dtype, 2, 2, N, 32, 64, regime, layout="slice")
    assert tuple(path) == ("mma", "mma", True)


# ------------------------------------------------------------------------------------------------ fast VALU
FAST = ([(F32, N, rg) for N in (1, 9, 31, 33, 63, 64, 65, 130) for rg in _regimes(N)]       # 32-query tile, 64-key staging chunk
        + [(dt, N, rg) for dt in (F16, BF16) for N in (9, 31, 33, 65) for rg in _regimes(N)])   # off MFMA through N % 4 or N < 32


@pytest.mark.parametrize("dtype,N,regime", FAST, ids=_ids(FAST))
def test_fast(dtype, N, regime):
    path = _run(dtype, 2, 2, N, 32, 64, regime)
    assert tuple(path) == ("fast", "fast", False)


FALLBACK_PATH = {"qkv+8B": ("fast", "fast", False), "qkv_ld": ("fast", "fast", False), "dqkv_ld": ("mma", "fast", False),
                 "o_ld": ("fast", "mma", False)}        # o_ld: the forward writes o (scalar stores); the backward stays MFMA and drops the row sums from o
FALLBACK = [(dt, lay, rg) for dt in (F16, BF16) for lay in FALLBACK_PATH for rg in _regimes(68)]


@pytest.mark.parametrize("dtype,layout,regime", FALLBACK, ids=_ids(FALLBACK))
def test_fallback_off_mma(dtype, layout, regime):
    path = _run(dtype, 2, 2, 68, 32, 64, regime, layout=layout)
    assert tuple(path) == FALLBACK_PATH[layout]


# ------------------------------------------------------------------------------------------------ generic VALU
GENERIC = [(dt, kd, hd, N, rg) for dt in (F32, F16) for kd, hd in ((16, 32), (64, 64), (24, 104), (5, 7)) for N in (9, 33, 65) for rg in _regimes(N)]


@pytest.mark.parametrize("dtype,kd,hd,N,regime", GENERIC, ids=_ids(GENERIC))
def test_generic(dtype, kd, hd, N, regime):
    path = _run(dtype, 2, 2, N, kd, hd, regime)
    assert tuple(path) == ("generic", "generic", False)


def test_head_sizes_past_the_limit_are_rejected_and_nothing_is_written():
    o_ = ops()
    B, heads, N, kd, hd, dtype = 2, 2, 9, 64, 128, F16
    assert not R.supported(kd, hd)
    qkv, dO = R.inputs(B, heads, N, kd, hd, dtype, "flat")
    qv = qkv.reshape(B, 1, N, -1).to(DEV, dtype)
    dov = dO.reshape(B, 1, N, -1).to(DEV, dtype)
    ov = torch.full((B, 1, N, heads * hd), NAN, dtype=dtype, device=DEV)
    p = torch.full((B, heads, N, N), NAN, dtype=F32, device=DEV)
    dqkv = torch.full((B, 1, N, heads * (2 * kd + hd)), NAN, dtype=dtype, device=DEV)
    ws = torch.full((B * heads * N * N,), NAN, dtype=F32, device=DEV)
    with pytest.raises(lib().Sy11Error, match="kd<=64, hd<=128"):
        o_.attention_fwd(qv, heads, kd, hd, ov, p)
    with pytest.raises(lib().Sy11Error, match="kd<=64, hd<=128"):
        o_.attention_bwd(qv, heads, kd, hd, torch.zeros_like(p), dov, dqkv, ws)
    with pytest.raises(lib().Sy11Error, match="kd<=64, hd<=128"):
        o_.attention_bwd(qv, heads, kd, hd, torch.zeros_like(p), dov, dqkv, ws, o=torch.zeros_like(ov))
    torch.cuda.synchronize()
    for name, t in (("o", ov), ("P", p), ("dqkv", dqkv), ("workspace", ws)):
        assert bool(torch.isnan(t.float()).all()), f"{name} was written by a rejected call"


# ------------------------------------------------------------------------------------------------ score rows outside LDS
#        dtype N     kd  hd   forward  backward
BIG = [(F32, 1125, 32, 64, "gs", "gs"),          # 35 full query tiles + 5 rows
       (F16, 1125, 32, 64, "gs", "gs"),          # the 16-bit VALU GS forward
       (BF16, 2404, 32, 64, "mma", "gs"),        # MFMA forward; the backward's K image (76 tiles x 2 KB) is past 150 KB
       (F32, 1400, 16, 32, "gs", "gs")]
BIG = [c + (rg,) for c in BIG for rg in ("flat", "peaked")]


@pytest.mark.parametrize("dtype,N,kd,hd,fwd,bwd,regime", BIG, ids=_ids(BIG))
def test_score_rows_outside_lds(dtype, N, kd, hd, fwd, bwd, regime):
    path = _run(dtype, 1, 1, N, kd, hd, regime)
    assert tuple(path) == (fwd, bwd, False)


# ------------------------------------------------------------------------------------------------ end to end, one per family
E2E = [(F16, 132, 32, 64, "peaked", ("mma", "mma", True)), (BF16, 132, 32, 64, "flat", ("mma", "mma", True)),
       (F32, 65, 32, 64, "peaked", ("fast", "fast", False)), (F16, 33, 24, 104, "peaked", ("generic", "generic", False)),
       (F32, 1125, 32, 64, "peaked", ("gs", "gs", False))]


@pytest.mark.parametrize("dtype,N,kd,hd,regime,want", E2E, ids=_ids([c[:5] for c in E2E]))
def test_end_to_end_backward_from_the_device_forward(dtype, N, kd, hd, regime, want):
    big = N > 1000
    path = _run(dtype, 1 if big else 2, 1 if big else 2, N, kd, hd, regime, end_to_end=True)
    assert tuple(path) == want


# ------------------------------------------------------------------------------------------------ the copies around the core
@contextlib.contextmanager
def _row_map(value):
    _lib = lib()
    prev = _lib.get_option("row_map")
    try:
        _lib.set_option("row_map", value)
        yield
    finally:
        _lib.set_option("row_map", prev)


COPY = [(dt, hd, M, rm) for dt in (F16, BF16, F32) for hd in (64, 24, 7) for M in (1, 255, 1125) for rm in (1, 0)]


@pytest.mark.parametrize("dtype,hd,M,row_map", COPY, ids=_ids(COPY))
def test_v_gather_and_gradient_accumulate(dtype, hd, M, row_map):
    """Attention._run: v of head h is copied out of qkv at channel h * hc + 2 * kd into channels [h * hd, (h + 1) * hd) of a C-channel
    tensor; the pe-branch gradient is added back into the same slices of dqkv.  hd 64: 16-byte vectors; hd 24: 3 vectors per row in
    the 16-bit types (256 threads = 85 rows + one idle thread); hd 7 (kd 3): the scalar path.  Copy: bit-exact.  Accumulate: one rounding of
    the f32 sum.  Everything outside the slice keeps its bits."""
    o_ = ops()
    heads, kd = 2, hd // 2
    hc = 2 * kd + hd
    qkv = rnd(1, 1, M, heads * hc, seed=5).to(DEV, dtype)
    gv = rnd(1, 1, M, heads * hd, seed=6).to(DEV, dtype)
    with _row_map(row_map):
        for h in range(heads):
            v = torch.full((1, 1, M, heads * hd), FILL, dtype=dtype, device=DEV)
            src = qkv[..., h * hc + 2 * kd:(h + 1) * hc]
            o_.copy2d(src, v[..., h * hd:(h + 1) * hd])
            want = torch.full_like(v, FILL)
            want[..., h * hd:(h + 1) * hd] = src
            assert torch.equal(_bits(v), _bits(want)), f"v gather of head {h}"

            dqkv = rnd(1, 1, M, heads * hc, seed=7).to(DEV, dtype)
            want = dqkv.clone()
            sl = slice(h * hc + 2 * kd, (h + 1) * hc)
            want[..., sl] = (dqkv[..., sl].float() + gv[..., h * hd:(h + 1) * hd].float()).to(dtype)
            o_.copy2d(gv[..., h * hd:(h + 1) * hd], dqkv[..., sl], accumulate=True)
            assert torch.equal(_bits(dqkv), _bits(want)), f"gradient accumulate of head {h}"
    torch.cuda.synchronize()
