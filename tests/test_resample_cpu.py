"""CPU: the DDC's plan and filter (sy11/data/resample.py), the float64 restatement against scipy, the chunked reads of
``ResampledCapture``, and every argument error that is raised before anything touches a GPU."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import _ddc_ref as R

RATIOS = [(1, 2), (2, 3), (3, 2), (5, 16), (125, 192), (1, 8), (4, 1), (25, 64), (1, 1)]


def _plan(P, Q, shift=0.0, fs_in=1.0e6):
    from sy11.data.resample import plan_resample
    return plan_resample(fs_in, Fraction(fs_in) * P / Q, shift)


def _capture(n, seed=0):
    g = np.random.default_rng(seed)
    return (g.standard_normal(n) + 1j * g.standard_normal(n)).astype(np.complex64)


# ------------------------------------------------------------------------------------------------------------- the plan
@pytest.mark.parametrize("P,Q", RATIOS)
def test_plan_ratio_table_and_index_maps(P, Q):
    p = _plan(P, Q)
    Rr = max(P, Q)
    assert (p.P, p.Q) == (P, Q) and p.c == 16 * Rr and p.N == 32 * Rr + 1 and p.T == -(-p.N // P)
    assert p.taps.shape == (P, p.T) and p.taps.dtype == np.float32
    assert abs(p.h.sum() - P) < 1e-12 and np.array_equal(p.h, p.h[::-1]) and p.h.argmax() == p.c
    flat = np.zeros(P * p.T)
    flat[:p.N] = p.h
    for phi in (0, P // 2, P - 1):
        assert np.array_equal(p.taps[phi], flat[phi::P].astype(np.float32))
    for n in (1, 2, 1000, 6001):
        M = p.n_out(n)
        assert M == (n if P == Q else (n - 1) * P // Q + 1)
        assert (M - 1) * Q <= (n - 1) * P < M * Q or P == Q                 # the last output sits at or before the last sample
    if P != Q:
        for m0, m1 in ((0, 1), (5, 77), (3 * 10 ** 9, 3 * 10 ** 9 + 10)):
            a, b = p.support(m0, m1)
            # tap k of output m meets sample i where m Q + c - k = i P: the oldest is ceil((m0 Q + c - (P T - 1)) / P), over the
            # table's P T entries, the newest floor(((m1 - 1) Q + c) / P)
            lo = -((-(m0 * Q + p.c - (P * p.T - 1))) // P)
            hi = ((m1 - 1) * Q + p.c) // P
            assert (a, b) == (lo, hi + 1) and a == (m0 * Q + p.c) // P - (p.T - 1)
    else:
        assert p.support(3, 9) == (3, 9) and not p.filters
    with pytest.raises(ValueError):
        p.support(4, 4)


def test_plan_quantised_shift_and_skipped_steps():
    from sy11.data.resample import plan_resample
    fs = 61.44e6
    p = plan_resample(fs, 15.36e6, 7.0e6)
    assert (p.P, p.Q) == (1, 4)
    want = round(-7.0e6 / fs * 2 ** 32) % 2 ** 32
    assert p.dphi == want and 0 < p.dphi < 2 ** 32
    assert abs(p.shift_hz - 7.0e6) <= fs / 2 ** 33 and p.shift_hz == -(want - 2 ** 32) / 2.0 ** 32 * fs
    n = plan_resample(fs, 15.36e6, -7.0e6)
    assert n.dphi == 2 ** 32 - p.dphi and n.shift_hz == -p.shift_hz
    assert plan_resample(20e6, 20e6).identity and not plan_resample(20e6, 20e6).filters
    m = plan_resample(20e6, 20e6, 1e6)
    assert not m.identity and not m.filters and (m.P, m.Q) == (1, 1)
    assert not plan_resample(25e6, 20e6).identity and (plan_resample(25e6, 20e6).P, plan_resample(25e6, 20e6).Q) == (4, 5)
    assert plan_resample(20e6, 20e6, 1e-9).identity                       # a shift below half a step quantises to none


@pytest.mark.parametrize("fs_in,fs_out,near", [(1e6, 1e6 / 3, None), (20e6, 20e6 * 4097 / 4096, None), (1e6, 65e6, "64/1"), (64e6, 0.9e6, "1/64"),
                                                (1e6, 1e6 * 4099 / 4093, None)])
def test_plan_refuses_inexact_or_out_of_range_ratios_and_names_the_nearest(fs_in, fs_out, near):
    from sy11.data.resample import plan_resample
    with pytest.raises(ValueError, match="nearest admissible ratio is") as e:
        plan_resample(fs_in, fs_out)
    msg = str(e.value)
    got = Fraction(msg.split("nearest admissible ratio is ")[1].split(" ")[0])
    assert got.numerator <= 4096 and got.denominator <= 4096 and Fraction(1, 64) <= got <= 64
    assert abs(float(got) - min(max(fs_out / fs_in, 1 / 64), 64.0)) < 1.0 / 4096
    if near:
        assert got == Fraction(near)


def test_plan_refuses_bad_rates_and_shifts():
    from sy11.data.resample import plan_resample
    for bad in ((0.0, 1e6), (1e6, -1.0), (float("nan"), 1e6), (1e6, float("inf"))):
        with pytest.raises(ValueError):
            plan_resample(*bad)
    for shift in (float("nan"), 0.6e6, -0.6e6):
        with pytest.raises(ValueError, match="shift_hz"):
            plan_resample(1e6, 0.5e6, shift)


# ------------------------------------------------------------------------------------------------------------- the filter
def _response_db(p):
    """|H(f)| / P in dB on a grid of the up-sampled band [0, fs_up / 2], and that grid in units of min(fs_in, fs_out)."""
    n = 1 << 20
    H = np.abs(np.fft.rfft(p.h, n)) / p.P
    f = np.arange(H.shape[0]) / n * max(p.P, p.Q)                          # f / fs_up * R = f / min(fs_in, fs_out)
    return 20 * np.log10(np.maximum(H, 1e-300)), f


@pytest.mark.parametrize("P,Q", RATIOS)
def test_filter_meets_the_passband_and_rejection_bars(P, Q):
    """Passband deviation <= 0.01 dB over |f| <= 0.4 min(fs), rejection >= 75 dB at |f| >= 0.6 min(fs) (all that folds into the
    passband).  h is real and symmetric, so the one-sided grid covers both signs."""
    p = _plan(P, Q)
    db, f = _response_db(p)
    dev = np.abs(db[f <= 0.4]).max()
    stop = db[f >= 0.6]                                                     # 1/1: the grid ends at 0.5 min(fs), nothing can fold
    rej = -stop.max() if stop.size else np.inf
    print(f"P/Q = {P}/{Q}: N = {p.N}, T = {p.T}, passband deviation {dev:.5f} dB, rejection {rej:.2f} dB")
    assert dev <= 0.01 and rej >= 75.0


# ------------------------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("P,Q", [(1, 2), (2, 3), (3, 2), (5, 16), (4, 1)])
def test_reference_equals_scipy_upfirdn_shifted_by_the_centre(P, Q):
    sig = pytest.importorskip("scipy.signal")
    p = _plan(P, Q)
    x = _capture(3001, 5).astype(np.complex128)
    full = sig.upfirdn(p.h, x, P, Q)                                       # full[k] = sum_j h[j] u[k Q - j]
    M = p.n_out(len(x))
    got = R.ddc_ref(x, R.table_of(p.h, P), P, Q, p.c)
    assert got.shape == (M,)
    # y[m] = sum_k h[k] u[m Q + c - k] = the full convolution at index m Q + c: c is a multiple of Q only for some ratios, so
    # compare on the up-sampled grid instead
    up = sig.upfirdn(p.h, x, P, 1)
    want = up[p.c + Q * np.arange(M)]
    assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    if p.c % Q == 0:
        assert np.abs(got - full[p.c // Q:p.c // Q + M]).max() <= 1e-12 * max(1.0, np.abs(want).max())


def test_reference_mixer_phase_is_exact_far_from_the_origin():
    x = np.ones(64, dtype=np.complex64)
    dphi = 0x12345679
    n0 = 3 * 10 ** 9 + 1
    got = R.mixed(x, n0, dphi)
    for k in (0, 1, 63):
        ph = ((n0 + k) * dphi) % 2 ** 32                                  # Python integers
        assert abs(got[k] - np.exp(2j * np.pi * ph / 2 ** 32)) < 1e-14
    p = _plan(1, 1, 1234.5)
    assert np.array_equal(R.plan_ref(x, p, n0=10, m0=12, M=5), R.mixed(x, 10, p.dphi)[2:7])
    e = R.plan_ref(_capture(500), _plan(2, 3), f32=True) - R.plan_ref(_capture(500), _plan(2, 3))
    assert 0 < np.abs(e).max() < 1e-5


# ------------------------------------------------------------------------------------------------------------- chunked reads
class _Recording:
    """A capture that notes every slice it is asked for."""

    def __init__(self, x):
        self.x, self.asked = x, []

    def __len__(self):
        return self.x.shape[0]

    def __getitem__(self, sl):
        self.asked.append((sl.start, sl.stop))
        return self.x[sl]


@pytest.mark.parametrize("P,Q,shift", [(2, 3, 0.0), (5, 16, 1.0e5), (3, 2, -2.0e5), (1, 1, 3.0e5), (1, 1, 0.0)])
def test_resampled_capture_reads_only_the_support_and_chunks_concatenate(monkeypatch, P, Q, shift):
    from sy11 import ops
    from sy11.data import resample as rs
    from sy11.data.spectrogram import read_samples
    calls = []

    def fake(x, plan, n0, m0, M, out=None, n_total=None):
        calls.append((n0, x.shape[0], m0, M))
        return torch.from_numpy(R.plan_ref(x.numpy(), plan, n0, m0, M))

    monkeypatch.setattr(ops, "iq_resample", fake)
    monkeypatch.setattr(rs.ResampledCapture, "_to_device", lambda self, a, b: torch.from_numpy(read_samples(self.src, a, b)))
    plan = _plan(P, Q, shift)
    src = _Recording(_capture(6007, 2))
    cap = rs.ResampledCapture(src, plan, "cpu")
    M = plan.n_out(6007)
    assert len(cap) == M
    whole = cap[0:M].numpy()
    assert whole.shape == (M,)
    if plan.identity:
        assert np.array_equal(whole, src.x) and not calls
    else:
        assert np.array_equal(whole, R.plan_ref(src.x, plan))
    for step in (1000, 4097):
        src.asked.clear()
        parts = []
        for lo in range(0, M, step):
            hi = min(lo + step, M)
            parts.append(cap[lo:hi].numpy())
            a, b = plan.support(lo, hi)
            assert src.asked[-1] == (max(a, 0), min(b, 6007)) and len(src.asked) == len(parts)      # one read, of the support alone
        assert np.array_equal(np.concatenate(parts), whole)
    assert cap[M:M + 5].shape == (0,) and cap[M - 3:M + 100].shape == (3,)
    with pytest.raises(TypeError):
        cap[::2]


# ------------------------------------------------------------------------------------------------------------- argument errors
def test_cabi_argument_errors_without_gpu():
    from sy11 import _lib
    lib = _lib.load()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    ok = dict(P=2, Q=3, T=49, c=48, taps=p, n0=0, n_in=16, x=p, dphi=0, m0=0, M=4, out=p)

    def rc(**kw):
        a = {**ok, **kw}
        return lib.sy11_iq_resample(a["P"], a["Q"], a["T"], a["c"], a["taps"], a["n0"], a["n_in"], a["x"], a["dphi"], a["m0"], a["M"], a["out"], None)

    for kw, word in (({"taps": None}, b"null"), ({"x": None}, b"null"), ({"out": None}, b"null"), ({"P": 0}, b"positive"), ({"Q": -1}, b"positive"),
                     ({"T": 0}, b"positive"), ({"M": 0}, b"positive"), ({"n_in": 0}, b"positive"), ({"M": -2 ** 31}, b"2^31"),
                     ({"n_in": -1}, b"2^31"), ({"c": 98}, b"centre tap"), ({"c": -1}, b"centre tap"), ({"P": 4097, "Q": 4096}, b"4096"),
                     ({"P": 65, "Q": 1}, b"1/64"), ({"n0": -1}, b"non-negative"), ({"m0": -5}, b"non-negative"),
                     ({"x": C.c_void_p(p.value + 4)}, b"aligned"), ({"P": 1, "Q": 1, "m0": 14, "M": 4}, b"mixer outputs")):
        assert rc(**kw) == -1, kw
        assert word in lib.sy11_last_error(), (kw, lib.sy11_last_error())


def test_ops_wrapper_refuses_host_tensors():
    from sy11 import _lib, ops
    with pytest.raises(_lib.Sy11Error):
        ops.iq_resample(torch.zeros(100, dtype=torch.complex64), _plan(1, 2), 0, 0, 10)


def test_scan_argument_errors():
    """The band that is kept must lie inside the capture's, and "model" needs a checkpoint that records a rate: both are raised
    by YOLO.scan before anything touches a device."""
    from sy11.engine.model import YOLO
    from sy11.engine.predictor import plan_scan_ddc
    y = YOLO("yolo11n.yaml", nc=2, device="cpu")
    x = torch.zeros(1 << 20, dtype=torch.complex64)
    with pytest.raises(ValueError, match="not inside"):
        y.scan(x, 40e6, 2.4e9, resample_to=20e6, tune_to=2.4e9 + 10.1e6)
    with pytest.raises(ValueError, match="not inside"):
        y.scan(x, 40e6, 2.4e9, tune_to=2.4e9 + 1.0)                        # same rate: any retune leaves the band
    with pytest.raises(ValueError, match="records no sample_rate"):
        y.scan(x, 40e6, 2.4e9, resample_to="model")
    with pytest.raises(ValueError, match="records no center_freq"):
        y.scan(x, 40e6, 2.4e9, tune_to="model")
    with pytest.raises(ValueError, match="'model'"):
        y.scan(x, 40e6, 2.4e9, resample_to="native")
    with pytest.raises(ValueError, match="nearest admissible"):
        y.scan(x, 40e6, 2.4e9, resample_to=40e6 / 3)
    # what "model" resolves to
    trained = {"sample_rate": 15.36e6, "center_freq": 3.5e9 + 10e6, "n_fft": 1024, "hop": 256}
    p = plan_scan_ddc(61.44e6, 3.5e9, "model", None, trained)
    assert (p.P, p.Q) == (1, 4) and abs(p.shift_hz - 10e6) < 0.01
    p = plan_scan_ddc(61.44e6, 3.5e9, "model", None, {**trained, "center_freq": 0.0})
    assert p.dphi == 0
    p = plan_scan_ddc(25e6, 0.0, 20e6)
    assert (p.P, p.Q) == (4, 5) and p.dphi == 0
    assert plan_scan_ddc(40e6, 2.4e9, 20e6, 2.4e9 + 10e6).dphi == 2 ** 32 - 2 ** 30       # exactly on the edge is inside
