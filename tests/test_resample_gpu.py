"""GPU: the DDC kernel (sy11_iq_resample) against the float64 restatement of tests/_ddc_ref.py, its skipped steps, the chunk
independence of ``ResampledCapture``, what it does to tones, and a resampled / retuned scan against a scan of the DDC's own output.

The parity bar is not a constant: per case it is 4x the error of the float32 emulation in _ddc_ref (same sum order, mixed samples
and taps rounded to float32) against the float64 reference on the same input, relative to max |y|.  The emulation's error is what
float32 storage and a sequential float32 sum cost (2e-7 .. 4e-7 here; 3e-8 for the pure mixer, whose only rounding is the one of
the product); the factor 4 covers fma contraction and whatever the kernel's rotation adds to that one rounding."""
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import _ddc_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FS_IN = 1.0e6
SHIFT = 0.0371e6


def _plan(P, Q, shift=0.0):
    from sy11.data.resample import plan_resample
    return plan_resample(FS_IN, Fraction(FS_IN) * P / Q, shift)


def _capture(n, seed=0):
    g = np.random.default_rng(seed)
    return (g.standard_normal(n) + 1j * g.standard_normal(n)).astype(np.complex64)


def _check(name, got, x, plan, n0=0, m0=0, M=None):
    want = R.plan_ref(x, plan, n0, m0, M)
    emu = R.plan_ref(x, plan, n0, m0, M, f32=True)
    scale = np.abs(want).max()
    e_emu = np.abs(emu - want).max() / scale
    e_gpu = np.abs(got.astype(np.complex128) - want).max() / scale
    print(f"iq_resample[{name}]: {len(want)} outputs, float32 emulation {e_emu:.3e}, kernel {e_gpu:.3e} (bar {4 * e_emu:.3e})")
    assert got.shape == want.shape and got.dtype == np.complex64
    assert e_emu > 0 and e_gpu <= 4 * e_emu, (name, e_gpu, e_emu)


# ------------------------------------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("shift", [0.0, SHIFT])
@pytest.mark.parametrize("P,Q,n", [(1, 2, 8191), (2, 3, 6000), (3, 2, 6001), (5, 16, 20000), (125, 192, 7003)])
def test_kernel_matches_the_float64_reference_on_every_output(P, Q, n, shift):
    """The whole capture in one call: every output, both zero-extended ends included."""
    from sy11 import ops
    plan = _plan(P, Q, shift)
    assert (plan.dphi != 0) == (shift != 0)
    x = _capture(n, P * 100 + Q)
    M = plan.n_out(n)
    got = ops.iq_resample(torch.from_numpy(x).to(DEV), plan, 0, 0, M).cpu().numpy()
    _check(f"{P}/{Q} dphi={plan.dphi}", got, x, plan)


def test_pure_mixer_matches_the_float64_reference():
    from sy11 import ops
    plan = _plan(1, 1, SHIFT)
    assert not plan.filters and plan.dphi != 0
    x = _capture(6001, 9)
    dev = torch.from_numpy(x).to(DEV)
    got = ops.iq_resample(dev, plan, 0, 0, 6001).cpu().numpy()
    _check("1/1 mixer", got, x, plan)
    part = ops.iq_resample(dev[1001:3002], plan, 1001, 1500, 1001, n_total=6001).cpu().numpy()       # odd base, inner range
    assert np.array_equal(part, got[1500:2501])


@pytest.mark.parametrize("P,Q", [(2, 3), (5, 16)])
def test_phase_wraps_exactly_near_three_billion_samples(P, Q):
    """in[] = samples [n0, n0 + n) with n0 near 3e9 (past 2^31 and close to 2^32): (uint32) i * dphi must wrap, not lose bits."""
    from sy11 import ops
    plan = _plan(P, Q, SHIFT)
    n = 9000
    m0 = 3 * 10 ** 9 * P // Q + 17
    n0 = plan.support(m0, m0 + 1)[0] - 3
    M = ((n - 2 * plan.T) * P) // Q - 8
    a, b = plan.support(m0, m0 + M)
    assert n0 <= a and b <= n0 + n and n0 > 2 ** 31 and M > 1000
    x = _capture(n, 21)
    got = ops.iq_resample(torch.from_numpy(x).to(DEV), plan, n0, m0, M, n_total=n0 + n + 12345).cpu().numpy()
    _check(f"{P}/{Q} at n0={n0}", got, x, plan, n0, m0, M)


def test_odd_input_base_and_wrapper_checks():
    """The input starts at an odd sample of its allocation (8-byte, not 16-byte aligned): same outputs, bit for bit, as from an
    aligned copy; the wrapper refuses an input that does not cover the support."""
    from sy11 import _lib, ops
    plan = _plan(2, 3, SHIFT)
    n = 6001
    x = _capture(n, 4)
    buf = torch.zeros(n + 1, dtype=torch.complex64, device=DEV)
    buf[1:] = torch.from_numpy(x).to(DEV)
    odd = buf[1:]
    assert odd.data_ptr() % 16 == 8
    M = plan.n_out(n)
    got = ops.iq_resample(odd, plan, 0, 0, M)
    _check("2/3 odd base", got.cpu().numpy(), x, plan)
    assert torch.equal(got, ops.iq_resample(torch.from_numpy(x).to(DEV), plan, 0, 0, M))
    a, b = plan.support(1000, 2000)
    inner = ops.iq_resample(odd[a:b], plan, a, 1000, 1000, n_total=n)
    assert torch.equal(inner, got[1000:2000])
    out = torch.empty(1000, dtype=torch.complex64, device=DEV)
    assert ops.iq_resample(odd[a:b], plan, a, 1000, 1000, out=out, n_total=n) is out and torch.equal(out, inner)
    for bad in ((odd[a + 1:b], a + 1), (odd[a:b - 1], a)):
        with pytest.raises(_lib.Sy11Error, match="read samples"):
            ops.iq_resample(bad[0], plan, bad[1], 1000, 1000, n_total=n)
    with pytest.raises(_lib.Sy11Error):
        ops.iq_resample(odd, plan, 0, 0, M + 1)
    with pytest.raises(_lib.Sy11Error):
        ops.iq_resample(odd[a:b], plan, a, 1000, 1000)                     # n0 != 0 without the capture's length


# ------------------------------------------------------------------------------------------------------------- skipped steps
def test_identity_plan_returns_the_source_bit_for_bit():
    from sy11 import ops
    from sy11.data.resample import ResampledCapture
    plan = _plan(7, 7, 0.0)
    assert plan.identity
    x = _capture(6000, 1)
    dev = torch.from_numpy(x).to(DEV)
    assert torch.equal(ops.iq_resample(dev, plan, 0, 0, 6000), dev)
    assert torch.equal(ops.iq_resample(dev, plan, 0, 100, 50), dev[100:150])
    for src in (x, dev):
        cap = ResampledCapture(src, plan, DEV)
        assert len(cap) == 6000 and torch.equal(cap[0:6000], dev) and torch.equal(cap[999:2001], dev[999:2001])


# ------------------------------------------------------------------------------------------------------------- chunks
@pytest.mark.parametrize("P,Q,shift", [(2, 3, SHIFT), (5, 16, 0.0), (3, 2, SHIFT), (1, 1, SHIFT)])
def test_resampled_capture_is_bit_identical_for_every_chunking_and_source(tmp_path, P, Q, shift):
    from sy11 import ops
    from sy11.data.resample import ResampledCapture
    from sy11.data.spectrogram import open_iq
    plan = _plan(P, Q, shift)
    n = 12001
    x = _capture(n, 6)
    x.view(np.float32).tofile(tmp_path / "capture.cf32")
    dev = torch.from_numpy(x).to(DEV)
    M = plan.n_out(n)
    whole = ops.iq_resample(dev, plan, 0, 0, M)
    for name, src in (("host array", open_iq(x)), ("memmap", open_iq(str(tmp_path / "capture.cf32"))), ("device tensor", open_iq(dev))):
        cap = ResampledCapture(src, plan, DEV)
        assert len(cap) == M
        for step in (1000, 4097, M):
            parts = [cap[lo:min(lo + step, M)] for lo in range(0, M, step)]
            assert all(p.is_cuda and p.dtype == torch.complex64 for p in parts)
            assert torch.equal(torch.cat(parts), whole), (name, step)


# ------------------------------------------------------------------------------------------------------------- physics
def test_tones_keep_frequency_and_amplitude_and_the_alias_is_rejected():
    """fs_out = fs_in / 2, retuned by ~0.1 fs_in.  Three unit tones: in band, at 0.39 fs_out from the new centre, and at 0.7 fs_out
    (outside the kept band; it would fold to -0.3 fs_out).  All three sit on bins of an L-point FFT of the output, so the FFT of L
    outputs away from the ends reads each level with no window."""
    from sy11 import ops
    plan = _plan(1, 2, 0.1 * FS_IN)
    fs_out, L = FS_IN / 2, 4096
    bins = {"in band": 300, "0.39 fs_out": round(0.39 * L), "out of band": round(0.7 * L)}
    n = 2 * (L + 400)
    i = np.arange(n, dtype=np.float64)
    x = sum(np.exp(2j * np.pi * (((k / L) * fs_out + plan.shift_hz) / FS_IN) * i) for k in bins.values())
    y = ops.iq_resample(torch.from_numpy(x.astype(np.complex64)).to(DEV), plan, 0, 0, plan.n_out(n)).cpu().numpy()
    m0 = 200                                                                # past the filter's run-in (T / 2 = 32 outputs)
    seg = y[m0:m0 + L].astype(np.complex128)                               # output m sits at m / fs_out: no delay to undo
    db = 20 * np.log10(np.maximum(np.abs(np.fft.fft(seg)) / L, 1e-30))
    top2 = sorted(np.argsort(db)[-2:].tolist())
    print(f"ddc tones: bins {top2}, levels {db[top2[0]]:+.5f} dB / {db[top2[1]]:+.5f} dB; alias bin {bins['out of band'] - L} at "
          f"{db[bins['out of band'] - L]:.2f} dB; highest other bin {np.sort(db)[-3]:.2f} dB")
    assert all(abs(g - w) <= 1 for g, w in zip(top2, sorted((bins["in band"], bins["0.39 fs_out"]))))
    assert all(abs(db[k]) <= 0.02 for k in top2)
    assert np.sort(db)[-3] <= -70.0                                         # the folded tone, and everything else
    # the phase too: an output is the input tone's value at m / fs_out seconds (zero delay)
    k = bins["in band"]
    tone = np.exp(2j * np.pi * k / L * np.arange(m0, m0 + L))
    assert abs(np.vdot(tone, seg) / L - 1.0) < 1e-3


# ------------------------------------------------------------------------------------------------------------- end to end
def _model(nc=2):
    from oracle import yolo11_ref as Y
    from sy11.nn.tasks import DetectionModel
    m = DetectionModel("yolo11n.yaml", nc=nc, verbose=False)
    sd = Y.seeded_state_dict(Y.empty_state_dict(Y.resolve_graph("n", nc=nc)), seed=7)
    for k in sd:                                               # confident random head, as tests/test_scan_gpu.py builds it
        if ".cv3." in k and k.endswith("2.bias"):
            sd[k] = sd[k] + 1.0
    m.load_state_dict(sd)
    m.names = {i: f"class_{i}" for i in range(nc)}
    return m


def test_resampled_scan_equals_a_scan_of_the_ddc_output():
    from sy11 import ops
    from sy11.data import spectrogram as sp
    from sy11.engine.predictor import DetectionPredictor, plan_scan_ddc
    from tests import _scan_ref as S
    fs, fc, delta = 20e6, 2.4e9, 3.3e6
    x = S.capture(4.1)                                                      # at 2 fs: about two windows of output
    pred = DetectionPredictor(_model(2), device=DEV, conf=0.05, iou=0.7, producer=sp.SpectrogramProducer(DEV))
    plan = plan_scan_ddc(2 * fs, fc, fs, fc + delta)
    assert (plan.P, plan.Q) == (1, 2) and plan.dphi != 0 and abs(plan.shift_hz - delta) < 0.01
    y = ops.iq_resample(x.to(DEV), plan, 0, 0, plan.n_out(len(x)))
    for b in (1, 64):
        got = pred.scan(sp.open_iq(x), 2 * fs, fc, resample_to=fs, tune_to=fc + delta, batch=b)
        want = pred.scan(sp.open_iq(y), fs, fc + plan.shift_hz, batch=b)
        assert len(want) > 0 and len(want.start) >= 3
        for name in ("boxes", "window", "tf"):
            assert torch.equal(getattr(got, name), getattr(want, name)), (b, name)
        assert got.start.tolist() == want.start.tolist()
        assert got.sample_rate == fs == want.sample_rate and got.center_freq == fc + plan.shift_hz == want.center_freq
        assert want.resample is None and (got.resample.P, got.resample.Q, got.resample.dphi) == (1, 2, plan.dphi)
        # seconds of the ORIGINAL capture: frame X of the output starts at input sample 2 X hop
        assert torch.equal(got.tf, torch.from_numpy(np.stack((sp.cols_to_time(got.boxes[:, 0].numpy() - 0.5, fs),
                                                              sp.rows_to_freq(got.boxes[:, 1].numpy() - 0.5, fs, fc + plan.shift_hz),
                                                              sp.cols_to_time(got.boxes[:, 2].numpy() - 0.5, fs),
                                                              sp.rows_to_freq(got.boxes[:, 3].numpy() - 0.5, fs, fc + plan.shift_hz)), 1)))
        assert float(got.tf[:, 2].max()) <= len(x) / (2 * fs) and float(got.tf[:, 1].min()) >= fc + delta - fs / 2 - 1
    plain = pred.scan(sp.open_iq(y), fs, fc + plan.shift_hz, batch=64, resample_to=None, tune_to=None)
    for name in ("boxes", "window", "tf"):
        assert torch.equal(getattr(plain, name), getattr(want, name))
    assert plain.resample is None
