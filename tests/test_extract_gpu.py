"""GPU: the extraction kernel (sy11_iq_extract).  Its main oracle needs no tolerance: every clip is, bit for bit, what the shipped DDC
(``ops.iq_resample`` with P = 1, Q = D) gives over the same outputs.  Beside it: the float64 reference of tests/_extract_ref.py under the
rule of tests/test_resample_gpu.py (per clip, 4x the error of the float32 emulation of the same sum, which must be > 0), chunking and
source invariance, absolute sample indices past 2^31, an odd input base, the wrapper's errors, and ``extract`` behind the three kinds
of scan."""
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import _extract_ref as E

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FS, FC, N = 1.0e6, 2.4e9, 40000
PAD_T = 0.001
# [t0_s, f_lo - FC, t1_s, f_hi - FC]; with pad_f = 0.1 the band is 1.2 x the box: D = 64 up to 10.9 kHz, 16 in (21.9, 43.75] kHz,
# 4 in (87.5, 175] kHz, 2 in (175, 350] kHz, 1 above
BOXES = [
    (0.0100, 0.85e5, 0.0200, 1.15e5),      # 0  D = 16, three tiles
    (0.0150, 0.95e5, 0.0250, 1.25e5),      # 1  D = 16, overlaps 0 in time and in frequency
    (0.0003, -2.225e5, 0.0030, -2.175e5),  # 2  D = 64, starts before sample 0 once pad_t is taken off
    (0.0395, -2.5e5, 0.0400, 3.5e5),       # 3  D = 1, ends on the capture's last sample
    (0.0300, -2.25e5, 0.0340, -0.75e5),    # 4  D = 4, two tiles
    (0.0220, -1.0e4, 0.0260, 1.0e4),       # 5  D = 32, centred on FC: dphi = 0
    (0.0410, 0.5e5, 0.0420, 0.55e5),       # 6  D = 64, wholly past the end: a single output, the capture's last
    (0.0050, 0.75e5, 0.0110, 3.25e5),      # 7  D = 2, four tiles
    (0.0020, -3.02e5, 0.0380, -2.98e5),    # 8  D = 64, ten tiles
    (0.0200, -3.6e5, 0.0215, 2.4e5),       # 9  D = 1, four tiles
    (0.0000, 3.0e5, 0.0040, 3.3e5),        # 10 D = 16 from the first sample
    (0.0280, -0.6e5, 0.0281, 0.9e5),       # 11 D = 4, short
]
WANT_D = [16, 16, 64, 1, 4, 32, 64, 2, 64, 1, 16, 4]


def _capture(n, seed=0):
    g = np.random.default_rng(seed)
    return (g.standard_normal(n) + 1j * g.standard_normal(n)).astype(np.complex64)


def _ddc_plan(D, dphi):
    """The shipped DDC's plan for decimation D and the shift that ``dphi`` really applies."""
    from sy11.data.resample import plan_resample
    signed = dphi - (1 << 32) if dphi >= 1 << 31 else dphi
    rp = plan_resample(FS, Fraction(FS) / D, (FC + -signed / 2.0 ** 32 * FS) - FC)
    assert rp.dphi == dphi and (rp.P, rp.Q) == (1, D)
    return rp


def _bits(t):
    return torch.view_as_real(t).contiguous().view(torch.int32)


def _check(name, got, want, emu):
    scale = np.abs(want).max()
    e_emu = np.abs(emu - want).max() / scale
    e_gpu = np.abs(got.astype(np.complex128) - want).max() / scale
    print(f"iq_extract[{name}]: {len(want)} outputs, float32 emulation {e_emu:.3e}, kernel {e_gpu:.3e} (bar {4 * e_emu:.3e})")
    assert got.shape == want.shape and got.dtype == np.complex64
    assert e_emu > 0 and e_gpu <= 4 * e_emu, (name, e_gpu, e_emu)


@pytest.fixture(scope="module")
def case():
    """The capture, its plan and ONE launch over all twelve boxes; shared and left unchanged."""
    from sy11.data.extract import extract_capture, plan_extract, plan_extract_chunks
    x = _capture(N, 3)
    tf = np.array([(t0, FC + lo, t1, FC + hi) for t0, lo, t1, hi in BOXES])
    plan = plan_extract(tf, N, FS, FC, pad_t=PAD_T)
    assert plan.D.tolist() == WANT_D
    assert plan.m_first[2] == 0 and plan.m_first[10] == 0 and plan.M[6] == 1 and plan.dphi[5] == 0 and (np.delete(plan.dphi, 5) != 0).all()
    assert plan.m_first[3] + plan.M[3] == N and plan.m_first[6] == (N - 1) // 64 and plan.M[8] > 9 * 64
    dev = torch.from_numpy(x).to(DEV)
    assert len(plan_extract_chunks(plan, 1 << 24)) == 1
    return x, dev, plan, extract_capture(dev, plan, DEV)


# ------------------------------------------------------------------------------------------------------------- the main oracle
def test_every_clip_is_bit_identical_to_the_shipped_ddc(case):
    from sy11 import ops
    x, dev, plan, ex = case
    assert len(ex) == len(BOXES) and ex.packed.shape == (plan.total,) and ex.packed.is_cuda
    for k in range(len(plan)):
        rp = _ddc_plan(int(plan.D[k]), int(plan.dphi[k]))
        want = ops.iq_resample(dev, rp, 0, int(plan.m_first[k]), int(plan.M[k]))
        assert ex[k].shape == want.shape and ex[k].dtype == torch.complex64
        assert torch.equal(_bits(ex[k]), _bits(want)), (k, int(plan.D[k]))
    assert ex.sample_rate.tolist() == [FS / d for d in WANT_D] and ex.t0.tolist() == (plan.m_first * plan.D / FS).tolist()


def test_every_clip_matches_the_float64_reference(case):
    x, dev, plan, ex = case
    for k in range(len(plan)):
        _check(f"clip {k} D={plan.D[k]} dphi={plan.dphi[k]}", ex[k].cpu().numpy(), E.plan_clip(x, plan, k), E.plan_clip(x, plan, k, f32=True))


# ------------------------------------------------------------------------------------------------------------- chunks and sources
def test_smallest_chunks_and_every_source_give_the_same_bits(case, tmp_path):
    from sy11 import _lib
    from sy11.data.extract import MIN_CHUNK, extract_capture, plan_extract_chunks
    from sy11.data.spectrogram import open_iq
    x, dev, plan, ex = case
    x.view(np.float32).tofile(tmp_path / "capture.cf32")
    chunks = plan_extract_chunks(plan, MIN_CHUNK)
    pieces = np.bincount(np.concatenate([c.clip for c in chunks]), minlength=len(plan))
    assert len(chunks) > 10 and pieces.max() > 4 and pieces[6] == 1         # split clips, many launches
    for name, src in (("device tensor", open_iq(dev)), ("host array", open_iq(x)), ("memmap", open_iq(str(tmp_path / "capture.cf32")))):
        for chunk_samples, launches in ((MIN_CHUNK, len(chunks)), (15000, None), (1 << 24, 1)):
            _lib.PROFILE = []
            try:
                got = extract_capture(src, plan, DEV, chunk_samples)
                calls = [c[0] for c in _lib.PROFILE]
            finally:
                _lib.PROFILE = None
            assert torch.equal(_bits(got.packed), _bits(ex.packed)), (name, chunk_samples)
            assert set(calls) == {"sy11_iq_extract"} and (launches is None or len(calls) == launches)      # one launch per chunk


# ------------------------------------------------------------------------------------------------------------- far into a capture
def test_absolute_indices_near_three_billion_samples():
    """x holds samples [n0, n0 + 9000) of a long capture, n0 near 3e9 (past 2^31, close to 2^32): (uint32) i * dphi must wrap, not lose
    bits, and the grid index m D must be formed in 64 bits."""
    from sy11 import ops
    from sy11.data.extract import SEGMENT, taps_on
    from sy11.data.resample import plan_resample
    n, n0 = 9000, 3 * 10 ** 9 + 7
    n_total = n0 + n + 12345
    x = _capture(n, 21)
    dev = torch.from_numpy(x).to(DEV)
    dphi = plan_resample(FS, FS, 0.0371e6).dphi
    seg = np.zeros(5, dtype=SEGMENT)
    for i, (l, M) in enumerate(((0, 3000), (1, 2100), (2, 1100), (4, 300), (6, 100))):
        D = 1 << l
        m0 = -(-n0 // D) + (16 if l else 0) + 1
        assert (m0 - (16 if l else 0)) * D >= n0 and (m0 + M + (15 if l else 0)) * D + 1 <= n0 + n
        seg[i] = (m0, 0, M, l, dphi, 0)
    seg["out_off"] = np.cumsum(seg["M"]) - seg["M"]
    out = torch.zeros(int(seg["M"].sum()), dtype=torch.complex64, device=DEV)
    assert ops.iq_extract(dev, n0, n_total, seg, taps_on(DEV), out) is out
    for s in seg:
        D, m0, M = 1 << int(s["log2d"]), int(s["m0"]), int(s["M"])
        got = out[int(s["out_off"]):int(s["out_off"]) + M]
        want = ops.iq_resample(dev, _ddc_plan(D, dphi), n0, m0, M, n_total=n_total)
        assert torch.equal(_bits(got), _bits(want)), D
        _check(f"D={D} at n0={n0}", got.cpu().numpy(), E.clip(x, D, dphi, m0, M, n0), E.clip(x, D, dphi, m0, M, n0, f32=True))


# ------------------------------------------------------------------------------------------------------------- odd base, wrapper checks
def test_odd_input_base_and_wrapper_checks(case):
    """The input starts at an odd sample of its allocation (8-byte, not 16-byte aligned): same bits as from an aligned copy, whole and
    as an inner slice; every refusal of the wrapper."""
    from sy11 import _lib, ops
    from sy11.data.extract import SEGMENT, plan_extract_chunks, taps_on
    x, dev, plan, ex = case
    buf = torch.zeros(N + 1, dtype=torch.complex64, device=DEV)
    buf[1:] = dev
    odd = buf[1:]
    assert odd.data_ptr() % 16 == 8
    seg = plan_extract_chunks(plan, 1 << 24)[0].segments
    taps = taps_on(DEV)
    out = torch.zeros_like(ex.packed)
    ops.iq_extract(odd, 0, N, seg, taps, out)
    assert torch.equal(_bits(out), _bits(ex.packed))
    inner = seg[[int(np.flatnonzero(plan_extract_chunks(plan, 1 << 24)[0].clip == k)[0]) for k in (0, 1, 9)]].copy()     # D = 16, 16, 1
    a, b = 8000, 27000                                                      # an odd base again; covers [9000 - 256, 26000 + 256] and [19000, 22500]
    o2 = torch.zeros_like(ex.packed)
    ops.iq_extract(odd[a:b], a, N, inner, taps, o2)
    for s in inner:
        sl = slice(int(s["out_off"]), int(s["out_off"]) + int(s["M"]))
        assert torch.equal(_bits(o2[sl]), _bits(ex.packed[sl]))

    def one(**kw):
        s = inner[:1].copy()
        for k, v in kw.items():
            s[k] = v
        return s
    E_ = _lib.Sy11Error
    for bad_x in (odd.to(torch.complex128), torch.view_as_real(odd)[:, 0], odd[::2], odd[:0], odd.cpu()):
        with pytest.raises(E_):
            ops.iq_extract(bad_x, 0, N, seg, taps, out)
    with pytest.raises(E_, match="leave the capture"):
        ops.iq_extract(odd, 1, N, seg, taps, out)
    with pytest.raises(E_, match="leave the capture"):
        ops.iq_extract(odd, -1, N, seg, taps, out)
    for bad_out in (out.to(torch.complex128), out[::2], out.cpu(), out[:0], out[:, None]):
        with pytest.raises(E_):
            ops.iq_extract(odd, 0, N, seg, taps, bad_out)
    for bad_taps in (taps[:-1], taps.double(), taps.cpu()):
        with pytest.raises(E_):
            ops.iq_extract(odd, 0, N, seg, bad_taps, out)
    for bad_seg in (seg[:0], np.zeros((2, 6), dtype=np.int64), seg.reshape(1, -1)):
        with pytest.raises(E_, match="SEGMENT"):
            ops.iq_extract(odd, 0, N, bad_seg, taps, out)
    for l in (-1, 7):
        with pytest.raises(E_, match="log2 D"):
            ops.iq_extract(odd, 0, N, one(log2d=l), taps, out)
    for kw in (dict(M=0), dict(m0=-1), dict(m0=N // 16, M=1), dict(m0=N // 16 - 10, M=11)):
        with pytest.raises(E_, match="not on the capture"):
            ops.iq_extract(odd, 0, N, one(**kw), taps, out)
    for off in (-1, out.shape[0] - int(inner[0]["M"]) + 1):
        with pytest.raises(E_, match="writes"):
            ops.iq_extract(odd, 0, N, one(out_off=off), taps, out)
    lo, hi = (int(inner[0]["m0"]) - 16) * 16, (int(inner[0]["m0"]) + int(inner[0]["M"]) + 15) * 16 + 1
    ops.iq_extract(odd[lo:hi], lo, N, inner[:1], taps, o2)                  # exactly the support: accepted
    for bad in ((odd[lo + 1:hi], lo + 1), (odd[lo:hi - 1], lo)):
        with pytest.raises(E_, match="reads samples"):
            ops.iq_extract(bad[0], bad[1], N, inner[:1], taps, o2)
    assert torch.equal(_bits(out), _bits(ex.packed))                        # no refused call wrote anything


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


def test_extract_follows_tf_behind_every_kind_of_scan():
    """``extract(capture, scan(...))`` after a plain, a resampled / retuned and a channelised scan of ONE capture: always with the
    capture's own rate and centre, always len(results) clips with the planned lengths, rates and centres, and the DDC's bits."""
    from sy11 import _lib, ops
    from sy11.data import spectrogram as sp
    from sy11.data.resample import USABLE_BAND
    from sy11.engine.predictor import DetectionPredictor, ScanResults
    from tests import _scan_ref as S
    fs, fc = 40e6, 2.4e9
    x = S.capture(3.1)
    src = sp.open_iq(x)
    dev = x.to(DEV)
    pred = DetectionPredictor(_model(2), device=DEV, conf=0.05, iou=0.7, producer=sp.SpectrogramProducer(DEV))
    scans = {"plain": pred.scan(src, fs, fc), "resampled": pred.scan(src, fs, fc, resample_to=fs / 2, tune_to=fc + 3.3e6),
             "channelised": pred.scan(src, fs, fc, channels=4)}
    assert scans["resampled"].sample_rate == fs / 2 == scans["channelised"].sample_rate        # not the capture's: hence the arguments
    for name, res in scans.items():
        assert len(res) > 0
        ex = pred.extract(src, res, fs, fc, pad_t=1e-4)
        tf = res.tf.numpy()
        assert len(ex) == len(res) and ex.rows.tolist() == list(range(len(res)))
        B = (tf[:, 3] - tf[:, 1]) * 1.2
        D = np.array([max([d for d in (1, 2, 4, 8, 16, 32, 64) if USABLE_BAND * fs / d >= b] or [1]) for b in B])
        first = np.clip(np.floor((tf[:, 0] - 1e-4) * fs / D), 0, (len(x) - 1) // D).astype(np.int64)
        last = np.clip(np.ceil((tf[:, 2] + 1e-4) * fs / D), 0, (len(x) - 1) // D).astype(np.int64)
        assert ex.decimation.tolist() == D.tolist() and [len(c) for c in ex.samples] == (last - first + 1).tolist()
        assert ex.sample_rate.tolist() == (fs / D).tolist() and ex.t0.tolist() == (first * D / fs).tolist()
        assert np.abs(ex.center_freq - (tf[:, 1] + tf[:, 3]) / 2).max() <= fs / 2.0 ** 33 + 1e-6
        assert ex.cls.tolist() == res.boxes[:, 5].long().tolist() and ex.names == res.names
        print(f"extract behind a {name} scan: {len(ex)} clips, {ex.plan.total} samples, D in {sorted(set(D.tolist()))}")
        for k in np.linspace(0, len(ex) - 1, 4).astype(int):                # a few clips against the shipped DDC
            from sy11.data.resample import plan_resample
            rp = plan_resample(fs, Fraction(fs) / int(D[k]), ex.center_freq[k] - fc)
            assert rp.dphi == ex.plan.dphi[k]
            assert torch.equal(_bits(ex[k]), _bits(ops.iq_resample(dev, rp, 0, int(first[k]), len(ex[k]))))
        some = pred.extract(src, res, fs, fc, pad_t=1e-4, rows=[len(res) - 1, 0])
        assert torch.equal(_bits(some[0]), _bits(ex[len(res) - 1])) and torch.equal(_bits(some[1]), _bits(ex[0]))
    res = scans["plain"]
    empty = ScanResults(res.boxes[:0], res.window[:0], res.tf[:0], res.names, res.start, res.sample_rate, res.center_freq)
    _lib.PROFILE = []
    try:
        none = [pred.extract(src, empty, fs, fc), pred.extract(src, res, fs, fc, rows=[])]
        calls = list(_lib.PROFILE)
    finally:
        _lib.PROFILE = None
    assert calls == [] and all(len(e) == 0 and e.samples == [] and e.packed.shape == (0,) for e in none)     # no launch
