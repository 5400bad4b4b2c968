"""CPU: the polyphase filter bank's definition (tests/_pfb_ref.py) against the per-channel float64 DDC reference it is defined by
(tests/_ddc_ref.py), the float32 emulation's distance from it, the plan's arithmetic and argument errors, what the bank does to
tones, and the cross-channel merge against a brute-force greedy.

Parity here is unpinned against the reference project (the feature has no counterpart there) and pinned against ``_ddc_ref``."""
import numpy as np
import pytest

from sy11.data.channelize import ChannelPlan, merge_channels, plan_channels, plan_scan_channels
from tests import _ddc_ref as R
from tests import _pfb_ref as P

FS_IN = 1.0e6
IDENTITY_CASES = [(8, 2, 700), (8, 1, 700), (16, 2, 1201), (4, 2, 333), (64, 2, 3000), (2, 1, 301), (2, 2, 301)]
GPU_CASES = [(2, 1, 4099), (2, 2, 4099), (4, 2, 6001), (8, 1, 8191), (16, 2, 20001), (64, 2, 40001), (64, 1, 70003)]


def _capture(n, seed=0):
    g = np.random.default_rng(seed)
    return (g.standard_normal(n) + 1j * g.standard_normal(n)).astype(np.complex64)


def _dphi(k, K):
    return (-k * ((1 << 32) // K)) % (1 << 32)


# ------------------------------------------------------------------------------------------------------------- definition
@pytest.mark.parametrize("K,r,n", IDENTITY_CASES)
def test_fold_and_fft_equal_the_per_channel_ddc_reference(K, r, n):
    plan = plan_channels(FS_IN, K, r)
    x = _capture(n, K * 10 + r)
    got = P.pfb_ref(x, plan.taps, K, plan.D, plan.c)
    assert got.shape == (K, plan.n_out(n))
    table = R.table_of(plan.taps, 1)
    worst = 0.0
    for k in range(K):
        want = R.ddc_ref(x, table, 1, plan.D, plan.c, _dphi(k, K))
        worst = max(worst, np.abs(got[k] - want).max() / np.abs(want).max())
    print(f"pfb_ref vs ddc_ref K={K} r={r} n={n}: {worst:.3e}")
    assert worst <= 1e-12


def test_absolute_index_folding_beyond_two_to_the_32():
    K, r = 16, 2
    plan = plan_channels(FS_IN, K, r)
    n0, n = 3 * 10 ** 9 + 1, 2000
    m0 = -(-(n0 + plan.N) // plan.D)
    M = 150
    a, b = plan.support(m0, m0 + M)
    assert n0 <= a and b <= n0 + n and m0 > 0 and n0 > 2 ** 32 * 0.69
    x = _capture(n, 5)
    got = P.pfb_ref(x, plan.taps, K, plan.D, plan.c, n0, m0, M)
    table = R.table_of(plan.taps, 1)
    for k in range(K):
        want = R.ddc_ref(x, table, 1, plan.D, plan.c, _dphi(k, K), n0, m0, M)
        assert np.abs(got[k] - want).max() <= 1e-12 * np.abs(want).max(), k


@pytest.mark.parametrize("K,r,n", GPU_CASES)
def test_float32_emulation_stays_within_its_cap(K, r, n):
    """A cap, so that a loose emulation cannot loosen the GPU bar (4x this error): the fold alone costs 0.8e-7 .. 1.5e-7 and the
    FFT adds at most log2 K roundings of that size."""
    plan = plan_channels(FS_IN, K, r)
    x = _capture(n, K * 100 + r)
    want = P.plan_ref(x, plan)
    emu = P.plan_ref(x, plan, f32=True)
    assert emu.dtype == np.complex64 and emu.shape == want.shape
    e = np.abs(emu - want).max() / np.abs(want).max()
    print(f"pfb_f32 vs pfb_ref K={K} r={r} n={n}: {e:.3e}")
    assert 0 < e <= 1e-6


# ------------------------------------------------------------------------------------------------------------- plan
def test_plan_arithmetic():
    for K, r in ((2, 1), (2, 2), (4, 2), (16, 1), (16, 2), (64, 2)):
        plan = plan_channels(FS_IN, K, r)
        D = K // r
        assert (plan.K, plan.D, plan.N, plan.c, plan.oversample) == (K, D, 32 * D + 1, 16 * D, r)
        assert plan.fs_out == FS_IN / D and plan.taps.dtype == np.float32 and plan.taps.shape == (plan.N,)
        assert abs(plan.h.sum() - 1.0) < 1e-12
        assert plan.twiddle.dtype == np.complex64 and plan.twiddle.shape == (max(K // 2, 1),)
        assert np.array_equal(plan.twiddle, P.twiddles(K))
        for n in (1, 2, D, D + 1, 5 * D, 5 * D + 1, 12345):
            assert plan.n_out(n) == len(range(0, n, D))
        assert plan.n_out(0) == 0
        for m0, m1 in ((0, 1), (0, 7), (5, 6), (11, 40)):
            read = [m * D + plan.c - t for m in range(m0, m1) for t in range(plan.N)]
            assert plan.support(m0, m1) == (min(read), max(read) + 1)
        with pytest.raises(ValueError):
            plan.support(3, 3)
        want = [k * FS_IN / K if k <= K // 2 else (k - K) * FS_IN / K for k in range(K)]
        assert plan.offset_hz.dtype == np.float64 and plan.offset_hz.tolist() == want
        for k in range(K):
            d = plan.ddc_plan(k)
            assert (d.P, d.Q, d.dphi, d.c, d.N) == (1, D, _dphi(k, K), plan.c, plan.N)
            assert d.shift_hz == plan.offset_hz[k]
            if D > 1:
                assert np.array_equal(d.taps.reshape(-1)[:plan.N], plan.taps)
        assert plan.default_select() == [k for k in range(K) if k != K // 2]


def test_argument_errors():
    for K in (3, 0, 128, 6, -4, 2.0, "8"):
        with pytest.raises(ValueError, match=r"2, 4, 8, 16, 32, 64"):
            plan_channels(FS_IN, K)
    for r in (3, 0, 4):
        with pytest.raises(ValueError, match=r"\(1, 2\)"):
            plan_channels(FS_IN, 8, r)
    with pytest.raises(ValueError):
        plan_channels(-1.0, 8)
    with pytest.raises(ValueError, match="tune_to"):
        plan_scan_channels(FS_IN, 8, tune_to=1.0e5)
    with pytest.raises(ValueError, match="resample_to"):
        plan_scan_channels(FS_IN, 8, resample_to=FS_IN / 4)
    with pytest.raises(ValueError, match="records no sample_rate"):
        plan_scan_channels(160e6, "model", trained={})
    with pytest.raises(ValueError, match="power of two"):
        plan_scan_channels(60e6, "model", trained={"sample_rate": 20e6})
    with pytest.raises(ValueError, match="power of two"):
        plan_scan_channels(20e6, "model", trained={"sample_rate": 30e6})
    with pytest.raises(ValueError, match="power of two"):
        plan_scan_channels(64 * 20e6, "model", trained={"sample_rate": 20e6})                   # K = 128
    with pytest.raises(ValueError):
        plan_scan_channels(FS_IN, "auto")
    for bad in ([], [8], [-1], ["a"]):
        with pytest.raises(ValueError, match="select"):
            plan_scan_channels(FS_IN, 8, select=bad)
    plan, sel = plan_scan_channels(160e6, "model", trained={"sample_rate": 20e6})
    assert (plan.K, plan.D, plan.oversample, plan.fs_out) == (16, 8, 2, 20e6) and sel == plan.default_select()
    plan, sel = plan_scan_channels(160e6, "model", oversample=1, select=(3, 1, 3), trained={"sample_rate": 20e6})
    assert (plan.K, plan.D) == (8, 8) and sel == [1, 3]
    ready = ChannelPlan(FS_IN, 4, 2)
    assert plan_scan_channels(FS_IN, ready)[0] is ready


def test_scan_rejects_channels_with_a_ddc_before_touching_a_device():
    from sy11.engine.model import YOLO
    y = YOLO.__new__(YOLO)                                                  # no model, no device: the errors come first
    y.ckpt = None
    x = np.zeros(8, dtype=np.complex64)
    with pytest.raises(ValueError, match="tune_to"):
        y.scan(x, FS_IN, channels=4, tune_to=1.0e5)
    with pytest.raises(ValueError, match="records no sample_rate"):
        y.scan(x, FS_IN, channels="model")
    with pytest.raises(ValueError, match="2, 4, 8, 16, 32, 64"):
        y.scan(x, FS_IN, channels=3)


# ------------------------------------------------------------------------------------------------------------- physics
@pytest.mark.parametrize("r", [2, 1])
def test_tone_levels(r):
    """K = 16, a unit tone exactly on a channel's centre: 0 dB in its own channel; with oversample 2 the neighbours see it on their
    band edge (-6.02 dB); every other channel <= -70 dB (measured about -102)."""
    K = 16
    plan = plan_channels(FS_IN, K, r)
    n = 4000
    i = np.arange(n, dtype=np.float64)
    for kc in (3, 8, 13):
        x = np.exp(2j * np.pi * (kc / K) * i).astype(np.complex64)
        y = P.pfb_ref(x, plan.taps, K, plan.D, plan.c)
        mid = slice(40, y.shape[1] - 40)                                    # past the filter's run-in and run-out (16 steps)
        db = 20 * np.log10(np.maximum(np.abs(y[:, mid]).max(axis=1), 1e-30))
        lo = 20 * np.log10(np.maximum(np.abs(y[:, mid]).min(axis=1), 1e-30))
        near = [(kc - 1) % K, (kc + 1) % K]
        far = [k for k in range(K) if k != kc and (r == 1 or k not in near)]
        print(f"pfb tone on channel {kc}, oversample {r}: own {db[kc]:+.4f} dB, neighbours {db[near[0]]:+.3f} / {db[near[1]]:+.3f} dB, "
              f"highest other {db[far].max():.1f} dB")
        assert abs(db[kc]) <= 0.02 and abs(lo[kc]) <= 0.02
        if r == 2:
            assert all(abs(db[k] + 6.02) <= 0.1 and abs(lo[k] + 6.02) <= 0.1 for k in near)
        assert db[far].max() <= -70.0


# ------------------------------------------------------------------------------------------------------------- merge
def _metric(a, b, metric):
    iw = max(0.0, min(a[2], b[2]) - max(a[0], b[0]))
    ih = max(0.0, min(a[3], b[3]) - max(a[1], b[1]))
    inter = iw * ih
    aa, ab = (a[2] - a[0]) * (a[3] - a[1]), (b[2] - b[0]) * (b[3] - b[1])
    return inter / min(aa, ab) if metric == "ios" else inter / (aa + ab - inter)


def _brute(tf, score, cls, ch, metric, thres, agnostic):
    n = len(score)
    keep = np.zeros(n, dtype=bool)
    for i in sorted(range(n), key=lambda q: (-score[q], q)):
        ok = True
        for j in np.flatnonzero(keep):
            if ch[j] != ch[i] and (agnostic or cls[j] == cls[i]) and _metric(tf[i], tf[j], metric) > thres:
                ok = False
                break
        keep[i] = ok
    return keep


@pytest.fixture(scope="module")
def rectangles():
    g = np.random.default_rng(11)
    n = 500
    t0 = g.uniform(0.0, 1.0, n)
    f0 = g.uniform(0.0, 100.0, n)
    tf = np.stack((t0, f0, t0 + g.uniform(0.01, 0.12, n), f0 + g.uniform(2.0, 25.0, n)), 1)
    score = np.round(g.uniform(0.05, 1.0, n), 2)                            # ties: the row number decides
    return tf, score, g.integers(0, 3, n), g.integers(0, 4, n)


@pytest.mark.parametrize("agnostic", [False, True])
@pytest.mark.parametrize("metric", ["ios", "iou"])
def test_merge_channels_equals_a_brute_force_greedy(rectangles, metric, agnostic):
    tf, score, cls, ch = rectangles
    thres = 0.5 if metric == "ios" else 0.3
    got = merge_channels(tf, score, cls, ch, metric, thres, agnostic)
    want = _brute(tf, score, cls, ch, metric, thres, agnostic)
    assert got.dtype == bool and np.array_equal(got, want)
    assert 0 < want.sum() < len(want)
    if not agnostic:
        assert want.sum() > _brute(tf, score, cls, ch, metric, thres, True).sum()       # the class matters on this set


def test_merge_channels_same_channel_and_strict_threshold():
    box = [0.0, 0.0, 1.0, 4.0]
    half = [0.0, 0.0, 1.0, 2.0]                                             # ios with box = 1, iou = 0.5 exactly
    tf = np.array([box, box, half])
    score, cls = np.array([0.9, 0.8, 0.7]), np.zeros(3, dtype=np.int64)
    assert merge_channels(tf, score, cls, np.array([1, 1, 1]), "ios", 0.5).tolist() == [True, True, True]      # one channel: never
    assert merge_channels(tf, score, cls, np.array([1, 2, 1]), "ios", 0.5).tolist() == [True, False, True]
    assert merge_channels(tf, score, cls, np.array([1, 1, 2]), "iou", 0.5).tolist() == [True, True, True]      # strict at equality
    assert merge_channels(tf, score, cls, np.array([1, 1, 2]), "iou", 0.4999).tolist() == [True, True, False]
    assert merge_channels(tf, score, np.array([0, 1, 1]), np.array([1, 2, 3]), "ios", 0.5).tolist() == [True, True, False]
    assert merge_channels(tf, score, np.array([0, 1, 2]), np.array([1, 2, 3]), "ios", 0.5, True).tolist() == [True, False, False]
    assert merge_channels(np.zeros((0, 4)), [], [], []).shape == (0,)
    with pytest.raises(ValueError):
        merge_channels(tf, score, cls, cls, "giou")
