"""CPU: the host side of the long-capture scan — window planning, the row -> Hz / column -> seconds maps, reading a capture
from a tensor / .npy / raw .cf32 file, the C-ABI surface of the two new entries, and the float64 merge reference that the GPU
test compares the seam-merge kernel against."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from sy11.data import spectrogram as sp
from tests import _scan_ref as R

ROOT = Path(__file__).resolve().parents[1]
N_FFT, HOP, N_FRAMES, N_MEL, ALPHA = 1024, 256, 640, 640, 1.25
N_SAMPLES = N_FFT + (N_FRAMES - 1) * HOP


def _fits(start, n_samples):
    return all(N_FFT + (int(s) + N_FRAMES - 1) * HOP <= n_samples for s in start)


def test_plan_windows_grid_and_end_aligned_last_window():
    n = N_SAMPLES + 700 * HOP + 100                                   # 1340 full frames: the grid 0, 320, 640 ends 60 frames early
    start = sp.plan_windows(n, overlap=0.5)
    assert start.dtype == np.int64 and start.tolist() == [0, 320, 640, 700]
    assert _fits(start, n) and not _fits([701], n)
    assert sp.plan_windows(n, stride_frames=200).tolist() == [0, 200, 400, 600, 700]
    assert sp.plan_windows(n, overlap=0.0).tolist() == [0, 640, 700]
    assert sp.plan_windows(n, overlap=0.75).tolist() == [0, 160, 320, 480, 640, 700]


def test_plan_windows_exact_fit_one_window_and_too_short():
    exact = N_SAMPLES + 2 * 320 * HOP                                  # ends on the grid: no duplicate last window
    assert sp.plan_windows(exact, overlap=0.5).tolist() == [0, 320, 640]
    assert sp.plan_windows(exact + HOP - 1, overlap=0.5).tolist() == [0, 320, 640]      # a partial frame is not a frame
    assert sp.plan_windows(N_SAMPLES).tolist() == [0]
    assert sp.plan_windows(N_SAMPLES + HOP).tolist() == [0, 1]
    with pytest.raises(ValueError, match=f"need >= {N_SAMPLES} IQ samples"):
        sp.plan_windows(N_SAMPLES - 1)
    with pytest.raises(ValueError):
        sp.plan_windows(10 * N_SAMPLES, overlap=1.0)
    for n in (N_SAMPLES, 3 * N_SAMPLES + 17, 10 * N_SAMPLES - 1):
        for kw in ({"overlap": 0.0}, {"overlap": 0.5}, {"overlap": 0.75}, {"stride_frames": 200}, {"stride_frames": 1}):
            start = sp.plan_windows(n, **kw)
            assert _fits(start, n) and np.all(np.diff(start) > 0) and start[0] == 0
            assert start[-1] == (n - N_FFT) // HOP + 1 - N_FRAMES


def test_plan_chunks_cover_their_windows_and_split_at_gaps():
    start = sp.plan_windows(12 * N_SAMPLES, overlap=0.5)
    for cw in (1, 3, 64):
        chunks = sp.plan_chunks(start, cw)
        assert [c[0] for c in chunks] == list(range(0, start.size, cw)) and chunks[-1][1] == start.size
        for w0, w1, lo, hi in chunks:
            assert w1 - w0 <= cw and lo == start[w0] * HOP and hi == N_FFT + (start[w1 - 1] + N_FRAMES - 1) * HOP < 2 ** 31
    far = np.array([0, 320, 5000, 5100, 3 * 10 ** 9], dtype=np.int64)
    assert [(c[0], c[1]) for c in sp.plan_chunks(far, 64)] == [(0, 2), (2, 4), (4, 5)]
    with pytest.raises(ValueError):
        sp.plan_chunks(np.array([5, 3]), 4)
    with pytest.raises(ValueError):
        sp.plan_chunks(start, 20000)


def test_rows_to_freq_inverts_freq_to_row_and_is_monotone():
    """rows_to_freq and oracle.synth_iq.freq_to_row are closed forms of each other: the bar (1e-12 absolute on a normalised
    frequency of magnitude <= 0.5, float64) is log1p / expm1 round-off, a few 1e-16."""
    from oracle.synth_iq import freq_to_row
    f = np.random.default_rng(5).uniform(-0.5, 0.5 - 1.0 / N_FFT, 1000)
    back = sp.rows_to_freq(freq_to_row(f, N_FFT, N_MEL, ALPHA), 1.0, 0.0, N_FFT, N_MEL, ALPHA)
    assert back.dtype == np.float64 and np.abs(back - f).max() <= 1e-12
    hz = sp.rows_to_freq(np.arange(N_MEL), 20e6, 2.4e9)
    assert np.all(np.diff(hz) > 0) and 2.4e9 - 10e6 < hz[0] and hz[-1] < 2.4e9 + 10e6
    assert np.allclose(sp.rows_to_freq(np.arange(N_MEL), 20e6, 2.4e9), 2.4e9 + 20e6 * sp.rows_to_freq(np.arange(N_MEL), 1.0), rtol=0, atol=1e-3)


def test_cols_to_time_is_linear_from_the_first_frame_centre():
    fs = 20e6
    t = sp.cols_to_time(np.array([0.0, 1.0, 2.5, 3e9]), fs)
    assert t.dtype == np.float64 and t[0] == (N_FFT / 2) / fs
    assert np.allclose(np.diff(t[:2]), HOP / fs, rtol=1e-15) and t[2] == (2.5 * HOP + N_FFT / 2) / fs and t[3] == (3e9 * HOP + 512) / fs


def test_sources_give_the_same_chunks_and_bytes(tmp_path):
    n = 3 * N_SAMPLES + 1234
    rng = np.random.default_rng(2)
    iq = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    np.save(tmp_path / "cap.npy", iq)
    iq.view(np.float32).tofile(tmp_path / "cap.cf32")
    srcs = {"tensor": sp.open_iq(torch.from_numpy(iq)), "array": sp.open_iq(iq), "npy": sp.open_iq(tmp_path / "cap.npy"),
            "raw": sp.open_iq(str(tmp_path / "cap.cf32"))}
    assert isinstance(srcs["raw"], np.memmap) and isinstance(srcs["npy"], np.memmap)          # never read whole
    plans = {k: sp.plan_chunks(sp.plan_windows(len(v), overlap=0.5), 2) for k, v in srcs.items()}
    assert all(p == plans["tensor"] for p in plans.values()) and len(plans["tensor"]) > 1
    for _, _, lo, hi in plans["tensor"]:
        want = iq[lo:hi].tobytes()
        for k, v in srcs.items():
            got = sp.read_samples(v, lo, hi)
            assert got.dtype == np.complex64 and got.flags.c_contiguous and got.tobytes() == want, k
    with pytest.raises(ValueError):
        sp.read_samples(srcs["raw"], n - 10, n + 10)
    (tmp_path / "odd.iq").write_bytes(b"\0" * 12)
    with pytest.raises(ValueError):
        sp.open_iq(tmp_path / "odd.iq")
    with pytest.raises(ValueError):
        sp.open_iq(tmp_path / "cap.wav")
    with pytest.raises(ValueError):
        sp.open_iq(torch.zeros(4, 4, dtype=torch.complex64))


def test_scan_entries_are_declared_bound_and_exported():
    from sy11 import _lib
    header = (ROOT / "include" / "sy11.h").read_text()
    lib = _lib.load()
    table = {**_lib.SIGNATURES, **{k: v[0] for k, v in _lib.OTHER.items()}}
    for name in ("sy11_stft_windows", "sy11_scan_merge", "sy11_scan_merge_workspace_bytes"):
        m = re.search(rf"\b{name}\s*\(([^;]*?)\)\s*;", header, re.S)
        assert m, f"{name} is not declared in include/sy11.h"
        assert name in table and hasattr(lib, name)
        assert len([p for p in m.group(1).split(",") if p.strip()]) == len(table[name])
    # argument validation returns before any launch
    assert lib.sy11_stft_windows(100, 640, 640, 1, None, None, None, None, None, None) == -1 and b"does not fit" in lib.sy11_last_error()
    assert lib.sy11_scan_merge(5, 1, 640, None, None, None, None, None, 1, 0.5, 0, None, None, None) == -1
    assert lib.sy11_scan_merge(5, 1, 640, None, None, None, None, None, 7, 0.5, 0, None, None, None) == -1 and b"metric" in lib.sy11_last_error()
    assert lib.sy11_scan_merge(0, 1, 640, None, None, None, None, None, 1, 0.5, 0, None, None, None) == 0        # empty input: nothing to do
    assert lib.sy11_scan_merge_workspace_bytes(0, 4) == 0
    small, big = lib.sy11_scan_merge_workspace_bytes(1000, 10), lib.sy11_scan_merge_workspace_bytes(2000, 10)
    assert 2 * 1000 <= small < big <= small + 2 * 1000 + 64                                                   # O(n): no pair matrix


def test_front_door_has_scan():
    from sy11.engine.model import YOLO
    from sy11.engine.predictor import DetectionPredictor, ScanResults
    from sy11 import ops
    assert callable(YOLO.scan) and callable(DetectionPredictor.scan) and callable(ops.stft_windows) and callable(ops.scan_merge)
    r = ScanResults(torch.zeros((0, 6), dtype=torch.float64), torch.zeros(0, dtype=torch.int64), torch.zeros((0, 4), dtype=torch.float64),
                    {0: "a"}, np.zeros(1, np.int64), 1.0, 0.0)
    assert len(r) == 0


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_reference_merge_agrees_with_nms_core_on_one_window(seed):
    """Pins tests/_scan_ref.merge_ref: one window, one class, IoU -> the kept set of oracle.nms_ref.nms_core (f32 there, f64 here:
    the generator keeps every pair's metric 1e-4 away from the threshold, far more than f32 round-off of an IoU)."""
    from oracle.nms_ref import nms_core
    for thres in (0.45, 0.7):
        window, boxes, score, cls, start = R.survivors(seed, 1, 640, 1, "iou", thres, False)
        assert len(window) > 100
        keep = R.merge_ref(window, boxes, score, cls, start, N_FRAMES, "iou", thres, False)
        assert np.array_equal(np.sort(nms_core(boxes, score, thres)), np.nonzero(keep)[0])
        assert 0 < keep.sum() < len(window)


def test_reference_merge_hand_cases():
    st = np.array([0, 320, 640], dtype=np.int64)
    one = np.ones
    # a box and its edge-cut twin in the next window: IoS merges them, IoU does not
    w = np.array([0, 1], np.int32)
    b = np.array([[500, 100, 640, 200], [180, 100, 420, 200]], np.float32)            # strip 500..640 (cut) and 500..740 (whole)
    s = np.array([0.6, 0.9], np.float32)
    assert R.merge_ref(w, b, s, one(2, np.int32), st, 640, "ios", 0.5).tolist() == [False, True]
    assert R.merge_ref(w, b, s, one(2, np.int32), st, 640, "iou", 0.7).tolist() == [True, True]
    assert R.merge_ref(w, b, s, np.array([0, 1], np.int32), st, 640, "ios", 0.5).tolist() == [True, True]
    assert R.merge_ref(w, b, s, np.array([0, 1], np.int32), st, 640, "ios", 0.5, agnostic=True).tolist() == [False, True]
    # A suppresses B; B would have suppressed C; C is kept
    w = np.array([0, 0, 1], np.int32)
    b = np.array([[300, 0, 400, 100], [350, 0, 450, 100], [80, 0, 180, 100]], np.float32)   # strip 300-400, 350-450, 400-500
    s = np.array([0.9, 0.8, 0.7], np.float32)
    assert R.merge_ref(w, b, s, one(3, np.int32), st, 640, "iou", 0.3).tolist() == [True, False, True]
