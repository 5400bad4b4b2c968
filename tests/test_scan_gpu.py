"""GPU: the long-capture scan — window images cut from one strip against the STFT oracle, their independence of stride and
chunking, the seam-merge kernel against the float64 reference of tests/_scan_ref.py, and the whole path (producer -> model ->
NMS -> merge -> seconds / Hz) against the per-window path the package already had."""
import itertools

import numpy as np
import pytest
import torch

from tests import _scan_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
STRIDES = (640, 320, 160, 200)
CHUNKS = (1, 3, 64)


def _producer():
    from sy11.data.spectrogram import SpectrogramProducer
    return SpectrogramProducer(DEV)


def _model(nc=2):
    from oracle import yolo11_ref as Y
    from sy11.nn.tasks import DetectionModel
    m = DetectionModel("yolo11n.yaml", nc=nc, verbose=False)
    sd = Y.seeded_state_dict(Y.empty_state_dict(Y.resolve_graph("n", nc=nc)), seed=7)
    for k in sd:                                               # confident random head, as tests/test_predict_gpu.py builds it
        if ".cv3." in k and k.endswith("2.bias"):
            sd[k] = sd[k] + 1.0
    m.load_state_dict(sd)
    m.names = {i: f"class_{i}" for i in range(nc)}
    return m, sd


# ------------------------------------------------------------------------------------------------------------- 1, 2: pixels
def test_window_images_match_the_oracle_and_do_not_depend_on_stride_or_chunking():
    """Every window image of every (stride, chunk_windows) equals the oracle's image of that window's own samples within 2e-3
    (min exactly 0, max within 1e-6 of 1: the bars of test_stft_logmel_matches_oracle), and the image of a given start frame is
    bit-identical across all strides and chunk sizes (a frame's transform reads only its own 1024 samples)."""
    from oracle import stft_ref as S
    from sy11.data import spectrogram as sp
    iq = R.capture(6.3)
    p = _producer()
    src = sp.open_iq(iq)
    oracle, first = {}, {}
    worst = 0.0
    for stride, cw in itertools.product(STRIDES, CHUNKS):
        start = sp.plan_windows(len(src), stride_frames=stride)
        assert start[-1] == (len(src) - S.N_FFT) // S.HOP + 1 - S.N_FRAMES
        seen = []
        for img, st in p.scan(src, start, chunk_windows=cw):
            assert img.shape == (len(st), 3, S.N_MEL, S.N_FRAMES) and img.dtype == torch.float32 and len(st) <= cw
            host = img.cpu()
            for k, s in enumerate(int(v) for v in st):
                seen.append(s)
                im = host[k]
                assert torch.equal(im[0], im[1]) and torch.equal(im[0], im[2])
                if s not in oracle:
                    oracle[s] = S.spectrogram_image(iq[None, s * S.HOP:s * S.HOP + S.N_SAMPLES])[0, 0]
                    first[s] = im[0].clone()
                err = (im[0] - oracle[s]).abs().max().item()
                worst = max(worst, err)
                assert err < 2e-3, (stride, cw, s, err)
                assert im.min().item() == 0.0 and abs(im.max().item() - 1.0) < 1e-6, (stride, cw, s)
                assert torch.equal(im[0], first[s]), f"window at frame {s} differs between (stride {stride}, chunk {cw}) and its first rendering"
        assert seen == start.tolist()
    print(f"windows checked at {len(oracle)} distinct starts, worst |image - oracle| = {worst:.3e}")


def test_window_minmax_is_the_exact_extreme_of_the_strip_rectangle():
    from sy11 import ops
    iq = R.capture(3.2).to(DEV)
    p = _producer()
    F = (iq.shape[0] - p.n_fft) // p.hop + 1
    db, _ = ops.stft_logmel(iq.view(1, -1), p.window, p.mel_start, p.mel_w, p.n_fft, p.hop, F, p.n_mel)
    start = torch.tensor([0, 1, 200, 200, 640, F - 640, 37], dtype=torch.int32, device=DEV)      # unordered and repeated starts are fine here
    img, mm = ops.stft_windows(db[0], start, p.n_frames)
    for k, s in enumerate(start.tolist()):
        rect = db[0, s:s + p.n_frames]
        assert mm[k, 0].item() == rect.amin().item() and mm[k, 1].item() == rect.amax().item()
        want = ops.stft_normalize(rect[None].contiguous(), mm[k:k + 1].contiguous())
        assert torch.equal(img[k], want[0])                    # the arithmetic of the per-image normalise kernel
    with pytest.raises(Exception):
        ops.stft_windows(db[0, :100], start[:1], p.n_frames)  # a strip shorter than one window is refused


# ------------------------------------------------------------------------------------------------------------- 3: merge
def _gpu_merge(window, boxes, score, cls, start, metric, thres, agnostic):
    from sy11 import ops
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)      # noqa: E731
    return ops.scan_merge(t(window), t(boxes), t(score), t(cls), torch.from_numpy(start), 640, metric=metric, thres=thres,
                          agnostic=agnostic).cpu().numpy()


def _merge_case(seed, W, stride, nc, metric, agnostic, first):
    thres = float(np.float32(0.5 if metric == "ios" else 0.45))
    window, boxes, score, cls, start = R.survivors(seed, W, stride, nc, metric, thres, agnostic, first_start=first)
    want = R.merge_ref(window, boxes, score, cls, start, 640, metric, thres, agnostic)
    got = _gpu_merge(window, boxes, score, cls, start, metric, thres, agnostic)
    assert got.dtype == bool and got.shape == want.shape
    assert np.array_equal(got, want), (int((got != want).sum()), len(want))
    return len(want), int(want.sum())


@pytest.mark.parametrize("first", [0, 3 * 10 ** 9])
@pytest.mark.parametrize("agnostic", [False, True])
@pytest.mark.parametrize("metric", ["ios", "iou"])
@pytest.mark.parametrize("nc", [1, 2, 8])
@pytest.mark.parametrize("stride", [160, 320, 640])
@pytest.mark.parametrize("W", [1, 2, 50])
def test_merge_equals_float64_reference(W, stride, nc, metric, agnostic, first):
    n, kept = _merge_case(100 + W, W, stride, nc, metric, agnostic, first)
    assert n > 0 and 0 < kept <= n


# 4 000 windows: every stride with both metrics; the class counts, class-aware / agnostic and the two first starts rotate through
# the six lists so that each of their values meets the long list at least twice (the full product is run at W <= 50 above).
_BIG = [(160, "ios", 8, False, 3 * 10 ** 9), (160, "iou", 1, True, 0), (320, "ios", 2, True, 0), (320, "iou", 8, False, 3 * 10 ** 9),
        (640, "ios", 1, False, 0), (640, "iou", 2, True, 3 * 10 ** 9)]


@pytest.mark.parametrize("stride,metric,nc,agnostic,first", _BIG)
def test_merge_equals_float64_reference_4000_windows(stride, metric, nc, agnostic, first):
    n, kept = _merge_case(4000, 4000, stride, nc, metric, agnostic, first)
    assert n > 20000 and 0 < kept < n


@pytest.mark.parametrize("first", [0, 3 * 10 ** 9])
def test_merge_hand_cases(first):
    one = lambda n: np.ones(n, np.int32)                     # noqa: E731
    st = first + np.array([0, 320, 640], dtype=np.int64)
    # a box and its edge-cut twin in the next window: IoS merges them (whichever scores higher stays), IoU does not
    w = np.array([0, 1], np.int32)
    b = np.array([[500, 100, 640, 200], [180, 100, 420, 200]], np.float32)            # strip 500..640 (cut) and 500..740 (whole)
    for s in (np.array([0.6, 0.9], np.float32), np.array([0.9, 0.6], np.float32)):
        for cls, metric, thres, agn in ((one(2), "ios", 0.5, False), (one(2), "iou", 0.7, False), (np.array([0, 1], np.int32), "ios", 0.5, False),
                                        (np.array([0, 1], np.int32), "ios", 0.5, True)):
            want = R.merge_ref(w, b, s, cls, st, 640, metric, thres, agn)
            assert np.array_equal(_gpu_merge(w, b, s, cls, st, metric, thres, agn), want)
    assert _gpu_merge(w, b, np.array([0.6, 0.9], np.float32), one(2), st, "ios", 0.5, False).tolist() == [False, True]
    assert _gpu_merge(w, b, np.array([0.6, 0.9], np.float32), one(2), st, "iou", 0.7, False).tolist() == [True, True]
    # a chain: A suppresses B, B would have suppressed C => C is kept
    w = np.array([0, 0, 1], np.int32)
    b = np.array([[300, 0, 400, 100], [350, 0, 450, 100], [80, 0, 180, 100]], np.float32)   # strip 300-400, 350-450, 400-500
    s = np.array([0.9, 0.8, 0.7], np.float32)
    assert _gpu_merge(w, b, s, one(3), st, "iou", 0.3, False).tolist() == [True, False, True]
    # a long alternating chain across many windows (one pass of the fixed point decides one link at a time)
    m = 41
    st_chain = first + 160 * np.arange(m, dtype=np.int64)
    w = np.arange(m, dtype=np.int32)
    b = np.tile(np.array([[100, 0, 360, 100]], np.float32), (m, 1))        # strip 160 k + 100 .. 160 k + 360: neighbours share 100 of 420
    s = np.linspace(0.9, 0.1, m).astype(np.float32)
    want = R.merge_ref(w, b, s, one(m), st_chain, 640, "iou", 0.2, False)
    assert want.tolist() == [k % 2 == 0 for k in range(m)]
    assert np.array_equal(_gpu_merge(w, b, s, one(m), st_chain, "iou", 0.2, False), want)
    # identical boxes in three overlapping windows: one survives, the best-scored (ties: the first row)
    w = np.array([0, 1, 2], np.int32)
    st3 = first + np.array([0, 160, 320], dtype=np.int64)
    b = np.array([[400.25, 50, 500.75, 90], [240.25, 50, 340.75, 90], [80.25, 50, 180.75, 90]], np.float32)
    for metric in ("ios", "iou"):
        assert _gpu_merge(w, b, np.array([0.5, 0.7, 0.6], np.float32), one(3), st3, metric, 0.5, False).tolist() == [False, True, False]
        assert _gpu_merge(w, b, np.array([0.5, 0.5, 0.5], np.float32), one(3), st3, metric, 0.5, False).tolist() == [True, False, False]
    # empty input
    e = _gpu_merge(np.zeros(0, np.int32), np.zeros((0, 4), np.float32), np.zeros(0, np.float32), np.zeros(0, np.int32), st, "ios", 0.5, False)
    assert e.shape == (0,) and e.dtype == bool


def test_merge_rejects_rows_that_are_not_grouped_by_window():
    from sy11 import _lib
    st = np.array([0, 320], dtype=np.int64)
    b = np.zeros((2, 4), np.float32)
    with pytest.raises(_lib.Sy11Error):
        _gpu_merge(np.array([1, 0], np.int32), b, np.ones(2, np.float32), np.zeros(2, np.int32), st, "ios", 0.5, False)
    with pytest.raises(_lib.Sy11Error):
        _gpu_merge(np.array([0, 2], np.int32), b, np.ones(2, np.float32), np.zeros(2, np.int32), st, "ios", 0.5, False)
    with pytest.raises(_lib.Sy11Error):
        _gpu_merge(np.array([0, 1], np.int32), b, np.ones(2, np.float32), np.zeros(2, np.int32), st[::-1].copy(), "ios", 0.5, False)


# ------------------------------------------------------------------------------------------------------------- 4: end to end
def test_scan_end_to_end_against_the_per_window_path(tmp_path):
    from oracle import stft_ref as S
    from sy11.data import spectrogram as sp
    from sy11.engine.model import YOLO
    from sy11.engine.predictor import DetectionPredictor, scan_boxes_to_tf
    iq = R.capture(6.3)
    fs, fc = 20e6, 2.4e9
    m, sd = _model(2)
    p = _producer()
    pred = DetectionPredictor(m, device=DEV, conf=0.05, iou=0.7, producer=p)
    # overlap 0, no merge: the rows of the existing path on the same windows, bit for bit after adding start[w]
    start = sp.plan_windows(len(iq), overlap=0.0)
    res = pred.scan(sp.open_iq(iq), fs, fc, overlap=0.0, batch=len(start), merge=None)
    assert res.start.tolist() == start.tolist() and len(res) > len(start), "the seeded model must give every window survivors"
    stacked = torch.stack([iq[s * S.HOP:s * S.HOP + S.N_SAMPLES] for s in start.tolist()])
    old = pred(stacked)
    assert len(old) == len(start)
    for w, r in enumerate(old):
        rows = res.boxes[res.window == w]
        want = r.boxes.data.cpu().to(torch.float64)
        want[:, [0, 2]] += float(start[w])
        assert len(rows) > 0 and torch.equal(rows, want), w
    assert res.boxes.dtype == torch.float64 and res.tf.dtype == torch.float64 and res.window.dtype == torch.int64
    # overlap 0.5 with the IoS merge: the reference merge of the unmerged rows; tf = the host maps of the boxes; repeatable
    raw = pred.scan(sp.open_iq(iq), fs, fc, overlap=0.5, batch=4, merge=None)
    out = pred.scan(sp.open_iq(iq), fs, fc, overlap=0.5, batch=4, merge="ios")
    again = pred.scan(sp.open_iq(iq), fs, fc, overlap=0.5, batch=4, merge="ios")
    local = raw.boxes[:, :4].clone()
    off = torch.from_numpy(raw.start)[raw.window].to(torch.float64)
    local[:, 0] -= off
    local[:, 2] -= off
    keep = R.merge_ref(raw.window.numpy(), local.numpy().astype(np.float32), raw.boxes[:, 4].numpy().astype(np.float32),
                       raw.boxes[:, 5].numpy().astype(np.int32), raw.start, 640, "ios", 0.5, False)
    assert 0 < keep.sum() < len(raw), "the seams of a 50 % overlap scan must produce duplicates to merge"
    assert torch.equal(out.boxes, raw.boxes[torch.from_numpy(keep)]) and torch.equal(out.window, raw.window[torch.from_numpy(keep)])
    for a, b in ((out.boxes, again.boxes), (out.window, again.window), (out.tf, again.tf)):
        assert torch.equal(a, b)
    assert torch.equal(out.tf, scan_boxes_to_tf(out.boxes, fs, fc, p))
    bx = out.boxes.numpy()
    assert np.array_equal(out.tf[:, 0].numpy(), sp.cols_to_time(bx[:, 0] - 0.5, fs)) and np.array_equal(out.tf[:, 3].numpy(), sp.rows_to_freq(bx[:, 3] - 0.5, fs, fc))
    assert (out.tf[:, 2] > out.tf[:, 0]).all() and (out.tf[:, 3] > out.tf[:, 1]).all()
    assert out.names == m.names and out.sample_rate == fs and out.center_freq == fc and len(out) == out.boxes.shape[0]
    # the front door, from a tensor and from a raw file
    y = YOLO("yolo11n.yaml", nc=2, device=DEV)
    y.model.load_state_dict(sd)
    a = y.scan(iq, fs, fc, conf=0.05, overlap=0.5, batch=4)
    iq.numpy().view(np.float32).tofile(tmp_path / "capture.cf32")
    b = y.scan(str(tmp_path / "capture.cf32"), fs, fc, conf=0.05, overlap=0.5, batch=4)
    assert len(a) > 0 and torch.equal(a.boxes, b.boxes) and torch.equal(a.window, b.window) and torch.equal(a.tf, b.tf)
    assert torch.equal(a.boxes, out.boxes)


# ------------------------------------------------------------------------------------------------------------- 5: ragged tail, big offsets
def test_scan_ragged_last_chunk_uses_a_second_signature():
    from oracle import stft_ref as S
    from sy11.data import spectrogram as sp
    from sy11.engine.predictor import DetectionPredictor
    n = S.N_FFT + (65 * S.N_FRAMES - 1) * S.HOP                         # exactly 64 + 1 windows at overlap 0
    g = torch.Generator().manual_seed(3)
    iq = torch.view_as_complex(torch.randn(n, 2, generator=g) * 0.1)
    iq[n // 3:n // 2] += torch.exp(2j * torch.pi * 0.1 * torch.arange(n // 2 - n // 3)).to(torch.complex64)
    m, _ = _model(2)
    pred = DetectionPredictor(m, device=DEV, conf=0.05, iou=0.7, producer=_producer())
    res = pred.scan(sp.open_iq(iq), 1e6, overlap=0.0, batch=64, merge="ios")
    assert res.start.tolist() == [640 * k for k in range(65)]
    shapes = {k[0][0][0][0] for k in m.__dict__["_sy11_graph_cfg"]["seen"]}
    assert shapes == {64, 1}, shapes
    assert len(res) > 0 and int(res.window.min()) >= 0 and int(res.window.max()) <= 64
    last = res.boxes[res.window == 64]
    assert ((last[:, 0] >= 64 * 640) & (last[:, 2] <= 65 * 640)).all()


class _Periodic:
    """A capture of 10^12 samples that repeats a base block: only the slices a scan asks for ever exist."""

    def __init__(self, base, n):
        self.base, self.n = base, n

    def __len__(self):
        return self.n

    def __getitem__(self, sl):
        idx = np.arange(sl.start, min(sl.stop, self.n), dtype=np.int64) % self.base.shape[0]
        return self.base[idx]


def test_scan_at_a_start_of_three_billion_frames():
    from oracle import stft_ref as S
    big = 3 * 10 ** 9
    base = R.capture(2.2).numpy()
    period = (base.shape[0] // S.HOP) * S.HOP                            # a whole number of frames, so frame k + period/hop == frame k
    base = base[:period]
    far = _Periodic(base, (big + 2000) * S.HOP)
    p = _producer()
    start = big + np.array([0, 320, 640, 700], dtype=np.int64)
    got = [(img.cpu(), st) for img, st in p.scan(far, start, chunk_windows=3)]
    assert np.concatenate([st for _, st in got]).tolist() == start.tolist()
    shift = (big * S.HOP) % period                                        # the same samples, read near the origin of a plain array
    near = np.concatenate([base, base, base, base])[shift:shift + (700 + 640) * S.HOP + S.N_FFT]
    want = [img.cpu() for img, _ in p.scan(near, start - big, chunk_windows=3)]
    for (a, _), b in zip(got, want):
        assert torch.equal(a, b)
