"""GPU: linking a scan's rows into tracks (sy11_scan_link).  Every comparison is exact: the relation is subtract / min / max / one multiply /
compare in float64 on both sides, and the labels are integers.  Hand cases on the thresholds and the launch geometry, pass counts that
tell hook-and-compress from neighbour propagation, random survivor lists against the union-find reference of tests/_link_ref.py,
independence of the row order, the table of tracks, the scan's ``link=`` keyword end to end, and ``extract`` on tracks."""
import functools

import numpy as np
import pytest
import torch

from tests import _link_ref as L
from tests import _scan_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
HOP_S = 256 / 20e6
GAP = 8 * HOP_S


def _gpu(tf, cls, gap_t, gap_f=None, align=0.5, agnostic=False):
    from sy11 import ops
    tf = np.ascontiguousarray(tf, dtype=np.float64).reshape(-1, 4)
    lab, passes = ops.scan_link(torch.from_numpy(tf).to(DEV), torch.from_numpy(np.asarray(cls, dtype=np.int64)).to(DEV), gap_t, gap_f, align,
                                agnostic, return_passes=True)
    assert lab.dtype == torch.int64 and lab.shape == (tf.shape[0],)
    return lab.cpu().numpy(), passes


def _both(tf, cls, gap_t, gap_f=None, align=0.5, agnostic=False):
    got, _ = _gpu(tf, cls, gap_t, gap_f, align, agnostic)
    assert np.array_equal(got, L.link_ref(tf, cls, gap_t, gap_f, align, agnostic))
    return got.tolist()


def _results(tf, conf, cls, fs=20e6, fc=2.4e9, channelizer=None):
    from sy11.engine.predictor import ScanResults
    n = len(tf)
    boxes = torch.zeros((n, 6), dtype=torch.float64)
    boxes[:, 4], boxes[:, 5] = torch.as_tensor(np.asarray(conf, dtype=np.float64)), torch.as_tensor(np.asarray(cls, dtype=np.float64))
    return ScanResults(boxes, torch.zeros(n, dtype=torch.int64), torch.as_tensor(np.asarray(tf, dtype=np.float64).reshape(-1, 4)),
                       {0: "class_0", 1: "class_1"}, np.zeros(1, np.int64), fs, fc, None, None, channelizer)


def _same_table(t, ref):
    for name in ("track", "tf", "conf", "cls", "count", "first_row"):
        assert np.array_equal(getattr(t, name).numpy(), ref[name]), name
    assert (t.tf.numpy() == ref["tf"]).all() and len(t) == len(ref["rows"])


# ------------------------------------------------------------------------------------------------------------- hand cases
def test_pieces_of_one_carrier_and_classes():
    a = [100 * HOP_S, 2.40e9, 640 * HOP_S, 2.41e9]                                                # cut by the end of window 0
    b = [320 * HOP_S, 2.40e9, 960 * HOP_S, 2.41e9]                                                # the same carrier in the window at stride 320
    tf = np.array([a, b])
    assert _both(tf, [0, 0], GAP) == [0, 0]
    assert _both(tf, [0, 1], GAP) == [0, 1]
    assert _both(tf, [0, 1], GAP, agnostic=True) == [0, 0]
    assert _both(tf[::-1], [0, 0], GAP) == [0, 0]
    # a third piece two windows on, an emission elsewhere in frequency, one far later
    tf = np.array([a, b, [960 * HOP_S, 2.40e9, 1600 * HOP_S, 2.41e9], [100 * HOP_S, 2.43e9, 900 * HOP_S, 2.44e9],
                   [5000 * HOP_S, 2.40e9, 5100 * HOP_S, 2.41e9]])
    assert _both(tf, np.zeros(5), GAP) == [0, 0, 0, 3, 4]
    assert _both(tf[[4, 3, 2, 1, 0]], np.zeros(5), GAP) == [0, 1, 2, 2, 2]


def test_thresholds_are_met_exactly_and_missed_by_one_ulp():
    up = lambda v: float(np.nextafter(v, np.inf))             # noqa: E731
    # a gap of exactly gap_t in time (the pair also sits on the very edge of the candidate range)
    a = [0.0, 0.0, 1.0, 10.0]
    assert _both([a, [1.25, 0.0, 2.0, 10.0]], [0, 0], 0.25) == [0, 0]
    assert _both([a, [up(1.25), 0.0, 2.0, 10.0]], [0, 0], 0.25) == [0, 1]
    assert _both([a, [1.0, 0.0, 2.0, 10.0]], [0, 0], 0.0) == [0, 0]
    assert _both([a, [up(1.0), 0.0, 2.0, 10.0]], [0, 0], 0.0) == [0, 1]
    big = 38400.0                                             # seconds: a start of three billion frames
    assert _both([[big, 0.0, big + 1.0, 10.0], [big + 1.25, 0.0, big + 2.0, 10.0]], [0, 0], 0.25) == [0, 0]
    assert _both([[big, 0.0, big + 1.0, 10.0], [up(big + 1.25), 0.0, big + 2.0, 10.0]], [0, 0], 0.25) == [0, 1]
    # ov_f of exactly align * min(bw)
    a = [0.0, 0.0, 1.0, 8.0]
    assert _both([a, [0.5, 4.0, 1.5, 20.0]], [0, 0], 0.0) == [0, 0]
    assert _both([a, [0.5, up(4.0), 1.5, 20.0]], [0, 0], 0.0) == [0, 1]
    assert _both([a, [0.5, 6.0, 1.5, 20.0]], [0, 0], 0.0, align=0.25) == [0, 0]
    assert _both([a, [0.5, up(6.0), 1.5, 20.0]], [0, 0], 0.0, align=0.25) == [0, 1]
    a = [0.0, 4.0, 1.0, 6.0]                                  # align = 1: the narrower band lies inside the other, or shifted by one ulp
    assert _both([a, [0.5, 4.0, 1.5, 6.0]], [0, 0], 0.0, align=1.0) == [0, 0]
    assert _both([a, [0.5, up(4.0), 1.5, up(6.0)]], [0, 0], 0.0, align=1.0) == [0, 1]
    # the frequency branch: a gap of exactly gap_f, and ov_t of exactly align * min(dur)
    a = [0.0, 0.0, 1.0, 1.0]
    assert _both([a, [0.0, 1.25, 1.0, 3.0]], [0, 0], 0.0, gap_f=0.25) == [0, 0]
    assert _both([a, [0.0, up(1.25), 1.0, 3.0]], [0, 0], 0.0, gap_f=0.25) == [0, 1]
    a = [0.0, 0.0, 8.0, 1.0]
    assert _both([a, [4.0, 1.0, 20.0, 2.0]], [0, 0], 0.0, gap_f=0.0) == [0, 0]
    assert _both([a, [up(4.0), 1.0, 20.0, 2.0]], [0, 0], 0.0, gap_f=0.0) == [0, 1]


def test_gap_f_none_leaves_frequency_neighbours_apart():
    lo = [100 * HOP_S, 2.40e9, 640 * HOP_S, 2.41e9]
    hi = [120 * HOP_S, 2.41e9, 600 * HOP_S, 2.42e9]                                               # the next band up, touching in Hz
    assert _both([lo, hi], [0, 0], GAP) == [0, 1]
    assert _both([lo, hi], [0, 0], GAP, gap_f=0.0) == [0, 0]
    assert _both([lo, hi], [0, 1], GAP, gap_f=0.0) == [0, 1]
    assert _both([lo, hi], [0, 1], GAP, gap_f=0.0, agnostic=True) == [0, 0]


@pytest.mark.parametrize("n", [1, 4, 5, 9])
def test_rows_per_workgroup(n):
    chain = np.array([[k, 0.0, k + 1.0, 1.0] for k in range(n)], dtype=np.float64)                # neighbours touch
    assert _both(chain, np.zeros(n), 0.0) == [0] * n
    assert _both(chain[::-1], np.zeros(n), 0.0) == [0] * n
    assert _both(chain, np.arange(n) % 2, 0.0, agnostic=True) == [0] * n
    apart = chain.copy()
    apart[:, 2] -= 0.5
    assert _both(apart, np.zeros(n), 0.25) == list(range(n))
    assert _both(chain, np.arange(n), 0.0) == list(range(n))                                      # every row a class of its own


@pytest.mark.parametrize("m", [1, 63, 64, 65, 129])
def test_the_last_candidate_of_a_row_is_tested(m):
    """Row 0 has exactly m candidates; only the last of them is linked to it (its lane: (m - 1) % 64)."""
    rows = [[0.0, 0.0, 1000.0, 1.0]]
    for k in range(1, m + 1):
        rows.append([float(k), 10.0 * k, k + 0.5, 10.0 * k + 1.0])                                # inside row 0's span, elsewhere in frequency
    rows[m][1:4:2] = [0.25, 1.25]
    rows.append([2000.0, 0.0, 2001.0, 1.0])                                                       # beyond the range
    want = list(range(m + 2))
    want[m] = 0
    assert _both(rows, np.zeros(m + 2), 0.0) == want


# ------------------------------------------------------------------------------------------------------------- pass counts
def test_a_chain_and_a_bridge_converge_in_few_passes():
    """passes < n / 8 is a condition, not a measurement: hooking roots needs a handful of passes on either list, propagating the
    smallest neighbour label about 2 000 on the bridge.  The count is reported per batch of two passes (measured on an MI355X: the
    chain 2, the bridge 4)."""
    n = 4000
    chain = np.array([[k, 0.0, k + 1.0, 1.0] for k in range(n)], dtype=np.float64)
    got, passes = _gpu(chain, np.zeros(n), 0.0)
    print(f"scan_link: chain of {n} rows: {passes} passes")
    assert (got == 0).all() and 0 < passes < n / 8
    perm = np.random.default_rng(0).permutation(n)
    got, p2 = _gpu(chain[perm], np.zeros(n), 0.0)
    assert (got == 0).all() and 0 < p2 < n / 8
    half = 2000
    low = [[k, 0.0, k + 1.0, 1.0] for k in range(half)]
    high = [[k, 10.0, k + 1.0, 11.0] for k in range(half)]
    apart = np.array([r for pair in zip(low, high) for r in pair], dtype=np.float64)
    got, _ = _gpu(apart, np.zeros(2 * half), 0.0)
    assert np.array_equal(got, np.arange(2 * half) % 2)                                           # two tracks without the bridge
    bridge = np.concatenate((apart, [[half - 0.5, 0.0, half + 1.0, 11.0]]))                       # meets only the last row of each chain
    got, passes = _gpu(bridge, np.zeros(2 * half + 1), 0.0)
    print(f"scan_link: bridge over two chains of {half} rows: {passes} passes")
    assert (got == 0).all() and 0 < passes < (2 * half + 1) / 8
    assert np.array_equal(L.link_ref(bridge, np.zeros(2 * half + 1), 0.0), got)


# ------------------------------------------------------------------------------------------------------------- random lists
@functools.lru_cache(maxsize=None)
def _survivors(W, stride, nc, first):
    window, boxes, score, cls, start = R.survivors(100 + W if W < 4000 else 4000, W, stride, nc, "ios", 0.5, False, first_start=first)
    return L.survivor_tf(window, boxes, start), score.astype(np.float64), cls.astype(np.int64)


@functools.lru_cache(maxsize=None)
def _ref_labels(W, stride, nc, first, agnostic, gap_f):
    tf, _, cls = _survivors(W, stride, nc, first)
    return L.link_ref(tf, cls, GAP, gap_f, 0.5, agnostic)


def _random_case(W, stride, nc, first, agnostic, gap_f):
    from sy11.data.link import link_results
    tf, conf, cls = _survivors(W, stride, nc, first)
    want = _ref_labels(W, stride, nc, first, agnostic, gap_f)
    got, passes = _gpu(tf, cls, GAP, gap_f, 0.5, agnostic)
    n, T = len(want), np.unique(want).size
    assert np.array_equal(got, want), (int((got != want).sum()), n)
    assert 1 <= T < n, (T, n)
    tracks = link_results(_results(tf, conf, cls), DEV, gap_t=GAP, gap_f=gap_f, agnostic=agnostic)
    _same_table(tracks, L.tracks_ref(tf, conf, cls, want))
    assert all(np.array_equal(tracks.rows(k).numpy(), np.flatnonzero(tracks.track.numpy() == k)) for k in range(0, T, max(T // 7, 1)))
    return n, T, passes


@pytest.mark.parametrize("first", [0, 3 * 10 ** 9])
@pytest.mark.parametrize("gap_f", [None, 0.0])
@pytest.mark.parametrize("agnostic", [False, True])
@pytest.mark.parametrize("nc", [1, 8])
@pytest.mark.parametrize("stride", [160, 320, 640])
@pytest.mark.parametrize("W", [1, 2, 50])
def test_link_equals_float64_reference(W, stride, nc, agnostic, gap_f, first):
    _random_case(W, stride, nc, first, agnostic, gap_f)


def test_link_equals_float64_reference_4000_windows():
    n, T, passes = _random_case(4000, 320, 8, 3 * 10 ** 9, False, None)
    print(f"scan_link: {n} rows of 4 000 windows -> {T} tracks in {passes} passes")
    assert n > 20000


@pytest.mark.parametrize("gap_f", [None, 0.0])
def test_the_row_order_does_not_matter(gap_f):
    from sy11.data.link import link_results
    tf, conf, cls = _survivors(50, 320, 8, 0)
    base = link_results(_results(tf, conf, cls), DEV, gap_t=GAP, gap_f=gap_f)
    perm = np.random.default_rng(1).permutation(len(tf))                                          # row k of the permuted list is row perm[k]
    other = link_results(_results(tf[perm], conf[perm], cls[perm]), DEV, gap_t=GAP, gap_f=gap_f)
    a, b = base.track.numpy()[perm], other.track.numpy()
    pairs = np.unique(np.stack((a, b), 1), axis=0)
    assert len(pairs) == len(base) == len(other)                                                  # one partition, two numberings
    _same_table(other, L.tracks_ref(tf[perm], conf[perm], cls[perm], a))                          # equal once numbered by first row


# ------------------------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def scanner():
    from sy11.data import spectrogram as sp
    from sy11.engine.predictor import DetectionPredictor
    from tests.test_scan_gpu import _model
    m, _ = _model(2)
    return DetectionPredictor(m, device=DEV, conf=0.05, iou=0.7, producer=sp.SpectrogramProducer(DEV)), R.capture(6.3)


def _same_results(a, b):
    for name in ("boxes", "window", "tf"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name


@pytest.mark.parametrize("kind", ["plain", "channels"])
def test_scan_with_the_link_keyword(scanner, kind):
    from sy11.data import spectrogram as sp
    pred, iq = scanner
    fs, fc = (20e6, 2.4e9) if kind == "plain" else (40e6, 2.4e9)
    kw = dict(overlap=0.5, batch=4) if kind == "plain" else dict(overlap=0.5, batch=4, channels=4)
    plain = pred.scan(sp.open_iq(iq), fs, fc, **kw)
    also = pred.scan(sp.open_iq(iq), fs, fc, link=None, **kw)
    linked = pred.scan(sp.open_iq(iq), fs, fc, link=True, **kw)
    loose = pred.scan(sp.open_iq(iq), fs, fc, link={"gap_t": 1e-3, "agnostic": True}, **kw)
    assert len(plain) > 0 and plain.track is None and plain.tracks is None and also.track is None and also.tracks is None
    for other in (also, linked, loose):
        _same_results(plain, other)                                                               # linking never touches the rows
    assert plain.hop == 256 and (plain.channelizer is None) == (kind == "plain")
    again = pred.link(plain)
    assert again is plain and torch.equal(plain.track, linked.track) and plain.track.dtype == torch.int64
    for name in ("track", "tf", "conf", "cls", "count", "first_row"):
        assert torch.equal(getattr(plain.tracks, name), getattr(linked.tracks, name)), name
    p = linked.tracks.plan
    assert p.gap_t == 8 * 256 / 20e6 and p.gap_f == (None if kind == "plain" else 0.0) and linked.tracks.names == plain.names
    tf, conf, cls = plain.tf.numpy(), plain.boxes[:, 4].numpy(), plain.boxes[:, 5].numpy().astype(np.int64)
    _same_table(linked.tracks, L.tracks_ref(tf, conf, cls, L.link_ref(tf, cls, p.gap_t, p.gap_f, 0.5, False)))
    _same_table(loose.tracks, L.tracks_ref(tf, conf, cls, L.link_ref(tf, cls, 1e-3, p.gap_f, 0.5, True)))
    assert 1 <= len(loose.tracks) <= len(linked.tracks) <= len(plain)
    print(f"scan(link=True) [{kind}]: {len(plain)} rows -> {len(linked.tracks)} tracks ({len(loose.tracks)} with gap_t = 1 ms, agnostic)")


def test_extract_on_tracks_cuts_one_clip_per_emission(scanner):
    pred, _ = scanner
    fs, fc, n = 1.0e6, 2.4e9, 40000
    g = np.random.default_rng(3)
    iq = torch.from_numpy((g.standard_normal(n) + 1j * g.standard_normal(n)).astype(np.complex64))
    pieces = np.array([(0.0100, 0.85e5, 0.0160, 1.15e5), (0.0300, -2.25e5, 0.0340, -1.50e5), (0.0160, 0.86e5, 0.0220, 1.16e5),
                       (0.0300, -1.50e5, 0.0340, -0.75e5), (0.0225, 0.85e5, 0.0280, 1.14e5), (0.0340, -2.25e5, 0.0360, -0.75e5)])
    pieces[:, [1, 3]] += fc
    res = _results(pieces, [0.5, 0.6, 0.9, 0.7, 0.4, 0.3], [0, 1, 0, 1, 0, 1], fs, fc)
    assert pred.link(res, gap_t=1e-3, gap_f=0.0) is res
    assert res.track.tolist() == [0, 1, 0, 1, 0, 1] and len(res.tracks) == 2
    union = np.array([(0.0100, fc + 0.85e5, 0.0280, fc + 1.16e5), (0.0300, fc - 2.25e5, 0.0360, fc - 0.75e5)])
    assert (res.tracks.tf.numpy() == union).all() and res.tracks.conf.tolist() == [0.9, 0.7] and res.tracks.cls.tolist() == [0, 1]
    from sy11.data import spectrogram as sp
    got = pred.extract(sp.open_iq(iq), res.tracks, fs, fc)
    want = pred.extract(sp.open_iq(iq), _results(union, [0.9, 0.7], [0, 1], fs, fc), fs, fc)
    each = pred.extract(sp.open_iq(iq), res, fs, fc)
    assert len(got) == 2 and len(each) == 6
    assert torch.equal(torch.view_as_real(got.packed).view(torch.int32), torch.view_as_real(want.packed).view(torch.int32))
    assert got.plan.M.tolist() == want.plan.M.tolist() and got.decimation.tolist() == want.decimation.tolist()
    assert got.cls.tolist() == [0, 1] and got.conf.tolist() == [0.9, 0.7] and got.names == res.names


def test_wrapper_errors():
    from sy11 import _lib, ops
    tf = torch.tensor([[0.0, 0.0, 1.0, 1.0], [0.5, 0.0, 2.0, 1.0]], dtype=torch.float64, device=DEV)
    cls = torch.zeros(2, dtype=torch.int64, device=DEV)
    bad_tf = tf.clone()
    bad_tf[1, 2] = float("nan")
    inverted = tf.clone()
    inverted[1, 2] = 0.25
    for args in ((tf.float(), cls, 0.0), (tf[:, :3], cls, 0.0), (tf, cls[:1], 0.0), (tf, cls.double(), 0.0), (bad_tf, cls, 0.0), (inverted, cls, 0.0),
                 (tf, cls, -1.0), (tf, cls, float("nan")), (tf, cls, 0.0, -1.0), (tf, cls, 0.0, None, 0.0), (tf, cls, 0.0, None, 1.5)):
        with pytest.raises(_lib.Sy11Error):
            ops.scan_link(*args)
    empty = ops.scan_link(tf[:0], cls[:0], 0.0)
    assert empty.shape == (0,) and empty.dtype == torch.int64
    assert ops.scan_link(tf, cls.to(torch.int32), 0.0).tolist() == [0, 0]
