"""CPU: linking a scan's rows into tracks — the C entries' argument checks (no launch), the host plan and its defaults, the float64
reference of tests/_link_ref.py against all pairs, the table of tracks from given labels, and the front door."""
import json
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import _link_ref as L
from tests import _scan_ref as R

ROOT = Path(__file__).resolve().parents[1]


def _results(tf, conf=None, cls=None, fs=20e6, fc=2.4e9, resample=None, channel=None, channelizer=None):
    """A hand-built ScanResults the way every scan builds one."""
    from sy11.engine.predictor import ScanResults
    tf = torch.as_tensor(np.asarray(tf, dtype=np.float64).reshape(-1, 4))
    n = tf.shape[0]
    boxes = torch.zeros((n, 6), dtype=torch.float64)
    boxes[:, 4] = torch.as_tensor(np.full(n, 0.5) if conf is None else np.asarray(conf, dtype=np.float64))
    boxes[:, 5] = torch.as_tensor(np.zeros(n) if cls is None else np.asarray(cls, dtype=np.float64))
    return ScanResults(boxes, torch.zeros(n, dtype=torch.int64), tf, {0: "a", 1: "b"}, np.zeros(1, np.int64), fs, fc, resample, channel,
                       channelizer)


# ------------------------------------------------------------------------------------------------------------- the C entries
def test_link_entries_are_declared_bound_and_exported():
    from sy11 import _lib
    header = (ROOT / "include" / "sy11.h").read_text()
    lib = _lib.load()
    table = {**_lib.SIGNATURES, **{k: v[0] for k, v in _lib.OTHER.items()}}
    for name in ("sy11_scan_link", "sy11_scan_link_workspace_bytes"):
        m = re.search(rf"\b{name}\s*\(([^;]*?)\)\s*;", header, re.S)
        assert m, f"{name} is not declared in include/sy11.h"
        assert name in table and hasattr(lib, name)
        assert len([p for p in m.group(1).split(",") if p.strip()]) == len(table[name])


def test_link_entry_checks_its_arguments_before_any_launch():
    from sy11 import _lib
    lib = _lib.load()
    link = lib.sy11_scan_link
    assert link(0, None, None, 1e-4, 0.0, 0, 0.5, 0, None, None, None, None) == 0                 # empty input: no pointer is touched
    assert link(-1, None, None, 1e-4, 0.0, 0, 0.5, 0, None, None, None, None) == -1
    for align in (0.0, -0.5, 1.0000001, float("nan"), float("inf")):
        assert link(5, None, None, 1e-4, 0.0, 0, align, 0, None, None, None, None) == -1 and b"align" in lib.sy11_last_error(), align
    for gap in (-1e-9, float("nan"), float("inf")):
        assert link(5, None, None, gap, 0.0, 0, 0.5, 0, None, None, None, None) == -1 and b"gap_t" in lib.sy11_last_error(), gap
        assert link(5, None, None, 1e-4, gap, 1, 0.5, 0, None, None, None, None) == -1 and b"gap_f" in lib.sy11_last_error(), gap
    assert link(5, None, None, 1e-4, -1.0, 0, 1.0, 0, None, None, None, None) == -1 and b"null pointer" in lib.sy11_last_error()   # gap_f unused
    assert link(5, None, None, 0.0, 0.0, 1, 0.5, 1, None, None, None, None) == -1 and b"null pointer" in lib.sy11_last_error()
    assert lib.sy11_scan_link_workspace_bytes(0) == 0 and lib.sy11_scan_link_workspace_bytes(-3) == 0
    small, big = lib.sy11_scan_link_workspace_bytes(1000), lib.sy11_scan_link_workspace_bytes(2000)
    assert 4 * 1000 <= small < big <= small + 4 * 1000 + 64                                       # O(n): no pair matrix, no edge list


def test_ops_scan_link_has_no_cpu_path():
    from sy11 import _lib, ops
    with pytest.raises(_lib.Sy11Error):
        ops.scan_link(torch.zeros((2, 4), dtype=torch.float64), torch.zeros(2, dtype=torch.int64), 1e-4)


# ------------------------------------------------------------------------------------------------------------- the plan
def test_plan_link_defaults():
    from sy11.data.channelize import plan_channels
    from sy11.data.link import plan_link
    from sy11.data.resample import plan_resample
    tf = [[0.0, 1.0, 1.0, 2.0]]
    p = plan_link(_results(tf, fs=20e6))
    assert p.gap_t == 8 * 256 / 20e6 and p.gap_f is None and p.align == 0.5 and p.agnostic is False
    r = _results(tf, fs=5e6, resample=plan_resample(20e6, 5e6, 0.0))                           # resampled: the DDC's output rate counts
    assert plan_link(r).gap_t == 8 * 256 / 5e6 and plan_link(r).gap_f is None
    r.hop = 128                                                                                   # what scan records
    assert plan_link(r).gap_t == 8 * 128 / 5e6 and plan_link(r, hop=512).gap_t == 8 * 512 / 5e6
    for oversample, want in ((2, 0.0), (1, None)):
        ch = plan_channels(80e6, 8, oversample)
        r = _results(tf, fs=ch.fs_out, channel=torch.zeros(1, dtype=torch.int64), channelizer=ch)
        p = plan_link(r)
        assert p.gap_t == 8 * 256 / ch.fs_out and p.gap_f == want and (want is None or isinstance(p.gap_f, float))
        assert plan_link(r, gap_f=None).gap_f is None and plan_link(r, gap_f=2.5e3).gap_f == 2.5e3
    p = plan_link(_results(tf), gap_t=0, gap_f=0, align=1, agnostic=True)                         # a gap_f is allowed for any scan
    assert (p.gap_t, p.gap_f, p.align, p.agnostic) == (0.0, 0.0, 1.0, True)
    assert plan_link(_results(np.zeros((0, 4)))).gap_t == 8 * 256 / 20e6                          # an empty result plans too


@pytest.mark.parametrize("kw", [dict(gap_t=-1e-9), dict(gap_t=float("nan")), dict(gap_t=float("inf")), dict(gap_t=None), dict(gap_t="hops"),
                                dict(gap_f=-1.0), dict(gap_f=float("nan")), dict(gap_f="band"), dict(align=0.0), dict(align=-0.1),
                                dict(align=1.5), dict(align=float("nan")), dict(align=None), dict(hop=0), dict(hop=2.5)])
def test_plan_link_argument_errors(kw):
    from sy11.data.link import plan_link
    with pytest.raises(ValueError):
        plan_link(_results([[0.0, 1.0, 1.0, 2.0]]), **kw)


@pytest.mark.parametrize("bad", [[0.0, 1.0, float("nan"), 2.0], [0.0, float("inf"), 1.0, 2.0], [1.0, 1.0, 0.5, 2.0], [0.0, 3.0, 1.0, 2.0]])
def test_plan_link_refuses_non_finite_and_inverted_rectangles(bad):
    from sy11.data.link import link_results, plan_link
    r = _results([[0.0, 1.0, 1.0, 2.0], bad])
    with pytest.raises(ValueError, match="row 1"):
        plan_link(r)
    with pytest.raises(ValueError, match="row 1"):
        link_results(r, "cuda")                                                                   # raised before anything touches the device


# ------------------------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("gap_f", [None, 0.0, 0.5])
@pytest.mark.parametrize("agnostic", [False, True])
@pytest.mark.parametrize("seed,n,nc", [(0, 300, 1), (1, 300, 3), (2, 257, 8), (3, 2, 1), (4, 1, 1)])
def test_sweep_reference_equals_all_pairs(seed, n, nc, agnostic, gap_f):
    g = np.random.default_rng(seed)
    t0, f0 = g.uniform(0, 1.0, n), g.uniform(0, 100.0, n)
    tf = np.stack((t0, f0, t0 + g.uniform(0, 0.03, n), f0 + g.uniform(0, 6.0, n)), 1)
    tf[::7, 2] = tf[::7, 0]                                                                       # zero-length rows
    tf[::11, 0] = tf[0, 0]                                                                        # ties in t0
    tf[::11, 2] = np.maximum(tf[::11, 2], tf[0, 0])
    cls = g.integers(0, nc, n)
    for gap_t in (0.0, 0.004):
        want = L.link_brute(tf, cls, gap_t, gap_f, 0.5, agnostic)
        got = L.link_ref(tf, cls, gap_t, gap_f, 0.5, agnostic)
        assert np.array_equal(got, want)
        assert (got <= np.arange(n)).all() and np.array_equal(got[got], got)                      # a label is its component's first row
        if n >= 257:
            assert 1 < np.unique(got).size < n


def test_reference_hand_cases():
    hop_s = 256 / 20e6
    a = [100 * hop_s, 2.40e9, 640 * hop_s, 2.41e9]                                                # cut by the end of window 0
    b = [320 * hop_s, 2.40e9, 960 * hop_s, 2.41e9]                                                # the same carrier in the window at stride 320
    far = [2000 * hop_s, 2.40e9, 2100 * hop_s, 2.41e9]
    up = [100 * hop_s, 2.41e9, 640 * hop_s, 2.42e9]                                               # the neighbouring band, touching in Hz
    tf = np.array([a, b, far, up])
    z = np.zeros(4, np.int64)
    assert L.link_ref(tf, z, 8 * hop_s).tolist() == [0, 0, 2, 3]
    assert L.link_ref(tf, [0, 1, 0, 0], 8 * hop_s).tolist() == [0, 1, 2, 3]
    assert L.link_ref(tf, [0, 1, 0, 0], 8 * hop_s, agnostic=True).tolist() == [0, 0, 2, 3]
    assert L.link_ref(tf, z, 8 * hop_s, gap_f=0.0).tolist() == [0, 0, 2, 0]
    assert L.link_ref(tf, z, 1360 * hop_s).tolist() == [0, 0, 0, 3]                               # far starts 1040 hops after b ends
    assert L.link_ref(tf[::-1], z, 8 * hop_s, gap_f=0.0).tolist() == [0, 1, 0, 0]                 # labels follow the caller's row order


# ------------------------------------------------------------------------------------------------------------- the table
def test_tracks_table_from_given_labels():
    from sy11.data.link import build_tracks
    tf = np.array([[5.0, 10.0, 6.0, 20.0], [0.0, 1.0, 1.0, 2.0], [5.5, 12.0, 7.0, 25.0], [1.0, 0.5, 1.5, 1.5], [9.0, 9.0, 9.0, 9.0],
                   [4.0, 15.0, 5.0, 18.0]])
    conf = np.array([0.3, 0.9, 0.7, 0.9, 0.1, 0.7])
    cls = np.array([1, 0, 2, 3, 4, 5])
    label = np.array([0, 1, 0, 1, 4, 0])
    t = build_tracks(torch.from_numpy(tf), torch.from_numpy(conf), torch.from_numpy(cls), torch.from_numpy(label), {0: "a"})
    assert len(t) == 3 and t.track.tolist() == [0, 1, 0, 1, 2, 0]
    assert t.tf.tolist() == [[4.0, 10.0, 7.0, 25.0], [0.0, 0.5, 1.5, 2.0], [9.0, 9.0, 9.0, 9.0]]
    assert t.conf.tolist() == [0.7, 0.9, 0.1] and t.cls.tolist() == [2, 0, 4]                     # ties in conf: the lowest row's class
    assert t.count.tolist() == [3, 2, 1] and t.first_row.tolist() == [0, 1, 4]
    assert [t.rows(k).tolist() for k in range(3)] == [[0, 2, 5], [1, 3], [4]]
    assert t.boxes.shape == (3, 6) and t.boxes.dtype == torch.float64 and bool(torch.isnan(t.boxes[:, :4]).all())
    assert t.boxes[:, 4].tolist() == [0.7, 0.9, 0.1] and t.boxes[:, 5].tolist() == [2.0, 0.0, 4.0] and t.names == {0: "a"}
    for f in (t.track, t.cls, t.count, t.first_row):
        assert f.dtype == torch.int64
    with pytest.raises(IndexError):
        t.rows(3)
    # any labelling that separates the tracks gives the same table, and so does the reference
    other = build_tracks(torch.from_numpy(tf), torch.from_numpy(conf), torch.from_numpy(cls), torch.tensor([7, 3, 7, 3, 0, 7]))
    ref = L.tracks_ref(tf, conf, cls, label)
    for name in ("track", "tf", "conf", "cls", "count", "first_row"):
        assert np.array_equal(getattr(t, name).numpy(), ref[name]) and torch.equal(getattr(t, name), getattr(other, name)), name
    assert all(np.array_equal(t.rows(k).numpy(), ref["rows"][k]) for k in range(3))


def test_tracks_table_on_a_random_list_equals_the_reference():
    from sy11.data.link import build_tracks
    window, boxes, score, cls, start = R.survivors(5, 50, 320, 2, "ios", 0.5, False)
    tf = L.survivor_tf(window, boxes, start)
    label = L.link_ref(tf, cls, 8 * 256 / 20e6)
    conf = score.astype(np.float64)
    conf[::3] = conf[0]                                                                           # ties
    t = build_tracks(torch.from_numpy(tf), torch.from_numpy(conf), torch.from_numpy(cls.astype(np.int64)), torch.from_numpy(label))
    ref = L.tracks_ref(tf, conf, cls, label)
    assert 1 < len(t) < len(window)
    for name in ("track", "tf", "conf", "cls", "count", "first_row"):
        assert np.array_equal(getattr(t, name).numpy(), ref[name]), name
    assert int(t.count.sum()) == len(window) and np.array_equal(t.first_row.numpy(), np.unique(label))


def test_empty_results_give_empty_tracks_without_a_device():
    from sy11.data.link import link_results
    t = link_results(_results(np.zeros((0, 4))), "cuda")                                          # no launch: passes on a machine with no GPU
    assert len(t) == 0 and t.track.shape == (0,) and t.tf.shape == (0, 4) and t.boxes.shape == (0, 6) and t.count.shape == (0,)
    assert t.plan.gap_t == 8 * 256 / 20e6 and t.names == {0: "a", 1: "b"}


def test_tracks_save_round_trips_through_json(tmp_path):
    from sy11.data.link import LinkPlan, build_tracks
    tf = np.array([[0.0, 1.0, 1.0, 2.0], [0.5, 1.0, 1.75, 2.5], [3.0, 1.0, 4.0, 2.0]])
    t = build_tracks(torch.from_numpy(tf), torch.tensor([0.25, 0.5, 0.125], dtype=torch.float64), torch.tensor([1, 0, 1]),
                     torch.tensor([0, 0, 2]), {0: "lte", 1: "chirp"}, LinkPlan(1e-4, None, 0.5, False))
    path = t.save(tmp_path / "tracks.json")
    d = json.loads(Path(path).read_text())
    assert d["rows"] == 3 and d["link"] == {"gap_t": 1e-4, "gap_f": None, "align": 0.5, "agnostic": False}
    assert d["tracks"] == [{"track": 0, "tf": [0.0, 1.0, 1.75, 2.5], "class": 0, "name": "lte", "confidence": 0.5, "count": 2, "rows": [0, 1]},
                           {"track": 1, "tf": [3.0, 1.0, 4.0, 2.0], "class": 1, "name": "chirp", "confidence": 0.125, "count": 1, "rows": [2]}]


# ------------------------------------------------------------------------------------------------------------- the front door
def test_front_door_has_link():
    import inspect

    from sy11 import ops
    from sy11.engine.model import YOLO
    from sy11.engine.predictor import DetectionPredictor, link_keywords
    assert callable(YOLO.link) and callable(DetectionPredictor.link) and callable(ops.scan_link)
    for f in (YOLO.scan, DetectionPredictor.scan):
        assert inspect.signature(f).parameters["link"].default is None
    for f in (YOLO.link, DetectionPredictor.link):
        p = inspect.signature(f).parameters
        assert (p["gap_t"].default, p["gap_f"].default, p["align"].default, p["agnostic"].default) == ("auto", "auto", 0.5, False)
    r = _results([[0.0, 1.0, 1.0, 2.0]])
    assert r.track is None and r.tracks is None
    assert link_keywords(None) is None and link_keywords(True) == {} and link_keywords({"align": 0.25}) == {"align": 0.25}
    for bad in ("yes", 1, {"align": 0.0}, {"gap_t": -1.0}, {"gap": 1.0}):
        with pytest.raises(ValueError):
            link_keywords(bad)
