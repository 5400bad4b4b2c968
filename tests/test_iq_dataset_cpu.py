"""CPU: the IQ dataset's host side — inverse maps, YAML rules, sidecars, windows, labels, the augmentation draws — and the float64
restatement (tests/_iq_ref.py) the GPU kernel test relies on: its Philox against published known answers, its noise statistics."""
import math
import random
from types import SimpleNamespace

import numpy as np
import pytest

from sy11.data import iq_augment as A
from sy11.data.iq_dataset import IQDataLoader, IQDataset, read_iq_sidecar
from sy11.data.spectrogram import cols_to_time, freq_to_rows, plan_windows, rows_to_freq, time_to_cols
from sy11.engine.model import _hyp_defaults, check_det_dataset

from . import _iq_ref as R
from ._iq_util import CAPTURES, FC, HOP, IMGSZ, L, N_FFT, SR, write_dataset


def hyp(**kw):
    return SimpleNamespace(**{**_hyp_defaults(), **kw}, imgsz=IMGSZ)


@pytest.fixture(scope="module")
def dataset_dir(tmp_path_factory):
    root = tmp_path_factory.mktemp("iqds")
    y, caps = write_dataset(root)
    return root, y, caps


def build(dataset_dir, mode="train", **kw):
    data = check_det_dataset(dataset_dir[1])
    return IQDataset(data[mode if mode != "train" else "train"], data, imgsz=IMGSZ, hyp=hyp(**kw), mode=mode, device="cpu")


# ---------------------------------------------------------------------------------------------------- maps
def test_inverse_maps_round_trip():
    """float64 round-off only: the measured maximum is asserted below 1e-9 (rows) / 1e-9 (columns)."""
    for n_fft, n_mel, sr, fc in ((1024, 640, 20e6, 2.4e9), (512, 320, SR, FC), (1024, 640, 1.0, 0.0)):
        r = np.arange(n_mel, dtype=np.float64)
        err = np.abs(freq_to_rows(rows_to_freq(r, sr, fc, n_fft, n_mel), sr, fc, n_fft, n_mel) - r).max()
        print(f"rows n_fft={n_fft} sr={sr:g} fc={fc:g}: max |err| = {err:.3e}")
        assert err <= 1e-9
        # the restatement's scalar arithmetic agrees with the product's
        assert abs(R.freq_to_row(rows_to_freq(17.25, sr, fc, n_fft, n_mel), sr, fc, n_fft, n_mel) - 17.25) <= 1e-9
        c = np.arange(10 ** 4, dtype=np.float64)
        err = np.abs(time_to_cols(cols_to_time(c, sr, n_fft, 256), sr, n_fft, 256) - c).max()
        print(f"cols: max |err| = {err:.3e}")
        assert err <= 1e-9


# ---------------------------------------------------------------------------------------------------- YAML and sidecars
def test_yaml_rules(dataset_dir, tmp_path):
    data = check_det_dataset(dataset_dir[1])
    assert data["kind"] == "iq" and data["sample_rate"] == SR and data["center_freq"] == FC and (data["n_fft"], data["hop"]) == (N_FFT, HOP)
    assert data["nc"] == 2
    with pytest.raises(SyntaxError, match="sample_rate"):
        check_det_dataset({"train": "x", "val": "x", "nc": 2, "kind": "iq"})
    d = check_det_dataset({"train": "x", "val": "x", "nc": 2, "kind": "iq", "sample_rate": 5e6})
    assert d["center_freq"] == 0.0 and (d["n_fft"], d["hop"]) == (1024, 256)
    img = check_det_dataset({"train": "x", "val": "x", "nc": 3})               # an image YAML parses as before: no IQ key appears
    assert not {"kind", "sample_rate", "center_freq", "n_fft", "hop"} & set(img) and img["nc"] == 3 and img["names"][2] == "class_2"


@pytest.mark.parametrize("row, what", [("0 0.2 0.1 1 2", "t1 <= t0"), ("0 0.1 0.2 5 5", "f_hi <= f_lo"), ("2 0.1 0.2 1 2", "class"),
                                       ("0 0.1 inf 1 2", "non-finite"), ("0 0.1 0.2 1", "five numbers")])
def test_sidecar_errors_name_the_file(tmp_path, row, what):
    p = tmp_path / "cap_17.txt"
    p.write_text("1 0.0 0.5 -3 4\n" + row + "\n")
    with pytest.raises(ValueError, match=what) as e:
        read_iq_sidecar(str(p), nc=2)
    assert "cap_17.txt" in str(e.value)
    assert read_iq_sidecar(str(tmp_path / "missing.txt"), 2).shape == (0, 5)
    (tmp_path / "empty.txt").write_text("\n")
    assert read_iq_sidecar(str(tmp_path / "empty.txt"), 2).shape == (0, 5)


# ---------------------------------------------------------------------------------------------------- windows
def test_val_windows_are_the_plan_grid_and_train_windows_stay_inside(dataset_dir):
    v = build(dataset_dir, "val")
    want = [(i, int(s)) for i, (_, n, _) in enumerate(CAPTURES) for s in plan_windows(n, overlap=0, n_fft=N_FFT, hop=HOP, n_frames=IMGSZ)]
    assert v.items == want and len(v) == 2 + 3 + 3 + 3
    assert [(r.a.cap, r.a.first) for r in (v[i] for i in range(len(v)))] == [(c, f * HOP) for c, f in want]
    random.seed(5)
    t = build(dataset_dir, "train")
    assert len(t) == len(v)
    moved = 0
    for _ in range(20):
        for i in range(len(t)):
            a = t[i].a
            assert a.first % HOP == 0 and 0 <= a.first and a.first + L <= CAPTURES[a.cap][1]
            assert abs(a.first // HOP - want[i][1]) <= IMGSZ // 2
            moved += a.first != want[i][1] * HOP
    assert moved > 100
    t0 = build(dataset_dir, "train", iq_jitter=0.0)
    assert [(t0[i].a.cap, t0[i].a.first) for i in range(len(t0))] == [(c, f * HOP) for c, f in want]


def test_short_capture_raises_at_construction(tmp_path):
    d = tmp_path / "iq"
    d.mkdir()
    np.save(d / "short.npy", np.zeros(L - 1, np.complex64))
    with pytest.raises(ValueError, match="short.npy"):
        IQDataset(str(d), {"sample_rate": SR, "nc": 1, "n_fft": N_FFT, "hop": HOP}, imgsz=IMGSZ, mode="val", device="cpu")


# ---------------------------------------------------------------------------------------------------- labels
G = A.Geometry(SR, FC, N_FFT, HOP, IMGSZ, IMGSZ)


def t_of_px(x, first=0):
    """The time whose box edge sits at pixel x of the window starting at sample `first`: column x - 0.5 = centre of that frame."""
    return (first + (x - 0.5) * HOP + N_FFT / 2) / SR


def f_of_px(y):
    return float(rows_to_freq(y - 0.5, SR, FC, N_FFT, IMGSZ))


def test_labels_hand_computed_cases():
    first = 7 * HOP
    src = A.IQSource(0, first)
    # (1) fully inside: x 10.5 .. 50.5 by hand (frames 10 and 50), y edges at the centre frequency and 0.1 MHz above
    y_c = (math.log1p(1.25 / 511) / math.log1p(1.25) + 1.0) * 321 / 2 - 1.0 + 0.5            # fc: bin 256, u = 512/511 - 1
    u = (0.6 * 512) / (256 * 511 / 512) - 1.0                                               # fc + 0.1 MHz: bin 0.6 * 512
    y_h = (math.log1p(1.25 * u) / math.log1p(1.25) + 1.0) * 321 / 2 - 1.0 + 0.5
    rows = np.array([[1, t_of_px(10.5, first), t_of_px(50.5, first), FC, FC + 0.1e6],
                     # (2) cut by the right window edge: 40 px wide, 15 inside -> kept, clipped to x in [305, 320]
                     [0, t_of_px(305.0, first), t_of_px(345.0, first), f_of_px(100.0), f_of_px(140.0)],
                     # (3) cut to < 0.1 of its area: 40 px wide, 3 inside -> dropped
                     [0, t_of_px(-37.0, first), t_of_px(3.0, first), f_of_px(100.0), f_of_px(140.0)],
                     # (4) thinner than 2 px in frequency -> dropped; (5) thinner than 2 px in time -> dropped
                     [1, t_of_px(20.0, first), t_of_px(60.0, first), f_of_px(200.0), f_of_px(201.5)],
                     [1, t_of_px(20.0, first), t_of_px(21.9, first), f_of_px(200.0), f_of_px(240.0)]])
    lb = A.window_labels(rows, src, G)
    assert lb.dtype == np.float32 and lb.shape == (2, 5)
    want = np.array([[1, 30.5 / 320, (y_c + y_h) / 2 / 320, 40.0 / 320, (y_h - y_c) / 320],
                     [0, 312.5 / 320, 120.0 / 320, 15.0 / 320, 40.0 / 320]])
    assert np.abs(lb - want).max() <= 2e-7                                    # float32 rounding of values <= 1
    assert abs(R.freq_to_row(FC + 0.1e6, SR, FC, N_FFT, IMGSZ) + 0.5 - y_h) < 1e-9 and abs(R.time_to_col(t_of_px(10.5), SR, N_FFT, HOP) - 10.0) < 1e-9


def test_shift_keeps_boxes_in_band_and_labels_follow_the_quantised_shift(dataset_dir):
    random.seed(11)
    ds = build(dataset_dir, "train", iq_shift=0.5, iq_conj=0.5)
    f_min, f_max = G.band()
    seen_conj = seen_clamped = n_boxes = 0
    for k in range(200):
        rec = ds[k % len(ds)]
        a = rec.a
        assert a.dphi == (int(round(a.shift_hz / SR * 2 ** 32)) & 0xFFFFFFFF) and abs(a.shift_hz) <= 0.5 * SR
        rows = A.boxes_in_time(ds.rows[a.cap], a.first, G)
        for c, t0, t1, flo, fhi in rows:                                      # every emission in the window stays inside the band
            e = sorted((2 * FC - f if a.conj else f) + a.shift_hz for f in (flo, fhi))
            assert f_min - 1e-3 <= e[0] and e[1] <= f_max + 1e-3
            y = [R.freq_to_row(f, SR, FC, N_FFT, IMGSZ) + 0.5 for f in e]
            assert -1e-6 <= y[0] and y[1] <= IMGSZ + 1e-6
        seen_conj += a.conj
        seen_clamped += len(rows) > 0 and abs(a.shift_hz) < 0.2 * SR
        lb = rec.labels
        n_boxes += len(lb)
        assert (lb[:, 1:] >= 0).all() and (lb[:, 1:] <= 1).all()
        assert np.abs(lb - A.window_labels(ds.rows[a.cap], a, G)).max(initial=0) == 0
        # label rows against the restatement: cy / h of every kept box from freq_to_row(f' ) of the mirrored + shifted edges
        kept = [r for r in rows if len(A.window_labels(r[None], a, G))]
        assert len(kept) == len(lb)
        for r, l in zip(kept, lb):
            y = sorted(R.freq_to_row((2 * FC - f if a.conj else f) + a.shift_hz, SR, FC, N_FFT, IMGSZ) + 0.5 for f in r[3:5])
            assert abs(l[2] - (y[0] + y[1]) / 2 / IMGSZ) <= 2e-7 and abs(l[4] - (y[1] - y[0]) / IMGSZ) <= 2e-7
    assert 60 < seen_conj < 140 and n_boxes > 100 and seen_clamped > 0


def test_mixing_concatenates_labels_and_close_mosaic_switches_it_off(dataset_dir):
    random.seed(3)
    ds = build(dataset_dir, "train", iq_mixup=1.0, iq_shift=0.25, iq_gain_db=6.0, iq_noise_db=10.0)
    mixed = 0
    for i in range(len(ds)):
        rec = ds[i]
        assert rec.b is not None
        la, lb = A.window_labels(ds.rows[rec.a.cap], rec.a, G), A.window_labels(ds.rows[rec.b.cap], rec.b, G)
        assert np.array_equal(rec.labels, np.concatenate([la, lb]))
        mixed += len(la) > 0 and len(lb) > 0
        assert 10 ** (-6 / 20) <= rec.a.gain <= 10 ** (6 / 20) and 10 ** (-6 / 20) <= rec.b.gain <= 10 ** (6 / 20)
        assert rec.sigma >= 0 and (rec.sigma == 0) == (rec.seed == 0)
    assert mixed > 0
    ds.close_mosaic(ds.hyp)
    assert all(ds[i].b is None for i in range(len(ds)))


def test_seeded_recipes_repeat_and_val_draws_nothing(dataset_dir):
    kw = dict(iq_shift=0.25, iq_conj=0.5, iq_gain_db=6.0, iq_noise_db=10.0, iq_mixup=0.5)
    runs = []
    for _ in range(2):
        random.seed(42)
        ds = build(dataset_dir, "train", **kw)
        runs.append([ds[i] for i in range(len(ds))] + [ds[0]])
    for a, b in zip(*runs):
        assert (a.a, a.b, a.sigma, a.seed) == (b.a, b.b, b.sigma, b.seed) and np.array_equal(a.labels, b.labels)
    assert any(r.sigma > 0 for r in runs[0]) and any(r.b is not None for r in runs[0]) and any(r.a.dphi for r in runs[0])
    random.seed(9)
    state = random.getstate()
    v = build(dataset_dir, "val", **kw)
    for i in range(len(v)):
        r = v[i]
        assert (r.a.dphi, r.a.phi0, r.a.conj, r.a.gain, r.sigma, r.b) == (0, 0, False, 1.0, 0.0, None)
    dl = IQDataLoader(v, 4, shuffle=False)
    assert len(dl) == 3
    assert random.getstate() == state


def test_noise_sigma_follows_the_window_power(dataset_dir):
    random.seed(1)
    ds = build(dataset_dir, "train", iq_noise_db=10.0, iq_jitter=0.0)
    p = A.noise_reference_power(ds.captures[3], 0, L)                        # the background-only capture: power 2 * 0.05^2
    assert abs(p / 0.005 - 1) < 0.1
    sig = [ds[len(ds) - 1].sigma for _ in range(40)]                          # item 10: capture d, last window
    on = [s for s in sig if s > 0]
    assert 5 < len(on) < 35 and all(0.9 * math.sqrt(0.005) <= s <= 1.1 * math.sqrt(0.05) for s in on)


# ---------------------------------------------------------------------------------------------------- the restatement itself
def test_philox_known_answers():
    """Philox4x32-10 known-answer vectors as published with Random123 (kat_vectors: zero / all-ones / digits-of-pi blocks); the
    zero block is also what the rounds in torch's ATen/core/PhiloxRNGEngine.h give for key 0, counter 0."""
    kat = (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)))
    for ctr, key, want in kat:
        got = R.philox4x32_10(np.array(ctr, dtype=np.uint64), key)
        assert tuple(int(v) for v in got) == want, [hex(int(v)) for v in got]


def test_restated_noise_statistics():
    n = 2 ** 16
    w = R.noise(0x1234567890abcdef, n)
    assert w.shape == (n,)
    for name, x in (("I", w.real), ("Q", w.imag)):
        m, v = x.mean(), x.var()
        se_m, se_v = math.sqrt(0.5 / n), 0.5 * math.sqrt(2.0 / n)               # normal: var of the sample variance = 2 s^4 / n
        print(f"{name}: mean {m:+.5f} (se {se_m:.5f})  var {v:.5f} (se {se_v:.5f})")
        assert abs(m) <= 4 * se_m and abs(v - 0.5) <= 4 * se_v
    assert np.array_equal(R.noise(7, 200)[100:200], R.noise(7, 4864)[100:200])
