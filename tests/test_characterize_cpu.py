"""CPU: the host side of ``characterize`` (sy11.data.characterize) against the float64 reference of tests/_characterize_ref.py — the plan's
arithmetic, every ``ValueError``, the derived columns on hand-made device tables, the empty extraction, ``save`` — and the reference itself
on generated clips with known truths (N = 1024, M = 8192).

Generated clips.  After ``extract`` a clip's band fills 42 - 84 % of its rate, so the keyed clips run at 3.3 samples per symbol; at 7 and
more the spectrum of x^2 of a four-phase signal is a hump over an empty band and its peak stands 19 dB above the median without any line.
Lines and offsets: RRC roll-off 0.35, 20 dB SNR, carrier offset 37.3 bins; seeds 1 and 2.  The reference's figures there (rate, x^2, x^4
line in dB): BPSK 16.1 - 16.4 / 34.8 / 30, QPSK 19.3 / 7.2 - 7.5 / 24.8, CW 2.4 - 2.9 / 41.4 / 36.0, noise 2.9 - 3.6 everywhere: every line
that decides ``order`` or ``keyed`` is 3 dB or more away from the 13 dB threshold.  Rate and offsets land within 0.02 bin.

c42.  The issue's truths (-2, -1, -1, 0) are those of the constellation; the definition reaches them only under conditions that the test
has to arrange, and says so: (a) ``|m20|^2`` is not invariant under a carrier offset — with 37.3 bins of offset m20 averages out and BPSK
reads -0.62, a bare carrier -0.98; at zero offset BPSK reads -1.73 and a bare carrier -1.96; (b) pulse shaping scales the cumulant by
``(1/T) int h^4 / ((1/T) int h^2)^2``, 0.85 for RRC 0.35 and 1.05 for RRC 0.75; (c) noise scales it by (S / (S + N))^2.  So c42 is checked on
BPSK at ZERO offset, QPSK and CW at 37.3 bins, all with roll-off 0.75 at 20 dB, and on noise."""
import json
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import _characterize_ref as R

N, M, FS, FC = 1024, 8192, 1.0e6, 2.4e9
SPS, OFF = 3.3, 37.3                                            # samples per symbol; carrier offset in bins of N
SEEDS = (1, 2)
LINE_DB = 13.0


def _extraction(Ms, fs, fc=FC, packed=None):
    """What ``characterize`` reads of an ``Extraction``, without a device."""
    Ms = np.asarray(Ms, dtype=np.int64)
    offset = np.concatenate(([0], np.cumsum(Ms))).astype(np.int64)
    n = Ms.shape[0]
    plan = SimpleNamespace(M=Ms, offset=offset)
    return SimpleNamespace(plan=plan, packed=torch.zeros(int(offset[-1]), dtype=torch.complex64) if packed is None else packed,
                           sample_rate=np.broadcast_to(np.asarray(fs, dtype=np.float64), (n,)).copy(),
                           center_freq=np.broadcast_to(np.asarray(fc, dtype=np.float64), (n,)).copy(), rows=np.arange(n), cls=np.arange(n) % 2,
                           conf=np.linspace(0.5, 0.9, n) if n else np.zeros(0), names={0: "a", 1: "b"})


# ------------------------------------------------------------------------------------------------------------- plan
@pytest.mark.parametrize("n_fft", [64, 128, 1024])
def test_plan_arithmetic_matches_the_reference(n_fft):
    from sy11.data.characterize import ITEM, ROW, group, plan_characterize
    H, G = n_fft // 2, group()
    assert G == R.G and ITEM.itemsize == 32 and ROW.itemsize == 32
    Ms = [n_fft - 1, n_fft, n_fft + H - 1, n_fft + H, 0, n_fft + 15 * H, n_fft + 16 * H, n_fft + 32 * H + 7, 5]
    fs = np.array([1e6, 2e6, 3e6, 1e6, 1e6, 5e5, 1e6, 4e6, 1e6])
    for min_rate in (None, 0.0, 5.0e4):
        p = plan_characterize((Ms, fs), n_fft, min_rate)
        ref = [R.plan(m, f, n_fft, min_rate or 0.0) for m, f in zip(Ms, fs)]
        for key in ("valid", "J", "L", "groups", "k_min"):
            assert getattr(p, key).tolist() == [r[key] for r in ref], (key, min_rate)
        assert p.J.tolist() == [0, 1, 1, 2, 0, 16, 17, 33, 0] and p.groups.tolist() == [0, 1, 1, 1, 0, 1, 2, 3, 0]
        assert p.offset.tolist() == np.concatenate(([0], np.cumsum(Ms)))[:-1].tolist() and p.total_rows == 9 and p.total_frames == 70
        it, clip = p.items()
        assert clip.tolist() == [1, 2, 3, 5, 6, 6, 7, 7, 7] and it["row"].tolist() == list(range(9))
        assert it["j0"].tolist() == [0, 0, 0, 0, 0, 16, 0, 16, 32] and it["nf"].tolist() == [1, 1, 2, 16, 16, 1, 16, 16, 1]
        assert it["last"].tolist() == [1, 1, 1, 1, 0, 1, 0, 0, 1] and it["len"].tolist() == [Ms[c] for c in clip] and it["off"].tolist() == p.offset[clip].tolist()
        rows = p.rows()
        assert rows["clip"].tolist() == [1, 2, 3, 5, 6, 7] and rows["row0"].tolist() == [0, 1, 2, 3, 4, 6] and rows["n_rows"].tolist() == [1, 1, 1, 1, 2, 3]
        W2 = R.window(n_fft)[1]
        assert rows["scale"].tolist() == [1.0 / (float(r["J"]) * float(n_fft) * W2) for r in ref if r["valid"]]
    assert plan_characterize((Ms, 1e6), n_fft).k_min.tolist() == [3] * len(Ms)                  # a scalar rate broadcasts
    assert plan_characterize((Ms, 1e6), n_fft, 1e6 * 10.5 / n_fft).k_min.tolist() == [11] * len(Ms)
    e = _extraction(Ms, fs)
    q = plan_characterize(e, n_fft, None)
    assert q.M.tolist() == Ms and q.offset.tolist() == e.plan.offset[:-1].tolist() and q.fs.tolist() == fs.tolist()


def test_every_argument_error_is_a_value_error():
    from sy11.data.characterize import characterize_extraction, plan_characterize
    ok = ([4096, 100], [1e6, 2e6])
    for n_fft in (48, 2048, 0, 1024.0, True, "1024", None):
        with pytest.raises(ValueError, match="n_fft"):
            plan_characterize(ok, n_fft)
    for min_rate in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="min_rate"):
            plan_characterize(ok, 1024, min_rate)
    assert plan_characterize(ok, 1024, 1e6 * 509.5 / 1024).k_min.tolist() == [510, 255]         # bins 510, 511: two are left
    with pytest.raises(ValueError, match="fewer than 2 searched bins for clip 0"):
        plan_characterize(ok, 1024, 1e6 * 510.5 / 1024)                                        # bin 511 alone at clip 0's rate
    with pytest.raises(ValueError, match="fewer than 2 searched bins"):
        plan_characterize(([4096], [1e6]), 64, 0.49e6)
    for fs in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="sample rate"):
            plan_characterize(([4096, 100], [1e6, fs]), 1024)
    for bad in (([4096.5], [1e6]), ([-1], [1e6]), ([[1, 2]], [1e6]), ([1, 2, 3], [1e6, 2e6]), 7, ([2 ** 31], [1e6])):
        with pytest.raises(ValueError):
            plan_characterize(bad, 1024)
    e = _extraction([4096], 1e6)
    for line_db in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="line_db"):
            characterize_extraction(e, 1024, None, line_db)
    with pytest.raises(ValueError, match="n_fft"):
        characterize_extraction(e, 100)
    with pytest.raises(ValueError, match="min_rate"):
        characterize_extraction(e, 1024, -5.0)


# ------------------------------------------------------------------------------------------------------------- derive
def _table(rows):
    """(n, 22) device table from per-clip dicts: peak / left / right / median / k / n (3 each), m20, m21, m42."""
    o = np.full((len(rows), 22), np.nan)
    for i, r in enumerate(rows):
        if r is None:
            continue
        for q in range(3):
            o[i, 4 * q:4 * q + 4] = r["peak"][q], r["left"][q], r["right"][q], r["median"][q]
            o[i, 16 + 2 * q], o[i, 17 + 2 * q] = r["k"][q], r["n_search"][q]
        o[i, 12:16] = r["m20"].real, r["m20"].imag, r["m21"], r["m42"]
    return o


def test_derive_on_hand_made_tables():
    from sy11.data.characterize import Characterization, plan_characterize
    n_fft = 64
    Ms, fs = [640, 640, 63, 640], np.array([1.0e6, 2.0e6, 1.0e6, 1.0e6])
    fc = np.array([1.0e9, 2.0e9, 3.0e9, 4.0e9])
    plan = plan_characterize((Ms, fs), n_fft)
    J, L = 19, 640
    assert plan.J.tolist() == [J, J, 0, J] and plan.L.tolist() == [L, L, 0, L]
    hand = [
        # clip 0: an order-2 signal; the rate peak has a ZERO neighbour (delta = 0), the x^2 peak is asymmetric, the x^4 peak symmetric
        dict(peak=[40.0, 800.0, 90.0], left=[0.0, 100.0, 30.0], right=[10.0, 200.0, 30.0], median=[1.0, 2.0, 3.0], k=[20, -7, -14], n_search=[29, 64, 64],
             m20=(0.9 + 0.1j) * L, m21=1.0 * L, m42=1.1 * L),
        # clip 1: order 4 (the x^2 line is 1 dB short of the threshold); a flat top (denominator 0) on the rate line
        dict(peak=[5.0, 10.0 ** 1.2, 50.0], left=[5.0, 1.0, 20.0], right=[5.0, 1.0, 10.0], median=[1.0, 1.0, 1.0], k=[31, 5, 10], n_search=[29, 64, 64],
             m20=0.0j, m21=2.0 * L, m42=4.0 * L),
        None,                                                                                    # clip 2: invalid (63 < 64 samples)
        # clip 3: nothing reaches the threshold -> order 0; a negative neighbour -> delta = 0
        dict(peak=[3.0, 2.0, 19.9], left=[1.0, -1.0, 1.0], right=[1.0, 1.0, 1.0], median=[1.0, 1.0, 1.0], k=[3, -32, 31], n_search=[29, 64, 64],
             m20=0.0j, m21=1.0 * L, m42=2.0 * L),
    ]
    spectra = torch.zeros((4, 3, n_fft), dtype=torch.float64)
    c = Characterization(plan, fc, spectra, _table(hand), LINE_DB, rows=np.arange(4))
    for i, r in enumerate(hand):
        if r is None:
            continue
        d = R.derive(r, (r["m20"], r["m21"], r["m42"]), n_fft, J, fs[i], fc[i], LINE_DB)
        for key in ("symbol_rate", "offset2", "offset4", "power", "c42", "carrier"):
            got = float(getattr(c, key)[i])
            assert (math.isnan(got) and math.isnan(d[key])) or got == d[key] or abs(got - d[key]) <= 1e-12 * abs(d[key]), (i, key, got, d[key])
        assert np.allclose(c.line_db[i], d["line_db"], rtol=1e-12, atol=0) and int(c.order[i]) == d["order"] and bool(c.keyed[i]) == d["keyed"]
    # by hand
    assert c.symbol_rate[0] == 20 / 64 * 1.0e6                                                   # a zero neighbour: no refinement
    a, b, cc = math.log(100.0), math.log(800.0), math.log(200.0)
    assert abs(c.offset2[0] - (-7 + 0.5 * (a - cc) / (a - 2 * b + cc)) / 64 * 1.0e6 / 2) < 1e-6 and c.offset2[0] > -7 / 64 * 1.0e6 / 2
    assert c.offset4[0] == -14 / 64 * 1.0e6 / 4 and c.order.tolist() == [2, 4, -1, 0] and c.keyed.tolist() == [True, False, False, False]
    assert c.carrier[0] == fc[0] + c.offset2[0] and c.carrier[1] == fc[1] + c.offset4[1] and math.isnan(c.carrier[3])
    assert c.symbol_rate[1] == 31 / 64 * 2.0e6 and abs(c.line_db[1, 1] - 12.0) < 1e-12            # a flat top: denominator 0
    assert c.offset2[3] == -32 / 64 * 1.0e6 / 2 and abs(c.line_db[3, 2] - 10 * math.log10(19.9)) < 1e-12
    assert abs(c.c42[0] - (1.1 - (0.81 + 0.01) - 2.0)) < 1e-12 and c.c42[1] == (4.0 - 0.0 - 8.0) / 4.0 and c.power.tolist()[:2] == [1.0, 2.0]
    # the invalid clip: NaN in every float column, -1 in every integer column
    for key in ("symbol_rate", "offset2", "offset4", "power", "c42", "carrier"):
        assert math.isnan(getattr(c, key)[2]), key
    assert np.isnan(c.line_db[2]).all() and np.isnan(c.line_freq[2]).all() and c.peak_bin[2].tolist() == [-1, -1, -1] and c.frames[2] == -1
    assert c.order[2] == -1 and not c.valid[2] and not c.keyed[2] and c.raw["n_search"][2].tolist() == [-1, -1, -1]
    assert c.valid.tolist() == [True, True, False, True] and c.frames.tolist() == [J, J, -1, J] and len(c) == 4
    assert c[0]["order"] == 2 and c[0]["symbol_rate"] == c.symbol_rate[0] and c[-1]["line4_db"] == c.line_db[3, 2]
    assert np.array_equal(c.freqs(1, 2), np.arange(-32, 32) * 2.0e6 / 64)


def test_a_tie_takes_the_first_maximum():
    """In the reference's ``reduce`` (the device's order): two equal maxima, the lower bin wins; for q = 0 only bins from k_min up count."""
    n_fft, J = 64, 1
    part = np.ones((1, 3, n_fft), dtype=np.float32)
    part[0, 0, [2, 9, 20]] = (50.0, 7.0, 7.0)               # bin 2 lies below k_min = 3
    part[0, 1, [64 - 5, 6]] = 9.0                            # bins -5 and 6
    part[0, 2, [64 - 32, 31]] = 4.0                          # bins -32 and 31
    r = R.reduce(part, n_fft, J, 3)
    assert r["k"] == [9, -5, -32] and r["n_search"] == [29, 64, 64]
    s = 1.0 / (J * n_fft * R.window(n_fft)[1])
    assert r["peak"] == [7.0 * s, 9.0 * s, 4.0 * s] and r["left"][2] == 4.0 * s and r["right"][2] == 1.0 * s      # the neighbours are cyclic
    assert r["median"] == [s, s, s]


# ------------------------------------------------------------------------------------------------------------- empty, save
def test_an_empty_extraction_gives_an_empty_characterization_with_no_launch():
    from sy11 import _lib
    from sy11.data.characterize import Characterization, characterize_extraction
    _lib.PROFILE = []
    try:
        c = characterize_extraction(_extraction([], 1e6))
        short = characterize_extraction(_extraction([10, 1023], 1e6))         # clips, but none holds a frame: nothing to launch either
        calls = list(_lib.PROFILE)
    finally:
        _lib.PROFILE = None
    assert calls == []
    assert isinstance(c, Characterization) and len(c) == 0 and c.spectra.shape == (0, 3, 1024) and c.symbol_rate.shape == (0,) and c.line_db.shape == (0, 3)
    assert c.order.shape == (0,) and c.valid.shape == (0,)
    assert len(short) == 2 and not short.valid.any() and short.order.tolist() == [-1, -1] and np.isnan(short.c42).all() and bool(torch.isnan(short.spectra).all())


def test_save_round_trip(tmp_path):
    from sy11.data.characterize import Characterization, plan_characterize
    plan = plan_characterize(([640, 10], [1.0e6, 1.0e6]), 64)
    row = dict(peak=[40.0, 800.0, 90.0], left=[8.0, 100.0, 30.0], right=[10.0, 200.0, 30.0], median=[1.0, 2.0, 3.0], k=[20, -7, -14], n_search=[29, 64, 64],
               m20=64.0 + 0j, m21=640.0, m42=700.0)
    spectra = torch.arange(2 * 3 * 64, dtype=torch.float64).reshape(2, 3, 64)
    c = Characterization(plan, [FC, FC + 1], spectra, _table([row, None]), LINE_DB, rows=np.array([5, 2]), cls=np.array([1, 0]), conf=np.array([0.9, 0.8]),
                         names={0: "a", 1: "b"})
    out = c.save(tmp_path / "c")
    assert out == str(tmp_path / "c")
    z = np.load(tmp_path / "c" / "characterize.npz")
    for key in ("symbol_rate", "offset2", "offset4", "carrier", "power", "c42", "line_db", "order", "keyed", "valid", "frames", "peak_bin"):
        assert np.array_equal(z[key], getattr(c, key), equal_nan=True), key
    assert np.array_equal(z["spectra"], spectra.numpy()) and z["rows"].tolist() == [5, 2]
    j = json.loads((tmp_path / "c" / "characterize.json").read_text())
    assert j["n_fft"] == 64 and j["line_db"] == LINE_DB and j["file"] == "characterize.npz" and len(j["clips"]) == 2
    a, b = j["clips"]
    assert a["row"] == 5 and a["name"] == "b" and a["confidence"] == 0.9 and a["order"] == 2 and a["keyed"] and a["symbol_rate"] == c.symbol_rate[0]
    assert a["carrier"] == c.carrier[0] and a["line2_db"] == c.line_db[0, 1]
    assert b["valid"] is False and b["order"] == -1 and b["symbol_rate"] is None and b["c42"] is None and b["frames"] == -1


# ------------------------------------------------------------------------------------------------------------- the reference on known signals
@pytest.fixture(scope="module")
def known():
    """kind -> [reference result per seed] for the line clips, and the c42 clips; computed once."""
    lines = {kind: [R.characterize(R.clip(kind, M, seed, SPS, OFF / N, 20.0, 0.35), FS, FC, N) for seed in SEEDS]
             for kind in ("bpsk", "qpsk", "cw", "noise")}
    c42 = {kind: [R.characterize(R.clip(kind, M, seed, SPS, off / N, 20.0, 0.75), FS, FC, N) for seed in SEEDS]
           for kind, off in (("bpsk", 0.0), ("qpsk", OFF), ("cw", OFF), ("noise", OFF))}
    return lines, c42


def test_the_reference_finds_rate_offset_and_order_of_known_signals(known):
    lines, _ = known
    bin_hz = FS / N
    for kind, order, keyed in (("bpsk", 2, True), ("qpsk", 4, True), ("cw", 2, False), ("noise", 0, False)):
        for seed, r in zip(SEEDS, lines[kind]):
            db = r["line_db"]
            print(f"reference[{kind} seed {seed}]: lines {db[0]:.1f} / {db[1]:.1f} / {db[2]:.1f} dB, rate {r['symbol_rate'] / bin_hz:.3f} bins "
                  f"(truth {N / SPS:.3f}), offset2 {r['offset2'] / bin_hz:.3f}, offset4 {r['offset4'] / bin_hz:.3f} bins (truth {OFF}), c42 {r['c42']:.3f}")
            assert r["J"] == 15 and r["order"] == order and r["keyed"] == keyed
            assert all(abs(v - LINE_DB) >= 3.0 for v in db), db                 # every line clears the threshold by 3 dB, either way
            if keyed:
                assert abs(r["symbol_rate"] - FS / SPS) <= 0.25 * bin_hz
            if order == 2:
                assert abs(r["offset2"] - OFF * bin_hz) <= 0.25 / 2 * bin_hz and r["carrier"] == FC + r["offset2"]
            if order in (2, 4):                                                  # BPSK and CW carry a line at order 4 too
                assert abs(r["offset4"] - OFF * bin_hz) <= 0.25 / 4 * bin_hz
            if order == 4:
                assert r["carrier"] == FC + r["offset4"]
            if order == 0:
                assert math.isnan(r["carrier"])


def test_the_reference_c42_of_known_signals(known):
    _, c42 = known
    for kind, want in (("bpsk", -2.0), ("qpsk", -1.0), ("cw", -1.0), ("noise", 0.0)):
        for seed, r in zip(SEEDS, c42[kind]):
            print(f"reference[{kind} seed {seed}, roll-off 0.75]: c42 {r['c42']:.3f} (truth {want}), power {r['power']:.4f}")
            assert abs(r["c42"] - want) <= 0.3
            assert abs(r["power"] - (1.0 if kind == "noise" else 1.01)) < 0.05


def test_reference_spectra_and_partials_agree():
    """``spectra`` (the definition) and ``reduce`` of the float64 per-group sums differ only by the order of the additions."""
    x = R.clip("qpsk", 64 + 32 * 40 + 5, 3, SPS, 0.07, 15.0)
    P = R.spectra(x, 64)
    r = R.reduce(R.partials64(x, 64), 64, 41, 3)
    assert R.plan(len(x), 1.0, 64)["J"] == 41 and np.abs(r["P"] - P).max() <= 1e-13 * P.max()
    m20, m21, m42 = R.moments(x, 64)
    xs = x[:64 + 32 * 40].astype(np.complex128)
    assert abs(m21 - (np.abs(xs) ** 2).sum()) <= 1e-12 * m21 and abs(m20 - (xs * xs).sum()) <= 1e-12 * m21 and abs(m42 - (np.abs(xs) ** 4).sum()) <= 1e-12 * m42
