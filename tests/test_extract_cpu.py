"""CPU: the host plan of the extraction (sy11/data/extract.py) — decimation choice, grid, mixer step, packed offsets, every argument
error, the chunker's invariants — the two figures of the prototype that the constant 0.84 rests on, what the float64 reference of a
clip (tests/_extract_ref.py) does to tones, and ``Extraction.save``."""
import json

import numpy as np
import pytest
import torch

from tests import _extract_ref as E

FS, FC, N = 1.0e6, 2.4e9, 40000


def _plan(tf, **kw):
    from sy11.data.extract import plan_extract
    kw.setdefault("n", N)
    return plan_extract(np.asarray(tf, dtype=np.float64), kw.pop("n"), FS, kw.pop("fc", FC), **kw)


# ------------------------------------------------------------------------------------------------------------- plan arithmetic
@pytest.mark.parametrize("D", [2, 4, 8, 16, 32, 64])
def test_decimation_flips_exactly_at_084_of_the_output_rate(D):
    from sy11.data.resample import USABLE_BAND
    assert USABLE_BAND == 0.84
    w = 0.84 * FS / D                                                       # centre 0 and +- w / 2: the box's width is w exactly
    wide = w * (1 + 1e-12)
    p = _plan([[0.01, -w / 2, 0.02, w / 2], [0.01, -wide / 2, 0.02, wide / 2]], fc=0.0, pad_f=0.0)
    assert (-w / 2) * -2 == w and wide > w
    assert p.D.tolist() == [D, D // 2]
    assert p.log2d.tolist() == [int(np.log2(D)), int(np.log2(D)) - 1]
    assert p.sample_rate.tolist() == [FS / D, FS / (D // 2)]
    # the default pad_f = 0.1 widens the band by 1.2: a box of 0.5 w keeps D, one of 0.9 w does not
    assert _plan([[0.01, -0.25 * w, 0.02, 0.25 * w], [0.01, -0.45 * w, 0.02, 0.45 * w]], fc=0.0).D.tolist() == [D, D // 2]


def test_decimation_limits_and_override():
    p = _plan([[0.01, -1.0, 0.02, 1.0], [0.01, -0.45 * FS, 0.02, 0.45 * FS], [0.01, 10.0, 0.02, 10.0]], fc=0.0)
    assert p.D.tolist() == [64, 1, 64]                                      # narrow: D stops at 64; wider than 0.84 fs / 2: none qualifies
    for d in (1, 2, 64):
        assert _plan([[0.01, -1.0, 0.02, 1.0], [0.01, -0.45 * FS, 0.02, 0.45 * FS]], fc=0.0, decimate=d).D.tolist() == [d, d]


def test_grid_is_anchored_at_sample_zero_and_clipped_to_the_capture():
    tf = [[0.0101234, FC - 2e4, 0.0205678, FC + 2e4],                       # D = 16, inside
          [0.0005, FC - 2e4, 0.003, FC + 2e4],                              # starts before sample 0 once pad_t is taken off
          [0.035, FC - 2e4, 0.05, FC + 2e4],                                # runs past the end
          [0.02, FC - 4e5, 0.0200001, FC + 4e5]]                            # D = 1
    p = _plan(tf, pad_t=0.001)
    assert p.D.tolist() == [16, 16, 16, 1]
    for k in range(4):
        D = int(p.D[k])
        first = int(np.floor((tf[k][0] - 0.001) * FS / D))
        last = int(np.ceil((tf[k][2] + 0.001) * FS / D))
        hi = (N - 1) // D
        assert p.m_first[k] == min(max(first, 0), hi) and p.m_first[k] + p.M[k] - 1 == min(max(last, 0), hi)
        assert p.t0[k] == p.m_first[k] * D / FS                             # the clip starts at exactly m_first D / fs seconds
    assert p.m_first[1] == 0 and p.t0[1] == 0.0
    assert (p.m_first[2] + p.M[2] - 1) * 16 <= N - 1 < (p.m_first[2] + p.M[2]) * 16
    assert p.offset.tolist() == np.concatenate(([0], np.cumsum(p.M))).tolist() and p.total == int(p.M.sum())
    assert p.rows.tolist() == [0, 1, 2, 3] and np.array_equal(p.tf, np.asarray(tf))
    q = _plan(tf, pad_t=0.001, rows=[2, 0])
    assert q.rows.tolist() == [2, 0] and q.M.tolist() == [p.M[2], p.M[0]] and q.offset.tolist() == [0, p.M[2], p.M[2] + p.M[0]]
    assert len(_plan(np.zeros((0, 4)))) == 0 and _plan(np.zeros((0, 4))).total == 0
    assert len(_plan(tf, rows=[])) == 0
    late = _plan([[1.0, FC - 2e4, 2.0, FC + 2e4]])                          # wholly past the end: the capture's last output
    assert late.M.tolist() == [1] and late.m_first.tolist() == [(N - 1) // 16]


def test_mixer_step_is_quantised_as_the_ddc_does_and_the_applied_centre_is_reported():
    from sy11.data.resample import plan_resample
    offs = [12345.678, -3.3e5, 0.0, 0.25 * FS, 1e-5]
    p = _plan([[0.01, FC + o - 1e3, 0.02, FC + o + 1e3] for o in offs])
    for k, o in enumerate(offs):
        centre = ((FC + o - 1e3) + (FC + o + 1e3)) / 2
        want = int(round(-(centre - FC) / FS * 2.0 ** 32)) % (1 << 32)
        assert p.dphi[k] == want
        ddc = plan_resample(FS, FS / int(p.D[k]), centre - FC)
        assert ddc.dphi == want and p.center_freq[k] == FC + ddc.shift_hz
        assert abs(p.center_freq[k] - centre) <= FS / 2.0 ** 33 + 1e-6     # + the float64 spacing at 2.4e9
    assert p.dphi[2] == 0 and p.center_freq[2] == FC and p.dphi[3] == 3 << 30 and p.dphi[4] == 0


# ------------------------------------------------------------------------------------------------------------- argument errors
def test_every_argument_error_is_a_value_error_before_the_device():
    from sy11.data.extract import MIN_CHUNK, plan_extract_chunks
    ok = [0.01, FC - 1e4, 0.02, FC + 1e4]
    for bad in ([np.nan, FC - 1e4, 0.02, FC + 1e4], [0.01, FC - 1e4, np.inf, FC + 1e4]):
        with pytest.raises(ValueError, match="not finite"):
            _plan([ok, bad])
    for bad in ([0.02, FC - 1e4, 0.01, FC + 1e4], [0.01, FC + 1e4, 0.02, FC - 1e4]):
        with pytest.raises(ValueError, match="box 1 is inverted"):
            _plan([ok, bad])
    for off in (0.51 * FS, -0.6 * FS):
        with pytest.raises(ValueError, match="outside the capture"):
            _plan([[0.01, FC + off - 1e3, 0.02, FC + off + 1e3]])
    for d in (3, 128, 0, -2, "fast", 2.0, True):
        with pytest.raises(ValueError, match="power of two"):
            _plan([ok], decimate=d)
    for rows in ([1], [-1], [0, 5], [0.5]):
        with pytest.raises(ValueError, match="rows"):
            _plan([ok], rows=rows)
    for kw in (dict(pad_t=-1.0), dict(pad_f=np.nan)):
        with pytest.raises(ValueError, match="pad_t and pad_f"):
            _plan([ok], **kw)
    full = _plan([ok, ok], decimate=1)
    with pytest.raises(ValueError, match=f"hold {full.total} samples.*rows="):
        _plan([ok, ok], decimate=1, max_samples=full.total - 1)
    assert _plan([ok, ok], decimate=1, max_samples=full.total).total == full.total
    assert MIN_CHUNK == 63 * 64 + 32 * 64 + 1 == 6081
    with pytest.raises(ValueError, match="chunk_samples"):
        plan_extract_chunks(full, MIN_CHUNK - 1)
    assert plan_extract_chunks(full, MIN_CHUNK)


# ------------------------------------------------------------------------------------------------------------- chunker
@pytest.fixture(scope="module")
def crowded():
    """About 200 random boxes on 3e6 samples: every D, overlaps, and durations up to 0.2 s (longer than the two small budgets)."""
    g = np.random.default_rng(5)
    n, k = 3_000_000, 200
    t0 = g.uniform(-0.01, n / FS, k)
    dur = g.choice([1e-4, 3e-3, 0.05, 0.2], k) * g.uniform(0.5, 1.0, k)
    bw = g.choice([5e3, 2e4, 1e5, 3e5, 6e5], k)
    fc = FC + g.uniform(-0.1, 0.1, k) * FS
    tf = np.stack((t0, fc - bw / 2, t0 + dur, fc + bw / 2), 1)
    tf[:3] = [0.5, FC - 2e3, 1.9, FC + 2e3]                                # three long, identical boxes
    return _plan(tf, n=n)


@pytest.mark.parametrize("chunk_samples", [6081, 50000, 1 << 24])
def test_chunks_cover_every_output_once_within_budget(crowded, chunk_samples):
    from sy11.data.extract import SEGMENT, plan_extract_chunks, support
    p = crowded
    assert {1, 2, 4, 32, 64} <= set(p.D.tolist())
    chunks = plan_extract_chunks(p, chunk_samples)
    seen = np.zeros(p.total, dtype=np.int32)
    pieces = np.zeros(len(p), dtype=np.int64)
    starts = []
    for ch in chunks:
        assert 0 <= ch.a < ch.b <= p.n and ch.b - ch.a <= chunk_samples
        assert ch.segments.dtype == SEGMENT and len(ch.segments) == len(ch.clip) > 0
        union = np.zeros(ch.b - ch.a, dtype=bool)
        for s, k in zip(ch.segments, ch.clip):
            assert s["log2d"] == p.log2d[k] and s["dphi"] == p.dphi[k] and s["M"] > 0
            assert p.m_first[k] <= s["m0"] and s["m0"] + s["M"] <= p.m_first[k] + p.M[k]
            assert s["out_off"] == p.offset[k] + s["m0"] - p.m_first[k]
            seen[s["out_off"]:s["out_off"] + s["M"]] += 1
            a, b = support(s["m0"], s["M"], s["log2d"], p.n)
            assert ch.a <= a < b <= ch.b                                    # the segment's clipped support lies inside its chunk
            union[a - ch.a:b - ch.a] = True
            pieces[k] += 1
        read = np.zeros(ch.b - ch.a, dtype=bool)
        for lo, hi in ch.reads:
            assert ch.a <= lo < hi <= ch.b and not read[lo - ch.a:hi - ch.a].any()
            read[lo - ch.a:hi - ch.a] = True
        assert np.array_equal(read, union)                                  # only the union of the supports is read from the source
        starts.append(ch.a)
    assert (seen == 1).all()                                                # every output of every clip exactly once
    assert starts == sorted(starts)
    long_rows = np.flatnonzero(p.M * p.D + 32 * p.D > chunk_samples)
    if chunk_samples < 1 << 24:
        assert len(long_rows) >= 3 and (pieces[long_rows] > 1).all()        # a box longer than the budget is split along m
        assert len(chunks) > 10
    else:
        assert (pieces == 1).all() and len(chunks) == 1                     # 3e6 samples fit one chunk: overlapping boxes share one copy


# ------------------------------------------------------------------------------------------------------------- prototype
@pytest.mark.parametrize("D", [2, 4, 8, 16, 32, 64])
def test_prototype_is_flat_to_042_and_80_db_down_from_058_of_the_output_rate(D):
    """What USABLE_BAND = 0.84 rests on, in float64: |H| within 0.01 dB for f <= 0.42 fs_out, <= -80 dB for f >= 0.58 fs_out (measured:
    0.427 and 0.5795), so everything that folds into |f| <= 0.42 fs_out is at least 80 dB down."""
    from sy11.data.resample import prototype
    h, c = prototype(1, D)
    assert h.shape[0] == 32 * D + 1 and c == 16 * D and abs(h.sum() - 1.0) < 1e-12
    L = 1 << 19
    H = np.abs(np.fft.rfft(h, L))
    f = np.arange(H.shape[0]) / L * D                                       # in units of fs_out
    db = 20 * np.log10(np.maximum(H, 1e-30))
    ripple, stop = np.abs(db[f <= 0.42]).max(), db[f >= 0.58].max()
    flat_to, down_from = f[np.argmax(np.abs(db) > 0.01)], f[len(f) - 1 - np.argmax(db[::-1] > -80.0)]
    print(f"prototype(1, {D}): ripple {ripple:.5f} dB to 0.42 fs_out (0.01 dB up to {flat_to:.4f}), stop band {stop:.2f} dB from 0.58 "
          f"(-80 dB from {down_from:.4f})")
    assert ripple <= 0.01 and stop <= -80.0


# ------------------------------------------------------------------------------------------------------------- tones
def test_reference_keeps_an_inband_tone_and_rejects_058_of_the_output_rate():
    """A tone inside the box comes out at f - centre_applied with its amplitude within 0.01 dB (and its phase: output m IS capture
    sample m D); a tone 0.58 fs / D from the centre is at least 80 dB down."""
    box = [0.012, FC + 1.0e5 - 2.5e4, 0.028, FC + 1.0e5 + 2.5e4]            # B = 60 kHz -> D = 8 (0.84 fs / 8 = 105 kHz, / 16 = 52.5 kHz)
    p = _plan([box])
    D = int(p.D[0])
    assert D == 8 and p.m_first[0] * D >= 16 * D and (p.m_first[0] + p.M[0] + 16) * D < N         # no edge of the capture in reach
    i = np.arange(N, dtype=np.float64)
    ca = p.center_freq[0]
    m = np.arange(p.m_first[0], p.m_first[0] + p.M[0], dtype=np.float64)
    for f_tone in (FC + 1.0e5 + 2.0e4, FC + 1.0e5 - 2.4e4, ca):
        x = np.exp(2j * np.pi * ((f_tone - FC) / FS) * i)
        y = E.plan_clip(x.astype(np.complex64), p, 0)
        want = np.exp(2j * np.pi * ((f_tone - ca) / FS) * m * D)
        gain = np.vdot(want, y) / len(y)
        print(f"tone at centre {f_tone - ca:+.1f} Hz: {20 * np.log10(abs(gain)):+.5f} dB, phase {np.angle(gain):+.2e} rad, "
              f"worst sample off by {np.abs(y - want).max():.2e}")
        assert abs(20 * np.log10(abs(gain))) <= 0.01 and abs(np.angle(gain)) < 1e-4
        assert np.abs(y - want).max() < 2e-3
    x = np.exp(2j * np.pi * ((ca + 0.58 * FS / D - FC) / FS) * i)
    y = E.plan_clip(x.astype(np.complex64), p, 0)
    level = 20 * np.log10(np.abs(y).max())
    print(f"tone at centre + 0.58 fs / D: {level:.2f} dB")
    assert level <= -80.0


# ------------------------------------------------------------------------------------------------------------- save
def test_save_round_trips_bit_exactly_through_open_iq(tmp_path):
    from sy11.data.extract import Extraction
    from sy11.data.spectrogram import open_iq
    p = _plan([[0.010, FC - 2e4, 0.012, FC + 2e4], [0.02, FC + 1e5, 0.0201, FC + 4e5], [0.03, FC - 1e3, 0.03, FC + 1e3]], rows=[2, 0, 1])
    g = np.random.default_rng(2)
    packed = torch.from_numpy((g.standard_normal(p.total) + 1j * g.standard_normal(p.total)).astype(np.complex64))
    ex = Extraction(p, packed, cls=np.array([1, 0, 1]), conf=np.array([0.5, 0.25, 0.75]), names={0: "a", 1: "b"})
    assert len(ex) == 3 and [len(c) for c in ex.samples] == p.M.tolist() and ex[1] is ex.samples[1]
    assert ex.rows.tolist() == [2, 0, 1] and ex.decimation is p.D and ex.plan is p
    out = ex.save(tmp_path / "clips")
    meta = json.loads((tmp_path / "clips" / "clips.json").read_text())
    assert meta["capture"] == {"samples": N, "sample_rate": FS, "center_freq": FC} and len(meta["clips"]) == 3
    for k, c in enumerate(meta["clips"]):
        assert c["file"] == f"clip_{p.rows[k]}.cf32" and c["row"] == p.rows[k] and c["samples"] == p.M[k]
        got = open_iq(str(tmp_path / "clips" / c["file"]))
        assert got.dtype == np.complex64 and np.array_equal(np.asarray(got).view(np.uint32), ex[k].numpy().view(np.uint32))
        assert c["sample_rate"] == p.sample_rate[k] and c["center_freq"] == p.center_freq[k] and c["t0"] == p.t0[k]
        assert c["decimation"] == p.D[k] and c["tf"] == p.tf[k].tolist()
        assert c["class"] == [1, 0, 1][k] and c["name"] == {0: "a", 1: "b"}[c["class"]] and c["confidence"] == [0.5, 0.25, 0.75][k]
    assert str(out) == str(tmp_path / "clips")
