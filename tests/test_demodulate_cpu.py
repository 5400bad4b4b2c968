"""CPU: the host side of ``demodulate`` (sy11.data.demodulate) against the float64 reference of tests/_demod_ref.py — the plan's arithmetic
(every ``ValueError``, every ``reason``, tile and block counts at both sides of a boundary, Ws / Wc and the tap packing), the host stages
``fit``, ``phase_track`` and ``columns`` on reference-made tables to 1e-12 — and the algorithm itself: the reference alone recovers the
transmitted symbols of every clip the GPU tests use with ZERO errors, up to one of the ``order`` rotations and a shift of at most one symbol,
and its smallest decision margin on them is far above the 2^-20 |s| below which the GPU test exempts a decision."""
import math
from types import SimpleNamespace

import numpy as np
import pytest

from tests import _demod_ref as R

FS = 1.0e6


class _Char(SimpleNamespace):
    """What ``plan_demodulate`` reads of a ``Characterization``."""

    def __len__(self):
        return len(self.order)


@pytest.fixture(scope="module")
def chains():
    """The reference chain of every valid shared clip, computed once and left unchanged."""
    out = []
    for c in R.case_clips():
        p = R.plan(len(c["x"]), c["fs"], c["rate"], c["offset"], c["order"], R.SPAN)
        out.append((c, p, R.demodulate(c["x"], c["fs"], c["rate"], c["offset"], c["order"], fc=2.4e9, span=R.SPAN) if p["valid"] else None))
    return out


# ------------------------------------------------------------------------------------------------------------- plan
def test_every_argument_error_is_a_value_error():
    from sy11.data.demodulate import plan_demodulate
    good = dict(symbol_rate=3.0e5, offset=1.0e3, order=2)
    clips = ([4000, 5000], FS)
    plan_demodulate(clips, **good)
    char = _Char(order=np.array([2, 4]), symbol_rate=np.array([3e5, 3e5]), offset2=np.zeros(2), offset4=np.zeros(2), keyed=np.ones(2, dtype=bool),
                 valid=np.ones(2, dtype=bool))
    plan_demodulate(clips, char)
    for kw in (dict(), dict(symbol_rate=3e5), dict(symbol_rate=3e5, offset=0.0), dict(offset=0.0, order=2)):          # neither source, or half of one
        with pytest.raises(ValueError, match="characterization"):
            plan_demodulate(clips, **kw)
    for kw in (good, dict(order=2), dict(symbol_rate=3e5)):                                                          # both sources
        with pytest.raises(ValueError, match="not both"):
            plan_demodulate(clips, char, **kw)
    with pytest.raises(ValueError, match="characterization of 2"):
        plan_demodulate(([4000, 5000, 6000], FS), char)
    for key, n in (("symbol_rate", 3), ("offset", 3), ("order", 3)):                                                 # lengths that do not match
        with pytest.raises(ValueError, match=key):
            plan_demodulate(clips, **dict(good, **{key: [2] * n}))
    with pytest.raises(ValueError, match="sample_rate"):
        plan_demodulate(([4000, 5000], [FS, FS, FS]), **good)
    for bad in (dict(beta=0.0), dict(beta=1.01), dict(beta=-0.1), dict(beta=float("nan")), dict(span=1), dict(span=17), dict(span=8.0), dict(span=True),
                dict(block=7), dict(block=257), dict(block=32.0)):
        with pytest.raises(ValueError, match=next(iter(bad))):
            plan_demodulate(clips, **good, **bad)
    for ok in (dict(beta=1.0), dict(beta=1e-3), dict(span=2), dict(span=16), dict(block=8), dict(block=256)):          # the bounds themselves are inside
        plan_demodulate(clips, **good, **ok)
    for bad_clips in (([4000.5], FS), ([-1], FS), ([4000], 0.0), ([4000], float("inf")), ([2 ** 31], FS), 7, ([[1, 2]], FS)):
        with pytest.raises(ValueError):
            plan_demodulate(bad_clips, **good)
    with pytest.raises(ValueError, match="integers"):
        plan_demodulate(clips, symbol_rate=3e5, offset=0.0, order=2.5)


def test_every_reason_and_both_sides_of_every_boundary():
    from sy11.data.demodulate import plan_demodulate, tile
    T = tile()
    assert T == R.TILE == 512
    span = 8
    # (M, rate, offset, order) -> reason
    hw33 = math.ceil(span * 3.3)
    rows = [
        (4000, FS / 3.3, 0.0, 2, ""), (4000, FS / 3.3, 0.0, 4, ""),
        (4000, FS / 3.3, 0.0, 0, "order is not 2 or 4"), (4000, FS / 3.3, 0.0, -1, "order is not 2 or 4"), (4000, FS / 3.3, 0.0, 8, "order is not 2 or 4"),
        (4000, float("nan"), 0.0, 2, "rate or offset not finite"), (4000, FS / 3.3, float("inf"), 2, "rate or offset not finite"),
        (4000, 0.0, 0.0, 2, "rate or offset not finite"),
        (4000, FS / 2.5, 0.0, 2, ""), (4000, FS / 2.4999, 0.0, 2, "samples per symbol outside [2.5, 16]"),
        (9000, FS / 16.0, 0.0, 2, ""), (9000, FS / 16.001, 0.0, 2, "samples per symbol outside [2.5, 16]"),
        (4000, FS / 3.3, np.nextafter(FS / 2, 0), 2, ""), (4000, FS / 3.3, FS / 2, 2, "offset beyond fs / 2"), (4000, FS / 3.3, -FS / 2, 4, "offset beyond fs / 2"),
        (2 * hw33 + T, FS / 3.3, 0.0, 2, ""), (2 * hw33 + T - 1, FS / 3.3, 0.0, 2, "too short"), (0, FS / 3.3, 0.0, 2, "too short"),
        (2 * hw33 + T + 1, FS / 3.3, 0.0, 2, ""), (2 * hw33 + 2 * T, FS / 3.3, 0.0, 2, ""),
    ]
    M, rate, off, order, reason = (list(v) for v in zip(*rows))
    p = plan_demodulate((M, FS), symbol_rate=rate, offset=off, order=order, span=span)
    assert p.reason.tolist() == reason and p.valid.tolist() == [r == "" for r in reason]
    ref = [R.plan(m, FS, r, o, k, span) for m, r, o, k in zip(M, rate, off, order)]
    assert [r["reason"] for r in ref] == reason
    for i, r in enumerate(ref):
        if r["valid"]:
            assert (int(p.hw[i]), int(p.n_taps[i]), int(p.tiles[i]), p.Ws[i], p.Wc[i]) == (r["hw"], r["n_taps"], r["tiles"], r["Ws"], r["Wc"]) and p.sps[i] == r["sps"]
        else:
            assert (int(p.hw[i]), int(p.n_taps[i]), int(p.tiles[i]), p.Ws[i], p.Wc[i]) == (0, 0, 0, 0, 0) and np.isnan(p.sps[i])
    assert p.tiles[-5:].tolist() == [1, 0, 0, 2, 2] and p.total_rows == int(p.tiles.sum()) and p.row0.tolist() == np.concatenate(([0], np.cumsum(p.tiles))).tolist()
    # a characterisation: its order, its rate, offset2 / offset4 by order; not keyed or not valid is a reason
    c = _Char(order=np.array([2, 4, 2, 0, -1]), symbol_rate=np.full(5, FS / 3.3), offset2=np.full(5, 1.0e3), offset4=np.full(5, -2.0e3),
              keyed=np.array([True, True, False, False, False]), valid=np.array([True, True, True, True, False]))
    q = plan_demodulate(([4000] * 5, FS), c)
    assert q.reason.tolist() == ["", "", "not keyed", "order is not 2 or 4", "order is not 2 or 4"] and q.carrier_offset[:2].tolist() == [1.0e3, -2.0e3]
    assert q.Wc[0] == int(math.ldexp(1.0e3 / FS, 64)) and q.Wc[1] == (1 << 64) + int(math.ldexp(-2.0e3 / FS, 64)) and q.Wc[2:] == [0, 0, 0]


def test_items_and_tap_packing_match_the_reference():
    from sy11.data.demodulate import BLOCK, DEC, ITEM, plan_demodulate
    assert (ITEM.itemsize, BLOCK.itemsize, DEC.itemsize) == (72, 56, 40)                    # sy11_demod_item / _block / _dec
    cs = R.case_clips()
    M = [len(c["x"]) for c in cs]
    p = plan_demodulate((M, [c["fs"] for c in cs]), symbol_rate=[c["rate"] for c in cs], offset=[c["offset"] for c in cs], order=[c["order"] for c in cs],
                        span=R.SPAN)
    ref = [R.plan(len(c["x"]), c["fs"], c["rate"], c["offset"], c["order"], R.SPAN) for c in cs]
    assert p.valid.tolist() == [False, True, True, True, True, False] and [r["valid"] for r in ref] == p.valid.tolist()
    assert p.reason[0] == "order is not 2 or 4" and p.reason[5] == "too short" and M[5] == 2 * math.ceil(R.SPAN * cs[5]["fs"] / cs[5]["rate"]) + 300
    assert p.n_taps.tolist() == [0, 107, 237, 83, 513, 0] and p.tiles.tolist() == [0, 3, 16, 6, 17, 0]
    assert [int(o) % 2 for o in p.offset] == [0, 1, 1, 1, 1, 1]                               # every clip but the first starts at an odd sample
    assert p.tap_off.tolist() == [0, 0, 107, 344, 427, 940, 940] and p.taps.dtype == np.float32 and p.taps.shape == (940,)
    it, clip = p.items()
    assert clip.tolist() == [1] * 3 + [2] * 16 + [3] * 6 + [4] * 17 and it["row"].tolist() == list(range(42))
    for i, r in enumerate(ref):
        if not r["valid"]:
            continue
        h = R.taps(r["sps"], r["hw"])
        got = p.taps[int(p.tap_off[i]):int(p.tap_off[i + 1])]
        assert np.array_equal(got, h) and abs(float(np.sum(h.astype(np.float64) ** 2)) - 1.0) < 1e-6 and np.array_equal(h, h[::-1])
        mine = it[clip == i]
        bounds = R.tile_bounds(M[i], r["hw"])
        assert mine["n0"].tolist() == [a for a, _ in bounds] and mine["cnt"].tolist() == [b - a for a, b in bounds]
        assert mine["first"].tolist() == [1] + [0] * (len(bounds) - 1) and mine["last"].tolist() == [0] * (len(bounds) - 1) + [1]
        assert set(mine["wc"].tolist()) == {r["Wc"]} and set(mine["ws"].tolist()) == {r["Ws"]} and set(mine["hw"].tolist()) == {r["hw"]}
        assert set(mine["off"].tolist()) == {int(p.offset[i])} and set(mine["len"].tolist()) == {M[i]} and set(mine["tap_off"].tolist()) == {int(p.tap_off[i])}
        assert np.array_equal(p.centres(i), np.array([(a + b - 1) / 2.0 for a, b in bounds]))
    assert 0 < it["cnt"][clip == 3][-1] < 512                                                # the ragged last tile
    assert ref[2]["Wc"] > 1 << 63                                                            # a negative offset wraps


# ------------------------------------------------------------------------------------------------------------- host stages
def _close(a, b, tol=1e-12):
    return a == b or abs(a - b) <= tol * max(abs(b), 1.0)


def test_host_stages_match_the_reference_on_reference_made_tables(chains):
    from sy11.data import demodulate as P
    for c, p, r in chains:
        if r is None:
            continue
        M, hw, order = len(c["x"]), p["hw"], c["order"]
        centres = np.array([(a + b - 1) / 2.0 for a, b in R.tile_bounds(M, hw)])
        for k in (len(centres), 2, 1):                                                           # the line, and the two short forms (a = 0)
            rows, Mk = r["timing_rows"][:k], M if k == len(centres) else 2 * hw + 512 * k
            f = P.fit(rows[:, 0] + 1j * rows[:, 1], centres[:k], p["Ws"], Mk, hw)
            want = R.fit(rows, Mk, hw, p["Ws"])
            assert (f["a"] == 0.0) == (len(rows) < 3)
            for key in ("a", "c", "sps", "timing"):
                assert _close(f[key], want[key]), (c["label"], key, f[key], want[key])
            assert np.allclose(f["psi"], want["psi"], rtol=0, atol=1e-12)
            if len(rows) == len(centres):                                                        # the integers: no tolerance
                assert (f["T0"], f["STEP"], f["i_first"], f["i_last"], f["n_symbols"]) == (want["T0"], want["STEP"], want["i_first"], want["i_last"], want["n_symbols"])
                k_first, k_last = (f["T0"] + f["i_first"] * f["STEP"]) >> 32, (f["T0"] + f["i_last"] * f["STEP"]) >> 32
                assert hw + 1 <= k_first and k_last <= M - hw - 3
                assert ((f["T0"] + (f["i_first"] - 1) * f["STEP"]) >> 32) < hw + 1 and ((f["T0"] + (f["i_last"] + 1) * f["STEP"]) >> 32) > M - hw - 3
        theta = P.phase_track(r["z_rows"][:, 0] + 1j * r["z_rows"][:, 1], order)
        assert np.allclose(theta, r["theta"], rtol=0, atol=1e-12) and np.abs(np.diff(theta)).max() < np.pi / order
        n = r["n_symbols"]
        assert np.array_equal(P.block_centres(n, 32), R.centres(n, 32))
        rows = R.block_rows(r["r"], r["d"], order, 32)
        rate_fit = c["fs"] / r["sps"]
        got = P.columns(rows, theta, P.block_centres(n, 32), rate_fit, 2.4e9 + c["offset"])
        want = R.columns(rows, r["theta"], n, 32, rate_fit, 2.4e9 + c["offset"])
        assert got["n_symbols"] == want["n_symbols"] == n
        for key in ("gain", "evm", "mer_db", "carrier_fit"):
            assert _close(got[key], want[key]), (c["label"], key, got[key], want[key])
    # block counts and centres at both sides of a boundary
    for n, want in ((31, [15.0]), (32, [15.5]), (33, [15.5, 32.0]), (64, [15.5, 47.5]), (65, [15.5, 47.5, 64.0]), (8, [3.5]), (9, [3.5, 8.0])):
        block = 8 if n < 10 else 32
        assert P.block_centres(n, block).tolist() == want and R.centres(n, block).tolist() == want and len(R.blocks(n, block)) == len(want)
    # the unwraps move by whole periods towards the entry before
    assert np.allclose(P.phase_track(np.exp(1j * 4 * np.array([0.1, 0.7, 1.3, 1.9])), 4), [0.1, 0.7, 1.3, 1.9], atol=1e-12)
    assert np.allclose(P.phase_track(-np.exp(1j * 2 * np.array([3.0, 3.3, 3.6])), 2), np.array([3.0, 3.3, 3.6]) - np.pi / 2, atol=1e-12)
    one = P.columns(np.array([[2.0, 2.0, 2.0]]), np.array([0.3]), np.array([0.5]), 1.0e5, 7.0)
    assert one["carrier_fit"] == 7.0 and one["gain"] == 1.0 and one["evm"] == 0.0 and one["mer_db"] == float("inf")


# ------------------------------------------------------------------------------------------------------------- the algorithm
def test_the_reference_recovers_every_shared_clip_without_a_symbol_error(chains):
    seen = 0
    for c, p, r in chains:
        if r is None:
            continue
        seen += 1
        k0 = (r["T0"] + r["i_first"] * r["STEP"]) / 2.0 ** 32
        bad, rot, shift = R.errors(r["r"], c["order"], k0, c["sps"], c["a"], c["u0"])
        rel = float((r["margin"] / np.abs(r["s"]).astype(np.float64)).min())
        print(f"{c['label']}: {r['n_symbols']} symbols in {len(r['theta'])} blocks, {r['tiles']} tiles, {bad} errors (rotation {rot}, shift {shift}), evm {r['evm']:.4f}, "
              f"smallest margin {float(r['margin'].min()) / r['gain']:.3f} of the gain = {rel:.3f} |s|, largest phase step {np.abs(np.diff(r['theta'])).max():.3f} rad, "
              f"rate {(r['symbol_rate_fit'] - c['true_rate']) / c['fs'] * 1024:+.4f} bins")
        assert bad == 0
        assert rel > 1000 * 2.0 ** -20                                     # the GPU test exempts decisions below 2^-20 |s|: none is near
        assert abs(r["symbol_rate_fit"] - c["true_rate"]) < 0.25 * c["fs"] / 1024       # the fit takes back the 1/4 bin the rate was handed over with
        assert abs(r["carrier_fit"] - 2.4e9 - c["true_offset"]) < c["fs"] / 1024 / 16
        assert r["n_symbols"] % 32 != 0 or c["label"] != "qpsk 2.5"        # the ragged last block
    assert seen == 4


@pytest.mark.parametrize("kind,order", [("bpsk", 2), ("qpsk", 4)])
def test_the_reference_recovers_the_embedded_emissions_of_the_end_to_end_test(kind, order):
    """3.3 samples per symbol, 8 400 samples, 37.3 bins off the centre, the rate 1/4 bin off and the offset 1/16 bin off, default span and block."""
    x, a, u0 = R.clip(kind, 8400, 20 + order, 3.3, 37.3 / 1024, 20.0)
    r = R.demodulate(x, FS, (1 / 3.3 - 0.25 / 1024) * FS, (37.3 + 1 / 16) / 1024 * FS, order)
    k0 = (r["T0"] + r["i_first"] * r["STEP"]) / 2.0 ** 32
    bad, rot, shift = R.errors(r["r"], order, k0, 3.3, a, u0)
    print(f"{kind}: {r['n_symbols']} symbols, {bad} errors (rotation {rot}, shift {shift}), evm {r['evm']:.4f}")
    assert bad == 0 and abs(r["symbol_rate_fit"] - FS / 3.3) < 0.25 * FS / 1024


def test_an_extraction_without_a_valid_clip_launches_nothing():
    import torch
    from sy11 import _lib
    from sy11.data.demodulate import Demodulation, demodulate_extraction
    Ms = np.array([100, 300], dtype=np.int64)
    off = np.concatenate(([0], np.cumsum(Ms))).astype(np.int64)
    ext = SimpleNamespace(plan=SimpleNamespace(M=Ms, offset=off), packed=torch.zeros(400, dtype=torch.complex64), sample_rate=np.full(2, FS),
                          center_freq=np.full(2, 2.4e9), rows=np.arange(2), cls=np.array([0, 1]), conf=np.array([0.5, 0.6]), names={0: "a", 1: "b"})
    _lib.PROFILE = []
    try:
        d = demodulate_extraction(ext, symbol_rate=FS / 3.3, offset=0.0, order=[2, 0])
        calls = list(_lib.PROFILE)
    finally:
        _lib.PROFILE = None
    assert isinstance(d, Demodulation) and calls == [] and len(d) == 2 and not d.valid.any() and d.reason.tolist() == ["too short", "order is not 2 or 4"]
    assert d.n_symbols.tolist() == [-1, -1] and np.isnan(d.evm).all() and d.phase_ambiguity.tolist() == [-1, -1] and d.symbols[0].shape == (0,)
    assert d[0]["reason"] == "too short" and d.bits(0).shape == (0,)
    with pytest.raises(ValueError):
        demodulate_extraction(ext, symbol_rate=FS / 3.3, offset=0.0, order=2, block=7)
