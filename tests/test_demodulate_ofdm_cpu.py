"""CPU: the plan of the OFDM demodulation (argument errors, the per-clip reasons, the item tables of launch 1), its two host fits on synthetic rows against the independent
reference of tests/_ofdm_ref.py, and the seed check of the GPU tests: the reference ALONE demodulates the parity cases and the three bursts of the end-to-end test with no
symbol error on the active OFDM symbols and the prefix found to within 2 samples."""
import math

import numpy as np
import pytest

from tests import _ofdm_ref as R

A = R.LAYOUT_A
KW = dict(n_fft=64, cp=16, carriers=A["data"], pilots=(A["pk"], A["pc"]))


def _plan(M, fs=R.FS, **kw):
    from sy11.data.demodulate_ofdm import plan_demodulate_ofdm
    a = dict(KW)
    a.update(kw)
    return plan_demodulate_ofdm((M, fs), **a)


def test_argument_errors_are_value_errors_raised_by_the_plan():
    bad = (dict(n_fft=96), dict(n_fft=2048), dict(n_fft=64.0), dict(n_fft=True), dict(cp=0), dict(cp=33), dict(cp=1.5), dict(advance=-1), dict(advance=17),
           dict(carriers=[]), dict(carriers=[1, 1, 2]), dict(carriers=[32]), dict(carriers=[-32]), dict(carriers=[1.5]), dict(carriers=np.zeros((2, 2), dtype=np.int64)),
           dict(carriers=[1, 2, 7]), dict(pilots={7: 1}), dict(pilots={7: 1, 21: 2}), dict(pilots={-21: 1, -7: 1, 8: 1}), dict(pilots=([7, 21], [1])),
           dict(pilots={7: 1, 40: 1}), dict(pilots=5), dict(order="x"), dict(order=[4, 4, 4]), dict(order=None), dict(offset=[0.0] * 3), dict(offset=math.nan),
           dict(spacing=0.0), dict(spacing=-1.0), dict(spacing=[1.0] * 5))
    for kw in bad:
        with pytest.raises(ValueError, match="plan_demodulate_ofdm"):
            _plan([1000, 2000], **kw)
    from sy11.data.demodulate_ofdm import plan_demodulate_ofdm
    for clips in (5, ([-1], 1e6), ([1.5], 1e6), ([10], 0.0), ([10], [1e6, 1e6]), ([2 ** 31], 1e6)):
        with pytest.raises(ValueError, match="plan_demodulate_ofdm"):
            plan_demodulate_ofdm(clips, **KW)


def test_reasons_layouts_and_the_split_rule():
    from sy11.data.demodulate_ofdm import FOLD_PERIODS, FOLD_TILE
    p = _plan([64 + 2 * 80, 64 + 2 * 80 - 1, 3160, 1000, 1000, 1000], order=[4, 4, 2, 3, 4, 4], offset=[0, 0, 0, 0, 5e5, 0],
              spacing=[R.FS / 64] * 5 + [R.FS / 64 * (1 + 2e-6)])
    assert p.valid.tolist() == [True, False, True, False, False, False] and p.reason.tolist() == ["", "short", "", "order", "offset", "rate"]
    assert _plan([1000], spacing=R.FS / 64 * (1 + 5e-7)).valid.all() and _plan([1000], offset=-499999.0).valid.all()
    assert len(p.layouts) == 1 and p.periods.tolist() == [2, 0, 38, 0, 0, 0] and p.splits.tolist() == [1, 0, 3, 0, 0, 0] and p.tiles.tolist() == [2, 0, 2, 0, 0, 0]
    lay = p.layouts[0]
    assert (lay.n_fft, lay.cp, lay.S, lay.advance, lay.d, lay.n_data, lay.n_pil, lay.n_used, lay.group) == (64, 16, 80, 4, 14, 48, 4, 52, 16)
    assert lay.used.tolist() == [k for k in range(-26, 27) if k] and lay.bins["pil"][lay.pilot_idx].tolist() == [1, 2, 3, -4] and not lay.bins["pil"][lay.data_idx].any()
    it = p.items()
    assert it.shape == (2 + 6,) and p.total_triples == 80 + 3 * 80
    assert it["r0"].tolist() == [0, 64] * 4 and it["cnt_r"].tolist() == [64, 16] * 4 and it["m0"].tolist() == [0, 0, 0, 0, 16, 16, 32, 32]
    assert it["cnt_m"].tolist() == [2, 2, 16, 16, 16, 16, 6, 6] and it["out_off"].tolist() == [0, 64, 80, 144, 160, 224, 240, 304]
    assert FOLD_TILE == 64 and FOLD_PERIODS == 16
    # the rule depends on the clip alone: the same clip alone in a call has the same items (but for where the clip and its rows lie)
    alone = _plan([3160], order=2).items()
    for key in ("len", "n_fft", "S", "r0", "cnt_r", "m0", "cnt_m"):
        assert alone[key].tolist() == it[key][2:].tolist()
    # one layout per clip, as lists
    q = _plan([1000, 3000], n_fft=[64, 256], cp=[16, 18], carriers=[A["data"], np.arange(1, 9)], pilots=[dict(zip(A["pk"].tolist(), A["pc"].tolist())), ([-5, 10], [1, -1])],
              advance=[None, 18])
    assert len(q.layouts) == 2 and q.layout.tolist() == [0, 1] and q.layouts[1].d == 15 and q.layouts[1].advance == 18 and q.bin0.tolist() == [0, 52, 62]
    with pytest.raises(ValueError, match="neither one value nor one per clip"):
        _plan([1000, 3000], n_fft=[64, 256, 64])
    assert len(_plan(np.zeros(0, dtype=np.int64))) == 0


def test_the_host_fits_equal_the_reference_on_synthetic_rows():
    from sy11.data import demodulate_ofdm as D
    g = np.random.default_rng(5)
    lay = D.make_layout(64, 16, A["data"], (A["pk"], A["pc"]))
    part = g.standard_normal((3, 80, 3))
    part[:, :, 2] = np.abs(part[:, :, 2]) + 1.0
    part[:, 23:39, :2] += 4.0 * np.array([math.cos(1.0), math.sin(1.0)])      # a prefix at 23 with eps = 1 / 2 pi
    F, E = D.fold_rows(part)
    assert np.array_equal(F, ((part[0] + part[1]) + part[2])[:, 0] + 1j * ((part[0] + part[1]) + part[2])[:, 1]) and np.array_equal(E, ((part[0] + part[1]) + part[2])[:, 2])
    f, want = D.fit1(F, E, 64, 16), R.fit1(F, E, 64, 16)
    assert f["theta"] == want["theta"] == 23 and abs(f["eps"] - want["eps"]) <= 1e-14 and abs(f["cp_corr"] - want["cp_corr"]) <= 1e-14 and abs(f["eps"] - 1 / (2 * np.pi)) < 0.02
    # an offset of 3.25 carrier spacings is taken off the angle; a whole number of spacings leaves it alone
    assert abs(D.fit1(F, E, 64, 16, 3.25 / 64)["eps"] - (f["eps"] - 0.25)) <= 1e-12 and abs(D.fit1(F, E, 64, 16, 3.0 / 64)["eps"] - f["eps"]) <= 1e-12
    z = D.fit1(np.zeros(80, dtype=np.complex128), np.zeros(80), 64, 16)
    assert (z["theta"], z["eps"], z["cp_corr"]) == (0, 0.0, 0.0)
    assert D.carrier_word(0.0, 0.25, 64) == 1 << 56 and D.carrier_word(-1.0 / 128, 0.0, 64) == (1 << 64) - (1 << 57) and D.carrier_word(0.0, 0.0, 64) == 0
    # the OFDM symbols: every integer m, negative included
    for theta, M in ((0, 1000), (5, 1000), (70, 1000), (79, 64 + 2 * 80), (67, 64 + 2 * 80), (68, 64 + 2 * 80)):
        st = R.starts(theta, M, A)
        assert D.symbol_starts(theta, M, lay) == (int(st[0]), len(st)), (theta, M)
    assert D.symbol_starts(70, 1000, lay)[0] == 2                             # 70 + 16 - 4 - 80: m = -1
    # the pilot fit
    u = (g.standard_normal((9, 4)) + 1j * g.standard_normal((9, 4))) * 0.05 + np.exp(1j * (0.7 + 0.02 * A["pk"]))[None, :] * 3.0
    u[6:] *= 0.01                                                             # three OFDM symbols without signal
    f, want = D.fit2(u, lay), R.fit2(u, A)
    assert f["active"].tolist() == want["active"].tolist() == [True] * 6 + [False] * 3 and abs(f["beta"] - 0.02) < 2e-3
    for key in ("beta", "A"):
        assert abs(f[key] - want[key]) <= 1e-13 * abs(want[key])
    for key in ("z", "phi", "rho", "tau"):
        assert np.abs(f[key] - want[key]).max() <= 1e-12 * np.abs(want[key]).max(), key
    zero = D.fit2(np.zeros((4, 4), dtype=np.complex128), lay)
    assert zero["A"] == 0.0 and zero["beta"] == 0.0 and not zero["rho"].any() and zero["active"].all() and np.isfinite(zero["tau"]).all()
    tw = D.twiddle_table()
    assert tw.shape == (512,) and np.abs(tw - np.exp(-2j * np.pi * np.arange(512) / 1024)).max() < 1e-15


def test_the_reference_alone_reads_the_parity_cases_without_a_symbol_error():
    cs, ref = R.case_clips(), R.case_reference()
    assert [c["kind"] for c in cs] == ["ofdm"] * 8 + ["short", "rate", "order", "zero"]
    for c, r in zip(cs[:8], ref[:8]):
        bad, exact, miss = R.symbol_errors(r["dec"], r["active"], r["starts"], c)
        z = np.abs(r["z"]) / np.abs(r["z"]).max()
        print(f"{c['label']}: theta {r['theta']} ({miss} off), eps {r['eps']:+.4f} (sent {c['eps']:+.2f}), cp_corr {r['cp_corr']:.3f}, beta {r['beta']:+.4f}, {len(r['starts'])} OFDM symbols, "
              f"{int(r['active'].sum())} active (smallest {z[r['active']].min():.2f}, largest inactive {z[~r['active']].max(initial=0):.2f}), {bad} symbol errors, evm {r['evm']:.3f}")
        assert bad == 0 and exact and miss <= 2 and abs(r["eps"] - c["eps"]) < 0.02
        # no decision of the reference sits within the GPU test's bar of a boundary on an active symbol
        comp = np.abs(r["r"][r["active"]].real) if c["order"] == 2 else np.minimum(np.abs(r["r"][r["active"]].real), np.abs(r["r"][r["active"]].imag))
        assert comp.min() > 2.0 ** -22
    assert len(ref[2]["starts"]) > 32 and len(ref[2]["starts"]) % 16                # two full groups of 16 and a ragged one
    z = ref[11]
    assert z["gain"] == 0.0 and not z["r32"].any() and not z["dec"].any() and z["cp_corr"] == 0.0 and z["theta"] == 0 and ref[8] is None


def test_the_reference_alone_reads_the_three_bursts_of_the_end_to_end_test():
    from tests import test_demodulate_ofdm_gpu as G
    for which in range(3):
        b = G.burst(which)
        x = G.extract_model(b["x"], 0.0, 0, len(b["x"]) // G.DECIMATE)
        r = R.demodulate(x.astype(np.complex64), A, b["order"])
        c = {"lay": A, "lead": G.LEAD // G.DECIMATE, "n_ofdm": b["dec"].shape[0], "dec": b["dec"]}
        bad, exact, miss = R.symbol_errors(r["dec"], r["active"], r["starts"], c)
        print(f"burst {which}: theta {r['theta']} ({miss} off), eps {r['eps']:+.4f}, {bad} symbol errors on {int(r['active'].sum())} active OFDM symbols, evm {r['evm']:.3f}")
        assert bad == 0 and exact and miss <= 2 and abs(r["eps"] - G.EPS) < 0.02
