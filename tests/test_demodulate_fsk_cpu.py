"""CPU: the host side of ``demodulate_fsk`` (sy11.data.demodulate_fsk) against the float64 reference of tests/_fsk_ref.py — the taps against their
closed forms, the plan's arithmetic on literals (tiles, hw, Ws / Wc, every ``ValueError``, every ``reason``), ``mean_and_line`` and ``level_fit`` on hand-made
rows, ``save`` on a hand-built result, the refusals of the three C entries that need no GPU — and the algorithm itself: the reference alone reads every
shared clip with ZERO bit errors up to polarity, no sample of them is within 1e-9 of the discriminator's wrap, and no symbol is within 2^-20 of
the decision boundary, so that the GPU test can ask for equal decisions everywhere."""
import ctypes as C
import json
import math
from types import SimpleNamespace

import numpy as np
import pytest

from tests import _fsk_ref as R

FS = 1.0e6


# ------------------------------------------------------------------------------------------------------------- taps
def test_taps_against_the_closed_forms():
    from sy11.data.demodulate_fsk import half_width, make_taps
    # rect at 4 samples per symbol: the symbol [-2, 2] covers the samples -1, 0, 1 and half of -2 and 2
    assert half_width(4.0, "rect", 7) == 2 and make_taps(4.0, 2, "rect").tolist() == [0.125, 0.25, 0.25, 0.25, 0.125]
    # rect at 2.5: [-1.25, 1.25] covers 0, 3/4 of -1 and 1, nothing of -2 and 2
    assert half_width(2.5, "rect", 1) == 2 and np.array_equal(make_taps(2.5, 2, "rect"), np.array([0.0, 0.3, 0.4, 0.3, 0.0], dtype=np.float32))
    assert half_width(16.0, "rect", 1) == 8 and half_width(8.37, "gauss", 2) == 17 and half_width(16.0, "gauss", 16) == 256
    for sps, pulse, bt, span in ((4.0, "gauss", 0.5, 2), (8.37, "gauss", 0.3, 2), (16.0, "gauss", 0.5, 16), (2.5, "rect", 0.5, 2), (5.3, "rect", 0.5, 2)):
        hw = half_width(sps, pulse, span)
        h, want = make_taps(sps, hw, pulse, bt), R.taps(sps, hw, pulse, bt)
        assert h.dtype == np.float32 and h.shape == (2 * hw + 1,) and np.array_equal(h, want) and np.array_equal(h, h[::-1])
        assert abs(float(h.astype(np.float64).sum()) - 1.0) < 1e-6
    # the Gaussian on one literal: h[k] / h[0] = exp(-2 pi^2 bt^2 (k / sps)^2 / ln 2)
    h = make_taps(4.0, 8, "gauss", 0.5).astype(np.float64)
    assert abs(h[8 + 4] / h[8] - math.exp(-2.0 * math.pi ** 2 * 0.25 / math.log(2.0))) < 1e-6     # one symbol off the centre


# ------------------------------------------------------------------------------------------------------------- plan
def test_the_plan_on_literals():
    from sy11.data.demodulate_fsk import BLOCK, DEC, ITEM, plan_demodulate_fsk
    assert (ITEM.itemsize, BLOCK.itemsize, DEC.itemsize) == (72, 56, 32)                    # sy11_fsk_item / _block / _dec
    M = [527, 517, 518, 2300, 1637]
    p = plan_demodulate_fsk((M, FS), symbol_rate=[FS / 4, FS / 4, FS / 4, FS / 8.37, FS / 16], offset=[0.0, 0.0, 0.0, 0.0195 * FS, -1.0e3],
                            pulse=["gauss", "rect", "rect", "gauss", "gauss"], bt=[0.5, 0.5, 0.5, 0.3, 0.5], span=[2, 2, 2, 2, 16])
    assert p.valid.tolist() == [False, True, True, True, True] and p.reason.tolist() == ["too short", "", "", "", ""]
    assert p.hw.tolist() == [0, 2, 2, 17, 256] and p.n_taps.tolist() == [0, 5, 5, 35, 513] and p.tiles.tolist() == [0, 1, 2, 5, 3]
    assert p.order.tolist() == [2] * 5 and p.offset.tolist() == [0, 527, 1044, 1562, 3862] and p.tap_off.tolist() == [0, 0, 5, 10, 45, 558]
    assert p.Ws[1] == 1 << 62 and p.Ws[4] == 1 << 60 and p.Ws[3] == int(math.ldexp((FS / 8.37) / FS, 64)) and p.Ws[0] == 0
    assert p.Wc[:3] == [0, 0, 0] and p.Wc[3] == int(math.ldexp(0.0195, 64)) and p.Wc[4] == (1 << 64) - int(math.ldexp(1.0e-3, 64))
    it, clip = p.items()
    assert clip.tolist() == [1, 2, 2, 3, 3, 3, 3, 3, 4, 4, 4] and it["row"].tolist() == list(range(11))
    assert it["n0"].tolist() == [3, 3, 515, 18, 530, 1042, 1554, 2066, 257, 769, 1281] and it["cnt"].tolist() == [512, 512, 1, 512, 512, 512, 512, 217, 512, 512, 100]
    assert it["first"].tolist() == [1, 1, 0, 1, 0, 0, 0, 0, 1, 0, 0] and it["last"].tolist() == [1, 0, 1, 0, 0, 0, 0, 1, 0, 0, 1]
    assert p.centres(2).tolist() == [258.5, 515.0] and p.centres(4).tolist() == [512.5, 1024.5, 1330.5]
    for i in range(5):
        r = R.plan(M[i], FS, float(p.symbol_rate[i]), float(p.carrier_offset[i]), p.pulse[i], p.bt[i], p.span[i])
        assert r["valid"] == bool(p.valid[i]) and r["reason"] == p.reason[i]
        if r["valid"]:
            assert (int(p.hw[i]), int(p.tiles[i]), p.Ws[i], p.Wc[i]) == (r["hw"], r["tiles"], r["Ws"], r["Wc"])
            mine = it[clip == i]
            assert [(int(a), int(a + c)) for a, c in zip(mine["n0"], mine["cnt"])] == R.tile_bounds(M[i], r["hw"])
            assert np.array_equal(p.taps[int(p.tap_off[i]):int(p.tap_off[i + 1])], R.taps(r["sps"], r["hw"], p.pulse[i], p.bt[i]))


def test_every_argument_error_is_a_value_error():
    from sy11.data.demodulate_fsk import plan_demodulate_fsk
    clips = ([4000, 5000], FS)
    plan_demodulate_fsk(clips, symbol_rate=2.5e5)
    for ok in (dict(bt=1.0), dict(bt=1e-3), dict(span=1), dict(span=16), dict(block=8), dict(block=256), dict(pulse="rect"), dict(pulse=["rect", "gauss"]),
               dict(offset=[1.0, 2.0]), dict(span=[1, 2]), dict(bt=[0.3, 0.5])):
        plan_demodulate_fsk(clips, symbol_rate=2.5e5, **ok)
    for bad in (dict(bt=0.0), dict(bt=1.01), dict(bt=float("nan")), dict(bt=True), dict(bt="x"), dict(span=0), dict(span=17), dict(span=2.0), dict(span=True),
                dict(span=[2, 2, 2]), dict(block=7), dict(block=257), dict(block=32.0), dict(block=[32, 32]), dict(pulse="rrc"), dict(pulse=3),
                dict(pulse=["rect"] * 3), dict(offset=[0.0] * 3), dict(offset=None)):
        with pytest.raises(ValueError, match=next(iter(bad))):
            plan_demodulate_fsk(clips, symbol_rate=2.5e5, **bad)
    for rate in ([1.0, 2.0, 3.0], None, "x"):
        with pytest.raises(ValueError):
            plan_demodulate_fsk(clips, symbol_rate=rate)
    for bad_clips in (([4000.5], FS), ([-1], FS), ([4000], 0.0), ([4000], float("inf")), ([2 ** 31], FS), 7, ([[1, 2]], FS), ([4000, 5000], [FS] * 3)):
        with pytest.raises(ValueError):
            plan_demodulate_fsk(bad_clips, symbol_rate=2.5e5)


def test_every_reason_and_both_sides_of_every_boundary():
    from sy11.data.demodulate_fsk import plan_demodulate_fsk
    # gauss, span 2, at 4 samples per symbol: hw = 8, 529 samples at least
    rows = [
        (4000, FS / 4, 0.0, ""), (529, FS / 4, 0.0, ""), (528, FS / 4, 0.0, "too short"), (0, FS / 4, 0.0, "too short"),
        (4000, FS / 2.5, 0.0, ""), (4000, FS / 2.4999, 0.0, "samples per symbol outside [2.5, 16]"),
        (4000, FS / 16.0, 0.0, ""), (4000, FS / 16.001, 0.0, "samples per symbol outside [2.5, 16]"),
        (4000, FS / 4, np.nextafter(FS / 2, 0), ""), (4000, FS / 4, FS / 2, "offset beyond fs / 2"), (4000, FS / 4, -FS / 2, "offset beyond fs / 2"),
        (4000, float("nan"), 0.0, "rate or offset not finite"), (4000, FS / 4, float("inf"), "rate or offset not finite"), (4000, 0.0, 0.0, "rate or offset not finite"),
        (4000, -FS / 4, 0.0, "rate or offset not finite"),
    ]
    M, rate, off, reason = (list(v) for v in zip(*rows))
    p = plan_demodulate_fsk((M, FS), symbol_rate=rate, offset=off)
    assert p.reason.tolist() == reason and p.valid.tolist() == [r == "" for r in reason]
    assert [R.plan(m, FS, r, o)["reason"] for m, r, o in zip(M, rate, off)] == reason
    assert p.tiles[:4].tolist() == [8, 1, 0, 0] and p.total_rows == int(p.tiles.sum())
    q = plan_demodulate_fsk(([517, 516], FS), symbol_rate=FS / 4, pulse="rect")                                   # rect: hw = 2, 517 samples at least
    assert q.reason.tolist() == ["", "too short"]


# ------------------------------------------------------------------------------------------------------------- host stages
def test_mean_and_line_and_level_fit_on_hand_made_rows():
    from sy11.data.demodulate_fsk import level_fit, mean_and_line
    rows = np.array([[4.0, 1.0, 2.0, -1.0, 0.5, 0.25, 6.0, 9.0], [2.0, 0.0, 1.0, 1.0, 0.0, -0.5, 2.0, 5.0]])
    m, T = mean_and_line(rows, 16)
    assert m == 0.5 and T.tolist() == [(4 + 1j) - (2 - 1j) + 0.25 * (0.5 + 0.25j), (2 + 0j) - (1 + 1j) + 0.25 * (0 - 0.5j)]
    m2, T2 = R.mean_and_line(rows, 16)
    assert m2 == m and np.array_equal(T2, T)
    lv = level_fit(np.array([[3.0, 0.9, -0.2, 1.0], [1.0, 0.3, -0.4, 1.0]]), 7)
    assert (lv["n_hi"], lv["n_lo"], lv["one_tone"]) == (4, 3, False) and lv["c_hi"] == 1.2 / 4 and lv["c_lo"] == -0.6000000000000001 / 3
    assert lv["f0"] == (lv["c_hi"] + lv["c_lo"]) / 2 and lv["dev"] == (lv["c_hi"] - lv["c_lo"]) / 2 and lv["dev"] > 0
    want = R.levels(np.array([[3.0, 0.9, -0.2, 1.0], [1.0, 0.3, -0.4, 1.0]]), 7)
    assert all(lv[k] == want[k] for k in ("n_hi", "n_lo", "c_hi", "c_lo", "f0", "dev"))
    for rows4, n in ((np.array([[5.0, 1.0, 0.0, 1.0]]), 5), (np.array([[0.0, 0.0, -1.0, 1.0], [0.0, 0.0, -2.0, 1.0]]), 9)):        # all above, all below
        one = level_fit(rows4, n)
        assert one["one_tone"] and math.isnan(one["f0"]) and math.isnan(one["dev"]) and R.levels(rows4, n)["one_tone"]


# ------------------------------------------------------------------------------------------------------------- the algorithm
def test_the_reference_reads_every_shared_clip_without_a_bit_error():
    cs, refs = R.case_clips(), R.case_reference()
    seen = 0
    for c, r in zip(cs, refs):
        if c["kind"] in ("short", "sps"):
            assert r is None and not R.plan(len(c["x"]), c["fs"], c["rate"], c["offset"], c["pulse"], c["bt"], c["span"])["valid"]
            continue
        wrap = float(np.min(0.5 - np.abs(r["f"][1:])))
        assert wrap >= 1e-9, (c["label"], wrap)                               # a device atan2 one ulp from numpy's can never wrap
        if c["kind"] == "tone":
            assert not r["valid"] and r["reason"] == "one tone" and r["n_lo"] == 0 and r["n_hi"] == r["n_symbols"]
            continue
        seen += 1
        k0 = (r["T0"] + r["i_first"] * r["STEP"]) / 2.0 ** 32
        bad, inv, shift = R.bit_errors(r["d"], k0, c["sps"], c["bits"], c["u0"], c["lead"])
        dev_true = c["h"] / 2.0 / c["sps"]
        f0_err = (r["carrier_fit"] - 2.4e9 - c["true_offset"]) / c["fs"]
        print(f"{c['label']}: {r['n_symbols']} symbols, {r['tiles']} tiles, {r['n_taps']} taps, {bad} errors (inverted {inv}, shift {shift}), evm {r['evm']:.4f}, "
              f"smallest |r| {float(np.abs(r['r']).min()):.3f}, wrap margin {wrap:.3f}, f0 {f0_err / dev_true:+.3f} dev off, mod_index {r['mod_index']:.3f} (h {c['h']})")
        assert bad == 0 and inv == 0                                          # a 1 is the lower tone: the decisions come out upright
        assert float(np.abs(r["r"]).min()) >= 2.0 ** -20                      # no decision of the GPU test is exempt
        assert r["dev"] > 0 and abs(r["deviation"] - r["dev"] * c["fs"]) == 0 and r["n_hi"] + r["n_lo"] == r["n_symbols"]
        assert abs(f0_err) < 0.5 * dev_true                                   # the midpoint lies between the tones, nearer the centre than either
    assert seen == 7
    # unbalanced data, 80 % ones, a full-response pulse and its integrate-and-dump: both levels are reached at the symbol centres whatever the
    # data, so the MIDPOINT is off by what interpolation and timing leave, a few per cent of the deviation (bar: a tenth), while the MEAN of y
    # sits 0.8 - 0.2 = 0.6 deviations towards the tone sent more often
    c, r = cs[6], refs[6]
    dev_true = c["h"] / 2.0 / c["sps"]
    assert c["label"] == "unbalanced" and abs(float(np.mean(c["bits"])) - 0.8) < 0.03 and r["n_lo"] > 3 * r["n_hi"]
    assert abs(r["f0"] - c["true_offset"] / c["fs"]) < 0.1 * dev_true and abs(r["m"] - c["true_offset"] / c["fs"]) > 0.5 * dev_true
    # the shapes the GPU test is about
    assert [len(c["x"]) % 2 for c in cs[:1]] == [1] and refs[1]["tiles"] == 1 and refs[2]["tiles"] == 2 and refs[3]["tiles"] >= 4 and refs[4]["n_taps"] == 513
    assert refs[3]["a"] != 0.0 and refs[5]["hw"] == 2 and max(len(c["x"]) for c in cs) <= 4000


@pytest.mark.parametrize("which", ["gfsk", "gmsk"])
def test_the_reference_alone_decodes_the_bursts_of_the_end_to_end_test(which):
    """The burst of tests/test_demodulate_fsk_gpu.py at its SNR, demodulated by the reference alone: every channel bit of the frame is read right."""
    from tests import test_demodulate_fsk_gpu as G
    b = G.burst(which)
    x = b["x"][::1]
    r = R.demodulate(x, G.FS_CLIP, G.FS_CLIP / G.SPS, 0.0, "gauss", b["bt"], 2, 32)
    k0 = (r["T0"] + r["i_first"] * r["STEP"]) / 2.0 ** 32
    bad, inv, shift = R.bit_errors(r["d"], k0, G.SPS, b["all_bits"], b["u0"], b["lead"])
    print(f"{which}: {r['n_symbols']} symbols, {bad} errors (inverted {inv}, shift {shift}), evm {r['evm']:.4f}, smallest |r| {float(np.abs(r['r']).min()):.3f}")
    assert r["valid"] and bad == 0 and inv == 0


# ------------------------------------------------------------------------------------------------------------- result, save
def _hand_built(tmp=None):
    import torch
    from sy11.data.demodulate_fsk import FskDemodulation, plan_demodulate_fsk
    plan = plan_demodulate_fsk(([600, 100], FS), symbol_rate=FS / 4, pulse="rect")
    n = 3
    cols = {k: np.array([v, np.nan]) for k, v in (("gain", 1.0), ("evm", 0.1), ("mer_db", 20.0), ("timing", 0.25), ("symbol_rate_fit", 2.5e5), ("carrier_fit", 2.4e9),
                                                    ("deviation", 6.25e4), ("mod_index", 0.5))}
    cols["n_symbols"] = np.array([n, -1])
    r = torch.tensor([1.0 + 0j, -1.0 + 0j, 0.5 + 0j], dtype=torch.complex64)
    d = torch.tensor([0, 1, 0], dtype=torch.uint8)
    raw = {"sym0": np.array([0, 3, 3]), "block0": np.array([0, 1, 1]), "row0": plan.row0, "T0": [0, 0], "STEP": [1 << 34, 0], "i_first": [1, 0], "i_last": [3, -1]}
    return FskDemodulation(plan, plan.valid.copy(), plan.reason.copy(), 2.4e9, cols, [r, r[:0]], [d, d[:0]], [torch.zeros(600), torch.zeros(0)], raw,
                           rows=np.array([4, 9]), cls=np.array([1, 0]), conf=np.array([0.9, 0.8]), names={0: "a", 1: "b"})


def test_save_round_trip_on_a_hand_built_result(tmp_path):
    from sy11.data.demodulate import Demodulation
    d = _hand_built()
    assert isinstance(d, Demodulation) and len(d) == 2 and d.valid.tolist() == [True, False] and d.reason.tolist() == ["", "too short"]
    assert d.order.tolist() == [2, 2] and d.phase_ambiguity.tolist() == [2, -1] and d.bits(0).tolist() == [0, 1, 0] and d.bits(1).shape == (0,)
    assert d[0]["deviation"] == 6.25e4 and d[0]["mod_index"] == 0.5 and d[1]["reason"] == "too short" and d.COLUMNS[-2:] == ("deviation", "mod_index")
    out = d.save(tmp_path / "f")
    z = np.load(tmp_path / "f" / "demodulate.npz")
    index = json.loads((tmp_path / "f" / "demodulate.json").read_text())
    assert out == str(tmp_path / "f")
    for k in d.COLUMNS + ("n_symbols", "order", "valid", "phase_ambiguity", "sample_rate", "center_freq"):
        assert np.array_equal(z[k], getattr(d, k), equal_nan=True), k
    assert z["rows"].tolist() == [4, 9] and z["decisions_4"].tolist() == [0, 1, 0] and "decisions_9" not in z.files
    assert index["modulation"] == "fsk" and index["pulse"] == ["rect", "rect"] and index["bt"] == [0.5, 0.5] and index["span"] == [2, 2] and index["block"] == 32
    c0, c1 = index["clips"]
    assert c0["file"] == "symbols_4.cf32" and c0["deviation"] == 6.25e4 and c0["mod_index"] == 0.5 and c0["name"] == "b" and c0["order"] == 2
    assert c1["file"] is None and c1["reason"] == "too short" and c1["deviation"] is None and c1["evm"] is None
    assert np.array_equal(np.fromfile(tmp_path / "f" / "symbols_4.cf32", dtype=np.complex64), np.array([1, -1, 0.5], dtype=np.complex64))


def test_an_extraction_without_a_valid_clip_launches_nothing():
    import torch
    from sy11 import _lib
    from sy11.data.demodulate_fsk import FskDemodulation, demodulate_fsk_extraction
    Ms = np.array([100, 300], dtype=np.int64)
    off = np.concatenate(([0], np.cumsum(Ms))).astype(np.int64)
    ext = SimpleNamespace(plan=SimpleNamespace(M=Ms, offset=off), packed=torch.zeros(400, dtype=torch.complex64), sample_rate=np.full(2, FS),
                          center_freq=np.full(2, 2.4e9), rows=np.arange(2), cls=np.array([0, 1]), conf=np.array([0.5, 0.6]), names={0: "a", 1: "b"})
    _lib.PROFILE = []
    try:
        d = demodulate_fsk_extraction(ext, symbol_rate=[FS / 4, FS / 20])
        calls = list(_lib.PROFILE)
    finally:
        _lib.PROFILE = None
    assert isinstance(d, FskDemodulation) and calls == [] and len(d) == 2 and not d.valid.any()
    assert d.reason.tolist() == ["too short", "samples per symbol outside [2.5, 16]"]
    assert d.n_symbols.tolist() == [-1, -1] and np.isnan(d.evm).all() and np.isnan(d.deviation).all() and d.phase_ambiguity.tolist() == [-1, -1]
    assert d.symbols[0].shape == (0,) and d.filtered[0].dtype == torch.float32 and d.bits(0).shape == (0,)
    with pytest.raises(ValueError, match="block"):
        demodulate_fsk_extraction(ext, symbol_rate=FS / 4, block=7)
    with pytest.raises(ValueError, match="pulse"):
        demodulate_fsk_extraction(ext, symbol_rate=FS / 4, pulse="sinc")


# ------------------------------------------------------------------------------------------------------------- the C-ABI without a GPU
def test_c_abi_refusals_that_need_no_gpu():
    """Every entry checks its arguments on the host before it launches: each call below has one defect and is refused with its message.  The
    pointers are host buffers, which a refused call never touches."""
    import torch
    from sy11 import _lib, ops
    from sy11.data.demodulate_fsk import BLOCK, DEC, plan_demodulate_fsk
    p = plan_demodulate_fsk(([1100], FS), symbol_rate=FS / 4)                 # hw = 8: tiles [9, 521) and [521, 1033) and [1033, 1092)
    items = p.items()[0]
    assert items["cnt"].tolist() == [512, 512, 59]
    buf = np.zeros(4096, dtype=np.float64)                                    # stands for every device buffer
    ptr = C.c_void_p(buf.ctypes.data)
    odd = C.c_void_p(buf.ctypes.data + 4)
    other = C.c_void_p(buf.ctypes.data + 8192)

    def one(table, k, **kw):
        s = table[k:k + 1].copy()
        for key, v in kw.items():
            s[key] = v
        return s

    def refused(name, args, match):
        with pytest.raises(_lib.Sy11Error, match=match):
            _lib.call(name, *args)

    def a1(t, n_tap=17, n_in=1100, n_rows=3, taps=ptr, x=ptr, y=other, rows=ptr, dev=ptr):
        return [t.shape[0], C.c_void_p(t.ctypes.data), dev, n_tap, taps, n_in, x, y, n_rows, rows, None]
    name = "sy11_iq_fsk_filter"
    for kw in (dict(taps=None), dict(x=None), dict(y=None), dict(rows=None), dict(dev=None)):
        refused(name, a1(items, **kw), "null")
    for kw in (dict(n_tap=0), dict(n_in=0), dict(n_rows=0), dict(n_in=2 ** 31)):
        refused(name, a1(items, **kw), "each below 2\\^31")
    for kw in (dict(x=odd), dict(rows=odd), dict(dev=odd), dict(y=C.c_void_p(buf.ctypes.data + 8194)), dict(y=ptr)):
        refused(name, a1(items, **kw), "aligned")
    refused(name, a1(items, n_in=1099), "packed samples")
    refused(name, a1(items, n_tap=16), "packed taps")
    refused(name, a1(items, n_rows=2), "writes row")
    for kw, what in ((dict(off=-1), "packed samples"), (dict(len=0), "packed samples"), (dict(off=1), "packed samples"), (dict(hw=0, n_taps=1), "half width"),
                     (dict(n_taps=16), "half width"), (dict(hw=257, n_taps=515), "half width"), (dict(tap_off=-1), "packed taps"), (dict(tap_off=1), "packed taps"),
                     (dict(n0=8, cnt=59), "not a tile"), (dict(n0=1034, cnt=58), "not a tile"), (dict(cnt=0), "not a tile"), (dict(cnt=60), "not a tile"),
                     (dict(cnt=513), "not a tile"), (dict(first=1), "first ="), (dict(first=2), "first ="), (dict(last=0), "last ="), (dict(last=2), "last ="),
                     (dict(cnt=58), "last ="), (dict(row=-1), "writes row"), (dict(row=3), "writes row")):
        refused(name, a1(one(items, 2, **kw)), "iq_fsk_filter: item 0.*" + what)
    refused(name, a1(one(items, 0, first=0)), "first =")
    refused(name, a1(one(items, 0, last=1)), "last =")
    refused(name, a1(np.concatenate((one(items, 0), one(items, 1, row=0)))), "an earlier item")
    # launch 2: two blocks of a clip of 1100 samples at 4 samples per symbol from sample 10
    bl = np.zeros(2, dtype=BLOCK)
    bl["len"], bl["step"], bl["t0"], bl["sym_off"], bl["n"], bl["row"], bl["m"] = 1100, 4 << 32, [10 << 32, (10 + 4 * 32) << 32], [0, 32], 32, [0, 1], 0.01

    def a2(t, n_in=1100, n_sym=64, n_rows=2, y=ptr, sym=other, rows=ptr, dev=ptr):
        return [t.shape[0], C.c_void_p(t.ctypes.data), dev, n_in, y, n_sym, sym, n_rows, rows, None]
    name = "sy11_fsk_symbols"
    for kw in (dict(y=None), dict(sym=None), dict(rows=None), dict(dev=None)):
        refused(name, a2(bl, **kw), "null")
    for kw in (dict(n_in=0), dict(n_sym=0), dict(n_rows=0)):
        refused(name, a2(bl, **kw), "each below 2\\^31")
    for kw in (dict(rows=odd), dict(dev=odd), dict(y=C.c_void_p(buf.ctypes.data + 2)), dict(sym=C.c_void_p(buf.ctypes.data + 8194)), dict(sym=ptr)):
        refused(name, a2(bl, **kw), "aligned")
    refused(name, a2(bl, n_in=1099), "packed samples")
    refused(name, a2(bl, n_sym=63), "packed symbols")
    refused(name, a2(bl, n_rows=1), "writes row")
    k_last = 10 + 4 * 63
    for kw, what in ((dict(off=-1), "packed samples"), (dict(len=3), "packed samples"), (dict(off=1), "packed samples"), (dict(n=0), "packed symbols"),
                     (dict(n=257), "packed symbols"), (dict(sym_off=-1), "packed symbols"), (dict(sym_off=33), "packed symbols"), (dict(step=2 ** 32 - 1), "Q32.32"),
                     (dict(step=2 ** 40 + 1), "Q32.32"), (dict(t0=2 ** 32 - 1), "Q32.32"), (dict(t0=1100 * 2 ** 32), "Q32.32"), (dict(len=k_last + 2), "Q32.32"),
                     (dict(m=float("nan")), "not finite"), (dict(m=float("inf")), "not finite"), (dict(row=-1), "writes row"), (dict(row=2), "writes row")):
        refused(name, a2(one(bl, 1, **kw)), "fsk_symbols: item 0.*" + what)
    refused(name, a2(np.concatenate((one(bl, 0), one(bl, 1, row=0)))), "an earlier item")
    # launch 3
    de = np.zeros(2, dtype=DEC)
    de["sym_off"], de["n"], de["row"], de["f0"], de["dev"] = [0, 32], 32, [0, 1], 0.01, 0.06

    def a3(t, n_sym=64, n_rows=2, sym=ptr, r=other, d=ptr, rows=ptr, dev=ptr):
        return [t.shape[0], C.c_void_p(t.ctypes.data), dev, n_sym, sym, r, d, n_rows, rows, None]
    name = "sy11_fsk_decide"
    for kw in (dict(sym=None), dict(r=None), dict(d=None), dict(rows=None), dict(dev=None)):
        refused(name, a3(de, **kw), "null")
    for kw in (dict(n_sym=0), dict(n_rows=0)):
        refused(name, a3(de, **kw), "each below 2\\^31")
    for kw in (dict(rows=odd), dict(dev=odd), dict(r=C.c_void_p(buf.ctypes.data + 8196)), dict(sym=C.c_void_p(buf.ctypes.data + 2)), dict(r=ptr)):
        refused(name, a3(de, **kw), "aligned")
    refused(name, a3(de, n_sym=63), "packed symbols")
    refused(name, a3(de, n_rows=1), "writes row")
    for kw, what in ((dict(n=0), "packed symbols"), (dict(n=257), "packed symbols"), (dict(sym_off=-1), "packed symbols"), (dict(sym_off=33), "packed symbols"),
                     (dict(dev=0.0), "dev positive"), (dict(dev=-0.06), "dev positive"), (dict(dev=float("nan")), "dev positive"), (dict(dev=float("inf")), "dev positive"),
                     (dict(f0=float("nan")), "dev positive"), (dict(row=-1), "writes row"), (dict(row=2), "writes row")):
        refused(name, a3(one(de, 1, **kw)), "fsk_decide: item 0.*" + what)
    refused(name, a3(np.concatenate((one(de, 0), one(de, 1, row=0)))), "an earlier item")
    assert not buf.any()                                                      # nothing was written
    # the wrappers refuse tensors that are not on a GPU
    x, y, rows = torch.zeros(1100, dtype=torch.complex64), torch.zeros(1100), torch.zeros((3, 8), dtype=torch.float64)
    with pytest.raises(_lib.Sy11Error):
        ops.iq_fsk_filter(x, items, torch.from_numpy(p.taps), y, rows)
    with pytest.raises(_lib.Sy11Error):
        ops.fsk_symbols(y, bl, torch.zeros(64), torch.zeros((2, 4), dtype=torch.float64))
    with pytest.raises(_lib.Sy11Error):
        ops.fsk_decide(torch.zeros(64), de, torch.zeros(64, dtype=torch.complex64), torch.zeros(64, dtype=torch.uint8), torch.zeros((2, 3), dtype=torch.float64))
