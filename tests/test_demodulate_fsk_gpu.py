"""GPU: the frequency-keyed demodulation kernels (sy11_iq_fsk_filter, sy11_fsk_symbols, sy11_fsk_decide) on the ten clips of tests/_fsk_ref.py in ONE
call of three launches.  y and s against the float64 reference under the rule of tests/test_demodulate_gpu.py (per clip, 4x the error of the
float32 emulation of the same sums, relative to the clip's maximum; the emulation's error must be > 0); every float64 table (timing rows, level
rows, decision rows) against the reference fed with the kernel's own float32 values, to 1e-12; the integers of the timing fit with no tolerance; r
to 2^-21 and the decisions equal (no symbol of these clips is within 2^-20 of the boundary: tests/test_demodulate_fsk_cpu.py); the columns to 1e-12;
one call against one call per clip and a permuted extraction, bit for bit; the refusals; and ``extract`` -> ``demodulate_fsk`` -> ``find_frames`` ->
``decode`` (and ``equalize``) on three bursts embedded in a noise capture, which come out as they were sent."""
import ctypes as C
import functools
import json

import numpy as np
import pytest
import torch

from tests import _fec_ref as FEC
from tests import _fsk_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FC = 2.4e9
BLOCK = R.BLOCK


def _extraction(clips, order=None, fs=R.FS, fc=FC):
    """A real ``Extraction`` around the given clips (numpy complex64), packed one after the other in ``order``."""
    from sy11.data.extract import Extraction, ExtractPlan
    order = list(range(len(clips))) if order is None else list(order)
    clips = [clips[i] for i in order]
    n = len(clips)
    M = np.array([len(c) for c in clips], dtype=np.int64)
    plan = ExtractPlan(int(M.sum()) * 64, fs, fc, np.array(order, dtype=np.int64), np.zeros((n, 4)), np.ones(n, dtype=np.int64), np.zeros(n, dtype=np.int64),
                       np.zeros(n, dtype=np.int64), M)
    packed = torch.from_numpy(np.concatenate(clips)).to(DEV)
    return Extraction(plan, packed, cls=np.arange(n) % 2, conf=np.linspace(0.5, 0.9, n), names={0: "a", 1: "b"})


def _demod(cs, order=None):
    from sy11.data.demodulate_fsk import demodulate_fsk_extraction
    order = list(range(len(cs))) if order is None else list(order)
    ext = _extraction([c["x"] for c in cs], order)
    pick = lambda key: [cs[i][key] for i in order]                            # noqa: E731
    return ext, demodulate_fsk_extraction(ext, symbol_rate=pick("rate"), offset=pick("offset"), pulse=pick("pulse"), bt=pick("bt"), span=pick("span"), block=BLOCK)


def _bits(t):
    t = torch.view_as_real(t) if t.is_complex() else t
    return t.contiguous().view({torch.float64: torch.int64, torch.float32: torch.int32, torch.uint8: torch.uint8}[t.dtype])


@pytest.fixture(scope="module")
def case():
    """The ten clips, their extraction and ONE demodulation (three launches); shared and left unchanged."""
    from sy11 import _lib
    cs = R.case_clips()
    _lib.PROFILE = []
    try:
        ext, d = _demod(cs)
        calls = [k[0] for k in _lib.PROFILE]
    finally:
        _lib.PROFILE = None
    assert calls == ["sy11_iq_fsk_filter", "sy11_fsk_symbols", "sy11_fsk_decide"]                 # three launches, whatever the number of clips
    assert int(ext.plan.offset[1]) % 2 == 1                                                       # the one-tile clip starts at an odd sample
    planned = [c["kind"] in ("fsk", "tone") for c in cs]
    assert d.plan.valid.tolist() == planned and d.valid.tolist() == [c["kind"] == "fsk" for c in cs]
    assert d.reason.tolist() == [{"fsk": "", "tone": "one tone", "short": "too short", "sps": "samples per symbol outside [2.5, 16]"}[c["kind"]] for c in cs]
    assert d.plan.n_taps.tolist() == [0, 5, 5, 35, 513, 5, 7, 27, 17, 0] and d.plan.tiles.tolist() == [0, 1, 2, 5, 3, 3, 6, 5, 3, 0]
    y, sym0 = d.raw["y"].cpu().numpy(), d.raw["sym0"]
    off = ext.plan.offset
    host = {"y": [y[int(off[i]):int(off[i + 1])] for i in range(len(cs))], "s": d.raw["s"].cpu().numpy(), "r": [v.cpu().numpy() for v in d.symbols],
            "d": [v.cpu().numpy() for v in d.decisions], "t": d.raw["timing_rows"].cpu().numpy(), "l": d.raw["level_rows"].cpu().numpy(),
            "e": d.raw["decision_rows"].cpu().numpy()}
    assert y.dtype == np.float32 and host["s"].dtype == np.float32 and host["s"].shape == (int(sym0[-1]),)
    return cs, ext, d, host


def _slices(d, i):
    return (slice(int(d.plan.row0[i]), int(d.plan.row0[i + 1])), slice(int(d.raw["block0"][i]), int(d.raw["block0"][i + 1])),
            slice(int(d.raw["sym0"][i]), int(d.raw["sym0"][i + 1])))


def _plan(c):
    return R.plan(len(c["x"]), c["fs"], c["rate"], c["offset"], c["pulse"], c["bt"], c["span"])


# ------------------------------------------------------------------------------------------------------------- launch 1
def test_filtered_samples_and_timing_rows_match_the_float64_reference(case):
    cs, ext, d, host = case
    over = []
    for i, c in enumerate(cs):
        p = _plan(c)
        if not p["valid"]:
            assert d.filtered[i].shape == (0,) and not host["y"][i].any() and int(d.plan.tiles[i]) == 0      # invalid before launch 1
            continue
        h = R.taps(p["sps"], p["hw"], c["pulse"], c["bt"])
        want, got = R.filter64(c["x"], p["Wc"], h), host["y"][i].astype(np.float64)
        assert got.shape == want.shape == (len(c["x"]),) and not got[:p["hw"] + 1].any() and not got[len(got) - p["hw"]:].any()
        if c["kind"] == "fsk":
            assert torch.equal(d.filtered[i], d.raw["y"][int(ext.plan.offset[i]):int(ext.plan.offset[i + 1])]) and d.filtered[i].dtype == torch.float32
            emu = R.filter32(c["x"], p["Wc"], h).astype(np.float64)
            scale = np.abs(want).max()
            e_emu, e_gpu = np.abs(emu - want).max() / scale, np.abs(got - want).max() / scale
            print(f"iq_fsk_filter[{c['label']}: M={len(c['x'])} taps={p['n_taps']}]: float32 emulation {e_emu:.3e}, kernel {e_gpu:.3e} (bar {4 * e_emu:.3e})")
            assert e_emu > 0
            if not e_gpu <= 4 * e_emu:
                over.append((c["label"], e_gpu, e_emu))
        else:                                                                 # the constant tone: every usable y is the one float32 value
            assert np.unique(got[p["hw"] + 1:len(got) - p["hw"]]).shape == (1,) and abs(got[p["hw"] + 1] - 0.25) < 1e-7
        rows, tr = _slices(d, i)[0], R.timing_rows(host["y"][i], p["hw"], p["Ws"])
        mine = host["t"][rows]
        assert mine.shape == tr.shape == (p["tiles"], 8)
        err = np.abs(mine - tr) / R.row_scales(host["y"][i], p["hw"])
        print(f"iq_fsk_filter[{c['label']}] timing rows: largest error {err.max():.2e} of the tile's sum of magnitudes")
        assert err.max() <= 1e-12, (c["label"], err)
    assert not over, over


# ------------------------------------------------------------------------------------------------------------- the timing fit
def test_mean_and_timing_fit_equal_the_reference_on_the_kernels_own_rows(case):
    cs, ext, d, host = case
    for i, c in enumerate(cs):
        p = _plan(c)
        if not p["valid"]:
            assert (d.n_symbols[i], d.raw["i_last"][i]) == (-1, -1) and np.isnan(d.timing[i]) and np.isnan(d.raw["m"][i])
            continue
        m, T = R.mean_and_line(host["t"][_slices(d, i)[0]], p["usable"])
        f = R.fit(T, len(c["x"]), p["hw"], p["Ws"])
        raw = d.raw
        assert abs(raw["m"][i] - m) <= 1e-12 * abs(m)
        n = raw["i_last"][i] - raw["i_first"][i] + 1
        assert (raw["T0"][i], raw["STEP"][i], raw["i_first"][i], raw["i_last"][i], n) == (f["T0"], f["STEP"], f["i_first"], f["i_last"], f["n_symbols"])
        assert n == _slices(d, i)[2].stop - _slices(d, i)[2].start and np.abs(raw["psi"][i] - f["psi"]).max() <= 1e-12
        if c["kind"] == "fsk":
            assert int(d.n_symbols[i]) == n and abs(d.timing[i] - f["timing"]) <= 1e-12 and abs(d.symbol_rate_fit[i] - c["fs"] / f["sps"]) <= 1e-12 * c["fs"]
            assert abs(d.symbol_rate_fit[i] / (c["fs"] / c["sps"]) - 1.0) < 1e-3
    assert d.raw["psi"][3].shape[0] >= 4 and int(d.plan.tiles[2]) == 2 and any(int(n) % BLOCK for n in d.n_symbols[d.valid])      # the fitted slope; the tile of one; a ragged block


# ------------------------------------------------------------------------------------------------------------- launch 2
def test_symbols_and_level_rows_match_the_reference_on_the_kernels_own_samples(case):
    cs, ext, d, host = case
    over = []
    for i, c in enumerate(cs):
        if not _plan(c)["valid"]:
            continue
        _, blocks, syms = _slices(d, i)
        T0, STEP, i0, n = d.raw["T0"][i], d.raw["STEP"][i], d.raw["i_first"][i], syms.stop - syms.start
        want, got = R.symbols64(host["y"][i], T0, STEP, i0, n), host["s"][syms].astype(np.float64)
        assert got.shape == want.shape == (n,)
        if c["kind"] == "fsk":
            emu = R.symbols32(host["y"][i], T0, STEP, i0, n).astype(np.float64)
            scale = np.abs(want).max()
            e_emu, e_gpu = np.abs(emu - want).max() / scale, np.abs(got - want).max() / scale
            print(f"fsk_symbols[{c['label']}: {n} symbols]: float32 emulation {e_emu:.3e}, kernel {e_gpu:.3e} (bar {4 * e_emu:.3e})")
            assert e_emu > 0
            if not e_gpu <= 4 * e_emu:
                over.append((c["label"], e_gpu, e_emu))
        else:
            assert np.array_equal(got, np.full(n, host["y"][i][100], dtype=np.float64))
        lr, mine = R.level_rows(host["s"][syms], d.raw["m"][i], BLOCK), host["l"][blocks]
        assert mine.shape == lr.shape == (-(-n // BLOCK), 4) and np.array_equal(mine[:, 0], lr[:, 0])
        mag = np.array([np.sum(np.abs(got[a:b])) for a, b in R.blocks(n, BLOCK)])
        err = max((np.abs(mine[:, 1:3] - lr[:, 1:3]).max(1) / mag).max(), (np.abs(mine[:, 3] - lr[:, 3]) / lr[:, 3]).max())
        print(f"fsk_symbols[{c['label']}] level rows: largest error {err:.2e}")
        assert err <= 1e-12
    assert not over, over


# ------------------------------------------------------------------------------------------------------------- levels, launch 3, columns
def test_levels_decisions_rows_and_columns_match_the_reference_on_the_kernels_own_symbols(case):
    cs, ext, d, host = case
    for i, c in enumerate(cs):
        if c["kind"] != "fsk":
            assert np.isnan([d.gain[i], d.evm[i], d.mer_db[i], d.carrier_fit[i], d.deviation[i], d.mod_index[i]]).all() and d.phase_ambiguity[i] == -1
            assert d.bits(i).shape == (0,) and d.symbols[i].shape == (0,) and d.decisions[i].shape == (0,) and int(d.n_symbols[i]) == -1 and not d.valid[i]
            if c["kind"] == "tone":                                           # it went through launches 1 and 2, and the levels refused it
                _, blocks, syms = _slices(d, i)
                lv = R.levels(host["l"][blocks], syms.stop - syms.start)
                assert lv["one_tone"] and lv["n_lo"] == 0 and np.isnan(d.raw["f0"][i]) and not host["e"][blocks].any()
            continue
        _, blocks, syms = _slices(d, i)
        s, n = host["s"][syms], int(d.n_symbols[i])
        lv = R.levels(host["l"][blocks], n)
        f0, dev = float(d.raw["f0"][i]), float(d.raw["dev"][i])
        assert not lv["one_tone"] and abs(f0 - lv["f0"]) <= 1e-12 * lv["dev"] and abs(dev - lv["dev"]) <= 1e-12 * lv["dev"] and dev > 0
        r, dec = R.decide(s, f0, dev)
        got = host["r"][i]
        assert got.dtype == np.complex64 and got.shape == (n,) and not got.imag.any()
        err = np.abs(got.real.astype(np.float64) - r)
        exempt = np.abs(r) < 2.0 ** -20
        print(f"fsk_decide[{c['label']}]: largest |r - ref| {err.max():.3e} (bar {2.0 ** -21:.3e}); {int(exempt.sum())} of {n} decisions exempt, smallest |r| {np.abs(r).min():.3f}")
        assert err.max() <= 2.0 ** -21
        assert int(exempt.sum()) == 0 and np.array_equal(host["d"][i], dec) and host["d"][i].dtype == np.uint8
        rows, mine = R.block_rows(got.real, BLOCK), host["e"][blocks]
        assert mine.shape == rows.shape and np.array_equal(mine[:, 2], rows[:, 2])
        assert (np.abs(mine[:, :2] - rows[:, :2]) <= 1e-12 * rows[:, :2]).all()
        col = R.columns(mine, f0, dev, c["fs"], FC, c["offset"], float(d.symbol_rate_fit[i]))
        assert int(d.n_symbols[i]) == col["n_symbols"] == n
        for key in ("gain", "evm", "mer_db", "carrier_fit", "deviation", "mod_index"):
            assert abs(float(getattr(d, key)[i]) - col[key]) <= 1e-12 * abs(col[key]), (c["label"], key)
        assert d.phase_ambiguity[i] == 2 and d.order[i] == 2 and np.array_equal(d.bits(i), host["d"][i])
        # what was sent: no bit error, upright (a 1 is the lower tone), a shift of one symbol at the most (the reference alone: the CPU tests)
        k0 = (d.raw["T0"][i] + d.raw["i_first"][i] * d.raw["STEP"][i]) / 2.0 ** 32
        bad, inv, shift = R.bit_errors(host["d"][i], k0, c["sps"], c["bits"], c["u0"], c["lead"])
        dev_true = c["h"] / 2.0 / c["sps"]
        print(f"demodulate_fsk[{c['label']}]: {bad} bit errors (inverted {inv}, shift {shift}), evm {d.evm[i]:.4f}, mod_index {d.mod_index[i]:.3f}, "
              f"carrier {(d.carrier_fit[i] - FC - c['true_offset']) / c['fs'] / dev_true:+.3f} dev off")
        assert bad == 0 and inv == 0 and abs(d.carrier_fit[i] - FC - c["true_offset"]) < 0.5 * dev_true * c["fs"]
    assert d[1]["valid"] and d[1]["reason"] == "" and d[8]["reason"] == "one tone" and d[0]["reason"] == "too short"
    assert d.cls.tolist() == ext.cls.tolist() and d.names == ext.names and d.rows.tolist() == ext.rows.tolist()


# ------------------------------------------------------------------------------------------------------------- invariance
def test_one_call_per_clip_and_a_permuted_extraction_give_the_same_bits(case):
    cs, ext, d, host = case
    perm = [4, 8, 2, 0, 9, 7, 5, 3, 1, 6]
    pext, p = _demod(cs, perm)
    assert p.rows.tolist() == perm
    for at, i in enumerate(perm):
        oext, one = _demod([cs[i]])
        for other, oe, k in ((p, pext, at), (one, oext, 0)):
            assert bool(other.valid[k]) == bool(d.valid[i]) and other.reason[k] == d.reason[i] and int(other.n_symbols[k]) == int(d.n_symbols[i])
            for a, b in zip(_slices(other, k), _slices(d, i)):
                assert a.stop - a.start == b.stop - b.start
            for key in ("filtered", "symbols", "decisions"):
                assert torch.equal(_bits(getattr(other, key)[k]), _bits(getattr(d, key)[i])), (i, at, key)
            if not d.plan.valid[i]:
                continue
            ya = other.raw["y"][int(oe.plan.offset[k]):int(oe.plan.offset[k + 1])]
            assert torch.equal(_bits(ya), _bits(d.raw["y"][int(ext.plan.offset[i]):int(ext.plan.offset[i + 1])]))
            for key, sl in zip(("timing_rows", "level_rows", "s"), (0, 1, 2)):
                assert torch.equal(_bits(other.raw[key][_slices(other, k)[sl]]), _bits(d.raw[key][_slices(d, i)[sl]])), (i, at, key)
            assert torch.equal(_bits(other.raw["decision_rows"][_slices(other, k)[1]]), _bits(d.raw["decision_rows"][_slices(d, i)[1]]))
            assert np.array_equal(other.raw["psi"][k], d.raw["psi"][i])
            assert (other.raw["T0"][k], other.raw["STEP"][k], other.raw["i_first"][k]) == (d.raw["T0"][i], d.raw["STEP"][i], d.raw["i_first"][i])
            for key in ("m", "f0", "dev"):
                assert np.array_equal(other.raw[key][k:k + 1], d.raw[key][i:i + 1], equal_nan=True)
            for key in d.COLUMNS:
                assert np.array_equal(getattr(other, key)[k:k + 1], getattr(d, key)[i:i + 1], equal_nan=True)


# ------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_raise_and_write_nothing(case):
    from sy11 import _lib, ops
    from sy11.data.demodulate_fsk import BLOCK as BLK, DEC
    cs, ext, d, host = case
    E_ = _lib.Sy11Error
    p = lambda v: C.c_void_p(v.data_ptr())                                    # noqa: E731
    keep = []

    def table(host_items):
        t = torch.from_numpy(host_items.view(np.uint8).copy()).to(DEV)
        keep.extend((host_items, t))
        return [host_items.shape[0], C.c_void_p(host_items.ctypes.data), p(t)]

    def one(items, k, **kw):
        s = items[k:k + 1].copy()
        for key, v in kw.items():
            s[key] = v
        return s
    # ---- launch 1
    x, items = ext.packed, d.plan.items()[0]
    taps = torch.from_numpy(d.plan.taps).to(DEV)
    n_in, n_tap, n_rows = x.shape[0], taps.shape[0], d.plan.total_rows
    y = torch.full((n_in,), -7.0, dtype=torch.float32, device=DEV)
    rows = torch.full((n_rows, 8), -7.0, dtype=torch.float64, device=DEV)
    k = int(np.flatnonzero(items["n_taps"] == 513)[-1])                      # the last tile of the 513-tap clip
    it = items[k]
    assert int(it["last"]) == 1 and int(it["first"]) == 0 and int(it["cnt"]) == 100
    hw, ln = int(it["hw"]), int(it["len"])
    end = int(ext.plan.offset[9])                                             # where the last clip with items (the tone) ends; a clip without items follows it
    entry1 = ((dict(off=-1), "packed samples"), (dict(len=0), "packed samples"), (dict(off=n_in - ln + 1), "packed samples"), (dict(len=n_in + 1, off=0), "packed samples"),
              (dict(hw=0, n_taps=1), "half width"), (dict(n_taps=511), "half width"), (dict(n_taps=512), "half width"), (dict(hw=257, n_taps=515), "half width"),
              (dict(tap_off=-1), "packed taps"), (dict(tap_off=n_tap - 512), "packed taps"),
              (dict(n0=int(it["n0"]) + 1, cnt=99), "not a tile"), (dict(n0=hw), "not a tile"), (dict(n0=hw + 1 - 512), "not a tile"), (dict(cnt=0), "not a tile"),
              (dict(cnt=101), "not a tile"), (dict(n0=hw + 1, cnt=513), "not a tile"),
              (dict(first=1), "first ="), (dict(first=2), "first ="), (dict(last=0), "last ="), (dict(last=2), "last ="), (dict(cnt=99), "last ="),
              (dict(row=-1), "writes row"), (dict(row=n_rows), "writes row"))
    for kw, what in entry1:
        with pytest.raises(E_, match=what):
            ops.iq_fsk_filter(x, one(items, k, **kw), taps, y, rows)
    with pytest.raises(E_, match="first ="):
        ops.iq_fsk_filter(x, one(items, 0, first=0), taps, y, rows)
    with pytest.raises(E_, match="last ="):
        ops.iq_fsk_filter(x, one(items, 1, last=1), taps, y, rows)               # a full first tile of two may not own the clip's end
    with pytest.raises(E_, match="a row takes one item"):
        ops.iq_fsk_filter(x, np.concatenate((one(items, 0), one(items, 1, row=int(items["row"][0])))), taps, y, rows)
    for bad in (dict(x=x.to(torch.complex128)), dict(x=x[::2]), dict(x=x.cpu()), dict(y=y[:-1]), dict(y=y.double()), dict(y=torch.view_as_real(x)[:, 0]),
                dict(taps=taps.double()), dict(taps=taps[:0]), dict(taps=taps.cpu()), dict(rows=rows.float()), dict(rows=rows[:, :3]), dict(rows=rows[:0]),
                dict(items=items[:0]), dict(items=np.zeros((2, 9), dtype=np.int64))):
        a = dict(x=x, y=y, taps=taps, rows=rows, items=items)
        a.update(bad)
        with pytest.raises(E_):
            ops.iq_fsk_filter(a["x"], a["items"], a["taps"], a["y"], a["rows"])

    def lib1(host_items):
        return table(host_items) + [n_tap, p(taps), n_in, p(x), p(y), n_rows, p(rows), None]
    for pos, v in ((0, 0), (1, None), (2, None), (4, None), (6, None), (7, None), (9, None), (3, 0), (3, n_tap - 1), (5, 0), (5, end - 1), (8, 0), (8, n_rows - 1),
                   (6, C.c_void_p(x.data_ptr() + 4)), (7, C.c_void_p(y.data_ptr() + 2)), (7, p(x)), (9, C.c_void_p(rows.data_ptr() + 4))):
        bad = lib1(items)
        bad[pos] = v
        with pytest.raises(E_):
            _lib.call("sy11_iq_fsk_filter", *bad)
    for kw, _ in entry1:
        with pytest.raises(E_, match="iq_fsk_filter: item 0"):
            _lib.call("sy11_iq_fsk_filter", *lib1(one(items, k, **kw)))
    with pytest.raises(E_, match="an earlier item"):
        _lib.call("sy11_iq_fsk_filter", *lib1(np.concatenate((one(items, 0), one(items, 1, row=int(items["row"][0]))))))
    torch.cuda.synchronize()
    assert bool((y == -7.0).all()) and bool((rows == -7.0).all())                  # no refused call wrote anything
    # ---- launch 2: rebuild the item tables of the shared call from its raw fit
    n_sym, n_blk = int(d.raw["sym0"][-1]), int(d.raw["block0"][-1])
    blocks, decs = np.zeros(n_blk, dtype=BLK), []
    for i in np.flatnonzero(d.plan.valid):
        _, bs, ss = _slices(d, i)
        q = np.arange(bs.stop - bs.start)
        n = ss.stop - ss.start
        blocks["off"][bs], blocks["len"][bs], blocks["step"][bs], blocks["m"][bs] = d.plan.offset[i], d.plan.M[i], d.raw["STEP"][i], d.raw["m"][i]
        blocks["t0"][bs] = [d.raw["T0"][i] + (d.raw["i_first"][i] + int(j) * BLOCK) * d.raw["STEP"][i] for j in q]
        blocks["sym_off"][bs], blocks["n"][bs], blocks["row"][bs] = ss.start + q * BLOCK, np.minimum(n - q * BLOCK, BLOCK), bs.start + q
        if d.valid[i]:
            e = np.zeros(len(q), dtype=DEC)
            e["sym_off"], e["n"], e["row"], e["f0"], e["dev"] = blocks["sym_off"][bs], blocks["n"][bs], blocks["row"][bs], d.raw["f0"][i], d.raw["dev"][i]
            decs.append(e)
    decs = np.concatenate(decs)
    yk = d.raw["y"]
    sym = torch.full((n_sym,), -7.0, dtype=torch.float32, device=DEV)
    lr = torch.full((n_blk, 4), -7.0, dtype=torch.float64, device=DEV)
    good_s, good_l = ops.fsk_symbols(yk, blocks, torch.zeros_like(sym), torch.zeros_like(lr))         # the table is the shared call's: the same bits
    assert torch.equal(_bits(good_s), _bits(d.raw["s"])) and torch.equal(_bits(good_l), _bits(d.raw["level_rows"]))
    lb = n_blk - 1                                                            # the last block of the last planned clip (the tone): it ends the symbol buffer
    b = blocks[lb]
    ln = int(b["len"])
    assert int(b["sym_off"]) + int(b["n"]) == n_sym
    k_last = (int(b["t0"]) + (int(b["n"]) - 1) * int(b["step"])) >> 32
    entry2 = ((dict(off=-1), "packed samples"), (dict(len=3), "packed samples"), (dict(off=n_in - ln + 1), "packed samples"),
              (dict(n=0), "packed symbols"), (dict(n=257), "packed symbols"), (dict(sym_off=-1), "packed symbols"), (dict(sym_off=int(b["sym_off"]) + 1), "packed symbols"),
              (dict(step=2 ** 32 - 1), "Q32.32"), (dict(step=2 ** 40 + 1), "Q32.32"), (dict(t0=2 ** 32 - 1), "Q32.32"), (dict(t0=ln * 2 ** 32), "Q32.32"),
              (dict(len=k_last + 2), "Q32.32"), (dict(m=float("nan")), "not finite"), (dict(m=-float("inf")), "not finite"), (dict(row=-1), "writes row"),
              (dict(row=n_blk), "writes row"))
    for kw, what in entry2:
        with pytest.raises(E_, match=what):
            ops.fsk_symbols(yk, one(blocks, lb, **kw), sym, lr)
    with pytest.raises(E_, match="a row takes one item"):
        ops.fsk_symbols(yk, np.concatenate((one(blocks, 0), one(blocks, 1, row=int(blocks["row"][0])))), sym, lr)
    for bad in (dict(y=yk.double()), dict(y=yk.cpu()), dict(y=yk[::2]), dict(sym=sym.double()), dict(sym=sym[:0]), dict(sym=yk), dict(rows=lr.float()),
                dict(rows=lr[:, :3]), dict(items=blocks[:0]), dict(items=np.zeros((2, 7), dtype=np.int64))):
        a = dict(y=yk, sym=sym, rows=lr, items=blocks)
        a.update(bad)
        with pytest.raises(E_):
            ops.fsk_symbols(a["y"], a["items"], a["sym"], a["rows"])

    def lib2(host_items):
        return table(host_items) + [n_in, p(yk), n_sym, p(sym), n_blk, p(lr), None]
    for pos, v in ((0, 0), (1, None), (2, None), (4, None), (6, None), (8, None), (3, 0), (3, end - 1), (5, 0), (5, n_sym - 1), (7, 0), (7, n_blk - 1),
                   (4, C.c_void_p(yk.data_ptr() + 2)), (6, C.c_void_p(sym.data_ptr() + 2)), (6, p(yk)), (8, C.c_void_p(lr.data_ptr() + 4))):
        bad = lib2(blocks)
        bad[pos] = v
        with pytest.raises(E_):
            _lib.call("sy11_fsk_symbols", *bad)
    for kw, _ in entry2:
        with pytest.raises(E_, match="fsk_symbols: item 0"):
            _lib.call("sy11_fsk_symbols", *lib2(one(blocks, lb, **kw)))
    with pytest.raises(E_, match="an earlier item"):
        _lib.call("sy11_fsk_symbols", *lib2(np.concatenate((one(blocks, 0), one(blocks, 1, row=int(blocks["row"][0]))))))
    torch.cuda.synchronize()
    assert bool((sym == -7.0).all()) and bool((lr == -7.0).all())
    # ---- launch 3
    r = torch.full((n_sym,), -7.0, dtype=torch.complex64, device=DEV)
    dd = torch.full((n_sym,), 7, dtype=torch.uint8, device=DEV)
    er = torch.full((n_blk, 3), -7.0, dtype=torch.float64, device=DEV)
    g_r, g_d, g_e = ops.fsk_decide(good_s, decs, torch.zeros_like(r), torch.zeros_like(dd), torch.zeros_like(er))
    for i in np.flatnonzero(d.valid):
        _, bs, ss = _slices(d, i)
        assert torch.equal(_bits(g_r[ss]), _bits(d.symbols[i])) and torch.equal(g_d[ss], d.decisions[i]) and torch.equal(_bits(g_e[bs]), _bits(d.raw["decision_rows"][bs]))
    le = decs.shape[0] - 1
    e = decs[le]
    entry3 = ((dict(n=0), "packed symbols"), (dict(n=257), "packed symbols"), (dict(sym_off=-1), "packed symbols"), (dict(sym_off=n_sym - int(e["n"]) + 1), "packed symbols"),
              (dict(dev=0.0), "dev positive"), (dict(dev=-1.0), "dev positive"), (dict(dev=float("nan")), "dev positive"), (dict(dev=float("inf")), "dev positive"),
              (dict(f0=float("inf")), "dev positive"), (dict(row=-1), "writes row"), (dict(row=n_blk), "writes row"))
    for kw, what in entry3:
        with pytest.raises(E_, match=what):
            ops.fsk_decide(good_s, one(decs, le, **kw), r, dd, er)
    with pytest.raises(E_, match="a row takes one item"):
        ops.fsk_decide(good_s, np.concatenate((one(decs, 0), one(decs, 0))), r, dd, er)
    for bad in (dict(sym=good_s.double()), dict(sym=good_s.cpu()), dict(r=r[:-1]), dict(r=r.to(torch.complex128)), dict(d=dd[:-1]), dict(d=dd.to(torch.int32)),
                dict(rows=er.float()), dict(rows=er[:, :2]), dict(items=decs[:0]), dict(items=np.zeros((2, 4), dtype=np.int64))):
        a = dict(sym=good_s, r=r, d=dd, rows=er, items=decs)
        a.update(bad)
        with pytest.raises(E_):
            ops.fsk_decide(a["sym"], a["items"], a["r"], a["d"], a["rows"])

    def lib3(host_items):
        return table(host_items) + [n_sym, p(good_s), p(r), p(dd), n_blk, p(er), None]
    for pos, v in ((0, 0), (1, None), (2, None), (4, None), (5, None), (6, None), (8, None), (3, 0), (3, int(e["sym_off"]) + int(e["n"]) - 1), (7, 0), (7, int(e["row"])),
                   (4, C.c_void_p(good_s.data_ptr() + 2)), (5, C.c_void_p(r.data_ptr() + 4)), (5, p(good_s)), (8, C.c_void_p(er.data_ptr() + 4))):
        bad = lib3(decs)
        bad[pos] = v
        with pytest.raises(E_):
            _lib.call("sy11_fsk_decide", *bad)
    for kw, _ in entry3:
        with pytest.raises(E_, match="fsk_decide: item 0"):
            _lib.call("sy11_fsk_decide", *lib3(one(decs, le, **kw)))
    with pytest.raises(E_, match="an earlier item"):
        _lib.call("sy11_fsk_decide", *lib3(np.concatenate((one(decs, 0), one(decs, 0)))))
    torch.cuda.synchronize()
    assert bool((torch.view_as_real(r) == torch.tensor([-7.0, 0.0], device=DEV)).all()) and bool((dd == 7).all()) and bool((er == -7.0).all())


# ------------------------------------------------------------------------------------------------------------- end to end
FS_CAP, DECIMATE, SPS = 4.0e6, 4, 4.0                                         # the capture; the clips are at FS_CLIP with SPS samples per symbol
FS_CLIP = FS_CAP / DECIMATE
CRC = "crc16-ccitt-false"
N_U, N_INFO, N_NEED = 64, 80, 172                                             # message bits; with the check field; channel bits = payload symbols (rate 1/2, six tail bits)
WORD = tuple(int(b) for b in np.random.default_rng(101).integers(0, 2, 32))
OFF_HZ = 2.0e4                                                                # the bursts sit this far off the centre of their boxes
CENTRES = (-1.1e6, 0.6e6, 1.2e6)                                              # of the boxes, Hz from the capture's centre
GAP = 2000


@functools.lru_cache(maxsize=None)
def burst(which):
    """"gfsk" (bt 0.5) or "gmsk" (bt 0.3), both h = 0.5: 24 random bits, the sync word, the K = 7 coded frame of a 64-bit message with its CRC-16, 24 random
    bits -> dict: s (complex128 at the capture's rate, 16 samples per symbol, no noise, ``OFF_HZ`` off 0), x (the same with the capture's noise at the
    clips' rate, as a 4-sample mean makes it: what the CPU test feeds the reference), u, all_bits, u0, lead, bt."""
    bt, seed = (0.5, 31) if which == "gfsk" else (0.3, 32)
    g = np.random.default_rng(seed)
    u = g.integers(0, 2, N_U).astype(np.uint8)
    channel, info = FEC.frame_bits(u, FEC.CRCS[CRC])
    assert channel.shape == (N_NEED,) and info.shape == (N_INFO,)
    bits = np.concatenate((g.integers(0, 2, 24), WORD, channel, g.integers(0, 2, 24))).astype(np.uint8)
    sps = SPS * DECIMATE
    M = int(len(bits) * sps)
    s, all_bits, u0, lead = R.synth(M, seed, sps, 0.5, "gauss", bt, None, OFF_HZ / FS_CAP, bits=bits, u0=0.0)
    noisy = s.astype(np.complex128) + (g.standard_normal(M) + 1j * g.standard_normal(M)) * np.sqrt(0.02)
    x = noisy.reshape(-1, DECIMATE).mean(1).astype(np.complex64)
    # at the clips' rate sample k is the mean of the capture's 4 k .. 4 k + 3: symbol time (4 k + 1.5) / 16 = k / 4 + u0 with u0 = 1.5 / 16
    return {"s": s.astype(np.complex128), "x": x, "u": u, "all_bits": all_bits, "u0": 1.5 / sps, "lead": lead, "bt": bt}


def _capture():
    """A noise capture at 4 MHz (0.04 over 4 MHz: 0.01 in a clip's 1 MHz, 20 dB below a burst) with the GFSK burst, its conjugate (the spectrum
    inverted) and the GMSK burst one after the other, each off the capture's centre in a hand-written box.  -> (capture complex64, tf (3, 4))."""
    parts = (burst("gfsk")["s"], np.conj(burst("gfsk")["s"]), burst("gmsk")["s"])
    n_each = len(parts[0])
    g = np.random.default_rng(6)
    n = 3 * (n_each + GAP) + GAP
    x = (g.standard_normal(n) + 1j * g.standard_normal(n)) * np.sqrt(0.02)
    tf = []
    for i, (s, fcen) in enumerate(zip(parts, CENTRES)):
        a = GAP + i * (n_each + GAP)
        x[a:a + n_each] += s * np.exp(2j * np.pi * fcen / FS_CAP * np.arange(a, a + n_each))
        tf.append((a / FS_CAP, FC + fcen - 2.5e5, (a + n_each - 1) / FS_CAP, FC + fcen + 2.5e5))
    return x.astype(np.complex64), np.array(tf)


@pytest.fixture(scope="module")
def chain():
    """``extract`` (decimation 4) -> ``demodulate_fsk`` -> ``find_frames`` -> ``decode``, and ``equalize`` -> ``decode``, of the three boxes, once; shared and left
    unchanged."""
    from sy11 import _lib
    from sy11.data.spectrogram import open_iq
    from sy11.engine.model import YOLO
    from sy11.engine.predictor import DetectionPredictor, ScanResults
    x, tf = _capture()
    boxes = torch.zeros((3, 6), dtype=torch.float64)
    boxes[:, 4], boxes[:, 5] = torch.tensor([0.9, 0.8, 0.7], dtype=torch.float64), torch.tensor([1.0, 0.0, 1.0], dtype=torch.float64)
    res = ScanResults(boxes, torch.zeros(3, dtype=torch.int64), torch.from_numpy(tf), {0: "a", 1: "b"}, np.zeros(1, dtype=np.int64), FS_CAP, FC)
    pred = DetectionPredictor.__new__(DetectionPredictor)                     # the chain reads the device alone
    pred.device = DEV
    y = YOLO.__new__(YOLO)
    y.device = DEV
    src = open_iq(torch.from_numpy(x))
    ext = pred.extract(src, res, FS_CAP, FC, decimate=DECIMATE)
    _lib.PROFILE = []
    try:
        d = y.demodulate_fsk(ext, symbol_rate=FS_CLIP / SPS, bt=[0.5, 0.5, 0.3])
        calls = [k[0] for k in _lib.PROFILE]
    finally:
        _lib.PROFILE = None
    assert calls == ["sy11_iq_fsk_filter", "sy11_fsk_symbols", "sy11_fsk_decide"]
    f = y.find_frames(d, [list(WORD)], payload=N_NEED, threshold=0.6, t0=ext.t0)
    dec = y.decode(f, d, n_info=N_INFO, crc=CRC)
    eq = y.equalize(f, d)
    dec_eq = pred.decode(f, eq, n_info=N_INFO, crc=CRC)
    return pred, y, src, res, ext, d, f, dec, eq, dec_eq


def test_extract_demodulate_fsk_find_frames_decode_reads_the_bursts_as_sent(chain):
    from sy11.data.demodulate import Demodulation
    from sy11.data.demodulate_fsk import FskDemodulation
    pred, y, src, res, ext, d, f, dec, eq, dec_eq = chain
    assert isinstance(d, FskDemodulation) and isinstance(d, Demodulation) and len(d) == 3 and d.valid.all() and ext.sample_rate.tolist() == [FS_CLIP] * 3
    assert d.order.tolist() == [2, 2, 2] and d.phase_ambiguity.tolist() == [2, 2, 2] and d.cls.tolist() == [1, 0, 1] and d.rows.tolist() == [0, 1, 2]
    assert f.clip.tolist() == [0, 1, 2] and f.rotation.tolist() == [0, 1, 0]     # one frame each; the conjugate's is found inverted
    assert all(15 <= int(v) <= 26 for v in f.position) and f.n_payload.tolist() == [N_NEED] * 3      # 24 bits lead the word, less what the clip's start costs
    sent = [burst("gfsk")["u"], burst("gfsk")["u"], burst("gmsk")["u"]]
    for k in range(3):
        print(f"burst {k}: rho {f.rho[k]:.3f}, position {f.position[k]}, word errors {f.errors[k]}, rotation {f.rotation[k]}, evm {d.evm[k]:.3f}, mod_index {d.mod_index[k]:.3f}, carrier "
              f"{d.carrier_fit[k] - FC - CENTRES[k]:+.0f} Hz off its box, channel errors {dec.channel_errors[k]} of {dec.n_channel[k]}, crc {bool(dec.crc_ok[k])}")
        assert dec.valid[k] and dec.crc_ok[k] and dec.message(k) == np.packbits(sent[k]).tobytes()
        want = OFF_HZ if k != 1 else -OFF_HZ                                  # the conjugate sits on the other side of its box's centre
        assert abs(d.carrier_fit[k] - FC - CENTRES[k] - want) < 0.25 * FS_CLIP / SPS / 4      # a quarter of the deviation h Rs / 2
        assert 0.25 < d.mod_index[k] < 0.5                                    # h = 0.5, less what the two Gaussian filters take off the level means
    # the GMSK burst through the equaliser: the word fits better, and the frame still checks
    assert eq.frames.valid.all() and eq.frames.mse_after[2] < eq.frames.mse_before[2]
    print(f"equalize: mse {np.round(eq.frames.mse_before, 4).tolist()} -> {np.round(eq.frames.mse_after, 4).tolist()}; channel errors {dec.channel_errors.tolist()} -> "
          f"{dec_eq.channel_errors.tolist()}")
    assert dec_eq.valid.all() and dec_eq.crc_ok.all() and dec_eq.message(2) == np.packbits(sent[2]).tobytes()


def test_public_entry_save_and_the_empty_extraction(chain, tmp_path):
    from sy11 import _lib
    pred, y, src, res, ext, d, f, dec, eq, dec_eq = chain
    d2 = pred.demodulate_fsk(ext, symbol_rate=[FS_CLIP / SPS] * 3, offset=0.0, pulse="gauss", bt=[0.5, 0.5, 0.3], span=2, block=32)
    for i in range(3):
        assert torch.equal(_bits(d2.symbols[i]), _bits(d.symbols[i])) and torch.equal(d2.decisions[i], d.decisions[i]) and torch.equal(_bits(d2.filtered[i]), _bits(d.filtered[i]))
    with pytest.raises(ValueError, match="pulse"):
        y.demodulate_fsk(ext, symbol_rate=FS_CLIP / SPS, pulse="rrc")
    out = d.save(tmp_path / "d")
    z = np.load(tmp_path / "d" / "demodulate.npz")
    index = json.loads((tmp_path / "d" / "demodulate.json").read_text())
    assert out == str(tmp_path / "d") and np.array_equal(z["deviation"], d.deviation) and np.array_equal(z["evm"], d.evm) and np.array_equal(z["decisions_1"], d.decisions[1].cpu().numpy())
    assert [k["file"] for k in index["clips"]] == ["symbols_0.cf32", "symbols_1.cf32", "symbols_2.cf32"] and index["bt"] == [0.5, 0.5, 0.3] and index["modulation"] == "fsk"
    assert index["clips"][2]["mod_index"] == float(d.mod_index[2])
    assert np.array_equal(np.fromfile(tmp_path / "d" / "symbols_1.cf32", dtype=np.complex64), d.symbols[1].cpu().numpy())
    none = pred.extract(src, res, FS_CAP, FC, rows=[], decimate=DECIMATE)      # an empty extraction: no launch
    _lib.PROFILE = []
    try:
        e = pred.demodulate_fsk(none, symbol_rate=FS_CLIP / SPS)
        calls = [k[0] for k in _lib.PROFILE]
    finally:
        _lib.PROFILE = None
    assert calls == [] and len(e) == 0 and e.symbols == [] and e.deviation.shape == (0,)
