"""GPU: the OFDM demodulation kernels (sy11_iq_ofdm_fold, sy11_ofdm_fft, sy11_ofdm_decide) on the twelve clips of tests/_ofdm_ref.py in ONE call of three launches.  The fold
rows against the float64 reference to 1e-12 of the row's sum of magnitudes; fit 1 on the kernel's own rows (theta with no tolerance, eps and cp_corr to 1e-12); the pilot and power
rows to 1e-12 of the OFDM symbol's sum of |Y|, Yc to 2^-22 of its largest |Y| (one float32 rounding is 2^-24 relative, a rounding-boundary flip doubles it, the rest is margin); r to
2^-22 on the kernel's own Yc, the decisions equal wherever the reference is further than that from a boundary, the rows and columns to 1e-12; no symbol error against what was sent;
one call against one call per clip and a permuted extraction, bit for bit; the refusals; and ``extract`` -> ``demodulate_ofdm`` -> ``find_frames`` -> ``decode`` on three bursts
embedded in a noise capture, which come out as they were sent.

Largest errors seen on an MI355X (DESIGN.md §5 has the table): fold rows 3.7e-16 (F) and 1.0e-15 (E) of the row's sum of magnitudes; pilot rows 2.5e-17 and power rows 1.9e-14 of the
OFDM symbol's sum of |Y|; Yc equal to f32 of the reference in every entry; r 0.25 of its bar (the one rounding); no symbol error; carrier_fit at most 0.0022 carrier spacings off."""
import ctypes as C
import functools
import json

import numpy as np
import pytest
import torch

from tests import _fec_ref as FEC
from tests import _ofdm_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FC = 2.4e9
A = R.LAYOUT_A


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
    from sy11.data.demodulate_ofdm import demodulate_ofdm_extraction
    order = list(range(len(cs))) if order is None else list(order)
    ext = _extraction([c["x"] for c in cs], order)
    lay = lambda key: [cs[i]["lay"][key] for i in order]                      # noqa: E731
    return ext, demodulate_ofdm_extraction(ext, n_fft=lay("N"), cp=lay("G"), carriers=lay("data"), pilots=[(cs[i]["lay"]["pk"], cs[i]["lay"]["pc"]) for i in order],
                                           order=[cs[i]["order"] for i in order], spacing=[cs[i]["spacing"] for i in order])


def _bits(t):
    t = torch.view_as_real(t) if t.is_complex() else t
    return t.contiguous().view({torch.float64: torch.int64, torch.float32: torch.int32, torch.uint8: torch.uint8}[t.dtype])


def _sl(d, key, i):
    return slice(int(d.raw[key][i]), int(d.raw[key][i + 1]))


@pytest.fixture(scope="module")
def case():
    """The twelve clips, their extraction and ONE demodulation (three launches); shared and left unchanged."""
    from sy11 import _lib
    cs = R.case_clips()
    _lib.PROFILE = []
    try:
        ext, d = _demod(cs)
        calls = [k[0] for k in _lib.PROFILE]
    finally:
        _lib.PROFILE = None
    assert calls == ["sy11_iq_ofdm_fold", "sy11_ofdm_fft", "sy11_ofdm_decide"]                    # three launches, whatever the number of clips and layouts
    assert d.valid.tolist() == [c["kind"] in ("ofdm", "zero") for c in cs]
    assert d.reason.tolist() == [{"ofdm": "", "zero": "", "short": "short", "rate": "rate", "order": "order"}[c["kind"]] for c in cs]
    assert len(d.plan.layouts) == 5 and d.plan.splits[:8].tolist() == [1, 1, 3, 1, 1, 1, 1, 3] and int(ext.plan.offset[1]) % 2 == 1      # a clip at an odd sample
    host = {"yc": d.raw["yc"].cpu().numpy(), "u": d.raw["pilots"].cpu().numpy(), "pw": d.raw["power"].cpu().numpy(), "rows": d.raw["decision_rows"].cpu().numpy(),
            "r": [v.cpu().numpy() for v in d.symbols], "d": [v.cpu().numpy() for v in d.decisions], "fold": d.raw["fold"].cpu().numpy()}
    assert host["yc"].dtype == np.complex64 and host["u"].dtype == np.complex128 and host["pw"].dtype == np.float64
    return cs, ext, d, host


def _live(cs):
    return [i for i, c in enumerate(cs) if c["kind"] in ("ofdm", "zero")]


# ------------------------------------------------------------------------------------------------------------- launch 1 and fit 1
def test_fold_rows_match_the_float64_reference(case):
    cs, ext, d, host = case
    for i, c in enumerate(cs):
        if i not in _live(cs):
            assert d.raw["F"][i].shape == (0,) and int(d.plan.splits[i]) == 0 and int(d.raw["fold0"][i]) == int(d.raw["fold0"][i + 1])
            continue
        lay = c["lay"]
        F, E, sF, sE = R.fold(c["x"], lay["N"], lay["G"])
        assert d.raw["F"][i].shape == F.shape == (lay["S"],)
        part = host["fold"][_sl(d, "fold0", i)].reshape(int(d.plan.splits[i]), lay["S"], 3)
        assert np.array_equal(d.raw["F"][i], part[..., 0].sum(0) + 1j * part[..., 1].sum(0)) or int(d.plan.splits[i]) > 2      # two rows add in one order only
        with np.errstate(invalid="ignore", divide="ignore"):
            eF, eE = np.nan_to_num(np.abs(d.raw["F"][i] - F) / sF), np.nan_to_num(np.abs(d.raw["E"][i] - E) / sE)
        print(f"iq_ofdm_fold[{c['label']}: M={len(c['x'])} S={lay['S']} splits={int(d.plan.splits[i])}]: largest error F {eF.max():.2e}, E {eE.max():.2e} of the row's sum of magnitudes")
        assert (np.abs(d.raw["F"][i] - F) <= 1e-12 * sF).all() and (np.abs(d.raw["E"][i] - E) <= 1e-12 * sE).all()


def test_fit_1_equals_the_reference_on_the_kernels_own_rows(case):
    cs, ext, d, host = case
    for i in _live(cs):
        c, lay = cs[i], cs[i]["lay"]
        f = R.fit1(d.raw["F"][i], d.raw["E"][i], lay["N"], lay["G"])
        assert int(d.raw["theta"][i]) == f["theta"] == int(d.timing[i]) and abs(d.cfo[i] - f["eps"]) <= 1e-12 and abs(d.cp_corr[i] - f["cp_corr"]) <= 1e-12
        st = R.starts(f["theta"], len(c["x"]), lay)
        assert (d.raw["start"][i], int(d.n_ofdm[i])) == (int(st[0]), len(st)) and d.raw["W"][i] == R.word(0.0, float(d.cfo[i]), lay["N"])
        assert d.raw["T0"][i] == int(st[0]) << 32 and d.raw["STEP"][i] == round(lay["S"] / len(lay["data"]) * 2 ** 32) and d.raw["i_first"][i] == 0


# ------------------------------------------------------------------------------------------------------------- launch 2
def test_carrier_values_pilot_rows_and_power_rows_match_the_reference(case):
    cs, ext, d, host = case
    for i in _live(cs):
        c, lay = cs[i], cs[i]["lay"]
        n, st = int(d.n_ofdm[i]), d.raw["start"][i] + np.arange(int(d.n_ofdm[i])) * lay["S"]
        Y, u, pw, k = R.spectra(c["x"], st, d.raw["W"][i], lay)
        yc, gu, gp = host["yc"][_sl(d, "yc0", i)].reshape(n, len(k)), host["u"][_sl(d, "pil0", i)].reshape(n, len(lay["pk"])), host["pw"][_sl(d, "pow0", i)]
        assert torch.equal(d.filtered[i], d.raw["yc"][_sl(d, "yc0", i)].view(n, len(k))) and k.tolist() == d.plan.lay(i).used.tolist()
        mag, top = np.abs(Y).sum(1), np.abs(Y).max(1)
        e_u, e_p = np.abs(gu - u).max(1), np.abs(gp - pw)
        want = Y.astype(np.complex64)
        e_y = np.maximum(np.abs(yc.real.astype(np.float64) - want.real), np.abs(yc.imag.astype(np.float64) - want.imag)).max(1)
        with np.errstate(invalid="ignore", divide="ignore"):
            print(f"ofdm_fft[{c['label']}: N={lay['N']} {n} OFDM symbols]: largest error pilots {np.nan_to_num(e_u / mag).max():.2e}, power {np.nan_to_num(e_p / mag).max():.2e} of sum |Y|; "
                  f"Yc {np.nan_to_num(e_y / top).max() * 2.0 ** 22:.2f} of 2^-22 max |Y|")
        assert (e_u <= 1e-12 * mag).all() and (e_p <= 1e-12 * mag).all() and (e_y <= 2.0 ** -22 * top).all()
        if c["kind"] == "zero":
            assert not yc.any() and not gu.any() and not gp.any()


# ------------------------------------------------------------------------------------------------------------- fit 2, launch 3, columns
def test_decisions_rows_and_columns_match_the_reference_on_the_kernels_own_values(case):
    cs, ext, d, host = case
    for i, c in enumerate(cs):
        if i not in _live(cs):
            assert np.isnan([d.gain[i], d.evm[i], d.cfo[i], d.carrier_fit[i], d.slope[i]]).all() and d.phase_ambiguity[i] == -1 and int(d.n_symbols[i]) == -1
            assert d.symbols[i].shape == (0,) and d.decisions[i].shape == (0,) and d.filtered[i].shape == (0,) and int(d.n_ofdm[i]) == -1
            continue
        lay, order = c["lay"], c["order"]
        n, nd = int(d.n_ofdm[i]), len(lay["data"])
        u = host["u"][_sl(d, "pil0", i)].reshape(n, len(lay["pk"]))
        f = R.fit2(u, lay)
        assert np.array_equal(d.raw["active"][i], f["active"]) and abs(d.slope[i] - f["beta"]) <= 1e-12 and int(d.n_active[i]) == int(f["active"].sum())
        assert np.abs(d.raw["phi"][i] - f["phi"]).max() <= 1e-12 and abs(d.raw["A"][i] - f["A"]) <= 1e-12 * f["A"]
        k = d.plan.lay(i).used
        yc = host["yc"][_sl(d, "yc0", i)].reshape(n, len(k))
        r, r32, dec = R.decide(yc, f["rho"], f["tau"], lay, order, k)
        got, gd = host["r"][i].reshape(n, nd), host["d"][i].reshape(n, nd)
        assert got.dtype == np.complex64 and gd.dtype == np.uint8 and int(d.n_symbols[i]) == n * nd and np.isfinite(got.view(np.float32)).all()
        err = np.maximum(np.abs(got.real.astype(np.float64) - r.real), np.abs(got.imag.astype(np.float64) - r.imag))
        far = np.abs(r.real) > 2.0 ** -22 if order == 2 else (np.abs(r.real) > 2.0 ** -22) & (np.abs(r.imag) > 2.0 ** -22)
        print(f"ofdm_decide[{c['label']}]: largest |r - ref| {err.max() * 2.0 ** 22:.2f} of 2^-22; {int((~far).sum())} of {n * nd} decisions exempt")
        assert err.max() <= 2.0 ** -22 and np.array_equal(gd[far], dec[far])
        rows, mine = R.rows_of(got, gd, order), host["rows"][_sl(d, "pow0", i)]
        scale = np.stack(((np.abs(got.astype(np.complex128)) ** 2).sum(1), np.abs(got.astype(np.complex128)).sum(1) * np.sqrt(2.0), np.ones(n)), axis=1)
        assert mine.shape == rows.shape == (n, 3) and np.array_equal(mine[:, 2], rows[:, 2]) and (np.abs(mine - rows) <= 1e-12 * scale).all()
        col = R.columns(mine, f["active"])
        for key in ("gain", "evm", "mer_db"):
            assert np.array_equal([getattr(d, key)[i]], [col[key]], equal_nan=True) or abs(getattr(d, key)[i] - col[key]) <= 1e-12 * abs(col[key]), (c["label"], key)
        df = R.FS / lay["N"]
        assert abs(d.carrier_fit[i] - (FC + d.cfo[i] * df)) <= 1e-12 * FC and abs(d.symbol_rate_fit[i] - nd * R.FS / lay["S"]) <= 1e-9
        assert d.phase_ambiguity[i] == 1 and d.order[i] == order and np.array_equal(d.bits(i).reshape(n * nd, -1), np.stack(((gd.reshape(-1) >> 1) & 1, gd.reshape(-1) & 1), 1)[:, 2 - order // 2:])
        if c["kind"] == "zero":
            assert d.gain[i] == 0.0 and not got.any() and not gd.any() and not mine[:, :2].any() and d.cp_corr[i] == 0.0 and d.raw["active"][i].all()
            continue
        st = d.raw["start"][i] + np.arange(n) * lay["S"]
        bad, exact, miss = R.symbol_errors(gd, d.raw["active"][i], st, c)
        print(f"demodulate_ofdm[{c['label']}]: {bad} symbol errors on {int(d.n_active[i])} active of {n} OFDM symbols, theta {int(d.timing[i])} ({miss} off), evm {d.evm[i]:.4f}, "
              f"carrier {(d.carrier_fit[i] - FC) / df - c['eps']:+.4f} spacings off, cp_corr {d.cp_corr[i]:.3f}")
        assert bad == 0 and exact and miss <= 2 and abs(d.carrier_fit[i] - FC - c["eps"] * df) < 0.02 * df
    assert d[0]["valid"] and d[0]["reason"] == "" and d[8]["reason"] == "short" and d[9]["reason"] == "rate" and d[10]["reason"] == "order"
    assert d.cls.tolist() == ext.cls.tolist() and d.names == ext.names and d.rows.tolist() == ext.rows.tolist()
    assert int(d.n_ofdm[2]) > 32 and int(d.n_ofdm[2]) % 16 and int(d.n_active[2]) == 37                 # two full groups and a ragged one


# ------------------------------------------------------------------------------------------------------------- invariance
def test_one_call_per_clip_and_a_permuted_extraction_give_the_same_bits(case):
    cs, ext, d, host = case
    perm = [4, 11, 8, 2, 0, 9, 7, 5, 10, 3, 1, 6]
    pext, p = _demod(cs, perm)
    assert p.rows.tolist() == perm
    for at, i in enumerate(perm):
        for other, k in ((p, at), (_demod([cs[i]])[1], 0)):
            assert bool(other.valid[k]) == bool(d.valid[i]) and other.reason[k] == d.reason[i] and int(other.n_symbols[k]) == int(d.n_symbols[i])
            for key in ("symbols", "decisions", "filtered"):
                assert torch.equal(_bits(getattr(other, key)[k]), _bits(getattr(d, key)[i])), (i, at, key)
            if not d.valid[i]:
                continue
            for key, off in (("fold", "fold0"), ("pilots", "pil0"), ("power", "pow0"), ("decision_rows", "pow0")):
                assert torch.equal(_bits(other.raw[key][_sl(other, off, k)]), _bits(d.raw[key][_sl(d, off, i)])), (i, at, key)
            assert np.array_equal(other.raw["F"][k], d.raw["F"][i]) and np.array_equal(other.raw["phi"][k], d.raw["phi"][i])
            assert (other.raw["start"][k], other.raw["W"][k], other.raw["T0"][k]) == (d.raw["start"][i], d.raw["W"][i], d.raw["T0"][i])
            for key in d.COLUMNS:
                assert np.array_equal(getattr(other, key)[k:k + 1], getattr(d, key)[i:i + 1], equal_nan=True), (i, at, key)


# ------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_raise_and_write_nothing(case):
    from sy11 import _lib, ops
    from sy11.data.demodulate_ofdm import twiddle_table
    cs, ext, d, host = case
    E_ = _lib.Sy11Error
    p = lambda v: C.c_void_p(v.data_ptr())                                    # noqa: E731
    keep = []

    def table(host_items):
        host_items = np.ascontiguousarray(host_items)
        t = torch.from_numpy(host_items.view(np.uint8).copy()).to(DEV)
        keep.extend((host_items, t))
        return [host_items.shape[0], C.c_void_p(host_items.ctypes.data), p(t)]

    def one(items, k, **kw):
        s = items[k:k + 1].copy()
        for key, v in kw.items():
            s[key] = v
        return s
    T = d.raw["tables"]
    x, n_in = ext.packed, ext.packed.shape[0]
    # ---- launch 1
    fold_items, n_out = T["fold"], d.plan.total_triples
    out = torch.full((n_out, 3), -7.0, dtype=torch.float64, device=DEV)
    good = ops.iq_ofdm_fold(x, fold_items, torch.zeros_like(out))                 # the table is the shared call's: the same bits
    assert torch.equal(_bits(good), _bits(d.raw["fold"]))
    k = int(np.flatnonzero((fold_items["S"] == 80) & (fold_items["m0"] == 32) & (fold_items["r0"] == 64))[0])      # the last split and tile of the clip of 38 periods
    it = fold_items[k]
    assert (int(it["cnt_m"]), int(it["cnt_r"])) == (6, 16)
    ln = int(it["len"])
    entry1 = ((dict(n_fft=96), "not one of"), (dict(n_fft=2048), "not one of"), (dict(n_fft=0), "not one of"), (dict(S=64), "a period"), (dict(S=97), "a period"),
              (dict(off=-1), "packed samples"), (dict(len=0), "packed samples"), (dict(off=n_in - ln + 1), "packed samples"), (dict(len=n_in + 1, off=0), "packed samples"),
              (dict(r0=-64), "not a tile"), (dict(r0=60, cnt_r=20), "not a tile"), (dict(r0=128, cnt_r=16), "not a tile"), (dict(cnt_r=17), "not a tile"), (dict(cnt_r=15), "not a tile"),
              (dict(cnt_r=0), "not a tile"), (dict(m0=-16), "not a split"), (dict(m0=30, cnt_m=8), "not a split"), (dict(cnt_m=7), "not a split"), (dict(cnt_m=5), "not a split"),
              (dict(cnt_m=0), "not a split"), (dict(m0=48, cnt_m=1), "not a split"), (dict(len=64 + 38 * 80 - 1), "not a split"), (dict(m0=16, cnt_m=17), "not a split"),
              (dict(out_off=-1), "writes triples"), (dict(out_off=n_out - 15), "writes triples"))
    for kw, what in entry1:
        with pytest.raises(E_, match=what):
            ops.iq_ofdm_fold(x, one(fold_items, k, **kw), out)
    with pytest.raises(E_, match="an earlier item"):
        ops.iq_ofdm_fold(x, np.concatenate((one(fold_items, 0), one(fold_items, 1, out_off=int(fold_items["out_off"][0]) + 63))), out)
    with pytest.raises(ValueError, match="records"):
        ops.iq_ofdm_fold(x, np.zeros((2, 6), dtype=np.int64), out)
    with pytest.raises(ValueError, match="records"):
        ops.iq_ofdm_fold(x, fold_items[:0], out)
    for bad in (dict(x=x.to(torch.complex128)), dict(x=x[::2]), dict(x=x.cpu()), dict(out=out.float()), dict(out=out[:, :2]), dict(out=out[:0])):
        a = dict(x=x, out=out)
        a.update(bad)
        with pytest.raises(E_):
            ops.iq_ofdm_fold(a["x"], fold_items, a["out"])

    def lib1(host_items):
        return table(host_items) + [n_in, p(x), n_out, p(out), None]
    end = int(max(fold_items["off"] + fold_items["len"]))
    for pos, v in ((0, 0), (1, None), (2, None), (4, None), (6, None), (3, 0), (3, end - 1), (5, 0), (5, n_out - 1), (4, C.c_void_p(x.data_ptr() + 4)),
                   (6, C.c_void_p(out.data_ptr() + 4))):
        bad = lib1(fold_items)
        bad[pos] = v
        with pytest.raises(E_):
            _lib.call("sy11_iq_ofdm_fold", *bad)
    for kw, _ in entry1:
        with pytest.raises(E_, match="iq_ofdm_fold: item 0"):
            _lib.call("sy11_iq_ofdm_fold", *lib1(one(fold_items, k, **kw)))
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())                                          # no refused call wrote anything
    # ---- launch 2
    fft_items, bins = T["fft"], T["bins"]
    tw = torch.view_as_real(torch.from_numpy(twiddle_table())).contiguous().to(DEV)
    n_yc, n_pil, n_pow, n_bin = d.raw["yc"].shape[0], d.raw["pilots"].shape[0], d.raw["power"].shape[0], bins.shape[0]
    yc = torch.full((n_yc,), -7.0, dtype=torch.complex64, device=DEV)
    pil = torch.full((n_pil,), -7.0, dtype=torch.complex128, device=DEV)
    pw = torch.full((n_pow,), -7.0, dtype=torch.float64, device=DEV)
    gy, gp, gw = torch.zeros_like(yc), torch.zeros_like(pil), torch.zeros_like(pw)
    ops.ofdm_fft(x, fft_items, bins, tw, gy, gp, gw)
    assert torch.equal(_bits(gy), _bits(d.raw["yc"])) and torch.equal(_bits(gp), _bits(d.raw["pilots"])) and torch.equal(_bits(gw), _bits(d.raw["power"]))
    k = int(np.flatnonzero(fft_items["n_fft"] == 64)[2])                      # the clip of 37 OFDM symbols: its first group (the first two clips have one group each)
    it = fft_items[k]
    assert int(it["nf"]) == 16 and int(fft_items["nf"][k + 2]) < 16
    ln, st = int(it["len"]), int(it["start"])
    entry2 = ((dict(n_fft=96), "not one of"), (dict(n_fft=32), "not one of"), (dict(S=64), "a period"), (dict(S=97), "a period"), (dict(a=-1), "a period"), (dict(a=17), "a period"),
              (dict(off=-1), "packed samples"), (dict(len=0), "packed samples"), (dict(off=n_in - ln + 1), "packed samples"),
              (dict(nf=0), "OFDM symbols"), (dict(nf=17), "OFDM symbols"), (dict(start=-1), "OFDM symbols"), (dict(start=ln - 64 - 15 * 80 + 1), "OFDM symbols"),
              (dict(len=st + 15 * 80 + 63), "OFDM symbols"), (dict(n_fft=128, S=160, a=8, nf=9), "OFDM symbols"),
              (dict(n_used=0), "carriers"), (dict(n_used=64), "carriers"), (dict(n_pil=0), "carriers"), (dict(n_pil=53), "carriers"), (dict(bin_off=-1), "carriers"),
              (dict(bin_off=n_bin - 51), "carriers"), (dict(bin_off=1), "pilot|ascending"), (dict(n_pil=3), "names pilot"), (dict(n_pil=5), "of its 5 pilots"),
              (dict(n_fft=64, bin_off=int(d.plan.bin0[1]), n_used=52, n_pil=4), "ascending|pilot"),
              (dict(yc_off=-1), "writes carrier values"), (dict(yc_off=n_yc - 16 * 52 + 1), "writes carrier values"), (dict(pil_off=-1), "writes carrier values"),
              (dict(pil_off=n_pil - 16 * 4 + 1), "writes carrier values"), (dict(pow_off=-1), "writes carrier values"), (dict(pow_off=n_pow - 15), "writes carrier values"))
    for kw, what in entry2:
        with pytest.raises(E_, match=what):
            ops.ofdm_fft(x, one(fft_items, k, **kw), bins, tw, yc, pil, pw)
    nk = bins.copy()
    nk["k"][3] = 32
    with pytest.raises(E_, match="ascending"):
        ops.ofdm_fft(x, one(fft_items, k), nk, tw, yc, pil, pw)
    for key, v in (("yc_off", int(it["yc_off"]) + 16 * 52 - 1), ("pil_off", int(it["pil_off"]) + 63), ("pow_off", int(it["pow_off"]) + 15)):
        far = dict(yc_off=int(fft_items["yc_off"][0]), pil_off=int(fft_items["pil_off"][0]), pow_off=int(fft_items["pow_off"][0]), nf=int(fft_items["nf"][0]))
        far[key] = v
        with pytest.raises(E_, match="an earlier item"):
            ops.ofdm_fft(x, np.concatenate((one(fft_items, k), one(fft_items, k, **far))), bins, tw, yc, pil, pw)
    with pytest.raises(ValueError, match="records"):
        ops.ofdm_fft(x, np.zeros((2, 11), dtype=np.int64), bins, tw, yc, pil, pw)
    with pytest.raises(ValueError, match="records"):
        ops.ofdm_fft(x, fft_items, bins.view(np.int64), tw, yc, pil, pw)
    for bad in (dict(x=x.cpu()), dict(x=x[::2]), dict(tw=tw[:256]), dict(tw=tw.float()), dict(tw=tw.cpu()), dict(yc=yc.to(torch.complex128)), dict(yc=yc[:0]), dict(pil=pil.to(torch.complex64)),
                dict(pil=pil[1:]), dict(pw=pw.float()), dict(pw=pw[:0])):
        a = dict(x=x, tw=tw, yc=yc, pil=pil, pw=pw)
        a.update(bad)
        with pytest.raises(E_):
            ops.ofdm_fft(a["x"], fft_items, bins, a["tw"], a["yc"], a["pil"], a["pw"])

    def lib2(host_items, host_bins=bins):
        return table(host_items) + table(host_bins) + [p(tw), n_in, p(x), n_yc, p(yc), n_pil, p(pil), n_pow, p(pw), None]
    for pos, v in ((0, 0), (1, None), (2, None), (3, 0), (4, None), (5, None), (6, None), (8, None), (10, None), (12, None), (14, None), (3, n_bin - 1), (7, 0), (7, end - 1),
                   (9, 0), (9, n_yc - 1), (11, 0), (11, n_pil - 1), (13, 0), (13, n_pow - 1), (6, C.c_void_p(tw.data_ptr() + 8)), (8, C.c_void_p(x.data_ptr() + 4)),
                   (10, C.c_void_p(yc.data_ptr() + 4)), (10, p(x)), (12, C.c_void_p(pil.data_ptr() + 8)), (14, C.c_void_p(pw.data_ptr() + 4))):
        bad = lib2(fft_items)
        bad[pos] = v
        with pytest.raises(E_):
            _lib.call("sy11_ofdm_fft", *bad)
    for kw, _ in entry2:
        with pytest.raises(E_, match="ofdm_fft: item 0"):
            _lib.call("sy11_ofdm_fft", *lib2(one(fft_items, k, **kw)))
    torch.cuda.synchronize()
    assert bool((torch.view_as_real(yc) == -7.0).any(1).all()) and bool((torch.view_as_real(pil) == -7.0).any(1).all()) and bool((pw == -7.0).all())
    # ---- launch 3
    dec_items, cars = T["dec"], T["cars"]
    n_sym, n_rows, n_car = int(d.raw["sym0"][-1]), n_pow, cars.shape[0]
    r = torch.full((n_sym,), -7.0, dtype=torch.complex64, device=DEV)
    dd = torch.full((n_sym,), 7, dtype=torch.uint8, device=DEV)
    er = torch.full((n_rows, 3), -7.0, dtype=torch.float64, device=DEV)
    g_r, g_d, g_e = torch.zeros_like(r), torch.zeros_like(dd), torch.zeros_like(er)
    ops.ofdm_decide(gy, dec_items, cars, g_r, g_d, g_e)
    for i in _live(cs):
        assert torch.equal(_bits(g_r[_sl(d, "sym0", i)]), _bits(d.symbols[i])) and torch.equal(g_d[_sl(d, "sym0", i)], d.decisions[i])
        assert torch.equal(_bits(g_e[_sl(d, "pow0", i)]), _bits(d.raw["decision_rows"][_sl(d, "pow0", i)]))
    k = dec_items.shape[0] - 1                                                # the last OFDM symbol of the last valid clip: it ends every buffer
    it = dec_items[k]
    assert int(it["sym_off"]) + int(it["n_data"]) == n_sym and int(it["yc_off"]) + int(it["n_used"]) == n_yc and int(it["car_off"]) + int(it["n_data"]) == n_car
    entry3 = ((dict(n_used=0), "data carriers"), (dict(n_used=1024), "data carriers"), (dict(n_data=0), "data carriers"), (dict(n_data=53), "data carriers"), (dict(car_off=-1), "data carriers"),
              (dict(car_off=int(it["car_off"]) + 1), "data carriers"), (dict(yc_off=-1), "carrier values"), (dict(yc_off=int(it["yc_off"]) + 1), "carrier values"),
              (dict(sym_off=-1), "packed symbols"), (dict(sym_off=int(it["sym_off"]) + 1), "packed symbols"), (dict(order=3), "order 3"), (dict(order=0), "order 0"),
              (dict(rho_r=float("nan")), "rho"), (dict(rho_i=float("inf")), "rho"), (dict(n_used=48), "reads value"), (dict(row=-1), "writes row"), (dict(row=n_rows), "writes row"))
    for kw, what in entry3:
        with pytest.raises(E_, match=what):
            ops.ofdm_decide(gy, one(dec_items, k, **kw), cars, r, dd, er)
    for key, v in (("tr", float("nan")), ("ti", -float("inf")), ("idx", -1), ("idx", 52)):
        nc = cars.copy()
        nc[key][n_car - 2] = v
        with pytest.raises(E_, match="reads value"):
            ops.ofdm_decide(gy, one(dec_items, k), nc, r, dd, er)
    with pytest.raises(E_, match="an earlier item"):
        ops.ofdm_decide(gy, np.concatenate((one(dec_items, k), one(dec_items, k))), cars, r, dd, er)
    with pytest.raises(E_, match="an earlier item"):
        ops.ofdm_decide(gy, np.concatenate((one(dec_items, k), one(dec_items, k - 1, sym_off=int(it["sym_off"]) - 47))), cars, r, dd, er)
    with pytest.raises(ValueError, match="records"):
        ops.ofdm_decide(gy, np.zeros((2, 7), dtype=np.int64), cars, r, dd, er)
    with pytest.raises(ValueError, match="records"):
        ops.ofdm_decide(gy, dec_items, cars[:0], r, dd, er)
    for bad in (dict(yc=gy.to(torch.complex128)), dict(yc=gy.cpu()), dict(r=r[:-1], d=dd), dict(r=r.to(torch.complex128)), dict(d=dd[:-1]), dict(d=dd.to(torch.int32)),
                dict(rows=er.float()), dict(rows=er[:, :2]), dict(r=gy, d=torch.zeros(n_yc, dtype=torch.uint8, device=DEV))):
        a = dict(yc=gy, r=r, d=dd, rows=er)
        a.update(bad)
        with pytest.raises(E_):
            ops.ofdm_decide(a["yc"], dec_items, cars, a["r"], a["d"], a["rows"])

    def lib3(host_items, host_cars=cars):
        return table(host_items) + table(host_cars) + [n_yc, p(gy), n_sym, p(r), p(dd), n_rows, p(er), None]
    for pos, v in ((0, 0), (1, None), (2, None), (3, 0), (4, None), (5, None), (7, None), (9, None), (10, None), (12, None), (3, n_car - 1), (6, 0), (6, n_yc - 1), (8, 0),
                   (8, n_sym - 1), (11, 0), (11, n_rows - 1), (7, C.c_void_p(gy.data_ptr() + 4)), (9, C.c_void_p(r.data_ptr() + 4)), (9, p(gy)), (12, C.c_void_p(er.data_ptr() + 4))):
        bad = lib3(dec_items)
        bad[pos] = v
        with pytest.raises(E_):
            _lib.call("sy11_ofdm_decide", *bad)
    for kw, _ in entry3:
        with pytest.raises(E_, match="ofdm_decide: item 0"):
            _lib.call("sy11_ofdm_decide", *lib3(one(dec_items, k, **kw)))
    torch.cuda.synchronize()
    assert bool((torch.view_as_real(r) == torch.tensor([-7.0, 0.0], device=DEV)).all()) and bool((dd == 7).all()) and bool((er == -7.0).all())


# ------------------------------------------------------------------------------------------------------------- end to end
FS_CAP, DECIMATE = 4.0e6, 4                                                   # the capture; the clips are at FS_CLIP = 64 carrier spacings
FS_CLIP = FS_CAP / DECIMATE
DF = FS_CLIP / 64
CRC = "crc16-ccitt-false"
N_U, N_INFO, N_NEED = 64, 80, 172                                             # message bits; with the check field; channel bits (rate 1/2, six tail bits)
WORD = tuple(int(b) for b in np.random.default_rng(101).integers(0, 2, 32))
EPS = 0.2                                                                     # the bursts sit this many carrier spacings off the centre of their boxes
CENTRES = (-1.1e6, 0.6e6, 1.2e6)                                              # of the boxes, Hz from the capture's centre
LEAD, GAP, PRE = 200, 2000, 20                                                # capture samples of a box before its burst; between the boxes; random symbols before the word
ORDERS = (4, 2, 4)


@functools.lru_cache(maxsize=None)
def burst(which):
    """Burst 0 (QPSK), 1 (BPSK) or 2 (QPSK through the channel of case 8, its taps one clip sample apart), in the 802.11a layout: ``PRE`` random symbols, the sync word, the
    K = 7 coded frame of a 64-bit message with its CRC-16, random symbols up to whole OFDM symbols -> dict: s (complex128 at the capture's rate: a 256-point IFFT and a prefix of
    64, ``LEAD`` samples before and after, no noise, ``EPS`` carrier spacings off 0), x (the same with the capture's noise: what the CPU test feeds the reference), dec (the
    decisions sent, (OFDM symbols, 48)), u (the message bits), p0 (the word's first symbol), order."""
    order = ORDERS[which]
    g = np.random.default_rng(41 + which)
    w = order // 2
    u = g.integers(0, 2, N_U).astype(np.uint8)
    channel, info = FEC.frame_bits(u, FEC.CRCS[CRC], order=order)
    assert channel.shape == (N_NEED,) and info.shape == (N_INFO,)
    bits = np.concatenate((g.integers(0, 2, PRE * w), WORD, channel)).astype(np.uint8)
    n_ofdm = -(-(bits.shape[0] // w) // 48)
    bits = np.concatenate((bits, g.integers(0, 2, n_ofdm * 48 * w - bits.shape[0]).astype(np.uint8)))
    dec = (bits if order == 2 else 2 * bits[0::2] + bits[1::2]).astype(np.uint8).reshape(n_ofdm, 48)
    ch = None
    if which == 2:
        ch = np.zeros(4 * DECIMATE + 1, dtype=np.complex128)
        ch[::DECIMATE] = R.CHANNEL
    s, _ = R.synth(A, order, n_ofdm, LEAD, LEAD, EPS, np.inf, 51 + which, channel=ch, dec=dec, over=DECIMATE)
    x = s + (g.standard_normal(s.shape[0]) + 1j * g.standard_normal(s.shape[0])) * np.sqrt(0.02)
    return {"s": s, "x": x, "dec": dec, "u": u, "p0": PRE, "order": order}


def extract_model(x, centre, m_first, M):
    """What ``extract`` computes in numpy float64: the capture turned back by ``centre`` cycles per sample, the Kaiser-windowed sinc of 129 taps cut at an eighth of
    the rate, every fourth sample from ``4 m_first`` on."""
    n = np.arange(x.shape[0])
    h = np.sinc((np.arange(129) - 64) / 4.0) * np.kaiser(129, 8.0)
    y = np.convolve(x * np.exp(-2j * np.pi * centre * n), h / h.sum())
    return y[64 + 4 * (m_first + np.arange(M))]


def _capture():
    """A noise capture at 4 MHz (0.04 over 4 MHz: 0.01 in a clip's 1 MHz, 20 dB below a burst) with the three bursts one after the other, each off the capture's centre in a
    hand-written box.  -> (capture complex64, tf (3, 4))."""
    parts = [burst(i)["s"] for i in range(3)]
    g = np.random.default_rng(7)
    n = sum(len(s) for s in parts) + 4 * GAP
    x = (g.standard_normal(n) + 1j * g.standard_normal(n)) * np.sqrt(0.02)
    tf, a = [], GAP
    for s, fcen in zip(parts, CENTRES):
        x[a:a + len(s)] += s * np.exp(2j * np.pi * fcen / FS_CAP * np.arange(a, a + len(s)))
        tf.append((a / FS_CAP, FC + fcen - 5.0e5, (a + len(s) - 1) / FS_CAP, FC + fcen + 5.0e5))
        a += len(s) + GAP
    return x.astype(np.complex64), np.array(tf)


@pytest.fixture(scope="module")
def chain():
    """``extract`` (decimation 4) -> ``demodulate_ofdm`` -> ``find_frames`` -> ``decode`` of the three boxes, once; shared and left unchanged."""
    from sy11 import _lib
    from sy11.data.spectrogram import open_iq
    from sy11.engine.model import YOLO
    from sy11.engine.predictor import DetectionPredictor, ScanResults
    x, tf = _capture()
    boxes = torch.zeros((3, 6), dtype=torch.float64)
    boxes[:, 4], boxes[:, 5] = torch.tensor([0.9, 0.8, 0.7], dtype=torch.float64), torch.tensor([0.0, 0.0, 0.0], dtype=torch.float64)
    res = ScanResults(boxes, torch.zeros(3, dtype=torch.int64), torch.from_numpy(tf), {0: "ofdm", 1: "b"}, np.zeros(1, dtype=np.int64), FS_CAP, FC)
    pred = DetectionPredictor.__new__(DetectionPredictor)                     # the chain reads the device alone
    pred.device = DEV
    y = YOLO.__new__(YOLO)
    y.device = DEV
    src = open_iq(torch.from_numpy(x))
    ext = pred.extract(src, res, FS_CAP, FC, decimate=DECIMATE)
    kw = dict(n_fft=64, cp=16, carriers=A["data"], pilots=dict(zip(A["pk"].tolist(), A["pc"].tolist())), order=list(ORDERS), spacing=DF)
    _lib.PROFILE = []
    try:
        d = y.demodulate_ofdm(ext, **kw)
        calls = [k[0] for k in _lib.PROFILE]
    finally:
        _lib.PROFILE = None
    assert calls == ["sy11_iq_ofdm_fold", "sy11_ofdm_fft", "sy11_ofdm_decide"]
    f = y.find_frames(d, [list(WORD)], payload=N_NEED, threshold=0.8, max_errors=3, t0=ext.t0)
    dec = y.decode(f, d, n_info=N_INFO, crc=CRC)
    return pred, y, src, res, ext, d, f, dec, kw


def test_extract_demodulate_ofdm_find_frames_decode_reads_the_bursts_as_sent(chain):
    from sy11.data.demodulate import Demodulation
    from sy11.data.demodulate_ofdm import OfdmDemodulation
    pred, y, src, res, ext, d, f, dec, kw = chain
    assert isinstance(d, OfdmDemodulation) and isinstance(d, Demodulation) and len(d) == 3 and d.valid.all() and ext.sample_rate.tolist() == [FS_CLIP] * 3
    assert d.order.tolist() == list(ORDERS) and d.phase_ambiguity.tolist() == [1, 1, 1] and d.rows.tolist() == [0, 1, 2]
    assert f.clip.tolist() == [0, 1, 2] and f.rotation.tolist() == [0, 0, 0]     # one frame each, upright: the pilots fix the phase
    for k in range(3):
        b = burst(k)
        st = d.raw["start"][k] + np.arange(int(d.n_ofdm[k])) * 80
        c = {"lay": A, "lead": LEAD // DECIMATE, "n_ofdm": b["dec"].shape[0], "dec": b["dec"]}
        j, miss = R.sent_symbols(st, c)
        first = int(np.flatnonzero(j == 0)[0])                                # the OFDM symbol of the demodulation that reads the first one sent
        bad, exact, _ = R.symbol_errors(d.decisions[k].cpu().numpy().reshape(-1, 48), d.raw["active"][k], st, c)
        print(f"burst {k}: theta {int(d.timing[k])} ({miss} off), cfo {d.cfo[k]:+.4f}, cp_corr {d.cp_corr[k]:.3f}, evm {d.evm[k]:.3f}, {bad} symbol errors, rho {f.rho[k]:.3f}, position "
              f"{f.position[k]}, word errors {f.errors[k]}, carrier {d.carrier_fit[k] - FC - CENTRES[k]:+.0f} Hz off its box, channel errors {dec.channel_errors[k]} of {dec.n_channel[k]}, "
              f"crc {bool(dec.crc_ok[k])}")
        assert miss <= 2 and exact and bad == 0
        assert int(f.position[k]) == first * 48 + b["p0"]                     # where the synthesiser put the word
        assert dec.valid[k] and dec.crc_ok[k] and dec.message(k) == np.packbits(b["u"]).tobytes()
        assert abs(d.carrier_fit[k] - FC - CENTRES[k] - EPS * DF) < 0.02 * DF
        lo = LEAD // DECIMATE + (b["p0"] // 48) * 80                          # the OFDM symbol that carries the word's first symbol, prefix included
        assert lo <= f.sample[k] < lo + 80


def test_public_entry_save_and_the_empty_extraction(chain, tmp_path):
    from sy11 import _lib
    pred, y, src, res, ext, d, f, dec, kw = chain
    d2 = pred.demodulate_ofdm(ext, **dict(kw, offset=0.0, advance=4, pilots=(A["pk"], A["pc"])))
    for i in range(3):
        assert torch.equal(_bits(d2.symbols[i]), _bits(d.symbols[i])) and torch.equal(d2.decisions[i], d.decisions[i]) and torch.equal(_bits(d2.filtered[i]), _bits(d.filtered[i]))
    with pytest.raises(ValueError, match="n_fft"):
        y.demodulate_ofdm(ext, **dict(kw, n_fft=100))
    bad = y.demodulate_ofdm(ext, **dict(kw, spacing=DF * 1.01))
    assert not bad.valid.any() and bad.reason.tolist() == ["rate"] * 3
    out = d.save(tmp_path / "d")
    z = np.load(tmp_path / "d" / "demodulate_ofdm.npz")
    index = json.loads((tmp_path / "d" / "demodulate_ofdm.json").read_text())
    assert out == str(tmp_path / "d") and np.array_equal(z["cfo"], d.cfo) and np.array_equal(z["evm"], d.evm) and np.array_equal(z["decisions_1"], d.decisions[1].cpu().numpy())
    assert np.array_equal(z["active_2"], d.raw["active"][2]) and np.array_equal(z["n_ofdm"], d.n_ofdm)
    assert [k["file"] for k in index["clips"]] == ["symbols_0.cf32", "symbols_1.cf32", "symbols_2.cf32"] and index["modulation"] == "ofdm"
    assert index["clips"][2]["cp_corr"] == float(d.cp_corr[2]) and index["clips"][0]["n_fft"] == 64 and index["clips"][1]["name"] == "ofdm"
    assert np.array_equal(np.fromfile(tmp_path / "d" / "symbols_1.cf32", dtype=np.complex64), d.symbols[1].cpu().numpy())
    none = pred.extract(src, res, FS_CAP, FC, rows=[], decimate=DECIMATE)      # an empty extraction: no launch
    _lib.PROFILE = []
    try:
        e = pred.demodulate_ofdm(none, **dict(kw, order=4))
        invalid = y.demodulate_ofdm(ext, **dict(kw, order=3))                  # nor does one without a valid clip
        calls = [k[0] for k in _lib.PROFILE]
    finally:
        _lib.PROFILE = None
    assert calls == [] and len(e) == 0 and e.symbols == [] and e.cfo.shape == (0,) and invalid.reason.tolist() == ["order"] * 3 and invalid.symbols[0].shape == (0,)
