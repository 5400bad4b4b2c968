"""GPU: the demodulation kernels (sy11_iq_demod_filter, sy11_demod_symbols, sy11_demod_decide) on the six clips of
tests/_demod_ref.py in ONE call.  Stage 2 (y) and stage 5 (s) against the float64 reference under the rule of tests/test_measure_gpu.py
(per clip, 4x the error of the float32 emulation of the same sums, relative to the clip's maximum; the emulation's error must be > 0);
every float64 table (timing rows, block sums, decision rows) against the reference fed with the kernel's own float32 values, to 1e-12; the
integers of the timing fit with no tolerance; r to 2^-21 |s| and the decisions wherever the reference's margin is at least 2^-20 |s| (no
symbol of these clips may fall below it); one call against one call per clip and a permuted extraction, bit for bit; the refusals; and
``extract`` -> ``characterize`` -> ``demodulate`` on four emissions embedded in a noise capture, with zero symbol errors."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from tests import _demod_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FC = 2.4e9
BLOCK = 32


def _extraction(clips, D, order=None, fs=R.FS, fc=FC):
    """A real ``Extraction`` around the given clips (numpy complex64), packed one after the other in ``order``."""
    from sy11.data.extract import Extraction, ExtractPlan
    order = list(range(len(clips))) if order is None else list(order)
    clips = [clips[i] for i in order]
    n = len(clips)
    D = np.asarray(D, dtype=np.int64)[order]
    M = np.array([len(c) for c in clips], dtype=np.int64)
    plan = ExtractPlan(int(M.sum()) * 64, fs, fc, np.array(order, dtype=np.int64), np.zeros((n, 4)), D, np.zeros(n, dtype=np.int64),
                       np.zeros(n, dtype=np.int64), M)
    packed = torch.from_numpy(np.concatenate(clips)).to(DEV)
    return Extraction(plan, packed, cls=np.arange(n) % 2, conf=np.linspace(0.5, 0.9, n), names={0: "a", 1: "b"})


def _demod(cs, order=None):
    from sy11.data.demodulate import demodulate_extraction
    order = list(range(len(cs))) if order is None else list(order)
    ext = _extraction([c["x"] for c in cs], [c["D"] for c in cs], order)
    return ext, demodulate_extraction(ext, symbol_rate=[cs[i]["rate"] for i in order], offset=[cs[i]["offset"] for i in order],
                                      order=[cs[i]["order"] for i in order], span=R.SPAN, block=BLOCK)


def _bits(t):
    t = torch.view_as_real(t) if t.is_complex() else t
    return t.contiguous().view({torch.float64: torch.int64, torch.float32: torch.int32, torch.uint8: torch.uint8}[t.dtype])


@pytest.fixture(scope="module")
def case():
    """The six clips, their extraction and ONE demodulation (three launches); shared and left unchanged."""
    from sy11 import _lib
    cs = R.case_clips()
    _lib.PROFILE = []
    try:
        ext, d = _demod(cs)
        calls = [k[0] for k in _lib.PROFILE]
    finally:
        _lib.PROFILE = None
    assert calls == ["sy11_iq_demod_filter", "sy11_demod_symbols", "sy11_demod_decide"]           # three launches, whatever the number of clips
    assert [int(o) % 2 for o in ext.plan.offset[:-1]] == [0, 1, 1, 1, 1, 1] and ext.sample_rate.tolist() == [R.FS / c["D"] for c in cs]
    assert d.valid.tolist() == [False, True, True, True, True, False] and d.reason.tolist() == ["order is not 2 or 4", "", "", "", "", "too short"]
    assert d.plan.n_taps.tolist() == [0, 107, 237, 83, 513, 0] and d.plan.tiles.tolist() == [0, 3, 16, 6, 17, 0]
    host = {"y": [v.cpu().numpy() for v in d.filtered], "r": [v.cpu().numpy() for v in d.symbols], "d": [v.cpu().numpy() for v in d.decisions],
            "s": d.raw["s"].cpu().numpy(), "t": d.raw["timing_rows"].cpu().numpy(), "z": d.raw["z_rows"].cpu().numpy(), "e": d.raw["decision_rows"].cpu().numpy()}
    return cs, ext, d, host


def _slices(d, i):
    return (slice(int(d.plan.row0[i]), int(d.plan.row0[i + 1])), slice(int(d.raw["block0"][i]), int(d.raw["block0"][i + 1])),
            slice(int(d.raw["sym0"][i]), int(d.raw["sym0"][i + 1])))


# ------------------------------------------------------------------------------------------------------------- stage 2, 3
def test_filtered_samples_and_timing_rows_match_the_float64_reference(case):
    cs, ext, d, host = case
    over = []
    for i, c in enumerate(cs):
        if not d.valid[i]:
            assert host["y"][i].shape == (0,)
            continue
        p = R.plan(len(c["x"]), c["fs"], c["rate"], c["offset"], c["order"], R.SPAN)
        h = R.taps(p["sps"], p["hw"])
        want, emu, got = R.filter64(c["x"], p["Wc"], h), R.filter32(c["x"], p["Wc"], h).astype(np.complex128), host["y"][i].astype(np.complex128)
        assert got.shape == want.shape == (len(c["x"]),)
        scale = np.abs(want).max()
        e_emu, e_gpu = np.abs(emu - want).max() / scale, np.abs(got - want).max() / scale
        print(f"iq_demod_filter[{c['label']}: M={len(c['x'])} taps={p['n_taps']}]: float32 emulation {e_emu:.3e}, kernel {e_gpu:.3e} (bar {4 * e_emu:.3e})")
        assert e_emu > 0
        if not e_gpu <= 4 * e_emu:
            over.append((c["label"], e_gpu, e_emu))
        rows, tr = _slices(d, i)[0], R.timing_rows(host["y"][i], p["hw"], p["Ws"])
        mine = host["t"][rows]
        assert mine.shape == tr.shape == (p["tiles"], 3)
        err = np.abs(mine - tr).max(1) / tr[:, 2]
        print(f"iq_demod_filter[{c['label']}] timing rows: largest error {err.max():.2e} of a tile's sum |y|^2")
        assert err.max() <= 1e-12, (c["label"], err)
    assert not over, over
    assert ext.packed.shape == (sum(len(c["x"]) for c in cs),)


# ------------------------------------------------------------------------------------------------------------- stage 4
def test_timing_fit_equals_the_reference_on_the_kernels_own_rows(case):
    cs, ext, d, host = case
    for i, c in enumerate(cs):
        if not d.valid[i]:
            assert (d.n_symbols[i], d.raw["i_last"][i]) == (-1, -1) and np.isnan(d.timing[i]) and np.isnan(d.symbol_rate_fit[i])
            continue
        p = R.plan(len(c["x"]), c["fs"], c["rate"], c["offset"], c["order"], R.SPAN)
        f = R.fit(host["t"][_slices(d, i)[0]], len(c["x"]), p["hw"], p["Ws"])
        raw = d.raw
        assert (raw["T0"][i], raw["STEP"][i], raw["i_first"][i], raw["i_last"][i], int(d.n_symbols[i])) == (f["T0"], f["STEP"], f["i_first"], f["i_last"], f["n_symbols"])
        assert np.abs(raw["psi"][i] - f["psi"]).max() <= 1e-12
        assert abs(d.timing[i] - f["timing"]) <= 1e-12 and abs(d.symbol_rate_fit[i] - c["fs"] / f["sps"]) <= 1e-12 * c["fs"]
        assert abs(d.symbol_rate_fit[i] - c["true_rate"]) < 0.25 * c["fs"] / 1024
    assert int(d.n_symbols[3]) % BLOCK != 0 and int(d.plan.M[3] - 2 * d.plan.hw[3]) % 512 != 0               # the ragged last block and tile


# ------------------------------------------------------------------------------------------------------------- stage 5
def test_symbols_and_block_sums_match_the_reference_on_the_kernels_own_samples(case):
    cs, ext, d, host = case
    over = []
    for i, c in enumerate(cs):
        if not d.valid[i]:
            continue
        _, blocks, syms = _slices(d, i)
        T0, STEP, i0, n = d.raw["T0"][i], d.raw["STEP"][i], d.raw["i_first"][i], int(d.n_symbols[i])
        want, emu = R.symbols64(host["y"][i], T0, STEP, i0, n), R.symbols32(host["y"][i], T0, STEP, i0, n).astype(np.complex128)
        got = host["s"][syms].astype(np.complex128)
        assert got.shape == want.shape == (n,)
        scale = np.abs(want).max()
        e_emu, e_gpu = np.abs(emu - want).max() / scale, np.abs(got - want).max() / scale
        print(f"demod_symbols[{c['label']}: {n} symbols]: float32 emulation {e_emu:.3e}, kernel {e_gpu:.3e} (bar {4 * e_emu:.3e})")
        assert e_emu > 0
        if not e_gpu <= 4 * e_emu:
            over.append((c["label"], e_gpu, e_emu))
        z, mine = R.z_rows(host["s"][syms], c["order"], BLOCK), host["z"][blocks]
        assert mine.shape == z.shape == (-(-n // BLOCK), 3)
        mag = np.array([np.sum(np.abs(host["s"][syms][a:b].astype(np.complex128)) ** c["order"]) for a, b in R.blocks(n, BLOCK)])
        err = max(np.abs(mine[:, :2] - z[:, :2]).max(1) / mag), np.abs(mine[:, 2] - z[:, 2]).max() / z[:, 2].min()
        print(f"demod_symbols[{c['label']}] block sums: largest errors {err[0].max():.2e} of sum |s|^order, {err[1]:.2e} of sum |s|^2")
        assert err[0].max() <= 1e-12 and err[1] <= 1e-12
    assert not over, over


# ------------------------------------------------------------------------------------------------------------- stage 6, 7, 8
def test_decisions_rows_and_columns_match_the_reference_on_the_kernels_own_symbols(case):
    cs, ext, d, host = case
    for i, c in enumerate(cs):
        if not d.valid[i]:
            assert np.isnan([d.gain[i], d.evm[i], d.mer_db[i], d.carrier_fit[i]]).all() and d.phase_ambiguity[i] == -1 and d.bits(i).shape == (0,)
            continue
        order = c["order"]
        _, blocks, syms = _slices(d, i)
        s, n = host["s"][syms], int(d.n_symbols[i])
        theta = R.phase_track(host["z"][blocks], order)
        assert np.abs(d.raw["theta"][i] - theta).max() <= 1e-12 and np.abs(np.diff(theta)).max() < np.pi / order
        r, dec, margin = R.decide(s, d.raw["theta"][i], order, BLOCK)
        mag = np.abs(s.astype(np.complex128))
        err = np.abs(host["r"][i].astype(np.complex128) - r) / mag
        exempt = margin < 2.0 ** -20 * mag
        print(f"demod_decide[{c['label']}]: largest |r - ref| / |s| {err.max():.3e} (bar {2.0 ** -21:.3e}); {int(exempt.sum())} of {n} decisions exempt, "
              f"smallest margin {float((margin / mag).min()):.3f} |s|")
        assert err.max() <= 2.0 ** -21
        assert int(exempt.sum()) == 0 and np.array_equal(host["d"][i][~exempt], dec[~exempt])
        assert np.array_equal(R.decide32(s, d.raw["theta"][i], order, BLOCK)[1], host["d"][i])
        rows, mine = R.block_rows(host["r"][i], host["d"][i], order, BLOCK), host["e"][blocks]
        assert mine.shape == rows.shape and np.array_equal(mine[:, 2], rows[:, 2])
        assert (np.abs(mine[:, :2] - rows[:, :2]) <= 1e-12 * rows[:, :1]).all()
        rate_fit = float(d.symbol_rate_fit[i])
        col = R.columns(mine, d.raw["theta"][i], n, BLOCK, rate_fit, FC + c["offset"])
        assert int(d.n_symbols[i]) == col["n_symbols"] == n
        for key in ("gain", "evm", "mer_db", "carrier_fit"):
            assert abs(float(getattr(d, key)[i]) - col[key]) <= 1e-12 * abs(col[key]), (c["label"], key)
        assert abs(d.carrier_fit[i] - FC - c["true_offset"]) < c["fs"] / 1024 / 16 and d.phase_ambiguity[i] == order
        # what was sent: no symbol error, up to the rotation and a shift of one symbol (the reference alone: tests/test_demodulate_cpu.py)
        k0 = (d.raw["T0"][i] + d.raw["i_first"][i] * d.raw["STEP"][i]) / 2.0 ** 32
        bad, rot, shift = R.errors(host["r"][i], order, k0, c["sps"], c["a"], c["u0"])
        print(f"demodulate[{c['label']}]: {bad} symbol errors (rotation {rot}, shift {shift}), evm {d.evm[i]:.4f}, mer {d.mer_db[i]:.1f} dB")
        assert bad == 0
        bits = d.bits(i)
        want_bits = host["d"][i] & 1 if order == 2 else np.stack(((host["d"][i] >> 1) & 1, host["d"][i] & 1), 1).reshape(-1)
        assert bits.dtype == np.uint8 and np.array_equal(bits, want_bits) and bits.shape == (n * order // 2,)
    assert d[1]["valid"] and d[1]["reason"] == "" and d[0]["reason"] == "order is not 2 or 4"
    assert d.cls.tolist() == ext.cls.tolist() and d.names == ext.names and d.rows.tolist() == ext.rows.tolist()


# ------------------------------------------------------------------------------------------------------------- invariance
def test_one_call_per_clip_and_a_permuted_extraction_give_the_same_bits(case):
    cs, ext, d, host = case
    perm = [4, 2, 0, 5, 3, 1]
    _, p = _demod(cs, perm)
    assert p.rows.tolist() == perm
    for at, i in enumerate(perm):
        _, one = _demod([cs[i]])
        for other, k in ((p, at), (one, 0)):
            assert bool(other.valid[k]) == bool(d.valid[i]) and other.reason[k] == d.reason[i] and int(other.n_symbols[k]) == int(d.n_symbols[i])
            for a, b in zip(_slices(other, k), _slices(d, i)):
                assert a.stop - a.start == b.stop - b.start
            for key in ("filtered", "symbols", "decisions"):
                assert torch.equal(_bits(getattr(other, key)[k]), _bits(getattr(d, key)[i])), (i, at, key)
            if not d.valid[i]:
                continue
            for key, sl in zip(("timing_rows", "z_rows", "s"), (0, 1, 2)):
                assert torch.equal(_bits(other.raw[key][_slices(other, k)[sl]]), _bits(d.raw[key][_slices(d, i)[sl]])), (i, at, key)
            assert torch.equal(_bits(other.raw["decision_rows"][_slices(other, k)[1]]), _bits(d.raw["decision_rows"][_slices(d, i)[1]]))
            for key in ("psi", "theta"):
                assert np.array_equal(other.raw[key][k], d.raw[key][i])
            assert (other.raw["T0"][k], other.raw["STEP"][k], other.raw["i_first"][k]) == (d.raw["T0"][i], d.raw["STEP"][i], d.raw["i_first"][i])
            for key in d.COLUMNS:
                assert getattr(other, key)[k] == getattr(d, key)[i]


# ------------------------------------------------------------------------------------------------------------- refusals
def _lib_refuses(name, args, pos, v, match=None):
    from sy11 import _lib
    bad = list(args)
    bad[pos] = v
    with pytest.raises(_lib.Sy11Error, match=match):
        _lib.call(name, *bad)


def test_refusals_raise_and_write_nothing(case):
    from sy11 import _lib, ops
    from sy11.data.demodulate import BLOCK as BLK, DEC
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
    y = torch.full((n_in,), -7.0, dtype=torch.complex64, device=DEV)
    rows = torch.full((n_rows, 3), -7.0, dtype=torch.float64, device=DEV)
    last = items.shape[0] - 1                                                 # the last tile of the 513-tap clip; its taps end the tap buffer
    it = items[last]
    assert int(it["last"]) == 1 and int(it["first"]) == 0 and int(it["n_taps"]) == 513 and int(it["tap_off"]) + 513 == n_tap and 0 < int(it["cnt"]) < 512
    hw, ln, end = int(it["hw"]), int(it["len"]), int(it["off"]) + int(it["len"])           # the clip ends at `end`; a clip without items follows it
    entry1 = ((dict(off=-1), "packed samples"), (dict(len=0), "packed samples"), (dict(off=n_in - ln + 1), "packed samples"), (dict(len=n_in + 1, off=0), "packed samples"),
              (dict(hw=0, n_taps=1), "half width"), (dict(n_taps=511), "half width"), (dict(n_taps=512), "half width"), (dict(hw=257, n_taps=515), "half width"),
              (dict(tap_off=-1), "packed taps"), (dict(tap_off=int(it["tap_off"]) + 1), "packed taps"),
              (dict(n0=int(it["n0"]) + 1, cnt=int(it["cnt"]) - 1), "not a tile"), (dict(n0=hw - 512), "not a tile"), (dict(cnt=0), "not a tile"),
              (dict(cnt=int(it["cnt"]) + 1), "not a tile"), (dict(n0=hw, cnt=513), "not a tile"),
              (dict(first=1), "first ="), (dict(first=2), "first ="), (dict(last=0), "last ="), (dict(last=2), "last ="),
              (dict(cnt=int(it["cnt"]) - 1), "last ="), (dict(row=-1), "writes row"), (dict(row=n_rows), "writes row"))
    for kw, what in entry1:
        with pytest.raises(E_, match=what):
            ops.iq_demod_filter(x, one(items, last, **kw), taps, y, rows)
    with pytest.raises(E_, match="first ="):
        ops.iq_demod_filter(x, one(items, 0, first=0), taps, y, rows)
    with pytest.raises(E_, match="last ="):
        ops.iq_demod_filter(x, one(items, 0, last=1), taps, y, rows)             # a full first tile may not own the clip's end
    with pytest.raises(E_, match="a row takes one item"):
        ops.iq_demod_filter(x, np.concatenate((one(items, 0), one(items, 1, row=int(items["row"][0])))), taps, y, rows)
    with pytest.raises(E_, match="packed samples"):
        ops.iq_demod_filter(x[:end - 1], one(items, last), taps, y[:end - 1], rows)   # the clip ends one sample past the buffer
    with pytest.raises(E_, match="packed taps"):
        ops.iq_demod_filter(x, one(items, last), taps[:-1], y, rows)
    for bad in (dict(x=x.to(torch.complex128)), dict(x=x[::2]), dict(x=x.cpu()), dict(y=y[:-1]), dict(y=x), dict(y=y.to(torch.complex128)),
                dict(taps=taps.double()), dict(taps=taps[:0]), dict(taps=taps.cpu()), dict(rows=rows.float()), dict(rows=rows[:, :2]), dict(rows=rows[:0]),
                dict(items=items[:0]), dict(items=np.zeros((2, 9), dtype=np.int64))):
        a = dict(x=x, y=y, taps=taps, rows=rows, items=items)
        a.update(bad)
        with pytest.raises(E_):
            ops.iq_demod_filter(a["x"], a["items"], a["taps"], a["y"], a["rows"])

    def lib1(host_items):
        return table(host_items) + [n_tap, p(taps), n_in, p(x), p(y), n_rows, p(rows), None]
    for pos, v in ((0, 0), (1, None), (2, None), (4, None), (6, None), (7, None), (9, None), (3, 0), (3, n_tap - 1), (5, 0), (5, end - 1), (8, 0), (8, n_rows - 1),
                   (6, C.c_void_p(x.data_ptr() + 4)), (7, C.c_void_p(y.data_ptr() + 4)), (7, p(x)), (9, C.c_void_p(rows.data_ptr() + 4))):
        _lib_refuses("sy11_iq_demod_filter", lib1(items), pos, v)
    for kw, _ in entry1:
        with pytest.raises(E_, match="iq_demod_filter: item 0"):
            _lib.call("sy11_iq_demod_filter", *lib1(one(items, last, **kw)))
    with pytest.raises(E_, match="an earlier item"):
        _lib.call("sy11_iq_demod_filter", *lib1(np.concatenate((one(items, 0), one(items, 1, row=int(items["row"][0]))))))
    torch.cuda.synchronize()
    assert bool((torch.view_as_real(y) == torch.tensor([-7.0, 0.0], device=DEV)).all()) and bool((rows == -7.0).all())    # no refused call wrote anything
    # ---- launch 2: rebuild the item table of the shared call from its raw fit
    n_sym, n_blk = int(d.raw["sym0"][-1]), int(d.raw["block0"][-1])
    yk = torch.zeros(n_in, dtype=torch.complex64, device=DEV)
    blocks = np.zeros(n_blk, dtype=BLK)
    decs = np.zeros(n_blk, dtype=DEC)
    for i in np.flatnonzero(d.valid):
        _, bs, ss = _slices(d, i)
        q = np.arange(bs.stop - bs.start)
        n = int(d.n_symbols[i])
        blocks["off"][bs], blocks["len"][bs], blocks["step"][bs], blocks["order"][bs] = d.plan.offset[i], d.plan.M[i], d.raw["STEP"][i], d.plan.order[i]
        blocks["t0"][bs] = [d.raw["T0"][i] + (d.raw["i_first"][i] + int(k) * BLOCK) * d.raw["STEP"][i] for k in q]
        blocks["sym_off"][bs], blocks["n"][bs], blocks["row"][bs] = ss.start + q * BLOCK, np.minimum(n - q * BLOCK, BLOCK), bs.start + q
        decs["sym_off"][bs], decs["n_sym"][bs], decs["row0"][bs], decs["nb"][bs], decs["b"][bs] = ss.start, n, bs.start, len(q), q
        decs["block"][bs], decs["order"][bs] = BLOCK, d.plan.order[i]
        yk[int(d.plan.offset[i]):int(d.plan.offset[i]) + int(d.plan.M[i])] = d.filtered[i]
    sym = torch.full((n_sym,), -7.0, dtype=torch.complex64, device=DEV)
    zr = torch.full((n_blk, 3), -7.0, dtype=torch.float64, device=DEV)
    good_s, good_z = ops.demod_symbols(yk, blocks, torch.zeros_like(sym), torch.zeros_like(zr))       # the table is the shared call's: the same bits
    assert torch.equal(_bits(good_s), _bits(d.raw["s"])) and torch.equal(_bits(good_z), _bits(d.raw["z_rows"]))
    lb = n_blk - 1                                                            # the last block of the last valid clip: it ends the symbol buffer
    b = blocks[lb]
    assert int(b["sym_off"]) + int(b["n"]) == n_sym and int(b["len"]) == 9000
    k_last = (int(b["t0"]) + (int(b["n"]) - 1) * int(b["step"])) >> 32
    entry2 = ((dict(off=-1), "packed samples"), (dict(len=3), "packed samples"), (dict(off=n_in - 9000 + 1), "packed samples"),
              (dict(n=0), "packed symbols"), (dict(n=257), "packed symbols"), (dict(sym_off=-1), "packed symbols"), (dict(sym_off=int(b["sym_off"]) + 1), "packed symbols"),
              (dict(step=2 ** 32 - 1), "Q32.32"), (dict(step=2 ** 40 + 1), "Q32.32"), (dict(t0=2 ** 32 - 1), "Q32.32"), (dict(t0=9000 * 2 ** 32), "Q32.32"),
              (dict(len=k_last + 2), "Q32.32"), (dict(order=0), "order"), (dict(order=3), "order"), (dict(row=-1), "writes row"), (dict(row=n_blk), "writes row"))
    for kw, what in entry2:
        with pytest.raises(E_, match=what):
            ops.demod_symbols(yk, one(blocks, lb, **kw), sym, zr)
    ops_ok = one(blocks, lb, len=k_last + 3)                                    # the last position may be len - 3 itself
    assert ((int(ops_ok["t0"][0]) + (int(ops_ok["n"][0]) - 1) * int(ops_ok["step"][0])) >> 32) == int(ops_ok["len"][0]) - 3
    with pytest.raises(E_, match="a row takes one item"):
        ops.demod_symbols(yk, np.concatenate((one(blocks, 0), one(blocks, 1, row=int(blocks["row"][0])))), sym, zr)
    for bad in (dict(y=yk.to(torch.complex128)), dict(y=yk.cpu()), dict(y=yk[::2]), dict(sym=sym.to(torch.complex128)), dict(sym=sym[:0]), dict(rows=zr.float()),
                dict(rows=zr[:, :2]), dict(items=blocks[:0]), dict(items=np.zeros((2, 7), dtype=np.int64))):
        a = dict(y=yk, sym=sym, rows=zr, items=blocks)
        a.update(bad)
        with pytest.raises(E_):
            ops.demod_symbols(a["y"], a["items"], a["sym"], a["rows"])

    def lib2(host_items):
        return table(host_items) + [n_in, p(yk), n_sym, p(sym), n_blk, p(zr), None]
    for pos, v in ((0, 0), (1, None), (2, None), (4, None), (6, None), (8, None), (3, 0), (3, end - 1), (5, 0), (5, n_sym - 1), (7, 0), (7, n_blk - 1),
                   (4, C.c_void_p(yk.data_ptr() + 4)), (6, C.c_void_p(sym.data_ptr() + 4)), (8, C.c_void_p(zr.data_ptr() + 4))):
        _lib_refuses("sy11_demod_symbols", lib2(blocks), pos, v)
    for kw, _ in entry2:
        with pytest.raises(E_, match="demod_symbols: item 0"):
            _lib.call("sy11_demod_symbols", *lib2(one(blocks, lb, **kw)))
    with pytest.raises(E_, match="an earlier item"):
        _lib.call("sy11_demod_symbols", *lib2(np.concatenate((one(blocks, 0), one(blocks, 1, row=int(blocks["row"][0]))))))
    torch.cuda.synchronize()
    assert bool((torch.view_as_real(sym) == torch.tensor([-7.0, 0.0], device=DEV)).all()) and bool((zr == -7.0).all())
    # ---- launch 3
    theta = torch.from_numpy(np.concatenate([d.raw["theta"][i] for i in range(len(d))])).to(DEV)
    r = torch.full((n_sym,), -7.0, dtype=torch.complex64, device=DEV)
    dd = torch.full((n_sym,), 7, dtype=torch.uint8, device=DEV)
    er = torch.full((n_blk, 3), -7.0, dtype=torch.float64, device=DEV)
    g_r, g_d, g_e = ops.demod_decide(good_s, decs, theta, torch.zeros_like(r), torch.zeros_like(dd), torch.zeros_like(er))
    assert torch.equal(_bits(g_r), _bits(torch.cat(d.symbols))) and torch.equal(g_d, torch.cat(d.decisions)) and torch.equal(_bits(g_e), _bits(d.raw["decision_rows"]))
    e = decs[lb]
    ns, nb = int(e["n_sym"]), int(e["nb"])
    assert int(e["sym_off"]) + ns == n_sym and int(e["row0"]) + nb == n_blk and int(e["b"]) == nb - 1 and ns % BLOCK != 0
    entry3 = ((dict(n_sym=0), "packed symbols"), (dict(sym_off=-1), "packed symbols"), (dict(sym_off=int(e["sym_off"]) + 1), "packed symbols"),
              (dict(block=7), "does not fit"), (dict(block=257), "does not fit"), (dict(nb=0), "does not fit"), (dict(nb=nb + 1), "does not fit"),
              (dict(nb=nb - 1, b=nb - 2), "does not fit"), (dict(b=-1), "does not fit"), (dict(b=nb), "does not fit"),
              (dict(row0=-1), "rows \\["), (dict(row0=int(e["row0"]) + 1), "rows \\["), (dict(order=0), "order"), (dict(order=8), "order"))
    for kw, what in entry3:
        with pytest.raises(E_, match=what):
            ops.demod_decide(good_s, one(decs, lb, **kw), theta, r, dd, er)
    with pytest.raises(E_, match="a row takes one item"):
        ops.demod_decide(good_s, np.concatenate((one(decs, 0), one(decs, 0))), theta, r, dd, er)
    for bad in (dict(sym=good_s.to(torch.complex128)), dict(sym=good_s.cpu()), dict(r=r[:-1]), dict(r=good_s), dict(d=dd[:-1]), dict(d=dd.to(torch.int32)),
                dict(theta=theta[:-1]), dict(theta=theta.float()), dict(rows=er.float()), dict(rows=er[:, :2]), dict(items=decs[:0]),
                dict(items=np.zeros((2, 5), dtype=np.int64))):
        a = dict(sym=good_s, r=r, d=dd, theta=theta, rows=er, items=decs)
        a.update(bad)
        with pytest.raises(E_):
            ops.demod_decide(a["sym"], a["items"], a["theta"], a["r"], a["d"], a["rows"])

    def lib3(host_items):
        return table(host_items) + [n_sym, p(good_s), n_blk, p(theta), p(r), p(dd), p(er), None]
    for pos, v in ((0, 0), (1, None), (2, None), (4, None), (6, None), (7, None), (8, None), (9, None), (3, 0), (3, n_sym - 1), (5, 0), (5, n_blk - 1),
                   (4, C.c_void_p(good_s.data_ptr() + 4)), (7, C.c_void_p(r.data_ptr() + 4)), (7, p(good_s)), (6, C.c_void_p(theta.data_ptr() + 4)),
                   (9, C.c_void_p(er.data_ptr() + 4))):
        _lib_refuses("sy11_demod_decide", lib3(decs), pos, v)
    for kw, _ in entry3:
        with pytest.raises(E_, match="demod_decide: item 0"):
            _lib.call("sy11_demod_decide", *lib3(one(decs, lb, **kw)))
    with pytest.raises(E_, match="an earlier item"):
        _lib.call("sy11_demod_decide", *lib3(np.concatenate((one(decs, 0), one(decs, 0)))))
    torch.cuda.synchronize()
    assert bool((torch.view_as_real(r) == torch.tensor([-7.0, 0.0], device=DEV)).all()) and bool((dd == 7).all()) and bool((er == -7.0).all())


# ------------------------------------------------------------------------------------------------------------- end to end
def _embedded():
    """A noise capture at 4 MHz with a BPSK, a QPSK and a CW emission (13.2 samples per symbol: 3.3 after decimation by 4) one after the
    other, each 37.3 bins of a 1024-point transform at 1 MHz off the centre of its hand-written box; the fourth box holds noise alone.
    -> (capture complex64, tf (4, 4), kinds, sent): ``sent[i]`` = (a, u0, first capture sample) of a keyed emission, else None."""
    fs, n_each, gap = 4.0e6, 4 * 8400, 2000
    kinds, centres = ("bpsk", "qpsk", "cw", "noise"), (-1.1e6, 0.6e6, 1.2e6, -0.3e6)
    g = np.random.default_rng(5)
    n = 4 * (n_each + gap) + gap
    x = (g.standard_normal(n) + 1j * g.standard_normal(n)) * np.sqrt(0.02)     # 0.04 over 4 MHz: 0.01 in a clip's 1 MHz, 20 dB below the signal
    tf, sent = [], []
    for i, (kind, fcen) in enumerate(zip(kinds, centres)):
        a = gap + i * (n_each + gap)
        sent.append(None)
        if kind != "noise":
            s, sym, u0 = R.clip(kind, n_each, 20 + i, 13.2, 37.3 / 1024 / 4, 300.0)                       # no noise of its own
            x[a:a + n_each] += s.astype(np.complex128) * np.exp(2j * np.pi * fcen / fs * np.arange(a, a + n_each))
            sent[-1] = None if sym is None else (sym, u0, a)
        tf.append((a / fs, FC + fcen - 2.5e5, (a + n_each - 1) / fs, FC + fcen + 2.5e5))
    return x.astype(np.complex64), np.array(tf), kinds, sent


@pytest.fixture(scope="module")
def embedded():
    """``extract`` (decimation 4) -> ``characterize`` -> ``demodulate`` of the four boxes, once; shared and left unchanged."""
    from sy11 import _lib
    from sy11.data.spectrogram import open_iq
    from sy11.engine.predictor import DetectionPredictor, ScanResults
    fs = 4.0e6
    x, tf, kinds, sent = _embedded()
    boxes = torch.zeros((4, 6), dtype=torch.float64)
    boxes[:, 4], boxes[:, 5] = torch.tensor([0.9, 0.8, 0.7, 0.6], dtype=torch.float64), torch.tensor([1.0, 0.0, 1.0, 0.0], dtype=torch.float64)
    res = ScanResults(boxes, torch.zeros(4, dtype=torch.int64), torch.from_numpy(tf), {0: "a", 1: "b"}, np.zeros(1, dtype=np.int64), fs, FC)
    pred = DetectionPredictor.__new__(DetectionPredictor)                     # extract, characterize and demodulate read the device alone
    pred.device = DEV
    src = open_iq(torch.from_numpy(x))
    ext = pred.extract(src, res, fs, FC, decimate=4)
    c = pred.characterize(ext)
    _lib.PROFILE = []
    try:
        d = pred.demodulate(ext, c)
        calls = [k[0] for k in _lib.PROFILE]
    finally:
        _lib.PROFILE = None
    assert calls == ["sy11_iq_demod_filter", "sy11_demod_symbols", "sy11_demod_decide"]
    host = ext.packed.cpu().numpy()
    refs = []
    for i in (0, 1):                                                          # the reference on the extraction's own samples
        order = int(c.order[i])
        refs.append(R.demodulate(host[int(ext.plan.offset[i]):int(ext.plan.offset[i + 1])], 1.0e6, float(c.symbol_rate[i]),
                                 float(c.offset2[i] if order == 2 else c.offset4[i]), order, fc=float(ext.center_freq[i])))
    return pred, src, res, ext, c, d, kinds, sent, refs


def test_extract_characterize_demodulate_reads_the_embedded_emissions_without_a_symbol_error(embedded):
    from sy11.data.demodulate import Demodulation
    pred, src, res, ext, c, d, kinds, sent, refs = embedded
    fs = 4.0e6
    assert c.order.tolist() == [2, 4, 2, 0] and c.keyed.tolist() == [True, True, False, False]
    assert isinstance(d, Demodulation) and len(d) == 4
    assert d.valid.tolist() == [True, True, False, False] and d.reason.tolist() == ["", "", "not keyed", "order is not 2 or 4"]
    assert d.cls.tolist() == [1, 0, 1, 0] and d.conf.tolist() == [0.9, 0.8, 0.7, 0.6] and d.names == res.names and d.rows.tolist() == [0, 1, 2, 3]
    for i in (0, 1):
        order, ref = int(c.order[i]), refs[i]
        a, u0, first = sent[i]
        # the clip's sample k sits at the capture's sample t0 fs + 4 k, which is sample t0 fs + 4 k - first of the emission
        k0 = float(ext.t0[i]) * fs + 4.0 * (d.raw["T0"][i] + d.raw["i_first"][i] * d.raw["STEP"][i]) / 2.0 ** 32 - first
        bad, rot, shift = R.errors(d.symbols[i].cpu().numpy(), order, k0, 13.2, a, u0)
        print(f"demodulate[{kinds[i]}]: {int(d.n_symbols[i])} symbols, {bad} errors (rotation {rot}, shift {shift}), evm {d.evm[i]:.5f}, mer {d.mer_db[i]:.1f} dB, "
              f"rate {(d.symbol_rate_fit[i] - 1.0e6 / 3.3) / (1.0e6 / 1024):+.4f} bins")
        assert bad == 0
        assert abs(d.symbol_rate_fit[i] - 1.0e6 / 3.3) < 0.25 * 1.0e6 / 1024
        assert int(d.n_symbols[i]) == ref["n_symbols"] and np.array_equal(d.decisions[i].cpu().numpy(), ref["d"])
        assert d.phase_ambiguity[i] == order and d.bits(i).shape == (int(d.n_symbols[i]) * order // 2,)
    for i in (2, 3):
        assert int(d.n_symbols[i]) == -1 and np.isnan(d.evm[i]) and d.symbols[i].shape == (0,) and d.reason[i] != ""


def test_evm_of_the_embedded_emissions_agrees_with_the_reference_on_the_extractions_own_samples(embedded):
    """1e-9 relative to the reference's evm, as the columns of ``test_extract_then_characterize_names_four_embedded_emissions`` are.  The
    device computes y, s and r in float64 and rounds each once, as the reference does; with float32 sums in their place evm sat 3.8e-9
    (BPSK) and 5.1e-9 (QPSK) of itself away from the reference."""
    pred, src, res, ext, c, d, kinds, sent, refs = embedded
    err = []
    for i in (0, 1):
        err.append(abs(d.evm[i] - refs[i]["evm"]) / refs[i]["evm"])
        print(f"demodulate[{kinds[i]}]: evm {d.evm[i]:.12f}, reference {refs[i]['evm']:.12f}: relative difference {err[-1]:.3e} (bar 1e-9); "
              f"gain {d.gain[i]:.9f} against {refs[i]['gain']:.9f}")
    assert max(err) <= 1e-9, err


def test_public_entry_explicit_parameters_save_and_the_empty_extraction(embedded, tmp_path):
    from sy11 import _lib
    from sy11.engine.model import YOLO
    pred, src, res, ext, c, d, kinds, sent, refs = embedded
    y = YOLO.__new__(YOLO)
    y.device = DEV
    d2 = y.demodulate(ext, c)
    for i in range(4):
        assert torch.equal(_bits(d2.symbols[i]), _bits(d.symbols[i])) and torch.equal(d2.decisions[i], d.decisions[i]) and torch.equal(_bits(d2.filtered[i]), _bits(d.filtered[i]))
    off = np.where(c.order == 2, c.offset2, c.offset4)
    d3 = y.demodulate(ext, symbol_rate=c.symbol_rate, offset=off, order=np.where(c.keyed, c.order, 0))
    assert d3.valid.tolist() == d.valid.tolist() and all(torch.equal(d3.decisions[i], d.decisions[i]) for i in range(4))
    out = d.save(tmp_path / "d")
    z = np.load(tmp_path / "d" / "demodulate.npz")
    index = json.loads((tmp_path / "d" / "demodulate.json").read_text())
    assert out == str(tmp_path / "d") and np.array_equal(z["evm"], d.evm, equal_nan=True) and np.array_equal(z["decisions_1"], d.decisions[1].cpu().numpy())
    assert [k["file"] for k in index["clips"]] == ["symbols_0.cf32", "symbols_1.cf32", None, None] and index["clips"][2]["reason"] == "not keyed"
    sym = np.fromfile(tmp_path / "d" / "symbols_1.cf32", dtype=np.complex64)
    assert np.array_equal(sym, d.symbols[1].cpu().numpy())
    # an empty extraction: no launch
    none = pred.extract(src, res, 4.0e6, FC, rows=[], decimate=4)
    _lib.PROFILE = []
    try:
        e = pred.demodulate(none, pred.characterize(none))
        calls = [k[0] for k in _lib.PROFILE]
    finally:
        _lib.PROFILE = None
    assert calls == [] and len(e) == 0 and e.symbols == [] and e.evm.shape == (0,)
