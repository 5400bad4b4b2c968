"""GPU: the characterisation kernels (sy11_iq_cyclo, sy11_cyclo_peaks).  Stage 1 against the float64 reference of
tests/_characterize_ref.py under the rule of tests/test_measure_gpu.py (per partial row, 4x the error of the float32 emulation of the same
sums, relative to the row's maximum; the emulation's error must be > 0), the moments to 1e-12; stage 2 against the same reference's
``reduce`` fed with the kernel's own partial table, bins and counts with no tolerance; one call against one call per clip and a permuted
extraction, bit for bit; the refusals; and ``extract`` -> ``characterize`` on four emissions embedded in a noise capture."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _characterize_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FS, FC = 1.0e6, 2.4e9
KINDS = ("noise", "bpsk", None, "qpsk", "cw")                  # None: the clip shorter than a frame


def _lengths(N):
    """J = 1, 16, (invalid), 17, 33: both sides of a group boundary; clips 1, 3 and 4 start at odd packed offsets."""
    H = N // 2
    return [N + 1, N + 15 * H + 3, N - 1, N + 16 * H, N + 32 * H + 7]


def _extraction(clips, fs=FS, fc=FC, D=None, order=None):
    """A real ``Extraction`` around the given clips (numpy complex64), packed one after the other in ``order``."""
    from sy11.data.extract import Extraction, ExtractPlan
    order = list(range(len(clips))) if order is None else list(order)
    clips = [clips[i] for i in order]
    n = len(clips)
    D = np.ones(n, dtype=np.int64) if D is None else np.asarray(D, dtype=np.int64)[order]
    M = np.array([len(c) for c in clips], dtype=np.int64)
    plan = ExtractPlan(int(M.sum()) * 64, fs, fc, np.array(order, dtype=np.int64), np.zeros((n, 4)), D, np.zeros(n, dtype=np.int64),
                       np.zeros(n, dtype=np.int64), M)
    packed = torch.from_numpy(np.concatenate(clips) if n else np.zeros(0, dtype=np.complex64)).to(DEV)
    return Extraction(plan, packed, cls=np.arange(n) % 2, conf=np.linspace(0.5, 0.9, n), names={0: "a", 1: "b"})


def _bits(t):
    t = torch.view_as_real(t) if t.is_complex() else t
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


@pytest.fixture(scope="module", params=[64, 128, 1024])
def case(request):
    """Five clips, their extraction and ONE characterisation (two launches); shared and left unchanged."""
    from sy11 import _lib
    from sy11.data.characterize import characterize_extraction
    N = request.param
    Ms = _lengths(N)
    clips = [R.clip(kind or "noise", m, 10 + i, 3.3, 5.3 / 64, 20.0) for i, (kind, m) in enumerate(zip(KINDS, Ms))]
    D = [1, 2, 1, 4, 1]                                                       # the clips run at FS, FS / 2, FS, FS / 4, FS
    ext = _extraction(clips, D=D)
    assert [int(o) % 2 for o in ext.plan.offset[:-1]] == [0, 1, 0, 1, 1] and ext.sample_rate.tolist() == [FS / d for d in D]
    _lib.PROFILE = []
    try:
        c = characterize_extraction(ext, N, 2.0e4, 13.0)
        calls = [k[0] for k in _lib.PROFILE]
    finally:
        _lib.PROFILE = None
    assert calls == ["sy11_iq_cyclo", "sy11_cyclo_peaks"]                      # ONE stage-1 launch, ONE stage-2 launch
    assert c.plan.J.tolist() == [1, 16, 0, 17, 33] and c.plan.groups.tolist() == [1, 1, 0, 2, 3] and c.valid.tolist() == [True, True, False, True, True]
    return N, clips, ext, c


# ------------------------------------------------------------------------------------------------------------- stage 1
def test_partial_rows_and_moments_match_the_float64_reference(case):
    N, clips, ext, c = case
    part, mom = c.partial.cpu().numpy(), c.mom.cpu().numpy()
    assert part.shape == (c.plan.total_rows, 3, N) and part.dtype == np.float32 and mom.shape == (c.plan.total_rows, 4) and c.plan.total_rows == 7
    over = []                                                                # every figure is printed before the verdict
    for i, x in enumerate(clips):
        if not c.valid[i]:
            continue
        want, emu = R.partials64(x, N), R.emulate32(x, N).astype(np.float64)
        got = part[int(c.plan.row0[i]):int(c.plan.row0[i + 1])].astype(np.float64)
        assert got.shape == want.shape == emu.shape
        for g in range(want.shape[0]):
            for q in range(3):
                scale = want[g, q].max()
                e_emu, e_gpu = np.abs(emu[g, q] - want[g, q]).max() / scale, np.abs(got[g, q] - want[g, q]).max() / scale
                print(f"iq_cyclo[N={N} clip {i} J={int(c.plan.J[i])} group {g} q={q}]: float32 emulation {e_emu:.3e}, kernel {e_gpu:.3e} (bar {4 * e_emu:.3e})")
                assert e_emu > 0
                if not e_gpu <= 4 * e_emu:
                    over.append((N, i, g, q, e_gpu, e_emu))
        m20, m21, m42 = R.moments(x, N)
        s = mom[int(c.plan.row0[i]):int(c.plan.row0[i + 1])].sum(0)
        err = (abs(complex(s[0], s[1]) - m20) / m21, abs(s[2] - m21) / m21, abs(s[3] - m42) / m42)
        print(f"iq_cyclo[N={N} clip {i}] moments: relative errors {err[0]:.2e} {err[1]:.2e} {err[2]:.2e}")
        assert max(err) <= 1e-12, (i, err)                                   # at most 2^14 float64 additions of a few 1e-16 each
    assert not over, over


# ------------------------------------------------------------------------------------------------------------- stage 2
def test_reduction_equals_the_reference_on_the_kernels_own_partials(case):
    """Bins and counts with no tolerance; the reference does the same IEEE operations in the same order on the same float32 table, so the
    floats agree far inside the 1e-12 asked of them."""
    N, clips, ext, c = case
    part, mom, spectra = c.partial.cpu().numpy(), c.mom.cpu().numpy(), c.spectra.cpu().numpy()
    assert spectra.shape == (5, 3, N) and np.isnan(spectra[2]).all()
    rel = lambda a, b: a == b or abs(a - b) <= 1e-12 * abs(b)                 # noqa: E731
    for i, x in enumerate(clips):
        if not c.valid[i]:
            continue
        rows = slice(int(c.plan.row0[i]), int(c.plan.row0[i + 1]))
        J, fs = int(c.plan.J[i]), float(ext.sample_rate[i])
        assert int(c.plan.k_min[i]) == R.plan(len(x), fs, N, 2.0e4)["k_min"]
        r = R.reduce(part[rows], N, J, int(c.plan.k_min[i]))
        assert c.peak_bin[i].tolist() == r["k"] and c.raw["n_search"][i].tolist() == r["n_search"]
        for key in ("peak", "left", "right", "median"):
            assert all(rel(float(a), b) for a, b in zip(c.raw[key][i], r[key])), (i, key, c.raw[key][i], r[key])
        assert np.abs(spectra[i] - r["P"]).max() <= 1e-12 * r["P"].max()
        m = np.zeros(4)
        for row in mom[rows]:                                                # ascending g, one after the other
            m = m + row
        assert (c.raw["m20"][i], c.raw["m21"][i], c.raw["m42"][i]) == (complex(m[0], m[1]), m[2], m[3])
        d = R.derive(r, (complex(m[0], m[1]), m[2], m[3]), N, J, fs, FC, 13.0)
        for key in ("symbol_rate", "offset2", "offset4", "power", "c42", "carrier"):
            got = float(getattr(c, key)[i])
            assert (np.isnan(got) and np.isnan(d[key])) or rel(got, d[key]), (i, key, got, d[key])
        assert np.allclose(c.line_db[i], d["line_db"], rtol=1e-12, atol=0) and int(c.order[i]) == d["order"] and bool(c.keyed[i]) == d["keyed"]
        assert np.array_equal(c.freqs(i, 1), np.arange(-N // 2, N // 2) * fs / N)
    assert c.order[2] == -1 and c.frames.tolist() == [1, 16, -1, 17, 33] and np.isnan(c.symbol_rate[2]) and c.peak_bin[2].tolist() == [-1, -1, -1]
    assert c.cls.tolist() == ext.cls.tolist() and c.names == ext.names and c.rows.tolist() == ext.rows.tolist()
    if N == 1024:                                                            # long enough to say what the clips are
        assert c.order.tolist() == [0, 2, -1, 4, 2] and c.keyed.tolist() == [False, True, False, True, False]
        assert abs(c.symbol_rate[1] - ext.sample_rate[1] / 3.3) < 0.25 * ext.sample_rate[1] / N
        assert abs(c.offset4[3] - 5.3 / 64 * ext.sample_rate[3]) < 0.25 / 4 * ext.sample_rate[3] / N


def test_a_tie_takes_the_first_maximum_and_the_neighbours_are_cyclic():
    """A hand-made partial table of two groups: equal maxima (the lower bin wins), a larger value below k_min (not searched at q = 0), a
    peak on bin -N/2 whose left neighbour is bin N/2 - 1; the second clip writes output row 0, the first row 2, row 1 is left alone."""
    from sy11 import ops
    N, J = 64, 17
    part = np.ones((4, 3, N), dtype=np.float32)
    part[0, 0, [2, 9, 20]] = (50.0, 4.0, 1.0)
    part[1, 0, [2, 9, 20]] = (50.0, 3.0, 6.0)                # bins 9 and 20 both sum to 7; bin 2 lies below k_min = 3
    part[0, 1, [64 - 5, 6]] = 9.0                            # bins -5 and 6
    part[1, 2, [64 - 32, 31]] = 4.0                          # bins -32 and 31
    part[2:, :, 7] = 3.0                                     # the other clip: one line on bin 7 everywhere
    mom = np.arange(16, dtype=np.float64).reshape(4, 4)
    from sy11.data.characterize import ROW
    rows = np.zeros(2, dtype=ROW)
    scale = 1.0 / (J * N * R.window(N)[1])
    rows["row0"], rows["n_rows"], rows["clip"], rows["k_min"], rows["scale"] = (0, 2), 2, (2, 0), (3, 8), scale
    spectra, out = ops.cyclo_peaks(torch.from_numpy(part).to(DEV), torch.from_numpy(mom).to(DEV), rows, 3)
    out, spectra = out.cpu().numpy(), spectra.cpu().numpy()
    r = R.reduce(part[:2], N, J, 3)
    assert r["k"] == [9, -5, -32] and out[2, 16:22].tolist() == [9, 29, -5, 64, -32, 64]
    for q in range(3):
        assert out[2, 4 * q:4 * q + 4].tolist() == [r["peak"][q], r["left"][q], r["right"][q], r["median"][q]]
    assert out[2, 10] == r["right"][2] and out[2, 9] == r["left"][2] == 5.0 * scale and r["right"][2] == 2.0 * scale      # bins 31 and -31
    assert out[2, 12:16].tolist() == [4.0, 6.0, 8.0, 10.0] and out[0, 12:16].tolist() == [20.0, 22.0, 24.0, 26.0]
    r2 = R.reduce(part[2:], N, J, 8)
    assert out[0, 16:22].tolist() == [8, 24, 7, 64, 7, 64] and r2["k"] == [8, 7, 7]             # bin 7 is not searched at q = 0: a flat set, the first bin
    assert np.isnan(out[1]).all() and np.isnan(spectra[1]).all() and (spectra[2] == r["P"]).all() and (spectra[0] == r2["P"]).all()


# ------------------------------------------------------------------------------------------------------------- invariance
def test_one_call_per_clip_and_a_permuted_extraction_give_the_same_bits(case):
    from sy11.data.characterize import characterize_extraction
    N, clips, ext, c = case
    D = [1, 2, 1, 4, 1]
    perm = [4, 2, 0, 3, 1]
    p = characterize_extraction(_extraction(clips, D=D, order=perm), N, 2.0e4, 13.0)
    assert p.rows.tolist() == perm
    for at, i in enumerate(perm):
        one = characterize_extraction(_extraction([clips[i]], D=[D[i]]), N, 2.0e4, 13.0)
        for other, k in ((p, at), (one, 0)):
            assert torch.equal(_bits(other.spectra[k]), _bits(c.spectra[i])), (i, at)
            for key in c.raw:
                assert np.array_equal(np.asarray(other.raw[key][k]), np.asarray(c.raw[key][i]), equal_nan=True), (i, key)
            assert bool(other.valid[k]) == bool(c.valid[i]) and int(other.order[k]) == int(c.order[i])
            if c.valid[i]:
                a = other.partial[int(other.plan.row0[k]):int(other.plan.row0[k + 1])]
                b = c.partial[int(c.plan.row0[i]):int(c.plan.row0[i + 1])]
                assert torch.equal(_bits(a), _bits(b))
                assert torch.equal(_bits(other.mom[int(other.plan.row0[k]):int(other.plan.row0[k + 1])]), _bits(c.mom[int(c.plan.row0[i]):int(c.plan.row0[i + 1])]))


# ------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_raise_and_write_nothing(case):
    from sy11 import _lib, ops
    from sy11.data.characterize import group
    from sy11.data.measure import tables_on
    N, clips, ext, c = case
    E_, G, H = _lib.Sy11Error, group(), N // 2
    items, rows = c.plan.items()[0], c.plan.rows()
    window, twiddle, _ = tables_on(DEV, N)
    x, n_rows = ext.packed, c.plan.total_rows
    part = torch.full((n_rows, 3, N), -7.0, dtype=torch.float32, device=DEV)
    mom = torch.full((n_rows, 4), -7.0, dtype=torch.float64, device=DEV)

    def one(k=0, **kw):
        s = items[k:k + 1].copy()
        for key, v in kw.items():
            s[key] = v
        return s
    last = items.shape[0] - 1                                                 # the J = 33 clip's third item: it ends the packed buffer
    assert int(items["off"][last] + items["len"][last]) == x.shape[0] and int(items["last"][last]) == 1 and int(items["j0"][last]) == 32
    for kw, what in ((dict(off=-1), "packed samples"), (dict(len=N - 1), "packed samples"), (dict(off=int(items["off"][last]) + 1), "packed samples"),
                     (dict(len=x.shape[0] + 1, off=0), "packed samples"),
                     (dict(nf=0), "one group"), (dict(nf=G + 1), "one group"), (dict(j0=-1), "one group"), (dict(j0=G - 1, nf=2), "one group"),
                     (dict(j0=32, nf=2), "leave the clip"), (dict(j0=48, nf=1), "leave the clip"),
                     (dict(last=0), "last ="), (dict(last=2), "last ="),
                     (dict(row=-1), "writes row"), (dict(row=n_rows), "writes row")):
        with pytest.raises(E_, match=what):
            ops.iq_cyclo(x, N, one(last, **kw), window, twiddle, part, mom)
    with pytest.raises(E_, match="last ="):
        ops.iq_cyclo(x, N, one(last - 1, last=1), window, twiddle, part, mom)    # a middle item may not own the clip's end
    with pytest.raises(E_, match="a row takes one item"):
        ops.iq_cyclo(x, N, np.concatenate((one(0), one(1, row=int(items["row"][0])))), window, twiddle, part, mom)
    with pytest.raises(E_, match="packed samples"):
        ops.iq_cyclo(x[:-1], N, one(last), window, twiddle, part, mom)           # the clip ends one sample past the buffer
    for n_fft in (48, 2048):
        with pytest.raises(E_, match="n_fft"):
            ops.iq_cyclo(x, n_fft, items, window, twiddle, part, mom)
    for bad in (dict(x=x.to(torch.complex128)), dict(x=x[::2]), dict(x=x.cpu()),
                dict(part=part[:, :, :-1]), dict(part=part.double()), dict(part=part[:, :2]), dict(mom=mom.float()), dict(mom=mom[:-1]), dict(mom=mom[:, :3]),
                dict(window=window[:-1]), dict(twiddle=twiddle[:-1]), dict(twiddle=twiddle.to(torch.complex64)),
                dict(items=items[:0]), dict(items=np.zeros((2, 6), dtype=np.int64))):
        a = dict(x=x, part=part, mom=mom, window=window, twiddle=twiddle, items=items)
        a.update(bad)
        with pytest.raises(E_):
            ops.iq_cyclo(a["x"], N, a["items"], a["window"], a["twiddle"], a["part"], a["mom"])
    # the library's own checks, behind the wrapper's: an unsupported size, null pointers, misalignment, every table-entry check once
    p = lambda v: C.c_void_p(v.data_ptr())                                    # noqa: E731
    keep = []

    def lib_args(host):
        t = torch.from_numpy(host.view(np.uint8).copy()).to(DEV)
        keep.extend((host, t))
        return [N, host.shape[0], C.c_void_p(host.ctypes.data), p(t), p(window), p(twiddle), x.shape[0], p(x), n_rows, p(part), p(mom), None]
    for pos, v in ((0, 48), (0, 2048), (1, 0), (2, None), (3, None), (4, None), (5, None), (7, None), (9, None), (10, None), (6, x.shape[0] - 1),
                   (6, 0), (8, n_rows - 1), (8, 0), (7, C.c_void_p(x.data_ptr() + 4)), (10, C.c_void_p(mom.data_ptr() + 4))):
        bad = lib_args(items)
        bad[pos] = v
        with pytest.raises(E_):
            _lib.call("sy11_iq_cyclo", *bad)
    for kw in (dict(off=-1), dict(len=N - 1), dict(off=int(items["off"][last]) + 1), dict(nf=0), dict(nf=G + 1), dict(j0=-1), dict(j0=G - 1, nf=2),
               dict(j0=32, nf=2), dict(last=0), dict(last=2), dict(row=-1), dict(row=n_rows)):
        with pytest.raises(E_, match="iq_cyclo: item 0"):
            _lib.call("sy11_iq_cyclo", *lib_args(one(last, **kw)))
    with pytest.raises(E_, match="an earlier item"):
        _lib.call("sy11_iq_cyclo", *lib_args(np.concatenate((one(0), one(1, row=int(items["row"][0]))))))
    torch.cuda.synchronize()
    assert bool((part == -7.0).all()) and bool((mom == -7.0).all())           # no refused call wrote anything
    # stage 2
    good_p, good_m = c.partial, c.mom
    spectra = torch.full((5, 3, N), -7.0, dtype=torch.float64, device=DEV)
    out = torch.full((5, 22), -7.0, dtype=torch.float64, device=DEV)

    def row(k=0, **kw):
        s = rows[k:k + 1].copy()
        for key, v in kw.items():
            s[key] = v
        return s
    entry = (dict(row0=-1), dict(n_rows=0), dict(row0=n_rows), dict(clip=-1), dict(clip=5), dict(k_min=0), dict(k_min=H), dict(scale=0.0),
             dict(scale=float("nan")), dict(scale=float("inf")))
    for kw in entry:
        with pytest.raises(E_, match="cyclo_peaks"):
            ops.cyclo_peaks(good_p, good_m, row(**kw), 5, spectra, out)
    with pytest.raises(E_, match="an output row takes one entry"):
        ops.cyclo_peaks(good_p, good_m, np.concatenate((row(0), row(1, clip=int(rows["clip"][0])))), 5, spectra, out)
    for bad in (dict(partial=good_p.double()), dict(partial=good_p[:, :, :-1]), dict(partial=good_p.cpu()), dict(partial=good_p[:0]), dict(mom=good_m[:-1]),
                dict(mom=good_m.float()), dict(rows=rows[:0]), dict(rows=np.zeros((2, 4), dtype=np.int64)), dict(n_clip=0), dict(spectra=spectra[:4]),
                dict(out=out[:, :21]), dict(out=out.float())):
        a = dict(partial=good_p, mom=good_m, rows=rows, n_clip=5, spectra=spectra, out=out)
        a.update(bad)
        with pytest.raises(E_):
            ops.cyclo_peaks(a["partial"], a["mom"], a["rows"], a["n_clip"], a["spectra"], a["out"])

    def lib_rows(host):
        t = torch.from_numpy(host.view(np.uint8).copy()).to(DEV)
        keep.extend((host, t))
        return [N, host.shape[0], C.c_void_p(host.ctypes.data), p(t), n_rows, p(good_p), p(good_m), 5, p(spectra), p(out), None]
    for pos, v in ((0, 48), (1, 0), (2, None), (3, None), (5, None), (6, None), (8, None), (9, None), (4, n_rows - 1), (7, 4), (7, 0),
                   (9, C.c_void_p(out.data_ptr() + 4))):
        bad = lib_rows(rows)
        bad[pos] = v
        with pytest.raises(E_):
            _lib.call("sy11_cyclo_peaks", *bad)
    for kw in entry:
        with pytest.raises(E_, match="cyclo_peaks: clip 0"):
            _lib.call("sy11_cyclo_peaks", *lib_rows(row(**kw)))
    with pytest.raises(E_, match="an earlier entry"):
        _lib.call("sy11_cyclo_peaks", *lib_rows(np.concatenate((row(0), row(1, clip=int(rows["clip"][0]))))))
    torch.cuda.synchronize()
    assert bool((spectra == -7.0).all()) and bool((out == -7.0).all())


# ------------------------------------------------------------------------------------------------------------- end to end
def _embedded():
    """A noise capture at 4 MHz with a BPSK, a QPSK and a CW emission (13.2 samples per symbol: 3.3 after decimation by 4) one after the
    other, each 37.3 bins of a 1024-point transform at 1 MHz off the centre of its hand-written box; the fourth box holds noise alone.
    -> (capture complex64, tf (4, 4), kinds)."""
    fs, n_each, gap = 4.0e6, 4 * 8400, 2000
    kinds, centres = ("bpsk", "qpsk", "cw", "noise"), (-1.1e6, 0.6e6, 1.2e6, -0.3e6)
    g = np.random.default_rng(5)
    n = 4 * (n_each + gap) + gap
    x = (g.standard_normal(n) + 1j * g.standard_normal(n)) * np.sqrt(0.02)     # 0.04 over 4 MHz: 0.01 in a clip's 1 MHz, 20 dB below the signal
    tf = []
    for i, (kind, fcen) in enumerate(zip(kinds, centres)):
        a = gap + i * (n_each + gap)
        if kind != "noise":
            s = R.clip(kind, n_each, 20 + i, 13.2, 37.3 / 1024 / 4, 300.0).astype(np.complex128)          # no noise of its own
            x[a:a + n_each] += s * np.exp(2j * np.pi * fcen / fs * np.arange(a, a + n_each))
        tf.append((a / fs, FC + fcen - 2.5e5, (a + n_each - 1) / fs, FC + fcen + 2.5e5))
    return x.astype(np.complex64), np.array(tf), kinds


def test_extract_then_characterize_names_four_embedded_emissions(tmp_path):
    from sy11 import _lib
    from sy11.data.characterize import Characterization
    from sy11.data.spectrogram import open_iq
    from sy11.engine.model import YOLO
    from sy11.engine.predictor import DetectionPredictor, ScanResults
    fs = 4.0e6
    x, tf, kinds = _embedded()
    boxes = torch.zeros((4, 6), dtype=torch.float64)
    boxes[:, 4], boxes[:, 5] = torch.tensor([0.9, 0.8, 0.7, 0.6], dtype=torch.float64), torch.tensor([1.0, 0.0, 1.0, 0.0], dtype=torch.float64)
    res = ScanResults(boxes, torch.zeros(4, dtype=torch.int64), torch.from_numpy(tf), {0: "a", 1: "b"}, np.zeros(1, dtype=np.int64), fs, FC)
    pred = DetectionPredictor.__new__(DetectionPredictor)                     # extract and characterize read the device alone
    pred.device = DEV
    src = open_iq(torch.from_numpy(x))
    ext = pred.extract(src, res, fs, FC, decimate=4)
    assert len(ext) == 4 and ext.sample_rate.tolist() == [1.0e6] * 4 and all(8400 <= m <= 8402 for m in ext.plan.M)
    _lib.PROFILE = []
    try:
        c = pred.characterize(ext)
        calls = [k[0] for k in _lib.PROFILE]
    finally:
        _lib.PROFILE = None
    assert isinstance(c, Characterization) and calls == ["sy11_iq_cyclo", "sy11_cyclo_peaks"] and len(c) == 4 and c.valid.all()
    assert c.cls.tolist() == [1, 0, 1, 0] and c.conf.tolist() == [0.9, 0.8, 0.7, 0.6] and c.names == res.names and c.rows.tolist() == [0, 1, 2, 3]
    host = ext.packed.cpu().numpy()
    bin_hz = 1.0e6 / 1024
    for i, (kind, order, keyed, c42) in enumerate(zip(kinds, (2, 4, 2, 0), (True, True, False, False), (None, -1.0, -1.0, 0.0))):
        clip = host[int(ext.plan.offset[i]):int(ext.plan.offset[i + 1])]
        r = R.characterize(clip, 1.0e6, float(ext.center_freq[i]), 1024)
        print(f"characterize[{kind}]: lines {c.line_db[i, 0]:.1f} / {c.line_db[i, 1]:.1f} / {c.line_db[i, 2]:.1f} dB, rate {c.symbol_rate[i] / bin_hz:.3f} bins, "
              f"offset2 {c.offset2[i] / bin_hz:.3f}, offset4 {c.offset4[i] / bin_hz:.3f} bins, c42 {c.c42[i]:.3f}, order {c.order[i]}, keyed {c.keyed[i]}")
        # the reference on the extraction's own samples: peak bins exact, derived columns to 1e-9
        assert c.peak_bin[i].tolist() == r["k"] and int(c.order[i]) == r["order"] and bool(c.keyed[i]) == r["keyed"] and int(c.frames[i]) == r["J"]
        for key in ("symbol_rate", "offset2", "offset4", "power", "c42", "carrier"):
            got = float(getattr(c, key)[i])
            assert (np.isnan(got) and np.isnan(r[key])) or abs(got - r[key]) <= 1e-9 * abs(r[key]), (kind, key, got, r[key])
        assert np.allclose(c.line_db[i], r["line_db"], rtol=1e-9, atol=0)
        # the truths of the CPU test
        off = (tf[i, 1] + tf[i, 3]) / 2 + 37.3 * bin_hz - float(ext.center_freq[i])        # from the centre the extraction really applied
        assert int(c.order[i]) == order and bool(c.keyed[i]) == keyed
        if keyed:
            assert abs(c.symbol_rate[i] - 1.0e6 / 3.3) <= 0.25 * bin_hz
        if order == 2:
            assert abs(c.offset2[i] - off) <= 0.25 / 2 * bin_hz and abs(c.carrier[i] - (float(ext.center_freq[i]) + off)) <= 0.25 / 2 * bin_hz
        if order == 4:
            assert abs(c.offset4[i] - off) <= 0.25 / 4 * bin_hz and abs(c.carrier[i] - (float(ext.center_freq[i]) + off)) <= 0.25 / 4 * bin_hz
        if order == 0:
            assert np.isnan(c.carrier[i])
        if c42 is not None:                                                  # BPSK off its centre reads about -0.6: see tests/test_characterize_cpu.py
            assert abs(c.c42[i] - c42) <= 0.3
    # the public entry and save
    y = YOLO.__new__(YOLO)
    y.device = DEV
    c2 = y.characterize(ext, n_fft=1024, min_rate=None, line_db=13.0)
    assert torch.equal(_bits(c2.spectra), _bits(c.spectra)) and c2.order.tolist() == c.order.tolist()
    out = c.save(tmp_path / "c")
    z = np.load(tmp_path / "c" / "characterize.npz")
    assert out == str(tmp_path / "c") and z["spectra"].shape == (4, 3, 1024) and np.array_equal(z["symbol_rate"], c.symbol_rate) and (tmp_path / "c" / "characterize.json").exists()
    # an empty extraction: no launch
    none = pred.extract(src, res, fs, FC, rows=[], decimate=4)
    _lib.PROFILE = []
    try:
        e = pred.characterize(none)
        calls = list(_lib.PROFILE)
    finally:
        _lib.PROFILE = None
    assert calls == [] and len(e) == 0 and e.spectra.shape == (0, 3, 1024) and e.spectra.is_cuda
