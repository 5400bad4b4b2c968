"""GPU: the measurement kernels (sy11_iq_psd, sy11_psd_measure).  Stage 1 against the float64 reference of tests/_measure_ref.py under the
rule of tests/test_resample_gpu.py (per box, 4x the error of the float32 emulation of the same sums, which must be > 0); stage 2 against
the same reference's ``reduce`` fed with the kernel's own partial table, with no tolerance at all; chunking, source and base invariance
bit for bit; absolute sample indices past 2^31; the refusals; and ``measure`` behind the three kinds of scan and ``link``."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _measure_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FS, FC, N_CAP = 1.0e6, 2.4e9, 40000
# (first frame, frames, f_lo - FC, f_hi - FC) at n_fft = 1024 (77 frames, G = 16); at n_fft = 64 the first frame is 16 j + 3 (aligned: 16 j),
# so the frame counts, which are what the groups see, stay.  None: the box is given in seconds instead.
SPEC = [
    (5, 20, 1.2e5, 1.8e5, False),          # 0  overlaps 1 in time and in frequency
    (10, 12, 1.0e5, 1.6e5, False),         # 1
    None,                                  # 2  starts before sample 0
    None,                                  # 3  ends on the last sample
    (33, 1, -2.4e5, -1.6e5, False),        # 4  J = 1
    (18, "G-1", -2.6e5, -1.4e5, False),    # 5  J = G - 1
    (16, "G", 2.8e5, 3.2e5, True),         # 6  J = G, one whole group
    (40, "G+1", 2.9e5, 3.1e5, False),      # 7  J = G + 1
    (13, 44, -2.5e5, -1.5e5, False),       # 8  three or four groups, both ends unaligned
    (20, 10, 100100.0, 100300.0, False),   # 9  narrower than a bin at either size: the nearest bin
    (50, 20, -5.0e5, 5.0e5, False),        # 10 the whole band: no noise bins
    (52, 9, -2.5e5, -1.5e5, False),        # 11 overlaps 8 and 10
    (23, "G", 1.0e5, 2.0e5, False),        # 12 J = G across two groups
]
IN_SECONDS = {2: (-0.002, -2.5e5, 0.0065, -1.5e5), 3: (0.0300, 2.85e5, N_CAP / FS, 3.15e5)}


def _capture(n, seed=0):
    """Noise of variance 0.01 and three band-limited bursts (the passband of an FFT mask), float32."""
    g = np.random.default_rng(seed)
    x = (g.standard_normal(n) + 1j * g.standard_normal(n)) * np.sqrt(0.005)
    for a, b, f0, bw, p in ((200, 2300, 1.5e5, 6.0e4, 0.05), (7000, 21000, -2.0e5, 1.0e5, 0.02), (24000, 39500, 3.0e5, 3.0e4, 0.1)):
        b = min(b, n)
        if b - a < 1000:
            continue
        spec = np.fft.fft(g.standard_normal(b - a) + 1j * g.standard_normal(b - a))
        f = np.fft.fftfreq(b - a, 1 / FS)
        spec[np.abs(f - f0) > bw / 2] = 0
        burst = np.fft.ifft(spec)
        x[a:b] += burst * np.sqrt(p / np.mean(np.abs(burst) ** 2))
    return x.astype(np.complex64)


def _boxes(N, G):
    H, tf = N // 2, []
    for i, s in enumerate(SPEC):
        if s is None:
            t0, lo, t1, hi = IN_SECONDS[i]
        else:
            j, J, lo, hi, aligned = s
            J = {"G-1": G - 1, "G": G, "G+1": G + 1}.get(J, J)
            j = j if N == 1024 else (16 * j if aligned else 16 * j + 3)
            t0, t1 = (j + 0.25) * H / FS, (j + J - 1 + 1.5) * H / FS    # floor(t0 fs / H) = j, ceil(t1 fs / H) - 2 = j + J - 1
        tf.append((t0, FC + lo, t1, FC + hi))
    return np.array(tf, dtype=np.float64)


def _bits(t):
    t = torch.view_as_real(t) if t.is_complex() else t
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _same(a, b):
    """Two Measurements agree bit for bit in everything the device wrote."""
    return all(torch.equal(_bits(u), _bits(v)) for u, v in ((a.partial, b.partial), (a.env, b.env), (a.psd, b.psd))) \
        and all(np.array_equal(a.raw[k], b.raw[k], equal_nan=True) for k in a.raw)


@pytest.fixture(scope="module", params=[64, 1024])
def case(request):
    """The capture, its plan and ONE stage-1 launch over all thirteen boxes; shared and left unchanged."""
    from sy11.data.measure import group, measure_capture, plan_measure, plan_measure_chunks
    N, G = request.param, group()
    x = _capture(N_CAP, 3)
    tf = _boxes(N, G)
    plan = plan_measure(tf, N_CAP, FS, FC, n_fft=N)
    ref = R.plan(tf, N_CAP, FS, FC, N)
    for key in ("j_first", "J", "k_lo", "k_hi", "s_lo", "s_hi", "n_noise"):
        assert getattr(plan, key).tolist() == ref[key].tolist(), key
    J = plan.J.tolist()
    assert [J[i] for i in (4, 5, 6, 7, 12)] == [1, G - 1, G, G + 1, G] and plan.groups[6] == 1 and plan.groups[12] == 2 and plan.groups[8] >= 3
    assert plan.j_first[2] == 0 and plan.j_first[3] + plan.J[3] - 1 == (N_CAP - N) // (N // 2)
    assert plan.j_first[8] % G != 0 and (plan.j_first[8] + plan.J[8]) % G != 0
    assert plan.k_lo[9] == plan.k_hi[9] and plan.n_noise[10] == 0 and (plan.k_lo[10], plan.k_hi[10]) == (-N // 2, N // 2 - 1)
    dev = torch.from_numpy(x).to(DEV)
    assert len(plan_measure_chunks(plan, 1 << 24)) == 1
    return N, G, x, dev, plan, measure_capture(dev, plan, DEV)


# ------------------------------------------------------------------------------------------------------------- stage 1
def test_welch_sums_and_envelope_match_the_float64_reference(case):
    N, G, x, dev, plan, m = case
    psd, env = m.psd.cpu().numpy(), m.env.cpu().numpy()
    assert psd.shape == (len(plan), N) and psd.dtype == np.float64 and env.shape == (plan.total_frames,) and m.partial.shape == (plan.total_rows, N)
    over = []                                                                # every figure is printed before the verdict
    for i in range(len(plan)):
        a = (int(plan.j_first[i]), int(plan.J[i]), int(plan.k_lo[i]), int(plan.k_hi[i]))
        P, E = R.welch(x, N, *a)
        part, E32 = R.emulate32(x, N, *a, G)
        P32 = R.reduce(part, N, a[1], a[2], a[3], int(plan.s_lo[i]), int(plan.s_hi[i]), plan.noise_l)["P"]
        t, Ek = m.envelope(i)
        assert np.array_equal(t, ((a[0] + np.arange(a[1])) * (N // 2) + N / 2) / FS)
        for what, got, want, emu in (("P", psd[i], P, P32), ("E", Ek.cpu().numpy().astype(np.float64), E, E32.astype(np.float64))):
            scale = np.abs(want).max()
            e_emu, e_gpu = np.abs(emu - want).max() / scale, np.abs(got - want).max() / scale
            print(f"iq_psd[N={N} box {i} J={a[1]} {what}]: float32 emulation {e_emu:.3e}, kernel {e_gpu:.3e} (bar {4 * e_emu:.3e})")
            assert got.shape == want.shape and e_emu > 0
            if not e_gpu <= 4 * e_emu:
                over.append((N, i, what, e_gpu, e_emu))
    assert not over, over


# ------------------------------------------------------------------------------------------------------------- stage 2
def test_reduction_equals_the_reference_on_the_kernels_own_partials(case):
    """No tolerance: the reference does the same IEEE operations in the same order on the same float32 table."""
    N, G, x, dev, plan, m = case
    part, psd = m.partial.cpu().numpy(), m.psd.cpu().numpy()
    want = [R.reduce(part[int(plan.row0[i]):int(plan.row0[i + 1])], N, int(plan.J[i]), int(plan.k_lo[i]), int(plan.k_hi[i]), int(plan.s_lo[i]),
                     int(plan.s_hi[i]), plan.noise_l, 0.99) for i in range(len(plan))]
    for key in ("k_dn", "k_up", "n_in", "n_noise"):
        assert np.array_equal(m.raw[key], np.array([w[key] for w in want])), key
    for key in ("p_in", "noise_median", "sum_c", "sum_kc"):
        a, b = m.raw[key], np.array([w[key] for w in want], dtype=np.float64)
        assert np.array_equal(np.isnan(a), np.isnan(b)) and (a[~np.isnan(a)] == b[~np.isnan(b)]).all(), (key, a, b)
    assert np.isnan(m.raw["noise_median"]).tolist() == [i == 10 for i in range(len(plan))]
    for i, w in enumerate(want):
        assert (psd[i] == w["P"]).all(), i
        d = R.derive(w, N, int(plan.J[i]), FS, FC)
        for key in ("power", "noise_density", "snr_db", "bandwidth", "centroid", "f_lo_meas", "f_hi_meas"):
            got, ref = float(getattr(m, key)[i]), d[key]
            assert (np.isnan(got) and np.isnan(ref)) or got == ref or abs(got - ref) <= 1e-12 * abs(ref), (i, key, got, ref)
    assert m.frames.tolist() == plan.J.tolist() and np.array_equal(m.freqs, FC + np.arange(-N // 2, N // 2) * FS / N)
    # the burst at +300 kHz (30 kHz wide, 0.1 against a noise of 0.01): box 3 sees it whole
    assert abs(m.centroid[3] - (FC + 3.0e5)) < max(3.0e3, FS / N / 2) and 2.0e4 < m.bandwidth[3] < 3.0e4 + 4 * FS / N and m.snr_db[3] > 10
    assert abs(m.noise_density[3] * FS / 0.01 - 1) < 0.2


# ------------------------------------------------------------------------------------------------------------- chunks and sources
def test_chunks_sources_and_an_odd_base_give_the_same_bits(case, tmp_path):
    from sy11 import _lib
    from sy11.data.measure import measure_capture, min_chunk, plan_measure_chunks
    from sy11.data.spectrogram import open_iq
    N, G, x, dev, plan, m = case
    x.view(np.float32).tofile(tmp_path / "capture.cf32")
    small = min_chunk(N)
    assert small == (G - 1) * (N // 2) + N and len(plan_measure_chunks(plan, small)) > 3
    buf = torch.zeros(N_CAP + 1, dtype=torch.complex64, device=DEV)
    buf[1:] = dev
    odd = buf[1:]
    assert odd.data_ptr() % 16 == 8
    for name, src in (("device tensor", open_iq(dev)), ("host array", open_iq(x)), ("memmap", open_iq(str(tmp_path / "capture.cf32"))),
                      ("odd base", open_iq(odd))):
        for chunk_samples, launches in ((small, len(plan_measure_chunks(plan, small))), (15000, None), (1 << 24, 1)):
            _lib.PROFILE = []
            try:
                got = measure_capture(src, plan, DEV, True, chunk_samples)
                calls = [c[0] for c in _lib.PROFILE]
            finally:
                _lib.PROFILE = None
            assert _same(got, m), (name, chunk_samples)
            assert calls[-1] == "sy11_psd_measure" and set(calls[:-1]) == {"sy11_iq_psd"} and (launches is None or len(calls) == launches + 1)
    bare = measure_capture(dev, plan, DEV, False)
    assert bare.env is None and torch.equal(_bits(bare.partial), _bits(m.partial)) and torch.equal(_bits(bare.psd), _bits(m.psd))
    with pytest.raises(ValueError, match="envelope=False"):
        bare.envelope(0)


# ------------------------------------------------------------------------------------------------------------- far into a capture
@pytest.mark.parametrize("N", [64, 1024])
def test_absolute_indices_near_three_billion_samples(N):
    """x holds samples [n0, n0 + 9000) of a long capture, n0 = 3e9 + 7.  Frames are anchored on absolute indices, so the frames inside x
    start at x[d], x[d + H], ... with d = -n0 mod H; with d taken mod G H instead, x[d] is also the first sample of a GROUP.  The same
    samples x[d:] declared to start at another multiple of G H — the one nearest to n0, and 0 — hold the same frames in the same groups,
    only renumbered by whole groups: every row and envelope value must be bit-identical.  (At N = 1024 the nearest multiple is n0 + d
    itself; the declaration at 0, where 32-bit indices would do, is what that case proves.)"""
    from sy11 import ops
    from sy11.data.measure import ITEM, group, tables_on
    G, H = group(), N // 2
    n, n0 = 9000, 3 * 10 ** 9 + 7
    x = _capture(n, 21)
    dev = torch.from_numpy(x).to(DEV)
    d = -n0 % (G * H)
    near = (n0 + G * H // 2) // (G * H) * (G * H)
    assert (n0 + d) % (G * H) == 0 and near in (n0 + d, n0 + d - G * H)
    frames = (n - d - N) // H + 1                               # whole frames of x[d:]
    assert frames >= 15

    def run(x_dev, base, n_total):
        j_first = -(-base // H)
        assert j_first % G == 0
        it = np.zeros(2 * -(-frames // G), dtype=ITEM)
        half = it.shape[0] // 2
        for b, (k_lo, k_hi) in enumerate(((-N // 4, N // 8), (3, 3))):       # two boxes over the same frames
            for g in range(half):
                nf = min(G, frames - g * G)
                it[b * half + g] = (j_first + g * G, b * frames + g * G, nf, b * half + g, k_lo, k_hi)
        part = torch.zeros((it.shape[0], N), dtype=torch.float32, device=DEV)
        env = torch.zeros((2 * frames,), dtype=torch.float32, device=DEV)
        assert ops.iq_psd(x_dev, base, n_total, N, it, *tables_on(DEV, N), part, env) is part
        return part, env, it
    part, env, it = run(dev[d:], n0 + d, n0 + n + 12345)
    for base in (near, 0):
        p2, e2, _ = run(dev[d:], base, base + n - d)
        assert torch.equal(_bits(p2), _bits(part)) and torch.equal(_bits(e2), _bits(env)), base
    p3 = torch.zeros_like(part)                                              # the same frames from the whole of x: in[] based at n0
    ops.iq_psd(dev, n0, n0 + n, N, it, *tables_on(DEV, N), p3, None)
    assert torch.equal(_bits(p3), _bits(part))
    half = it.shape[0] // 2
    for g in range(half):                                                     # and right: against float64, by the rule of stage 1
        j0, nf = int(it["j0"][g]), int(it["nf"][g])
        want = R.frame_powers(x, N, j0, nf, n0).sum(0)
        emu = R.emulate32(x, N, j0, nf, 0, 0, G, n0)[0][0].astype(np.float64)
        got = part[g].cpu().numpy().astype(np.float64)
        e_emu, e_gpu = np.abs(emu - want).max() / want.max(), np.abs(got - want).max() / want.max()
        print(f"iq_psd[N={N} at n0={n0} group {g}]: float32 emulation {e_emu:.3e}, kernel {e_gpu:.3e}")
        assert e_emu > 0 and e_gpu <= 4 * e_emu
        assert torch.equal(_bits(part[half + g]), _bits(part[g]))            # the sums do not depend on the box's bins


# ------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_raise_and_write_nothing(case):
    from sy11 import _lib, ops
    from sy11.data.measure import plan_measure_chunks, tables_on
    N, G, x, dev, plan, m = case
    E_ = _lib.Sy11Error
    items = plan_measure_chunks(plan, 1 << 24)[0].items
    window, twiddle, nw2 = tables_on(DEV, N)
    part = torch.full((plan.total_rows, N), -7.0, dtype=torch.float32, device=DEV)
    env = torch.full((plan.total_frames,), -7.0, dtype=torch.float32, device=DEV)

    def one(k=0, **kw):
        s = items[k:k + 1].copy()
        for key, v in kw.items():
            s[key] = v
        return s
    last, first = int(np.argmax(items["j0"] + items["nf"])), int(np.argmin(items["j0"]))
    end = (int(items["j0"][last]) + int(items["nf"][last]) - 1) * (N // 2) + N      # one past the last sample any item reads
    assert int(items["j0"][first]) == 0 and end == (N_CAP - N) // (N // 2) * (N // 2) + N
    ops.iq_psd(dev[:end], 0, N_CAP, N, items, window, twiddle, nw2, torch.empty_like(part), torch.empty_like(env))      # exactly the support
    with pytest.raises(E_, match="reads samples"):
        ops.iq_psd(dev[:end - 1], 0, N_CAP, N, items[last:last + 1], window, twiddle, nw2, part, env)
    with pytest.raises(E_, match="reads samples"):
        ops.iq_psd(dev[1:], 1, N_CAP, N, items[first:first + 1], window, twiddle, nw2, part, env)
    for row in (-1, plan.total_rows):
        with pytest.raises(E_, match="writes row"):
            ops.iq_psd(dev, 0, N_CAP, N, one(row=row), window, twiddle, nw2, part, env)
    with pytest.raises(E_, match="a row takes one item"):
        ops.iq_psd(dev, 0, N_CAP, N, np.concatenate((one(0), one(1, row=int(items["row"][0])))), window, twiddle, nw2, part, env)
    for off in (-1, plan.total_frames - int(items["nf"][0]) + 1):
        with pytest.raises(E_, match="envelope"):
            ops.iq_psd(dev, 0, N_CAP, N, one(env_off=off), window, twiddle, nw2, part, env)
    for kw in (dict(nf=0), dict(nf=G + 1), dict(j0=-1), dict(j0=G - 1, nf=2)):
        with pytest.raises(E_, match="one group"):
            ops.iq_psd(dev, 0, N_CAP, N, one(**kw), window, twiddle, nw2, part, env)
    for kw in (dict(k_lo=-N // 2 - 1), dict(k_hi=N // 2), dict(k_lo=5, k_hi=4)):
        with pytest.raises(E_, match="bins"):
            ops.iq_psd(dev, 0, N_CAP, N, one(**kw), window, twiddle, nw2, part, env)
    for n_fft in (48, 2048):
        with pytest.raises(E_, match="n_fft"):
            ops.iq_psd(dev, 0, N_CAP, n_fft, items, window, twiddle, nw2, part, env)
    for bad in (dict(x=dev.to(torch.complex128)), dict(x=dev[::2]), dict(x=dev.cpu()), dict(part=part[:, :-1]), dict(part=part.double()),
                dict(env=env.double()), dict(env=env[::2]), dict(window=window[:-1]), dict(twiddle=twiddle[:-1]),
                dict(items=items[:0]), dict(items=np.zeros((2, 6), dtype=np.int64))):
        a = dict(x=dev, part=part, env=env, window=window, twiddle=twiddle, items=items)
        a.update(bad)
        with pytest.raises(E_):
            ops.iq_psd(a["x"], 0, N_CAP, N, a["items"], a["window"], a["twiddle"], nw2, a["part"], a["env"])
    # the library's own checks, behind the wrapper's: an unsupported size, null pointers, a table entry out of range
    t = torch.from_numpy(items.view(np.uint8).copy()).to(DEV)
    p = lambda v: C.c_void_p(v.data_ptr())                                    # noqa: E731
    args = [N, items.shape[0], C.c_void_p(items.ctypes.data), p(t), p(window), p(twiddle), nw2, N_CAP, 0, N_CAP, p(dev), plan.total_rows,
            p(part), plan.total_frames, p(env), None]
    for pos, v in ((0, 48), (0, 2048), (2, None), (3, None), (4, None), (5, None), (10, None), (12, None), (14, None), (11, plan.total_rows - 1),
                   (13, plan.total_frames - 1), (9, end - 1)):
        bad = list(args)
        bad[pos] = v
        with pytest.raises(E_):
            _lib.call("sy11_iq_psd", *bad)
    torch.cuda.synchronize()
    assert bool((part == -7.0).all()) and bool((env == -7.0).all())           # no refused call wrote anything
    # stage 2
    boxes = plan.boxes()
    good = m.partial

    def box(**kw):
        s = boxes[:1].copy()
        for key, v in kw.items():
            s[key] = v
        return s
    for kw in (dict(row0=-1), dict(n_rows=0), dict(row0=plan.total_rows), dict(s_lo=-N // 2 - 1), dict(s_hi=N // 2), dict(k_lo=int(boxes["s_lo"][0]) - 1),
               dict(noise_l=N // 2 + 1), dict(scale=0.0), dict(corr=float("nan"))):
        with pytest.raises(E_, match="psd_measure"):
            ops.psd_measure(good, box(**kw), 0.005, 0.995)
    for fr in ((-0.1, 0.9), (0.6, 0.4), (0.1, 1.1)):
        with pytest.raises(E_, match="frac"):
            ops.psd_measure(good, boxes, *fr)
    for bad in (good.double(), good[:, :-1], good.cpu(), good[:0]):
        with pytest.raises(E_):
            ops.psd_measure(bad, boxes, 0.005, 0.995)
    with pytest.raises(E_):
        ops.psd_measure(good, boxes[:0], 0.005, 0.995)


# ------------------------------------------------------------------------------------------------------------- end to end
def _model(nc=2):
    from oracle import yolo11_ref as Y
    from sy11.nn.tasks import DetectionModel
    m = DetectionModel("yolo11n.yaml", nc=nc, verbose=False)
    sd = Y.seeded_state_dict(Y.empty_state_dict(Y.resolve_graph("n", nc=nc)), seed=7)
    for k in sd:                                               # confident random head, as tests/test_scan_gpu.py builds it
        if ".cv3." in k and k.endswith("2.bias"):
            sd[k] = sd[k] + 1.0
    m.load_state_dict(sd)
    m.names = {i: f"class_{i}" for i in range(nc)}
    return m


def test_measure_follows_tf_behind_every_kind_of_scan_and_link(tmp_path):
    """``measure(capture, scan(...))`` after a plain, a resampled / retuned and a channelised scan of ONE capture, and after ``link``: always
    with the capture's own rate and centre, one row per result (or per track) whose frames and bins follow from ``tf`` alone."""
    from sy11 import _lib
    from sy11.data import spectrogram as sp
    from sy11.data.measure import Measurement
    from sy11.engine.predictor import DetectionPredictor, ScanResults
    from tests import _scan_ref as S
    fs, fc, N = 40e6, 2.4e9, 256
    x = S.capture(3.1)
    src = sp.open_iq(x)
    pred = DetectionPredictor(_model(2), device=DEV, conf=0.05, iou=0.7, producer=sp.SpectrogramProducer(DEV))
    scans = {"plain": pred.scan(src, fs, fc), "resampled": pred.scan(src, fs, fc, resample_to=fs / 2, tune_to=fc + 3.3e6),
             "channelised": pred.scan(src, fs, fc, channels=4)}
    for name, res in scans.items():
        assert len(res) > 0
        m = pred.measure(src, res, fs, fc, n_fft=N)
        assert isinstance(m, Measurement) and len(m) == len(res) and m.rows.tolist() == list(range(len(res)))
        tf = res.tf.numpy()
        ref = R.plan(tf, len(x), fs, fc, N)
        assert m.frames.tolist() == ref["J"].tolist() and m.plan.j_first.tolist() == ref["j_first"].tolist()
        assert m.raw["n_in"].tolist() == ref["n_in"].tolist() and m.raw["n_noise"].tolist() == ref["n_noise"].tolist()
        assert m.plan.k_lo.tolist() == ref["k_lo"].tolist() and m.plan.s_hi.tolist() == ref["s_hi"].tolist() and np.array_equal(m.tf, tf)
        assert m.psd.shape == (len(res), N) and m.psd.is_cuda and bool((m.psd >= 0).all())
        assert ((m.raw["k_dn"] >= ref["s_lo"]) & (m.raw["k_dn"] <= m.raw["k_up"]) & (m.raw["k_up"] <= ref["s_hi"])).all()
        assert (m.power > 0).all() and m.cls.tolist() == res.boxes[:, 5].long().tolist() and m.names == res.names
        k = len(res) // 2                                                     # one row against the float64 reference
        P, _ = R.welch(x.numpy(), N, int(ref["j_first"][k]), int(ref["J"][k]), int(ref["k_lo"][k]), int(ref["k_hi"][k]))
        assert np.abs(m.psd[k].cpu().numpy() - P).max() <= 1e-4 * P.max()
        print(f"measure behind a {name} scan: {len(m)} rows, {m.plan.total_frames} frames in {m.plan.total_rows} groups")
        some = pred.measure(src, res, fs, fc, n_fft=N, rows=[len(res) - 1, 0])
        assert some.rows.tolist() == [len(res) - 1, 0] and torch.equal(_bits(some.psd[0]), _bits(m.psd[len(res) - 1]))
        assert torch.equal(_bits(some.psd[1]), _bits(m.psd[0])) and some.power.tolist() == [m.power[len(res) - 1], m.power[0]]
        linked = pred.link(res)
        mt = pred.measure(src, linked.tracks, fs, fc, n_fft=N)
        assert len(mt) == len(linked.tracks) and np.array_equal(mt.tf, linked.tracks.tf.numpy()) and mt.cls.tolist() == linked.tracks.cls.tolist()
        assert mt.frames.tolist() == R.plan(linked.tracks.tf.numpy(), len(x), fs, fc, N)["J"].tolist()
    out = m.save(tmp_path / "m")
    z = np.load(tmp_path / "m" / "measure.npz")
    assert out == str(tmp_path / "m") and np.array_equal(z["power"], m.power) and z["psd"].shape == (len(m), N) and (tmp_path / "m" / "measure.json").exists()
    assert set(m[0]) >= {"power", "snr_db", "bandwidth", "centroid"} and m[0]["power"] == m.power[0]
    res = scans["plain"]
    empty = ScanResults(res.boxes[:0], res.window[:0], res.tf[:0], res.names, res.start, res.sample_rate, res.center_freq)
    _lib.PROFILE = []
    try:
        none = [pred.measure(src, empty, fs, fc), pred.measure(src, res, fs, fc, rows=[])]
        calls = list(_lib.PROFILE)
    finally:
        _lib.PROFILE = None
    assert calls == [] and all(len(e) == 0 and e.psd.shape == (0, 1024) and e.power.shape == (0,) for e in none)     # no launch


def test_yolo_measure_is_the_public_entry():
    """``YOLO.measure`` opens the source as ``scan`` does and returns the predictor's measurement."""
    from sy11.data.link import Tracks
    from sy11.engine.model import YOLO
    assert callable(YOLO.measure)
    y = YOLO.__new__(YOLO)
    y.device = DEV
    x = torch.from_numpy(_capture(N_CAP, 3))
    tf = torch.tensor([[0.010, FC + 1.0e5, 0.020, FC + 2.0e5], [0.030, FC + 2.85e5, 0.040, FC + 3.15e5]], dtype=torch.float64)
    tr = Tracks(torch.tensor([0, 1]), tf, torch.tensor([0.9, 0.8], dtype=torch.float64), torch.tensor([1, 0]), torch.tensor([1, 1]),
                torch.tensor([0, 1]), names={0: "a", 1: "b"})
    m = y.measure(x, tr, FS, FC, n_fft=256)
    assert len(m) == 2 and m.cls.tolist() == [1, 0] and m.conf.tolist() == [0.9, 0.8] and abs(m.centroid[1] - (FC + 3.0e5)) < 3.0e3
