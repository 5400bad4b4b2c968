"""GPU: the frame decoder's kernels (sy11_fec_soft, sy11_fec_viterbi, sy11_fec_check) against tests/_fec_ref.py.  Every comparison is ``np.array_equal``:
the quantiser is one float32 product and a rounding, everything after it integer arithmetic, so no tolerance is due.  The kernel-level tests feed
synthetic buffers to ``ops.fec_*`` directly; one call over all frames, one call per frame and a permuted packing give the same bytes; every refusal
is raised by ``ops`` and by the library with the sentinel-filled outputs untouched; and ``demodulate`` -> ``find_frames`` -> ``decode`` on the three clips of
tests/test_decode_cpu.py decodes the embedded frames to what was sent, in exactly three launches."""
import copy
import ctypes as C
import json

import numpy as np
import pytest
import torch

from tests import _fec_ref as R
from tests import _frames_ref as F

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FC = 2.4e9
P_LONG = tuple(int(b) for b in np.random.default_rng(64).integers(0, 2, 64))


def _table(rows, **cols):
    from sy11.data.decode import FECFRAME
    fr = np.zeros(rows, dtype=FECFRAME)
    for k, v in cols.items():
        fr[k] = v
    return fr


def _mask(pattern):
    pat = (1, 1) if pattern is None else pattern
    return len(pat), sum(int(b) << i for i, b in enumerate(pat))


# ------------------------------------------------------------------------------------------------------------- launch 1
SCALES = (1.0, 32.0, 127.0)


def _components(g, n, scale):
    """``n`` float32 values whose product with ``scale`` lands on ties (k + 0.5: exact for the scales 1 and 32), on both saturations, on +-inf and NaN, on
    +-0, and anywhere."""
    k = g.integers(-130, 131, n).astype(np.float64)
    ties = ((k + 0.5) / scale).astype(np.float32)
    x = np.where(g.random(n) < 0.5, ties, (g.standard_normal(n) * 60.0 / scale).astype(np.float32)).astype(np.float32)
    special = np.array([np.inf, -np.inf, np.nan, 1e30, -1e30, 0.0, -0.0, 127.4 / scale, -127.6 / scale, 0.5 / scale, -0.5 / scale], dtype=np.float32)
    at = g.random(n) < 0.15
    x[at] = special[g.integers(0, special.shape[0], int(at.sum()))]
    return x


@pytest.mark.parametrize("pattern", [None, R.P64, P_LONG], ids=["unpunctured", "110110", "64-long"])
def test_soft_bits_every_order_rotation_scale_and_pattern(pattern):
    from sy11 import ops
    g = np.random.default_rng(11)
    period, mask = _mask(pattern)
    stretches, frames, want, T_top, total = [], [], [], 0, 0                   # every frame starts at an odd symbol of the packed buffer
    for order in (2, 4):
        for q in range(order):
            for scale in SCALES:
                T = int(g.integers(1, 200))
                T_top = max(T_top, T)
                need = R.n_need(T, pattern, order)[1]
                r = np.empty(need + 2, dtype=np.complex64)                      # the planes one by one: a complex product would spread a NaN
                r.real, r.imag = _components(g, need + 2, scale), _components(g, need + 2, scale)
                off = total + 1                                                 # one symbol of the stretch lies ahead of the frame
                stretches.append(np.concatenate((r, np.zeros((total + len(r)) % 2, dtype=np.complex64))))     # an even end: the next start is odd again
                total += len(stretches[-1])
                frames.append((off, T, order, q, np.float32(scale)))
                want.append(R.soft(r[1:1 + need], order, q, np.float32(scale), pattern, T))
    n = len(frames)
    assert n == 18 and all(f[0] % 2 == 1 for f in frames)
    perm = np.random.default_rng(3).permutation(n)                              # the rows in another order than the frames
    fr = _table(n, sym_off=[f[0] for f in frames], T=[f[1] for f in frames], order=[f[2] for f in frames], q=[f[3] for f in frames], tail=0, row=perm,
                scale=[f[4] for f in frames])
    sym = torch.from_numpy(np.concatenate(stretches)).to(DEV)
    soft = torch.full((n, 2 * T_top + 2), 99, dtype=torch.int8, device=DEV)
    ops.fec_soft(sym, fr, soft, period, mask)
    got = soft.cpu().numpy()
    seen = set()
    for k, y in enumerate(want):
        row = got[perm[k]]
        assert np.array_equal(row[:y.shape[0]], y), (k, frames[k])
        assert (row[y.shape[0]:] == 99).all()                                  # nothing beyond the frame's 2T
        seen |= set(y.tolist())
    assert {-127, 127, 0}.issubset(seen)
    if pattern is not None:
        sent = R.sent_mask(pattern, 2 * frames[0][1])
        assert not want[0][~sent].any()                                        # the erasures


def test_soft_bits_ties_round_to_even_and_saturate():
    from sy11 import ops
    x = np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 126.5, 127.5, -126.5, -127.5, 1e9, -1e9, np.inf, -np.inf, np.nan, 0.49999997], dtype=np.float32)
    want = [0, 2, 2, 0, -2, -2, 126, 127, -126, -127, 127, -127, 127, -127, 0, 0]
    assert R.quantize(x, 1.0).tolist() == want
    sym = torch.from_numpy((x + 0j).astype(np.complex64)).to(DEV)
    soft = torch.zeros((1, 16), dtype=torch.int8, device=DEV)
    ops.fec_soft(sym, _table(1, sym_off=0, T=8, order=2, q=0, tail=0, row=0, scale=1.0), soft)
    assert soft.cpu().numpy()[0].tolist() == want
    ops.fec_soft(sym, _table(1, sym_off=0, T=8, order=2, q=1, tail=0, row=0, scale=1.0), soft)
    assert soft.cpu().numpy()[0].tolist() == [-v for v in want]


# ------------------------------------------------------------------------------------------------------------- launch 2
T_MIX = (1, 6, 7, 63, 64, 65, 129, 1000, 8192)
KINDS = ("uniform", "zero", "full", "noise 0.7", "noise 1.0")


def _viterbi_frames(polys, seed=21):
    """64 frames: every T of ``T_MIX`` in both tail modes where legal, every kind of input; T = 8192 once per tail mode -> list of (T, tail, kind, y, u)."""
    g = np.random.default_rng(seed)
    shapes = [(T, tail) for T in T_MIX for tail in (0, 1) if T >= 7 or not tail]
    out = []
    for k in range(64):
        T, tail = shapes[k % len(shapes)] if k >= 2 else (8192, k)
        if T == 8192 and k >= 2:
            T = 1000
        kind = KINDS[(k * 7 + k // 5) % len(KINDS)] if k >= 2 else ("noise 1.0", "uniform")[k]
        u = g.integers(0, 2, T - 6 * tail)
        if kind == "uniform":
            y = g.integers(-127, 128, 2 * T).astype(np.int8)
        elif kind == "zero":
            y = np.zeros(2 * T, dtype=np.int8)
        elif kind == "full":
            y = (127 * (1 - 2 * g.integers(0, 2, 2 * T))).astype(np.int8)
        else:
            c = R.encode(u, polys, bool(tail)).astype(np.float64)
            y = R.quantize((1.0 - 2.0 * c) + float(kind.split()[1]) * g.standard_normal(2 * T), 32.0)
        out.append((T, tail, kind, y, u))
    return out


def _viterbi_reference(frames, polys):
    """The reference on every frame, batched by (T, tail) -> list of (u, metric, end)."""
    out = [None] * len(frames)
    groups = {}
    for k, f in enumerate(frames):
        groups.setdefault((f[0], f[1]), []).append(k)
    for (T, tail), ks in groups.items():
        u, metric, end = R.viterbi(np.stack([frames[k][3] for k in ks]), polys, bool(tail))
        for j, k in enumerate(ks):
            out[k] = (u[j], int(metric[j]), int(end[j]))
    return out


def _run_viterbi(frames, polys, rows=None, n_rows=None):
    from sy11 import ops
    n = len(frames)
    rows = np.arange(n) if rows is None else np.asarray(rows)
    n_rows = n if n_rows is None else n_rows
    T_top = max(f[0] for f in frames)
    soft = np.zeros((n_rows, 2 * T_top), dtype=np.int8)
    for k, f in enumerate(frames):
        soft[rows[k], :2 * f[0]] = f[3]
    soft = torch.from_numpy(soft).to(DEV)
    bits = torch.full((n_rows, min((T_top + 7) // 8 + 1, R.T_MAX // 8)), 0xA5, dtype=torch.uint8, device=DEV)
    out = torch.full((n_rows, 2), -7, dtype=torch.int32, device=DEV)
    fr = _table(n, sym_off=0, T=[f[0] for f in frames], order=2, q=0, tail=[f[1] for f in frames], row=rows, scale=1.0)
    ops.fec_viterbi(soft, fr, polys, bits, out)
    return bits.cpu().numpy(), out.cpu().numpy()


@pytest.mark.parametrize("polys", [(0o171, 0o133), (0o133, 0o171), (0o155, 0o117)], ids=["171 133", "133 171", "155 117"])
def test_viterbi_64_frames_of_mixed_length_equal_the_reference(polys):
    frames = _viterbi_frames(polys)
    assert len(frames) == 64 and {f[0] for f in frames} == set(T_MIX) and {(f[0], f[1]) for f in frames} >= {(8192, 0), (8192, 1), (1, 0), (6, 0), (7, 0), (7, 1)}
    assert {f[2] for f in frames} == set(KINDS)
    ref = _viterbi_reference(frames, polys)
    bits, out = _run_viterbi(frames, polys)
    wrong = {k: 0 for k in KINDS}
    for k, ((T, tail, kind, y, u), (ru, metric, end)) in enumerate(zip(frames, ref)):
        nb = (T + 7) // 8
        assert np.array_equal(np.unpackbits(bits[k, :nb])[:T], ru), (k, T, tail, kind)
        assert not np.unpackbits(bits[k, :nb])[T:].any() and not bits[k, nb:].any()                           # zeros after the T bits, to the end of the row
        assert out[k].tolist() == [metric, end], (k, T, tail, kind)
        if tail:
            assert end == 0
        if kind.startswith("noise"):
            wrong[kind] += int((ru[:u.shape[0]] != u).sum())
    print(f"viterbi[{polys[0]:o} {polys[1]:o}]: decoded bit errors of the reference, which the device repeats: {wrong}")
    assert wrong["noise 1.0"] > 0                                              # there the decoder makes errors, and they are the same errors


def test_viterbi_one_call_per_frame_and_a_permuted_packing_give_the_same_bytes():
    frames = [f for f in _viterbi_frames(R.POLYS) if f[0] <= 1000]
    bits, out = _run_viterbi(frames, R.POLYS)
    n = len(frames)
    perm = np.random.default_rng(5).permutation(n + 3)[:n]                      # other rows, of a larger table, in another order
    order = np.random.default_rng(6).permutation(n)
    pb, po = _run_viterbi([frames[k] for k in order], R.POLYS, rows=perm[order], n_rows=n + 3)
    width = bits.shape[1]
    for k, f in enumerate(frames):
        nb = (f[0] + 7) // 8
        assert np.array_equal(pb[perm[k], :nb], bits[k, :nb]) and po[perm[k]].tolist() == out[k].tolist()
        ob, oo = _run_viterbi([f], R.POLYS)
        assert np.array_equal(ob[0, :nb], bits[k, :nb]) and oo[0].tolist() == out[k].tolist() and ob.shape[1] <= width
    spare = np.setdiff1d(np.arange(n + 3), perm)
    assert (pb[spare] == 0xA5).all() and (po[spare] == -7).all()               # rows of no frame stay untouched


# ------------------------------------------------------------------------------------------------------------- launch 3
def _run_check(us, ys, n_info, tail, polys, whiten, spec):
    from sy11 import ops
    n, T = len(us), n_info + 6 * tail
    bits = np.zeros((n, (T + 7) // 8), dtype=np.uint8)
    soft = np.zeros((n, 2 * T), dtype=np.int8)
    for k in range(n):
        b = np.packbits(us[k])
        bits[k, :b.shape[0]], soft[k] = b, ys[k]
    data = torch.full((n, (n_info + 7) // 8 + 2), 0xA5, dtype=torch.uint8, device=DEV)
    rows = torch.full((n, 5), -7, dtype=torch.int32, device=DEV)
    fr = _table(n, sym_off=0, T=T, order=2, q=0, tail=tail, row=np.arange(n), scale=1.0)
    ops.fec_check(torch.from_numpy(soft).to(DEV), torch.from_numpy(bits).to(DEV), fr, polys, n_info, data, rows,
                  whiten=None if whiten is None else torch.from_numpy(np.asarray(whiten[:n_info], dtype=np.uint8)).to(DEV), crc=spec)
    return data.cpu().numpy(), rows.cpu().numpy()


SPECS = dict(R.CRCS, **{"none": None, "in only": dict(width=12, poly=0x80F, init=0x5A5, refin=True, refout=False, xorout=0x0FF),
                        "out only": dict(width=24, poly=0x864CFB, init=0xB704CE, refin=False, refout=True, xorout=0x000001)})


@pytest.mark.parametrize("name", list(SPECS))
def test_check_crc_whitening_and_channel_errors(name):
    spec = SPECS[name]
    W = spec["width"] if spec else 0
    g = np.random.default_rng(31)
    whiten = R.lfsr_bits((4, 7), [1, 1, 0, 1, 0, 0, 1], 200)
    msg = R.bits_of_bytes(b"123456789")
    for tail, wh in ((0, None), (1, whiten)):
        n_info, us, ys = 72 + W, [], []
        for k in range(4):
            m = msg if k == 0 else g.integers(0, 2, 72).astype(np.uint8)
            info = np.concatenate((m, R.int_bits(R.crc(m, spec), W))) if spec else m
            if k == 3 and spec:
                info[5] ^= 1                                                    # a wrong message under a good check field
            u = np.concatenate((info ^ (wh[:n_info] if wh is not None else 0), np.zeros(6 * tail, dtype=np.uint8)))
            c = R.encode(u, R.POLYS, tail=False).astype(np.int64)
            y = (1 - 2 * c) * g.integers(1, 128, c.shape[0])
            y[g.random(c.shape[0]) < 0.2] = 0                                   # erasures
            flip = g.random(c.shape[0]) < 0.1
            y[flip] = -y[flip]
            us.append(u), ys.append(y.astype(np.int8))
        data, rows = _run_check(us, ys, n_info, tail, R.POLYS, wh, spec)
        for k in range(4):
            want = R.check(ys[k], us[k], n_info, R.POLYS, wh, spec)
            nb = (n_info + 7) // 8
            assert np.array_equal(data[k, :nb], want["data"]) and not data[k, nb:].any(), (name, tail, k)
            assert rows[k].view(np.uint32)[:2].tolist() == [want["crc_calc"], want["crc_recv"]], (name, tail, k)
            assert rows[k, 2:].tolist() == [want["crc_ok"], want["channel_errors"], want["n_channel"]], (name, tail, k)
            assert want["channel_errors"] > 0 and want["n_channel"] < 2 * (n_info + 6 * tail)
            assert want["crc_ok"] == (-1 if spec is None else int(k != 3))
        if name in R.CRCS and tail == 0:                                        # the anchors on the device
            assert int(rows[0].view(np.uint32)[0]) == {"crc32": 0xCBF43926, "crc16-ccitt-false": 0x29B1, "crc16-x25": 0x906E, "crc8": 0xF4}[name]


# ------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_raise_and_write_nothing():
    from sy11 import _lib, ops
    E_ = _lib.Sy11Error
    p = lambda v: C.c_void_p(v.data_ptr())                                    # noqa: E731
    keep = []

    def table(host):
        t = torch.from_numpy(host.view(np.uint8).copy()).to(DEV)
        keep.extend((host, t))
        return [host.shape[0], C.c_void_p(host.ctypes.data), p(t)]

    def one(**kw):
        s = fr.copy()
        for key, v in kw.items():
            s[key][1] = v
        return s
    fr = _table(2, sym_off=[1, 50], T=[20, 14], order=[2, 4], q=[1, 3], tail=[1, 0], row=[0, 1], scale=[32.0, 16.0])
    sym = torch.from_numpy(np.random.default_rng(1).standard_normal(200).astype(np.float32).view(np.complex64)).to(DEV)
    assert sym.shape[0] == 100
    soft = torch.full((2, 40), 99, dtype=torch.int8, device=DEV)
    bits = torch.full((2, 3), 0xA5, dtype=torch.uint8, device=DEV)
    out = torch.full((2, 2), -7, dtype=torch.int32, device=DEV)
    data = torch.full((2, 2), 0xA5, dtype=torch.uint8, device=DEV)
    rows = torch.full((2, 5), -7, dtype=torch.int32, device=DEV)
    crc8 = R.CRCS["crc8"]
    # the table itself is good: the same calls on copies go through
    ops.fec_soft(sym, fr, soft.clone())
    ops.fec_viterbi(soft.clone(), fr, R.POLYS, bits.clone(), out.clone())
    ops.fec_check(soft.clone(), bits.clone(), fr, R.POLYS, 14, data.clone(), rows.clone(), crc=crc8)
    entry = ((dict(order=3), "order"), (dict(order=0), "order"), (dict(q=4), "rotation"), (dict(q=-1), "rotation"), (dict(tail=2), "tail"), (dict(T=0), "trellis steps"),
             (dict(T=8193), "trellis steps"), (dict(row=2), "writes row"), (dict(row=-1), "writes row"), (dict(row=0), "writes row"))
    e1 = entry + ((dict(sym_off=-1), "packed symbols"), (dict(sym_off=87), "packed symbols"), (dict(T=21), "steps leave"), (dict(scale=0.0), "scale"),
                  (dict(scale=float("nan")), "scale"), (dict(scale=float("inf")), "scale"))
    e2 = entry + ((dict(T=21), "steps leave"), (dict(T=6, tail=1), "trellis steps"))
    e3 = entry + ((dict(T=15), "information bits"), (dict(tail=1), "information bits"))

    def lib1(host, period=2, mask=3):
        return table(host) + [period, mask, 100, p(sym), 2, 40, p(soft), None]

    def lib2(host, g=R.POLYS):
        return table(host) + [g[0], g[1], 2, 40, p(soft), 3, p(bits), p(out), None]
    spec8 = _lib.FecCrc(8, 7, 0, 0, 0, 0)

    def lib3(host, spec=spec8):
        return table(host) + [R.POLYS[0], R.POLYS[1], 14, None, C.byref(spec), 2, 40, p(soft), 3, p(bits), 2, p(data), p(rows), None]
    for kw, what in e1:
        with pytest.raises(E_, match="fec_soft: frame [01].*" + what):
            ops.fec_soft(sym, one(**kw), soft)
        with pytest.raises(E_, match="fec_soft: frame [01].*" + what):
            _lib.call("sy11_fec_soft", *lib1(one(**kw)))
    for kw, what in e2:
        with pytest.raises(E_, match="fec_viterbi: frame [01].*" + what):
            ops.fec_viterbi(soft, one(**kw), R.POLYS, bits, out)
        with pytest.raises(E_, match="fec_viterbi: frame [01].*" + what):
            _lib.call("sy11_fec_viterbi", *lib2(one(**kw)))
    for kw, what in e3:
        with pytest.raises(E_, match="fec_check: frame [01].*" + what):
            ops.fec_check(soft, bits, one(**kw), R.POLYS, 14, data, rows, crc=crc8)
        with pytest.raises(E_, match="fec_check: frame [01].*" + what):
            _lib.call("sy11_fec_check", *lib3(one(**kw)))
    # arguments of the calls
    for period, mask in ((0, 3), (3, 3), (66, 3), (2, 0), (2, 4), (6, 64)):
        with pytest.raises(E_):
            ops.fec_soft(sym, fr, soft, period, mask)
        with pytest.raises(E_):
            _lib.call("sy11_fec_soft", *lib1(fr, period, mask))
    for g in ((0o170, 0o133), (0o171, 0o132), (0o71, 0o133), (0o371, 0o133)):
        with pytest.raises(E_, match="generators"):
            ops.fec_viterbi(soft, fr, g, bits, out)
        with pytest.raises(E_, match="generators"):
            _lib.call("sy11_fec_viterbi", *lib2(fr, g))
        with pytest.raises(E_, match="generators"):
            ops.fec_check(soft, bits, fr, g, 14, data, rows)
    for bad in (dict(width=7), dict(width=33), dict(poly=0x107), dict(init=0x100), dict(xorout=0x100), dict(refin=2), dict(refin=1), dict(width=16, poly=0x1021)):
        spec = dict(crc8, **bad)
        with pytest.raises(E_):
            ops.fec_check(soft, bits, fr, R.POLYS, 14, data, rows, crc=spec)
        with pytest.raises(E_):
            _lib.call("sy11_fec_check", *lib3(fr, _lib.FecCrc(spec["width"], spec["poly"], spec["init"], spec["xorout"], int(spec["refin"]), int(spec["refout"]))))
    for pos, v in ((0, 0), (1, None), (2, None), (6, None), (9, None), (5, 0), (5, 63), (7, 0), (7, 1), (8, 38), (8, 39), (6, C.c_void_p(sym.data_ptr() + 4)),
                   (9, C.c_void_p(soft.data_ptr() + 1))):
        a = lib1(fr)
        a[pos] = v
        with pytest.raises(E_):
            _lib.call("sy11_fec_soft", *a)
    for pos, v in ((0, 0), (1, None), (2, None), (7, None), (9, None), (10, None), (5, 0), (5, 1), (6, 38), (6, 39), (8, 2), (8, 0), (7, C.c_void_p(soft.data_ptr() + 1)),
                   (10, C.c_void_p(out.data_ptr() + 2))):
        a = lib2(fr)
        a[pos] = v
        with pytest.raises(E_):
            _lib.call("sy11_fec_viterbi", *a)
    for pos, v in ((0, 0), (1, None), (2, None), (7, None), (10, None), (12, None), (14, None), (15, None), (5, 0), (5, 13), (5, 17), (8, 0), (8, 1), (9, 38), (11, 2), (13, 1),
                   (15, C.c_void_p(rows.data_ptr() + 2))):
        a = lib3(fr)
        a[pos] = v
        with pytest.raises(E_):
            _lib.call("sy11_fec_check", *a)
    for bad in (dict(sym=sym.to(torch.complex128)), dict(sym=sym.cpu()), dict(sym=sym[::2]), dict(soft=soft.to(torch.uint8)), dict(soft=soft[:, :39]), dict(soft=soft[:1]),
                dict(soft=soft.cpu()), dict(frames=fr[:0]), dict(frames=np.zeros((2, 4), dtype=np.int64))):
        a = dict(sym=sym, soft=soft, frames=fr)
        a.update(bad)
        with pytest.raises(E_):
            ops.fec_soft(a["sym"], a["frames"], a["soft"])
    for bad in (dict(soft=soft.to(torch.uint8)), dict(bits=bits[:, :2]), dict(bits=bits[:1]), dict(bits=bits.to(torch.int8)), dict(out=out.to(torch.int64)), dict(out=out[:, :1]),
                dict(out=out.cpu()), dict(frames=fr[:0])):
        a = dict(soft=soft, bits=bits, out=out, frames=fr)
        a.update(bad)
        with pytest.raises(E_):
            ops.fec_viterbi(a["soft"], a["frames"], R.POLYS, a["bits"], a["out"])
    for bad in (dict(data=data[:, :1]), dict(data=data[:1]), dict(rows=rows[:, :4]), dict(rows=rows.to(torch.int64)), dict(n_info=13), dict(n_info=0), dict(n_info=14.0),
                dict(whiten=torch.zeros(13, dtype=torch.uint8, device=DEV)), dict(whiten=torch.zeros(14, dtype=torch.int32, device=DEV)), dict(crc="crc8"), dict(crc=dict(width=8))):
        a = dict(data=data, rows=rows, n_info=14, whiten=None, crc=crc8)
        a.update(bad)
        with pytest.raises(E_):
            ops.fec_check(soft, bits, fr, R.POLYS, a["n_info"], a["data"], a["rows"], whiten=a["whiten"], crc=a["crc"])
    torch.cuda.synchronize()
    assert bool((soft == 99).all()) and bool((bits == 0xA5).all()) and bool((out == -7).all()) and bool((data == 0xA5).all()) and bool((rows == -7).all())


# ------------------------------------------------------------------------------------------------------------- end to end
def _extraction(clips, D, fs=R.FS, fc=FC):
    """A real ``Extraction`` around the given clips (numpy complex64), packed one after the other."""
    from sy11.data.extract import Extraction, ExtractPlan
    n = len(clips)
    D = np.asarray(D, dtype=np.int64)
    M = np.array([len(c) for c in clips], dtype=np.int64)
    plan = ExtractPlan(int(M.sum()) * 64, fs, fc, np.arange(n, dtype=np.int64), np.zeros((n, 4)), D, np.zeros(n, dtype=np.int64), 1000 * np.arange(n, dtype=np.int64), M)
    packed = torch.from_numpy(np.concatenate(clips) if clips else np.zeros(0, dtype=np.complex64)).to(DEV)
    return Extraction(plan, packed, cls=np.arange(n) % 2, conf=np.linspace(0.5, 0.9, n), names={0: "a", 1: "b"})


@pytest.fixture(scope="module")
def chain():
    """``demodulate`` -> ``find_frames`` -> ``decode`` of the three shared clips, once; next to each clip its first 1 500 samples as a second clip, in which the second
    frame is cut short by the clip's end.  Shared and left unchanged."""
    from sy11 import _lib
    from sy11.engine.model import YOLO
    y = YOLO.__new__(YOLO)
    y.device = DEV
    out = []
    for c in R.case_clips():
        cut = int((c["at"][1] + 32 + c["n_need"] // 2) * c["sps"])
        ext = _extraction([c["x"], c["x"][:cut].copy()], [1, 1])
        d = y.demodulate(ext, symbol_rate=[c["rate"]] * 2, offset=[c["offset"]] * 2, order=[c["order"]] * 2, span=R.SPAN)
        f = y.find_frames(d, [list(c["bits"])], payload=c["n_need"], threshold=R.THRESHOLD)
        _lib.PROFILE = []
        try:
            dec = y.decode(f, d, n_info=c["n_info"], puncture=c["pattern"], crc=R.CRC)
            calls = [k[0] for k in _lib.PROFILE]
        finally:
            _lib.PROFILE = None
        assert calls == ["sy11_fec_soft", "sy11_fec_viterbi", "sy11_fec_check"]     # three launches, whatever the number of frames
        out.append((c, ext, d, f, dec))
    return y, out


def test_demodulate_find_frames_decode_reads_what_was_sent(chain):
    from sy11.data.decode import Decoded
    y, cases = chain
    for c, ext, d, f, dec in cases:
        assert isinstance(dec, Decoded) and len(dec) == len(f) >= 4 and d.valid.all()
        assert dec.cls.tolist() == ext.cls.tolist() and dec.names == ext.names and dec.data.device.type == "cuda" and dec.data.shape == (len(f), (c["n_info"] + 7) // 8)
        assert np.array_equal(dec.clip, f.clip) and np.array_equal(dec.word, f.word) and np.array_equal(dec.position, f.position)
        data = dec.data.cpu().numpy()
        sent_ok = 0
        for k in range(len(f)):
            i, p, q = int(f.clip[k]), int(f.position[k]), int(f.rotation[k])
            r = d.symbols[i].cpu().numpy()
            if int(f.n_payload[k]) < c["n_need"]:
                assert not dec.valid[k] and dec.reason[k] == "short" and not data[k].any() and not dec.soft(k).any().item() and np.isnan(dec.ber[k]) and not dec.crc_ok[k]
                assert [int(getattr(dec, a)[k]) for a in ("metric", "end_state", "channel_errors", "n_channel", "crc_calc", "crc_recv")] == [0] * 6
                continue
            # the reference on the device's own symbols, gain and hit: every column, exactly
            soft = R.soft(r[p + 32:p + 32 + c["n_need"]], c["order"], q, R.scale_of(32.0, d.gain[i], c["order"]), c["pattern"], c["T"])
            want = R.decode(soft, c["n_info"], R.POLYS, True, None, R.CRCS[R.CRC])
            assert dec.valid[k] and dec.reason[k] == "" and np.array_equal(dec.soft(k).cpu().numpy(), soft) and dec.soft(k).dtype == torch.int8
            assert np.array_equal(data[k], want["data"]) and np.array_equal(dec.bits(k), want["v"]) and dec.bits(k).dtype == np.uint8
            assert (int(dec.metric[k]), int(dec.end_state[k]), int(dec.channel_errors[k]), int(dec.n_channel[k])) == (want["metric"], 0, want["channel_errors"], want["n_channel"])
            assert (int(dec.crc_calc[k]), int(dec.crc_recv[k]), bool(dec.crc_ok[k])) == (want["crc_calc"], want["crc_recv"], bool(want["crc_ok"]))
            assert dec.ber[k] == want["channel_errors"] / want["n_channel"] and dec[k]["metric"] == want["metric"] and dec[k]["reason"] == ""
        # the frames at the embedded positions of the whole clip decode to what was sent
        m0 = F.stream_index(d.raw["T0"][0], d.raw["STEP"][0], d.raw["i_first"][0], c["sps"], c["u0"], R.SPAN)
        errs = []
        for j, at in enumerate(c["at"]):
            k = np.flatnonzero((f.clip == 0) & (f.position == at - m0))
            assert k.shape[0] == 1
            k = int(k[0])
            assert dec.valid[k] and dec.crc_ok[k] and np.array_equal(dec.bits(k), c["info"][j]) and dec.message(k) == np.packbits(c["u"][j]).tobytes()
            errs.append(int(dec.channel_errors[k]))
            sent_ok += 1
        short = np.flatnonzero((f.clip == 1) & ~dec.valid)
        assert sent_ok == 2 and max(errs) > 0 and short.shape[0] >= 1 and set(dec.reason[short].tolist()) == {"short"}
        first = np.flatnonzero((f.clip == 1) & dec.valid & dec.crc_ok)
        assert first.shape[0] >= 1 and dec.message(int(first[0])) == np.packbits(c["u"][0]).tobytes()          # the whole first frame of the cut clip
        print(f"decode[{c['label']}]: {len(f)} frames, {int(dec.valid.sum())} decoded, {int((dec.valid & dec.crc_ok).sum())} with a good check; channel errors of the embedded "
              f"frames {errs}")


def test_save_round_trip_message_bits_empty_and_invalid_frames(chain, tmp_path):
    from sy11 import _lib
    from sy11.engine.predictor import DetectionPredictor
    y, cases = chain
    c, ext, d, f, dec = cases[2]
    out = dec.save(tmp_path / "d")
    z = np.load(tmp_path / "d" / "decode.npz")
    index = json.loads((tmp_path / "d" / "decode.json").read_text())
    assert out == str(tmp_path / "d")
    for key in dec.COLUMNS:
        assert np.array_equal(z[key], getattr(dec, key), equal_nan=True), key
    assert np.array_equal(z["data"], dec.data.cpu().numpy()) and z["reason"].tolist() == [str(r) for r in dec.reason]
    assert index["n_info"] == c["n_info"] and index["puncture"] == list(R.P64) and index["crc"]["name"] == R.CRC and index["polys"] == list(R.POLYS) and len(index["frames"]) == len(dec)
    k = int(np.flatnonzero(dec.valid & dec.crc_ok)[0])
    assert index["frames"][k]["message"] == dec.message(k).hex() and index["frames"][k]["crc_ok"] is True and index["frames"][k]["name"] in ("a", "b")
    # without a check field the message is every bit; 311 bits are no whole bytes
    pred = DetectionPredictor.__new__(DetectionPredictor)
    pred.device = DEV
    plain = pred.decode(f, d, n_info=c["n_info"], puncture=c["pattern"])
    assert plain.crc_ok[plain.valid].all() and not plain.crc_calc.any() and np.array_equal(plain.data.cpu().numpy(), dec.data.cpu().numpy())
    assert plain.message(k) == np.packbits(dec.bits(k)).tobytes()
    odd = pred.decode(f, d, n_info=c["n_info"] - 1, puncture=c["pattern"], tail=False)
    assert isinstance(odd.message(k), np.ndarray) and odd.message(k).shape == (c["n_info"] - 1,) and np.array_equal(odd.message(k), odd.bits(k))
    # argument errors come before the device; an empty Frames, or one without a valid frame, launches nothing
    none = y.find_frames(d, [[0, 1] * 40], payload=c["n_need"], threshold=0.9)
    _lib.PROFILE = []
    try:
        with pytest.raises(ValueError, match="soft_scale"):
            y.decode(f, d, n_info=c["n_info"], soft_scale=0.0)
        with pytest.raises(ValueError, match="not found in this demodulation"):
            y.decode(f, cases[1][2], n_info=c["n_info"])
        with pytest.raises(ValueError, match="could be decoded"):
            y.decode(f, d, n_info=c["n_info"], crc=R.CRC)                      # unpunctured, the code needs more symbols than were read
        e = y.decode(none, d, n_info=c["n_info"], puncture=c["pattern"], crc=R.CRC)
        deaf = copy.copy(d)
        deaf.gain = np.zeros_like(d.gain)
        g = y.decode(f, deaf, n_info=c["n_info"], puncture=c["pattern"], crc=R.CRC)
        calls = [k[0] for k in _lib.PROFILE]
    finally:
        _lib.PROFILE = None
    assert calls == [] and len(none) == 0 and len(e) == 0 and e.data.shape == (0, (c["n_info"] + 7) // 8) and e.valid.shape == (0,) and e.raw["soft"] is None
    assert len(g) == len(f) and not g.valid.any() and set(g.reason.tolist()) <= {"gain", "short"} and "gain" in g.reason.tolist() and not g.data.any().item()
    assert not g.soft(0).any().item() and g.soft(0).shape == (2 * c["T"],)
