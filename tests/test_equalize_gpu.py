"""GPU: the equaliser's kernels (sy11_eq_solve, sy11_eq_apply) against tests/_eq_ref.py.  The taps are compared within the worst-case rounding bound of a Cholesky
solve of accumulated sums, 8 (Lt + N^2) cond(R) 2^-53 relative in the 2-norm; the rows against the reference evaluated with the device's own taps; the applied
symbols and their decisions, given the device's taps, with ``np.array_equal``.  One call over all frames, one call per frame and a permuted packing give the same
bytes; every refusal is raised by ``ops`` and by the library with the sentinel-filled outputs untouched; and ``demodulate`` -> ``find_frames`` -> ``equalize`` -> ``decode`` reads
two clips behind a two-path channel with fewer channel errors than without the equaliser, in exactly four launches."""
import copy
import ctypes as C
import json

import numpy as np
import pytest
import torch

from tests import _eq_ref as E
from tests import _fec_ref as R
from tests import _frames_ref as F
from tests._demod_ref import point

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FC = 2.4e9
REG = 1e-3
H = ([1.0], [1.0, 0.5 * np.exp(0.7j)], [1.0, 0.45 * np.exp(2.0j), 0.2 * np.exp(-1.0j)], [0.3 * np.exp(1.0j), 1.0, 0.35 * np.exp(-2.0j)])


def _frame_table(rows, **cols):
    from sy11.data.equalize import EQFRAME
    fr = np.zeros(rows, dtype=EQFRAME)
    for k, v in cols.items():
        fr[k] = v
    return fr


def _segment_table(rows, **cols):
    from sy11.data.equalize import EQSEGMENT
    sg = np.zeros(rows, dtype=EQSEGMENT)
    for k, v in cols.items():
        sg[k] = v
    return sg


def _items(segments, T=256):
    from sy11.data.equalize import EQITEM
    tiles = [(s, t) for s in range(segments.shape[0]) for t in range(-(-int(segments["end"][s] - segments["start"][s]) // T))]
    it = np.zeros(len(tiles), dtype=EQITEM)
    it["seg"], it["tile"] = [a for a, _ in tiles], [b for _, b in tiles]
    return it


# ------------------------------------------------------------------------------------------------------------- launch 1
def solve_case(N, seed=7):
    """64 frames for ``N`` taps, one clip each, packed one after the other: the orders alternate, the rotations run over all ``order`` of them, L over (2 N, 33, 256), the
    channels over ``H``, the gains over 0.5 .. 3; every fourth frame starts at p = 0, every fourth (another) ends on its clip's last symbol, so that the zero halo is
    read on both sides; frames 5, 26 and 47 train on 4096, 1000 and L + 1 symbols through the decisions, taken of the symbols as received: some of them are wrong.
    -> dict: sym (packed complex64), dec (packed uint8), words (packed uint8), frames (list of dicts: off, n, p, L, Lt, order, q, A, word_off)."""
    g = np.random.default_rng(seed)
    long = {5: 4096, 26: 1000, 47: None}
    clips, decs, words, frames, off, woff = [], [], [], [], 0, 0
    for k in range(64):
        order = (2, 4)[k % 2]
        q = (k // 2) % order
        L = (2 * N, 33, 256)[k % 3]
        Lt = (long[k] or L + 1) if k in long else L
        A = float(g.uniform(0.5, 3.0))
        p = 0 if k % 4 == 0 else int(g.integers(1, 20))
        tail = 0 if k % 4 == 2 else int(g.integers(1, 20))
        n = p + Lt + tail
        for draw in range(400):                                               # the first draw whose cond(R) is at most 2 Lt (see the test's docstring)
            d = g.integers(0, order, n).astype(np.uint8)
            x = E.channel(point(d, order), H[k % 4], float(g.uniform(10.0, 30.0)), 1000 * (1000 * N + k) + draw).astype(np.complex128)
            r = (A * np.exp(2j * np.pi * q / order) * x).astype(np.complex64)
            if np.linalg.cond(E.solve(r, p, np.zeros(Lt), N, REG)["R"]) <= 2.0 * Lt:
                break
        else:
            raise AssertionError(f"no draw of frame {k} has cond(R) <= {2 * Lt}")
        seen = F.decide(r, order)                                             # a first pass's decisions stand in: as received, of which some are wrong
        clips.append(r), decs.append(seen), words.append(d[p:p + L])
        frames.append(dict(off=off, n=n, p=p, L=L, Lt=Lt, order=order, q=q, A=A, word_off=woff))
        off, woff = off + n, woff + L
    return {"sym": np.concatenate(clips), "dec": np.concatenate(decs), "words": np.concatenate(words), "frames": frames}


def solve_targets(case, f):
    """The targets of frame ``f`` of ``solve_case``: the word turned forward, then the points of the packed decisions as they stand."""
    w = case["words"][f["word_off"]:f["word_off"] + f["L"]]
    t = E.target(w, f["order"], f["q"], f["A"])
    if f["Lt"] > f["L"]:
        t = np.concatenate((t, f["A"] * point(case["dec"][f["off"] + f["p"] + f["L"]:f["off"] + f["p"] + f["Lt"]], f["order"])))
    return t


def _solve_table(case, rows=None):
    fs = case["frames"]
    return _frame_table(len(fs), sym_off=[f["off"] for f in fs], n_sym=[f["n"] for f in fs], word_off=[f["word_off"] for f in fs], p=[f["p"] for f in fs],
                        L=[f["L"] for f in fs], Lt=[f["Lt"] for f in fs], order=[f["order"] for f in fs], q=[f["q"] for f in fs],
                        row=np.arange(len(fs)) if rows is None else rows, gain=[f["A"] for f in fs])


@pytest.mark.parametrize("N", [3, 5, 15])
def test_solve_64_frames_within_the_rounding_bound_of_the_reference(N):
    """The inputs are chosen, per frame, as the first seeded draw with cond(R) <= 2 Lt (asserted below, next to cond(R) <= 10^4).  The bar of the taps carries cond(R);
    the bar of the rows, Lt 2^-50 relative, does not, and the smallest pivot moves by about 0.4 cond(R) 2^-53 relative when R is summed in another order (a numpy
    emulation of the kernel's order of operations on a 6-symbol BPSK frame with cond(R) = 308 was 2.6 bars off the matrix-product reference, the two mse columns
    0.05 bars): with cond(R) <= 2 Lt the pivot has a tenth of its bar to spend.  Seen on the MI355X: |w - w_ref| at most 0.0131 (3 taps), 0.0054 (5) and 0.0034 (15) of
    its bar; the rows at most 0.159, 0.145 and 0.097 of theirs, the pivot the largest."""
    from sy11 import ops
    case = solve_case(N)
    fs = case["frames"]
    assert {f["p"] for f in fs} >= {0} and any(f["p"] + f["Lt"] == f["n"] for f in fs) and {f["Lt"] for f in fs} >= {4096, 1000, 2 * N, 33, 256}
    assert {(f["order"], f["q"]) for f in fs} == {(2, 0), (2, 1), (4, 0), (4, 1), (4, 2), (4, 3)}
    n = len(fs)
    perm = np.random.default_rng(3).permutation(n)                              # the rows in another order than the frames
    sym, dec, words = (torch.from_numpy(case[k]).to(DEV) for k in ("sym", "dec", "words"))
    w = torch.full((n, 15), 7.0 + 7.0j, dtype=torch.complex128, device=DEV)
    rows = torch.full((n, 4), -7.0, dtype=torch.float64, device=DEV)
    ops.eq_solve(sym, _solve_table(case, perm), words, N, REG, w, rows, decisions=dec)
    w, rows = w.cpu().numpy(), rows.cpu().numpy()
    worst_w = worst_row = 0.0
    for k, f in enumerate(fs):
        r = case["sym"][f["off"]:f["off"] + f["n"]]
        t = solve_targets(case, f)
        ref = E.solve(r, f["p"], t, N, REG)
        assert ref["ok"] and ref["cond"] <= min(1e4, 2.0 * f["Lt"]), (k, ref["cond"])
        got = w[perm[k]]
        assert not got[N:].any() and rows[perm[k], 3] == 1.0
        bar = 8.0 * (f["Lt"] + N * N) * ref["cond"] * 2.0 ** -53 * np.linalg.norm(ref["w"])
        err = np.linalg.norm(got[:N] - ref["w"])
        worst_w = max(worst_w, err / bar)
        assert err <= bar, (k, f, err, bar)
        want = (E.mse(r, f["p"], t, f["L"], f["A"]), E.mse(r, f["p"], t, f["L"], f["A"], got[:N]), ref["pivot_min"])
        for a, b in zip(rows[perm[k], :3], want):
            tol = f["Lt"] * 2.0 ** -50 * abs(b)
            worst_row = max(worst_row, abs(a - b) / tol)
            assert abs(a - b) <= tol, (k, f, a, b)
    print(f"eq_solve[{N} taps]: |w - w_ref| at most {worst_w:.4f} of the bar 8 (Lt + N^2) cond 2^-53 |w_ref|; the rows at most {worst_row:.3f} of Lt 2^-50")


def test_solve_one_call_per_frame_and_another_grouping_give_the_same_bytes():
    from sy11 import ops
    case = solve_case(5)
    fs = case["frames"]
    n = len(fs)
    sym, dec, words = (torch.from_numpy(case[k]).to(DEV) for k in ("sym", "dec", "words"))
    tab = _solve_table(case)
    w = torch.zeros((n, 15), dtype=torch.complex128, device=DEV)
    rows = torch.zeros((n, 4), dtype=torch.float64, device=DEV)
    ops.eq_solve(sym, tab, words, 5, REG, w, rows, decisions=dec)
    w1, rows1 = torch.full_like(w, 3.0), torch.full_like(rows, 3.0)
    order = np.random.default_rng(6).permutation(n)
    for k in order[:24]:                                                        # one call per frame
        ops.eq_solve(sym, tab[k:k + 1], words, 5, REG, w1, rows1, decisions=dec)
    ops.eq_solve(sym, tab[order[24:]], words, 5, REG, w1, rows1, decisions=dec)      # the rest in another order
    assert torch.equal(_tbits(w), _tbits(w1)) and torch.equal(rows.view(torch.int64), rows1.view(torch.int64))


def test_singular_frame_passes_its_symbols_through():
    """An all-zero word span with reg = 0: a zero pivot.  The kernel level, then ``equalize`` itself."""
    from sy11 import ops
    from sy11.data.equalize import equalize_frames
    g = np.random.default_rng(4)
    r = g.standard_normal(400).astype(np.float32).view(np.complex64).copy()
    r[20:70] = 0
    sym = torch.from_numpy(r).to(DEV)
    words = torch.zeros(32, dtype=torch.uint8, device=DEV)
    w = torch.full((2, 15), 7.0 + 7.0j, dtype=torch.complex128, device=DEV)
    rows = torch.full((2, 4), -7.0, dtype=torch.float64, device=DEV)
    ops.eq_solve(sym, _frame_table(2, sym_off=0, n_sym=200, word_off=0, p=[30, 100], L=32, Lt=32, order=2, q=0, row=[0, 1], gain=1.0), words, 7, 0.0, w, rows)
    w, rows = w.cpu().numpy(), rows.cpu().numpy()
    assert w[0].tolist() == [0, 0, 0, 1, 0, 0, 0] + [0] * 8 and rows[0, 3] == 0.0 and not rows[0, 2] > 0 and rows[0, 0] == rows[0, 1] == 1.0
    assert rows[1, 3] == 1.0 and rows[1, 2] > 0 and rows[1, 1] < rows[1, 0]
    # through equalize: the frame is listed as singular, its span goes through the unit impulse, which gives back every finite symbol
    f = _fake_frames([200], [2], clip=[0, 0], position=[30, 100], payload=40, word_bits=[0] * 32)
    d = _fake_demod([r[:200]], [2], [1.0])
    eq = equalize_frames(f, d, taps=7, reg=0.0)
    assert eq.frames.valid.tolist() == [False, True] and eq.frames.reason.tolist() == ["singular", ""] and eq.w[0].tolist() == [0, 0, 0, 1, 0, 0, 0]
    assert not eq.frames.pivot_min[0] > 0 and eq.frames.n_train.tolist() == [32, 32]
    e = eq.symbols[0].cpu().numpy()
    assert np.array_equal(e[:100], r[:100]) and not np.array_equal(e[100:172], r[100:172]) and np.array_equal(e[172:].view(np.uint32), r[172:200].view(np.uint32))


# ------------------------------------------------------------------------------------------------------------- launch 2
def _fake_frames(n_symbols, order, clip, position, payload, word_bits, rotation=None, n_payload=None, demod=None):
    """A ``Frames`` stand-in over a real ``FramePlan`` of one word: what ``equalize`` reads of it.  ``demod``: plan on this demodulation's packing, not on the clips one after
    the other."""
    from types import SimpleNamespace

    from sy11.data.frames import plan_frames
    plan = plan_frames((np.asarray(n_symbols), np.asarray(order)) if demod is None else demod, [list(word_bits)], payload, 0.6)
    clip, position = np.asarray(clip, dtype=np.int64), np.asarray(position, dtype=np.int64)
    n_pay = np.minimum(payload, plan.n_symbols[clip] - position - plan.L[clip, 0]) if n_payload is None else np.asarray(n_payload)
    return SimpleNamespace(plan=plan, clip=clip, word=np.zeros_like(clip), position=position, rotation=np.zeros_like(clip) if rotation is None else np.asarray(rotation),
                           n_payload=n_pay, payload=torch.zeros((clip.shape[0], 0), dtype=torch.uint8, device=DEV), rows=None, cls=None, conf=None, names=None)


def _fake_demod(clips, order, gain, perm=None):
    """A ``Demodulation`` stand-in around the clips (numpy complex64), packed in the order ``perm`` (the clips keep their indices)."""
    from types import SimpleNamespace
    n = len(clips)
    perm = list(range(n)) if perm is None else list(perm)
    ns = np.array([len(c) for c in clips], dtype=np.int64)
    start = np.zeros(n, dtype=np.int64)
    at = 0
    for i in perm:
        start[i], at = at, at + ns[i]
    packed = torch.from_numpy(np.concatenate([clips[i] for i in perm])).to(DEV)
    dec = torch.from_numpy(np.concatenate([F.decide(clips[i], order[i]) for i in perm])).to(DEV)
    sym0 = np.concatenate((start, [at]))
    return SimpleNamespace(n_symbols=ns, order=np.asarray(order, dtype=np.int64), gain=np.asarray(gain, dtype=np.float64), valid=np.ones(n, dtype=bool),
                           phase_ambiguity=np.asarray(order, dtype=np.int64), raw={"sym0": sym0, "T0": [0] * n, "STEP": [1 << 32] * n, "i_first": [0] * n},
                           symbols=[packed[int(start[i]):int(start[i] + ns[i])] for i in range(n)], decisions=[dec[int(start[i]):int(start[i] + ns[i])] for i in range(n)],
                           sample_rate=np.ones(n), center_freq=np.zeros(n), rows=None, cls=None, conf=None, names=None)


WORD = tuple(int(b) for b in np.random.default_rng(17).integers(0, 2, 32))


POSITIONS = ([0, 0, 0, 1, 3, 3, 3, 3], [0, 250, 300, 40, 0, 34, 68, 98], [300, 100, 100, 1000, 1, 1, 1, 1])       # clip, position, payload symbols wanted per frame


def apply_case():
    """Four clips and the eight frames of ``POSITIONS`` (a word of 64 bits: 64 symbols at order 2, 32 at order 4).
    0 (order 2, 700 symbols): spans [0, 364), [250, 414) and [300, 464) overlap, so the owners are 0 up to 250, 1 up to 300 and 2 up to 464; the first segment
    ends six symbols short of a tile boundary, nobody owns [464, 700), where a NaN with a payload, infinities, a -0 and a denormal lie.
    1 (order 4, 600): one span [40, 600), cut by the clip's end, across two tile boundaries.  2 (order 2, 90): no frame, and a NaN.
    3 (order 4, 131): spans [0, 33), [34, 67), [68, 101) and [98, 131): symbols 33 and 67 are segments of 1 symbol without an owner, the last span wins from 98 on
    and ends on the clip's last symbol."""
    g = np.random.default_rng(8)
    ns, order = [700, 600, 90, 131], [2, 4, 2, 4]
    clips = []
    for i, (n, o) in enumerate(zip(ns, order)):
        d = g.integers(0, o, n).astype(np.uint8)
        clips.append((1.3 * E.channel(point(d, o), H[1 + i % 3], 20.0, 300 + i).astype(np.complex128)).astype(np.complex64))
    odd = np.array([0x7FC12345, 0xFFC00001, 0x7F800000, 0x80000000, 0x00000001, 0xFF800000], dtype=np.uint32)
    clips[0].view(np.uint32)[1000:1006] = odd                                # symbols 500 .. 502, the planes as they are
    clips[0].view(np.uint32)[1011] = odd[0]
    clips[2].view(np.uint32)[14] = odd[1]
    return ns, order, clips


def apply_frames(ns, order, demod=None):
    clip, position, want = (np.array(v) for v in POSITIONS)
    L = np.where(np.array(order)[clip] == 2, 64, 32)
    return _fake_frames(ns, order, clip, position, 1000, WORD * 2, n_payload=np.minimum(want, np.array(ns)[clip] - position - L), demod=demod)


def _apply_reference(ns, order, clips, f, W, valid):
    out = []
    for i, r in enumerate(clips):
        ks = [k for k in range(len(f.clip)) if f.clip[k] == i]
        owner = E.owners(ns[i], [(int(f.position[k]), int(f.plan.L[i, 0] + f.n_payload[k]), bool(valid[k])) for k in ks])
        e = E.apply(r, owner, [W[k] for k in ks])
        out.append((e, F.decide(e, order[i]), owner))
    return out


def _tbits(x):
    """A complex device tensor as the integers of its planes."""
    v = torch.view_as_real(x)
    return v.view(torch.int32 if v.dtype == torch.float32 else torch.int64)


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def test_apply_equals_the_reference_bit_for_bit_on_every_kind_of_segment():
    from sy11.data.equalize import equalize_frames
    ns, order, clips = apply_case()
    f = apply_frames(ns, order)
    results = {}
    for taps in (3, 7, 15):
        d = _fake_demod(clips, order, [1.3] * 4)
        eq = equalize_frames(f, d, taps=taps)
        valid = eq.frames.valid
        assert valid.all() and eq.frames.n_train.tolist() == [64, 64, 64, 32, 32, 32, 32, 32]
        want = _apply_reference(ns, order, clips, f, eq.w, valid)
        kinds = set()
        for i, (e, dd, owner) in enumerate(want):
            got, gd = eq.symbols[i].cpu().numpy(), eq.decisions[i].cpu().numpy()
            assert np.array_equal(_bits(got), _bits(e)), (taps, i, np.flatnonzero(_bits(got).reshape(-1, 2) != _bits(e).reshape(-1, 2))[:8])
            assert np.array_equal(gd, dd) and gd.dtype == np.uint8
            free = owner < 0
            assert np.array_equal(_bits(got[free]), _bits(clips[i][free]))      # bit for bit where nobody owns the symbol
            kinds |= {(b - a) for a, b, _ in E.segments(owner)}
        assert 1 in kinds and max(kinds) > 512                                  # segments of one symbol; one across two tile boundaries
        assert (want[0][2][500:506] == -1).all() and np.isnan(eq.symbols[0].cpu().numpy()[500].real)
        assert (want[0][2][250:300] == 1).all() and (want[0][2][300:464] == 2).all() and (want[0][2][0:250] == 0).all() and (want[0][2][464:] == -1).all()
        assert (want[2][2] == -1).all() and (want[1][2][40:] == 0).all() and (want[1][2][:40] == -1).all() and np.flatnonzero(want[3][2] == -1).tolist() == [33, 67]
        assert (want[3][2][68:98] == 2).all() and (want[3][2][98:] == 3).all()
        results[taps] = eq
        # a permuted packing of the clips: the same bytes per clip, the same taps
        other = _fake_demod(clips, order, [1.3] * 4, perm=[2, 0, 3, 1])
        with pytest.raises(ValueError, match="lie elsewhere"):
            equalize_frames(f, other, taps=taps)
        again = equalize_frames(apply_frames(ns, order, other), other, taps=taps)
        assert again.raw["sym0"].tolist() == [90, 921, 0, 790, 1521]
        assert np.array_equal(again.w.view(np.float64).view(np.int64), eq.w.view(np.float64).view(np.int64))
        for i in range(4):
            assert torch.equal(_tbits(again.symbols[i]), _tbits(eq.symbols[i])) and torch.equal(again.decisions[i], eq.decisions[i])
    assert not np.array_equal(results[3].symbols[1].cpu().numpy(), results[7].symbols[1].cpu().numpy())


def test_apply_one_call_per_segment_gives_the_same_bytes():
    from sy11 import ops
    from sy11.data.equalize import equalize_frames
    ns, order, clips = apply_case()
    f = apply_frames(ns, order)
    d = _fake_demod(clips, order, [1.3] * 4)
    eq = equalize_frames(f, d, taps=7)
    sym = torch.from_numpy(np.concatenate(clips)).to(DEV)
    out, dec = torch.full_like(sym, 9.0), torch.full((sym.shape[0],), 9, dtype=torch.uint8, device=DEV)
    sg = eq.plan.segments
    for s in np.random.default_rng(2).permutation(sg.shape[0]):
        one = sg[s:s + 1]
        its = _items(one)
        for j in range(its.shape[0] - 1, -1, -1):                               # a call per tile, the last tile first
            ops.eq_apply(sym, its[j:j + 1], one, 7, eq.raw["w"], out, dec)
    assert torch.equal(_tbits(out), _tbits(eq.raw["symbols"])) and torch.equal(dec, eq.raw["decisions"])


# ------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_raise_and_write_nothing():
    from sy11 import _lib, ops
    p = lambda v: C.c_void_p(v.data_ptr())                                    # noqa: E731
    keep = []

    def table(host):
        t = torch.from_numpy(host.view(np.uint8).copy()).to(DEV)
        keep.extend((host, t))
        return [host.shape[0], C.c_void_p(host.ctypes.data), p(t)]

    def one(base, **kw):
        s = base.copy()
        for key, v in kw.items():
            s[key][1] = v
        return s
    fr = _frame_table(2, sym_off=[0, 100], n_sym=[100, 100], word_off=[0, 32], p=[10, 0], L=[32, 16], Lt=[32, 40], order=[2, 4], q=[1, 3], row=[0, 1], gain=[1.0, 2.0])
    sg = _segment_table(3, sym_off=[0, 0, 100], n_sym=100, start=[0, 10, 0], end=[10, 100, 100], frame=[-1, 0, 1], order=[2, 2, 4])
    it = _items(sg)
    sym = torch.from_numpy(np.random.default_rng(1).standard_normal(400).astype(np.float32).view(np.complex64)).to(DEV)
    assert sym.shape[0] == 200
    words = torch.zeros(48, dtype=torch.uint8, device=DEV)
    dec_in = torch.zeros(200, dtype=torch.uint8, device=DEV)
    w = torch.full((2, 15), 7.0 + 7.0j, dtype=torch.complex128, device=DEV)
    rows = torch.full((2, 4), -7.0, dtype=torch.float64, device=DEV)
    out = torch.full((200,), 9.0 + 9.0j, dtype=torch.complex64, device=DEV)
    dec = torch.full((200,), 9, dtype=torch.uint8, device=DEV)
    # the tables themselves are good: the same calls on copies go through
    wc = w.clone()
    ops.eq_solve(sym, fr, words, 7, REG, wc, rows.clone(), decisions=dec_in)
    ops.eq_apply(sym, it, sg, 7, wc, out.clone(), dec.clone())
    e1 = ((dict(order=3), "order"), (dict(order=0), "order"), (dict(q=4), "rotation"), (dict(q=-1), "rotation"), (dict(sym_off=101), "packed symbols"), (dict(sym_off=-1), "packed symbols"),
          (dict(n_sym=0), "packed symbols"), (dict(L=0), "training symbols"), (dict(L=257, Lt=257), "training symbols"), (dict(Lt=15), "training symbols"),
          (dict(Lt=4097), "training symbols"), (dict(word_off=33), "word symbols"), (dict(word_off=-1), "word symbols"), (dict(p=-1), "end after"), (dict(p=61), "end after"),
          (dict(gain=0.0), "gain"), (dict(gain=float("nan")), "gain"), (dict(gain=float("inf")), "gain"), (dict(gain=-1.0), "gain"), (dict(row=2), "writes row"),
          (dict(row=-1), "writes row"), (dict(row=0), "writes row"))

    def lib1(host, taps=7, reg=REG, d=dec_in):
        return table(host) + [taps, reg, 48, p(words), 200, p(sym), None if d is None else p(d), 2, p(w), p(rows), None]
    for kw, what in e1:
        with pytest.raises(ValueError, match="eq_solve: frame [01].*" + what):
            ops.eq_solve(sym, one(fr, **kw), words, 7, REG, w, rows, decisions=dec_in)
        with pytest.raises(_lib.Sy11Error, match="eq_solve: frame [01].*" + what):
            _lib.call("sy11_eq_solve", *lib1(one(fr, **kw)))
    with pytest.raises(ValueError, match="decisions are null"):
        ops.eq_solve(sym, fr, words, 7, REG, w, rows)
    with pytest.raises(_lib.Sy11Error, match="decisions are null"):
        _lib.call("sy11_eq_solve", *lib1(fr, d=None))
    for taps in (2, 4, 1, 17, 16, 7.0, None):
        with pytest.raises(ValueError, match="taps"):
            ops.eq_solve(sym, fr, words, taps, REG, w, rows, decisions=dec_in)
        with pytest.raises(ValueError, match="taps"):
            ops.eq_apply(sym, it, sg, taps, w, out, dec)
        if isinstance(taps, int):
            with pytest.raises(_lib.Sy11Error, match="taps"):
                _lib.call("sy11_eq_solve", *lib1(fr, taps=taps))
    for reg in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="reg"):
            ops.eq_solve(sym, fr, words, 7, reg, w, rows, decisions=dec_in)
        with pytest.raises(_lib.Sy11Error, match="reg"):
            _lib.call("sy11_eq_solve", *lib1(fr, reg=reg))
    for pos, v in ((0, 0), (1, None), (2, None), (6, None), (8, None), (11, None), (12, None), (5, 0), (7, 0), (10, 0), (8, C.c_void_p(sym.data_ptr() + 4)),
                   (11, C.c_void_p(w.data_ptr() + 4)), (12, C.c_void_p(rows.data_ptr() + 4))):
        a = lib1(fr)
        a[pos] = v
        with pytest.raises(_lib.Sy11Error):
            _lib.call("sy11_eq_solve", *a)
    for bad in (dict(sym=sym.to(torch.complex128)), dict(sym=sym.cpu()), dict(sym=sym[::2]), dict(words=words.to(torch.int8)), dict(words=words[:0]), dict(w=w[:, :14]),
                dict(w=w.to(torch.complex64)), dict(rows=rows[:1]), dict(rows=rows[:, :3]), dict(rows=rows.to(torch.float32)), dict(decisions=dec_in[:199]),
                dict(decisions=dec_in.to(torch.int8)), dict(frames=fr[:0]), dict(frames=np.zeros((2, 4), dtype=np.int64))):
        a = dict(sym=sym, words=words, w=w, rows=rows, decisions=dec_in, frames=fr)
        a.update(bad)
        with pytest.raises((ValueError, _lib.Sy11Error)):
            ops.eq_solve(a["sym"], a["frames"], a["words"], 7, REG, a["w"], a["rows"], decisions=a["decisions"])
    # launch 2
    e2 = ((1, dict(order=3), "order"), (1, dict(n_sym=201), "packed symbols"), (2, dict(sym_off=101), "packed symbols"), (1, dict(end=101), "inside the clip"),
          (1, dict(end=10), "inside the clip"), (1, dict(start=-1), "inside the clip"), (1, dict(frame=2), "owner"), (1, dict(frame=-2), "owner"), (1, dict(start=9), "which segment"))

    def lib2(seg=sg, item=it, taps=7, o=out):
        return table(item) + table(seg) + [taps, 2, p(w), 200, p(sym), p(o), p(dec), None]
    for k, kw, what in e2:
        bad = sg.copy()
        for key, v in kw.items():
            bad[key][k] = v
        with pytest.raises(ValueError, match="eq_apply: segment [0-2].*" + what):
            ops.eq_apply(sym, it, bad, 7, w, out, dec)
        with pytest.raises(_lib.Sy11Error, match="eq_apply: segment [0-2].*" + what):
            _lib.call("sy11_eq_apply", *lib2(seg=bad))
    for kw, what in ((dict(seg=3), "is not one of the"), (dict(seg=-1), "is not one of the"), (dict(tile=1), "tile"), (dict(tile=-1), "tile"), (dict(seg=0), "which item")):
        with pytest.raises(ValueError, match="eq_apply: item [0-2].*" + what):
            ops.eq_apply(sym, one(it, **kw), sg, 7, w, out, dec)
        with pytest.raises(_lib.Sy11Error, match="eq_apply: item [0-2].*" + what):
            _lib.call("sy11_eq_apply", *lib2(item=one(it, **kw)))
    with pytest.raises(_lib.Sy11Error, match="must not be the symbols"):
        _lib.call("sy11_eq_apply", *lib2(o=sym))
    with pytest.raises(_lib.Sy11Error, match="taps"):
        _lib.call("sy11_eq_apply", *lib2(taps=8))
    for pos, v in ((0, 0), (1, None), (2, None), (3, 0), (4, None), (5, None), (8, None), (10, None), (11, None), (12, None), (7, 0), (9, 0), (11, C.c_void_p(out.data_ptr() + 4))):
        a = lib2()
        a[pos] = v
        with pytest.raises(_lib.Sy11Error):
            _lib.call("sy11_eq_apply", *a)
    for bad in (dict(sym=sym.cpu()), dict(sym=sym[::2]), dict(out=sym), dict(out=out[:199]), dict(out=out.to(torch.complex128)), dict(dec=dec[:199]), dict(dec=dec.to(torch.int8)),
                dict(w=w[:, :14]), dict(w=w.to(torch.complex64)), dict(segments=sg[:0]), dict(items=it[:0]), dict(items=np.zeros(3, dtype=np.int64))):
        a = dict(sym=sym, out=out, dec=dec, w=w, segments=sg, items=it)
        a.update(bad)
        with pytest.raises((ValueError, _lib.Sy11Error)):
            ops.eq_apply(a["sym"], a["items"], a["segments"], 7, a["w"], a["out"], a["dec"])
    torch.cuda.synchronize()
    assert bool((w == 7.0 + 7.0j).all()) and bool((rows == -7.0).all()) and bool((out == 9.0 + 9.0j).all()) and bool((dec == 9).all())


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
    """``demodulate`` -> ``find_frames`` -> ``equalize`` -> ``decode`` of the two clips behind the two-path channel (tests/_eq_ref.py), once; next to each clip its first 1 500 samples as
    a second clip, in which the second frame is cut short by the clip's end.  Shared and left unchanged."""
    from sy11 import _lib
    from sy11.engine.model import YOLO
    y = YOLO.__new__(YOLO)
    y.device = DEV
    out = []
    for c in E.case_clips():
        cut = int((c["at"][1] + 32 + c["n_need"] // 2) * c["sps"])
        ext = _extraction([c["x"], c["x"][:cut].copy()], [1, 1])
        d = y.demodulate(ext, symbol_rate=[c["rate"]] * 2, offset=[c["offset"]] * 2, order=[c["order"]] * 2, span=R.SPAN)
        f = y.find_frames(d, [list(c["bits"])], payload=c["n_need"], threshold=R.THRESHOLD)
        _lib.PROFILE = []
        try:
            eq = y.equalize(f, d, taps=E.TAPS, refine=E.REFINE)
            calls = [k[0] for k in _lib.PROFILE]
        finally:
            _lib.PROFILE = None
        assert calls == ["sy11_eq_solve", "sy11_eq_apply", "sy11_eq_solve", "sy11_eq_apply"]     # four launches, whatever the number of frames and clips
        plain = y.decode(f, d, n_info=c["n_info"], crc=R.CRC)
        dec = y.decode(f, eq, n_info=c["n_info"], crc=R.CRC)
        out.append((c, ext, d, f, eq, plain, dec))
    return y, out


def _embedded(c, d, f):
    """-> the indices in ``f`` of the frames embedded in the whole clip (clip 0)."""
    m0 = F.stream_index(d.raw["T0"][0], d.raw["STEP"][0], d.raw["i_first"][0], c["sps"], c["u0"], R.SPAN)
    out = []
    for at in c["at"]:
        k = np.flatnonzero((f.clip == 0) & (f.position == at - m0))
        assert k.shape[0] == 1, (c["label"], at - m0, f.position[f.clip == 0])
        out.append(int(k[0]))
    return out


def test_demodulate_find_frames_equalize_decode_reads_what_was_sent(chain):
    """The test that fails without the feature.  Seen on the MI355X: channel errors of the embedded frames without -> with the equaliser [4, 5] -> [0, 0] (a) and
    [2, 3] -> [0, 0] (b), as the reference chain counts them; mse over the word 0.23 - 0.26 -> 0.065 - 0.080 (a), 0.68 - 0.73 -> 0.085 - 0.096 (b)."""
    from sy11.data.equalize import Equalized
    y, cases = chain
    for c, ext, d, f, eq, plain, dec in cases:
        assert isinstance(eq, Equalized) and len(eq) == 2 and len(eq.frames) == len(f) >= 3 and eq.valid.all() and eq.cls.tolist() == ext.cls.tolist() and eq.names == ext.names
        assert np.array_equal(eq.gain, d.gain) and np.array_equal(eq.n_symbols, d.n_symbols) and np.array_equal(eq.order, d.order) and np.array_equal(eq.phase_ambiguity, d.phase_ambiguity)
        assert np.array_equal(eq.raw["sym0"], d.raw["sym0"]) and eq.w.shape == (len(f), E.TAPS) and eq.w.dtype == np.complex128
        base = eq.raw["symbols"]
        for i in range(2):
            assert eq.symbols[i].dtype == torch.complex64 and eq.symbols[i].shape == d.symbols[i].shape and eq.symbols[i].data_ptr() == base.data_ptr() + 8 * int(d.raw["sym0"][i])
            assert eq.decisions[i].dtype == torch.uint8 and eq.decisions[i].shape == d.decisions[i].shape
            assert np.array_equal(eq.decisions[i].cpu().numpy(), F.decide(eq.symbols[i].cpu().numpy(), c["order"]))
        assert eq.frames.valid.all() and (eq.frames.pivot_min > 0).all()
        assert np.array_equal(eq.frames.n_train, np.minimum(E.REFINE, 32 + f.n_payload)) and np.array_equal(eq.frames.clip, f.clip) and np.array_equal(eq.frames.position, f.position)
        emb = _embedded(c, d, f)
        for j, k in enumerate(emb):
            assert eq.frames.mse_after[k] < eq.frames.mse_before[k]
            assert dec.valid[k] and dec.crc_ok[k] and np.array_equal(dec.bits(k), c["info"][j]) and dec.message(k) == np.packbits(c["u"][j]).tobytes()
            assert dec.channel_errors[k] <= plain.channel_errors[k]
        before, after = plain.channel_errors[emb].tolist(), dec.channel_errors[emb].tolist()
        print(f"equalize[{c['label']}]: {len(f)} frames; channel errors of the embedded frames without -> with the equaliser {before} -> {after}; mse "
              f"{np.round(eq.frames.mse_before[emb], 4).tolist()} -> {np.round(eq.frames.mse_after[emb], 4).tolist()}; pivot_min at least {eq.frames.pivot_min.min():.3f}")
        assert sum(after) < sum(before)
        # decode on the device's equalised symbols is the reference decoder on the same symbols, exactly
        for k in range(len(f)):
            i, p, q = int(f.clip[k]), int(f.position[k]), int(f.rotation[k])
            if not dec.valid[k]:
                assert dec.reason[k] == "short"
                continue
            e = eq.symbols[i].cpu().numpy()
            soft = R.soft(e[p + 32:p + 32 + c["n_need"]], c["order"], q, R.scale_of(32.0, d.gain[i], c["order"]), None, c["T"])
            want = R.decode(soft, c["n_info"], R.POLYS, True, None, R.CRCS[R.CRC])
            assert np.array_equal(dec.soft(k).cpu().numpy(), soft) and np.array_equal(dec.bits(k), want["v"])
            assert (int(dec.metric[k]), int(dec.channel_errors[k]), int(dec.n_channel[k]), bool(dec.crc_ok[k])) == (want["metric"], want["channel_errors"], want["n_channel"], bool(want["crc_ok"]))
        # the second pass is the reference's, given the device's taps: the ownership rule and the apply, bit for bit
        for i in range(2):
            ks = [k for k in range(len(f)) if f.clip[k] == i]
            owner = E.owners(int(d.n_symbols[i]), [(int(f.position[k]), int(32 + f.n_payload[k]), True) for k in ks])
            want = E.apply(d.symbols[i].cpu().numpy(), owner, [eq.w[k] for k in ks])
            assert np.array_equal(_bits(eq.symbols[i].cpu().numpy()), _bits(want)) and (owner >= 0).any() and (owner < 0).any()


def test_find_frames_on_the_equalised_symbols_finds_the_same_frames_with_no_smaller_rho(chain):
    y, cases = chain
    for c, ext, d, f, eq, plain, dec in cases:
        again = y.find_frames(eq, [list(c["bits"])], payload=c["n_need"], threshold=R.THRESHOLD)
        for k in _embedded(c, d, f):
            k2 = np.flatnonzero((again.clip == 0) & (again.position == f.position[k]))
            assert k2.shape[0] == 1 and again.rho[int(k2[0])] >= f.rho[k] and again.rotation[int(k2[0])] == f.rotation[k]
        third = y.decode(again, eq, n_info=c["n_info"], crc=R.CRC)             # and the chain goes on from there
        assert int((third.valid & third.crc_ok).sum()) >= 3


def test_save_round_trip_empty_and_invalid_frames(chain, tmp_path):
    from sy11 import _lib
    from sy11.engine.predictor import DetectionPredictor
    y, cases = chain
    c, ext, d, f, eq, plain, dec = cases[0]
    out = eq.save(tmp_path / "e")
    z = np.load(tmp_path / "e" / "equalize.npz")
    index = json.loads((tmp_path / "e" / "equalize.json").read_text())
    assert out == str(tmp_path / "e")
    for key in eq.frames.COLUMNS:
        assert np.array_equal(z[key], getattr(eq.frames, key), equal_nan=True), key
    assert np.array_equal(z["w"], eq.w) and z["reason"].tolist() == [str(r) for r in eq.frames.reason] and np.array_equal(_bits(z["symbols"]), _bits(eq.raw["symbols"].cpu().numpy()))
    assert np.array_equal(z["decisions"], eq.raw["decisions"].cpu().numpy()) and np.array_equal(z["sym0"], d.raw["sym0"]) and np.array_equal(z["gain"], d.gain)
    assert (index["taps"], index["reg"], index["refine"]) == (E.TAPS, 1e-3, E.REFINE) and len(index["frames"]) == len(f) and index["frames"][0]["name"] in ("a", "b")
    assert index["frames"][0]["w"][3] == [eq.w[0, 3].real, eq.w[0, 3].imag] and index["frames"][0]["valid"] is True
    # argument errors come before the device; an empty Frames, or one without a valid frame, launches nothing and gives the demodulation's symbols, copied
    pred = DetectionPredictor.__new__(DetectionPredictor)
    pred.device = DEV
    none = y.find_frames(d, [[0, 1] * 40], payload=10, threshold=0.95)
    _lib.PROFILE = []
    try:
        with pytest.raises(ValueError, match="taps"):
            y.equalize(f, d, taps=8)
        with pytest.raises(ValueError, match="reg"):
            y.equalize(f, d, reg=2.0)
        with pytest.raises(ValueError, match="refine"):
            pred.equalize(f, d, refine=5000)
        with pytest.raises(ValueError, match="not found in this demodulation"):
            y.equalize(f, cases[1][2])
        e = pred.equalize(none, d)
        deaf = copy.copy(d)
        deaf.gain = np.zeros_like(d.gain)
        g = y.equalize(f, deaf, taps=E.TAPS)
        calls = [k[0] for k in _lib.PROFILE]
        one = y.equalize(f, d, taps=3)
        two = [k[0] for k in _lib.PROFILE]
    finally:
        _lib.PROFILE = None
    assert calls == [] and two == ["sy11_eq_solve", "sy11_eq_apply"] and one.frames.valid.all() and one.w.shape == (len(f), 3)
    assert len(none) == 0 and len(e.frames) == 0 and e.w.shape == (0, 7) and e.raw["w"] is None
    for r in (e, g):
        for i in range(2):
            assert torch.equal(_tbits(r.symbols[i]), _tbits(d.symbols[i])) and torch.equal(r.decisions[i], d.decisions[i])
            assert r.symbols[i].data_ptr() != d.symbols[i].data_ptr()
    assert not g.frames.valid.any() and set(g.frames.reason.tolist()) == {"gain"} and np.isnan(g.frames.mse_after).all() and (g.w[:, 3] == 1).all() and not g.w[:, :3].any()


