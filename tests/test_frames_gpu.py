"""GPU: the frame search kernels (sy11_sync_correlate, sy11_sync_peaks, sy11_sync_frames) against tests/_frames_ref.py.  The kernel-level
tests feed synthetic symbol buffers (float32-rounded unit points x gain + seeded noise) to ``ops.sync_*`` directly: rho2, q, hit, the rows and
the packed payload are compared with ``==``, bit for bit — the definition fixes the order of every float64 sum, so no tolerance is due; one
call over all clips, one call per clip and a permuted packing give the same bits; every refusal is raised once by ``ops`` and once by the
library, with the sentinel-filled outputs untouched; and ``demodulate`` -> ``find_frames`` on the four clips of tests/test_frames_cpu.py finds the
embedded frames where the reference alone finds them."""
import ctypes as C
import json
import math

import numpy as np
import pytest
import torch

from tests import _demod_ref as R
from tests import _frames_ref as F

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FC = 2.4e9
T = F.TILE


def _same(a, b):
    """The same float64 values bit for bit (-0 is not 0); a NaN, whose sign and payload the definition leaves open, equals any NaN."""
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.int64), b[~nan].view(np.int64))


def _word(seed, n):
    return np.random.default_rng(seed).integers(0, 2, n).tolist()


def _stream(order, n, seed, q=0, gain=1.0, sigma=0.05, embed=None):
    """``n`` symbols: random decisions with the decision words of ``embed`` ({position: decisions}) written over them, as unit points turned
    forward by ``q`` steps of 2 pi / order, times ``gain``, plus noise -> (complex64, the decisions)."""
    g = np.random.default_rng(seed)
    d = g.integers(0, order, n).astype(np.uint8)
    for j, w in (embed or {}).items():
        assert 0 <= j and j + len(w) <= n
        d[j:j + len(w)] = w
    pts = F.points(d, order) / math.sqrt(order / 2) * np.exp(2j * np.pi * q / order)
    return (gain * pts + sigma * (g.standard_normal(n) + 1j * g.standard_normal(n))).astype(np.complex64), d


def _run(clips, orders, words, threshold=0.8, payload=0):
    """The three launches through ``ops`` on the clips packed in the given order, the outputs pre-filled with sentinels -> dict of host arrays."""
    from sy11 import ops
    from sy11.data.frames import FRAME, plan_frames
    plan = plan_frames((np.array([len(c) for c in clips]), np.array(orders)), words, payload, threshold)
    assert plan.clip_valid.all() and plan.total_positions > 0
    sym = torch.from_numpy(np.concatenate(clips)).to(DEV)
    items = plan.items()[0]
    wbuf = torch.from_numpy(plan.word_buf).to(DEV)
    n_pos = plan.total_positions
    rho2 = torch.full((n_pos,), -7.0, dtype=torch.float64, device=DEV)
    q = torch.full((n_pos,), 7, dtype=torch.uint8, device=DEV)
    hit = torch.full((n_pos,), 7, dtype=torch.uint8, device=DEV)
    ops.sync_correlate(sym, items, wbuf, rho2, q)
    ops.sync_peaks(rho2, items, threshold * threshold, hit, sym.shape[0], wbuf.shape[0])
    out = {"plan": plan, "rho2": rho2.cpu().numpy(), "q": q.cpu().numpy(), "hit": hit.cpu().numpy()}
    at = np.flatnonzero(out["hit"])
    W = len(words)
    pr = np.searchsorted(plan.pos0, at, side="right") - 1
    clip = pr // W
    fr = np.zeros(at.shape[0], dtype=FRAME)
    fr["sym_off"], fr["n_sym"], fr["word_off"], fr["p"] = plan.sym_off[clip], plan.n_symbols[clip], plan.word_off.reshape(-1)[pr], at - plan.pos0[pr]
    fr["L"], fr["order"], fr["q"], fr["payload"], fr["row"] = plan.L.reshape(-1)[pr], plan.order[clip], out["q"][at], payload, np.arange(at.shape[0])
    stride = (payload * 2 + 7) // 8                                           # the rows of an order-2 frame end in zeros
    out.update(frames=fr, pair=pr, stride=stride, rows=np.zeros((0, 3), dtype=np.int32), bits=np.zeros((0, stride), dtype=np.uint8))
    if at.shape[0]:
        rows = torch.full((at.shape[0], 3), -7, dtype=torch.int32, device=DEV)
        bits = torch.full((at.shape[0], stride), 7, dtype=torch.uint8, device=DEV)
        ops.sync_frames(sym, fr, wbuf, rows, bits)
        out.update(rows=rows.cpu().numpy(), bits=bits.cpu().numpy())
    return out


def _pair(out, i, j):
    W = len(out["plan"].words)
    return slice(int(out["plan"].pos0[i * W + j]), int(out["plan"].pos0[i * W + j + 1]))


def _check(out, clips, orders, words, threshold, payload):
    """Every pair of the call against the reference: validity and reason, then rho2, q and hit with ``==``; every hit's row and payload bytes with ``==``.
    -> {(clip, word): the hit positions}."""
    plan, hits, k = out["plan"], {}, 0
    for i, (r, o) in enumerate(zip(clips, orders)):
        for j, b in enumerate(words):
            why = F.pair_reason(len(r), o, len(b))
            assert plan.reason[i, j] == why and bool(plan.valid[i, j]) == (why == "")
            sl = _pair(out, i, j)
            if why:
                assert sl.stop == sl.start
                continue
            w = F.decisions(b, o)
            rho2, q = F.correlate(r, w, o)
            hit = F.peaks(rho2, len(w), threshold * threshold)
            assert sl.stop - sl.start == rho2.shape[0] == len(r) - len(w) + 1
            assert _same(out["rho2"][sl], rho2), (i, j, "rho2")
            assert np.array_equal(out["q"][sl], q), (i, j, "q")
            assert np.array_equal(out["hit"][sl], hit), (i, j, "hit")
            hits[i, j] = np.flatnonzero(hit)
            for p in hits[i, j]:
                e, be, n_pay, row = F.frames(r, w, o, int(p), int(q[p]), payload, out["stride"])
                assert out["pair"][k] == i * len(words) + j and int(out["frames"]["p"][k]) == p
                assert out["rows"][k].tolist() == [e, be, n_pay], (i, j, int(p))
                assert np.array_equal(out["bits"][k], row), (i, j, int(p))
                k += 1
    assert k == out["rows"].shape[0]
    return hits


# ------------------------------------------------------------------------------------------------------------- shapes
# (the two words' bit counts, the word each order's clips are sized by): L = 13, 16 | -, 8;  8, - | -, 256;  26, 256 | 13, 128
SETS = {"13 and 16 bits": ((13, 16), {2: 0, 4: 1}), "8 and 512 bits": ((8, 512), {2: 0, 4: 1}), "26 and 256 bits": ((26, 256), {2: 1, 4: 0})}


def _embedded_at(n, L):
    """Where a clip of ``n`` symbols holds the word of ``L``: across the first tile boundary where it has room, at 0 where that leaves both whole."""
    if T - L // 2 + L > n:
        return [0]
    return ([0] if L <= T - L // 2 else []) + [T - L // 2]


def _shape_clips(name):
    """An odd-length clip first, then per order a clip with P = 1, T - 1, T, T + 1 and 2 T + 3 positions of that order's word, which sits at
    position 0 and, where the clip has room, across the first tile boundary; every clip at its own rotation."""
    n_bits, primary = SETS[name]
    words = [_word(200 + n, n) for n in n_bits]
    clips, orders = [_stream(2, 77, 1)[0]], [2]
    for o in (2, 4):
        w = F.decisions(words[primary[o]], o)
        L = len(w)
        for k, P in enumerate((1, T - 1, T, T + 1, 2 * T + 3)):
            n = P + L - 1
            embed = {p: w for p in _embedded_at(n, L)}
            clips.append(_stream(o, n, 10 * o + k, q=(k + 1) % o, gain=0.5 + 0.25 * k, embed=embed)[0])
            orders.append(o)
    return clips, orders, words, primary


@pytest.mark.parametrize("name", list(SETS))
def test_every_tile_shape_matches_the_reference_bit_for_bit(name):
    clips, orders, words, primary = _shape_clips(name)
    out = _run(clips, orders, words, 0.8, payload=10)
    off = np.concatenate(([0], np.cumsum([len(c) for c in clips])))[:-1]
    assert off[1] % 2 == 1 and (off[1:] % 2 == 1).sum() >= 3                   # clips at odd packed offsets
    reasons = set(out["plan"].reason[np.array(orders) == 4].reshape(-1).tolist())
    assert ("bit count not divisible by log2(order)" in reasons) == any(n % 2 for n in SETS[name][0])
    hits = _check(out, clips, orders, words, 0.8, 10)
    for i, o in enumerate(orders[1:], 1):                                     # the embedded words are found, at their rotation, without an error
        L = len(F.decisions(words[primary[o]], o))
        sl, P = _pair(out, i, primary[o]), len(clips[i]) - L + 1
        assert P in (1, T - 1, T, T + 1, 2 * T + 3)
        want = _embedded_at(len(clips[i]), L)
        assert set(want) <= set(hits[i, primary[o]].tolist())
        k0 = (i - 1) % 5
        assert [int(out["q"][sl][p]) for p in want] == [(k0 + 1) % o] * len(want)
        for p in want:
            k = int(np.flatnonzero((out["pair"] == i * 2 + primary[o]) & (out["frames"]["p"] == p))[0])
            assert out["rows"][k, 0] == 0 and out["rows"][k, 1] == 0 and out["rows"][k, 2] == min(10, len(clips[i]) - p - L)


# ------------------------------------------------------------------------------------------------------------- edge cases
EDGE_WORD = [0, 0, 0, 0, 0, 1, 1, 0, 0, 1, 0, 1, 0, 0, 1, 1]


def _edge_clips():
    """-> (clips, orders, words, notes): one 16-bit word (L = 16 at order 2, 8 at order 4) and
    0  order 2: the word across the tile boundary, at T - 8
    1  order 4: the word across the tile boundary, at T - 4
    2  order 2: the word whole at T - 5, over the head of a copy at T + 3 (its last 8 symbols are left): the first survives
    3  order 2: the word whole at T + 3, over the tail of a copy at T - 5 (its first 8 symbols are left): the second survives
       (the word's autocorrelation at a lag of 8 symbols is 0, so the damaged copy keeps rho = 8 / 16, above the threshold of 0.4)
    4  order 2: the word at N - L - 3: three payload symbols are left of the ten asked for
    5  order 2: a run of 30 zero symbols (E == 0 at 15 positions), the word after it
    6  order 4: a NaN symbol at 100, the word at 60 (untouched by it) and at 101 (next to it)."""
    bits = EDGE_WORD
    w2, w4 = F.decisions(bits, 2), F.decisions(bits, 4)
    c = F.points(w2, 2).real
    assert float(np.sum(c[:8] * c[8:])) == 0.0
    n = 2 * T
    c0 = _stream(2, n, 30, q=1, embed={T - 8: w2})[0]
    c1 = _stream(4, n, 31, q=3, embed={T - 4: w4})[0]
    c2 = _stream(2, n, 32, sigma=0.02, embed={T + 3: w2, T - 5: w2})[0]      # the later entry is written last
    c3 = _stream(2, n, 35, sigma=0.02, embed={T - 5: w2, T + 3: w2})[0]
    c4 = _stream(2, 300, 36, q=1, embed={300 - 16 - 3: w2})[0]
    c5 = _stream(2, 200, 37, embed={90: w2})[0]
    c5[40:70] = 0
    c6 = _stream(4, 200, 38, q=2, embed={60: w4, 101: w4})[0]
    c6[100] = np.nan
    return [c0, c1, c2, c3, c4, c5, c6], [2, 4, 2, 2, 2, 2, 4], [bits]


def test_edges_tile_boundaries_neighbouring_frames_short_payload_zero_run_and_nan():
    clips, orders, words = _edge_clips()
    thr = 0.4
    out = _run(clips, orders, words, thr, payload=10)
    hits = _check(out, clips, orders, words, thr, 10)
    rho2 = [out["rho2"][_pair(out, i, 0)] for i in range(7)]
    assert T - 8 in hits[0, 0] and out["q"][_pair(out, 0, 0)][T - 8] == 1 and rho2[0][T - 8] > 0.9
    assert T - 4 in hits[1, 0] and out["q"][_pair(out, 1, 0)][T - 4] == 3 and rho2[1][T - 4] > 0.9
    # both of the neighbours pass the threshold; the stronger one alone is a hit, whichever side of the boundary it is on
    assert rho2[2][T - 5] > 0.9 and thr * thr <= rho2[2][T + 3] < rho2[2][T - 5] and T - 5 in hits[2, 0] and T + 3 not in hits[2, 0]
    assert rho2[3][T + 3] > 0.9 and thr * thr <= rho2[3][T - 5] < rho2[3][T + 3] and T + 3 in hits[3, 0] and T - 5 not in hits[3, 0]
    k = int(np.flatnonzero((out["pair"] == 4) & (out["frames"]["p"] == 300 - 16 - 3))[0])
    assert out["rows"][k].tolist() == [0, 0, 3] and not out["bits"][k, 1:].any() and out["bits"][k, 0] & 0x1f == 0
    assert (rho2[5][40:55] == 0.0).all() and not out["hit"][_pair(out, 5, 0)][40:55].any() and 90 in hits[5, 0]
    nan = np.isnan(rho2[6])
    assert np.flatnonzero(nan).tolist() == list(range(93, 101)) and not out["hit"][_pair(out, 6, 0)][nan].any()
    assert 60 in hits[6, 0] and 101 in hits[6, 0]                            # the NaN positions next to it do not suppress the frame at 101


def test_equal_peaks_across_a_tile_boundary_the_earliest_wins_at_threshold_one():
    bits = [0, 0, 1, 0] * 4
    d = np.concatenate((np.zeros(T - 6, dtype=np.uint8), np.array([0, 0, 1, 0] * 6, dtype=np.uint8)))
    clips = [F.points(d, 2).astype(np.complex64), (-F.points(d, 2)).astype(np.complex64)]
    out = _run(clips, [2, 2], [bits], 1.0, payload=4)
    hits = _check(out, clips, [2, 2], [bits], 1.0, 4)
    for i in (0, 1):
        rho2 = out["rho2"][_pair(out, i, 0)]
        assert np.flatnonzero(rho2 == 1.0).tolist() == [T - 6, T - 2, T + 2] and hits[i, 0].tolist() == [T - 6]
    assert out["frames"]["q"].tolist() == [0, 1] and out["rows"].tolist() == [[0, 0, 4], [0, 0, 4]] and out["bits"][:, 0].tolist() == [0x20, 0x20]


# ------------------------------------------------------------------------------------------------------------- invariance
def test_one_call_per_clip_and_a_permuted_packing_give_the_same_bits():
    clips, orders, words, _ = _shape_clips("13 and 16 bits")
    whole = _run(clips, orders, words, 0.8, payload=10)
    perm = [7, 2, 10, 0, 5, 9, 1, 8, 3, 6, 4]
    assert sorted(perm) == list(range(len(clips)))
    mixed = _run([clips[i] for i in perm], [orders[i] for i in perm], words, 0.8, payload=10)
    for at, i in enumerate(perm):
        one = _run([clips[i]], [orders[i]], words, 0.8, payload=10)
        for j in range(2):
            a = _pair(whole, i, j)
            for other, k in ((mixed, at), (one, 0)):
                b = _pair(other, k, j)
                assert b.stop - b.start == a.stop - a.start
                assert np.array_equal(other["rho2"][b].view(np.int64), whole["rho2"][a].view(np.int64)) and np.array_equal(other["q"][b], whole["q"][a])
                assert np.array_equal(other["hit"][b], whole["hit"][a])
                ra, rb = whole["pair"] == i * 2 + j, other["pair"] == k * 2 + j
                assert np.array_equal(other["rows"][rb], whole["rows"][ra]) and np.array_equal(other["bits"][rb], whole["bits"][ra])
                assert np.array_equal(other["frames"]["p"][rb], whole["frames"]["p"][ra])


# ------------------------------------------------------------------------------------------------------------- refusals
def _lib_refuses(name, args, pos, v, match=None):
    from sy11 import _lib
    bad = list(args)
    bad[pos] = v
    with pytest.raises(_lib.Sy11Error, match=match):
        _lib.call(name, *bad)


def test_refusals_raise_and_write_nothing():
    from sy11 import _lib, ops
    from sy11.data.frames import FRAME, plan_frames
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
    bits = _word(7, 16)
    clips, orders = [_stream(2, 300, 50, embed={20: F.decisions(bits, 2)})[0], _stream(4, 40, 51, q=1, embed={5: F.decisions(bits, 4)})[0]], [2, 4]
    plan = plan_frames((np.array([300, 40]), np.array(orders)), [bits], 10, 0.8)
    items = plan.items()[0]
    assert items["cnt"].tolist() == [T, 285 - T, 33] and items["L"].tolist() == [16, 16, 8]
    sym, wbuf = torch.from_numpy(np.concatenate(clips)).to(DEV), torch.from_numpy(plan.word_buf).to(DEV)
    n_sym, n_word, n_pos = 340, 24, 285 + 33
    assert (sym.shape[0], wbuf.shape[0], plan.total_positions) == (n_sym, n_word, n_pos)
    rho2 = torch.full((n_pos,), -7.0, dtype=torch.float64, device=DEV)
    q = torch.full((n_pos,), 7, dtype=torch.uint8, device=DEV)
    hit = torch.full((n_pos,), 7, dtype=torch.uint8, device=DEV)
    good = torch.rand(n_pos, dtype=torch.float64, device=DEV)                 # what launch 2 reads in the refused calls
    # ---- launches 1 and 2: the last item is the order-4 clip's, which ends the symbol, the word and the position buffers
    last = one(items, 2)
    assert int(last["sym_off"][0]) + 40 == n_sym and int(last["word_off"][0]) + 8 == n_word and int(last["pos_off"][0]) + 33 == n_pos
    entry = ((dict(sym_off=-1), "packed symbols"), (dict(sym_off=301), "packed symbols"), (dict(n_sym=0), "packed symbols"), (dict(n_sym=41), "packed symbols"),
             (dict(word_off=-1), "word symbols"), (dict(word_off=17), "word symbols"), (dict(L=7), "word of"), (dict(L=257), "word of"), (dict(L=41), "word of"),
             (dict(p0=1, cnt=32), "not a tile"), (dict(cnt=0), "not a tile"), (dict(cnt=32), "not a tile"), (dict(cnt=34), "not a tile"), (dict(p0=T, cnt=1), "not a tile"),
             (dict(p0=-T), "not a tile"), (dict(pos_off=-1), "packed positions"), (dict(pos_off=286), "packed positions"),
             (dict(order=0), "order"), (dict(order=3), "order"), (dict(order=8), "order"))
    short_first = one(items, 0, cnt=T - 1)                                     # a tile that is not the pair's last must be whole
    twice = np.concatenate((one(items, 0), one(items, 1), one(items, 1)))
    overlap = np.concatenate((one(items, 0), one(items, 2, pos_off=T - 1)))
    for kw, what in entry:
        with pytest.raises(E_, match="sync_correlate: item 0.*" + what):
            ops.sync_correlate(sym, one(items, 2, **kw), wbuf, rho2, q)
        with pytest.raises(E_, match="sync_peaks: item 0.*" + what):
            ops.sync_peaks(good, one(items, 2, **kw), 0.64, hit, n_sym, n_word)
    for bad_items, what in ((short_first, "not a tile"), (twice, "writes position"), (overlap, "writes position")):
        with pytest.raises(E_, match=what):
            ops.sync_correlate(sym, bad_items, wbuf, rho2, q)
        with pytest.raises(E_, match=what):
            ops.sync_peaks(good, bad_items, 0.64, hit, n_sym, n_word)
    with pytest.raises(E_, match="packed symbols"):
        ops.sync_correlate(sym[:-1], items, wbuf, rho2, q)                     # the last clip ends one symbol past the buffer
    with pytest.raises(E_, match="word symbols"):
        ops.sync_correlate(sym, items, wbuf[:-1], rho2, q)
    with pytest.raises(E_, match="packed positions"):
        ops.sync_correlate(sym, items, wbuf, rho2[:-1], q[:-1])
    for bad in (dict(sym=sym.to(torch.complex128)), dict(sym=sym[::2]), dict(sym=sym.cpu()), dict(sym=torch.view_as_real(sym)), dict(words=wbuf.to(torch.int32)),
                dict(words=wbuf[:0]), dict(words=wbuf.cpu()), dict(rho2=rho2.float()), dict(rho2=rho2[:0]), dict(rho2=rho2.view(-1, 1)), dict(q=q[:-1]),
                dict(q=q.to(torch.int32)), dict(items=items[:0]), dict(items=np.zeros((2, 7), dtype=np.int64))):
        a = dict(sym=sym, words=wbuf, rho2=rho2, q=q, items=items)
        a.update(bad)
        with pytest.raises(E_):
            ops.sync_correlate(a["sym"], a["items"], a["words"], a["rho2"], a["q"])
    for bad in (dict(rho2=good.float()), dict(rho2=good.cpu()), dict(hit=hit[:-1]), dict(hit=hit.to(torch.int32)), dict(thr=0.0), dict(thr=1.0000001), dict(thr=-0.64),
                dict(thr=float("nan")), dict(thr=None), dict(n_sym=0), dict(n_sym=n_sym - 1), dict(n_word=0), dict(n_word=n_word - 1), dict(items=items[:0])):
        a = dict(rho2=good, hit=hit, thr=0.64, n_sym=n_sym, n_word=n_word, items=items)
        a.update(bad)
        with pytest.raises(E_):
            ops.sync_peaks(a["rho2"], a["items"], a["thr"], a["hit"], a["n_sym"], a["n_word"])

    def lib1(host_items):
        return table(host_items) + [n_word, p(wbuf), n_sym, p(sym), n_pos, p(rho2), p(q), None]

    def lib2(host_items, thr2=0.64):
        return table(host_items) + [n_word, n_sym, n_pos, p(good), thr2, p(hit), None]
    for pos, v in ((0, 0), (1, None), (2, None), (4, None), (6, None), (8, None), (9, None), (3, 0), (3, n_word - 1), (5, 0), (5, n_sym - 1), (7, 0), (7, n_pos - 1),
                   (6, C.c_void_p(sym.data_ptr() + 4)), (8, C.c_void_p(rho2.data_ptr() + 4))):
        _lib_refuses("sy11_sync_correlate", lib1(items), pos, v)
    args = lib1(items)
    _lib_refuses("sy11_sync_correlate", args, 2, C.c_void_p(args[2].value + 4))                             # a misaligned device table
    for pos, v in ((0, 0), (1, None), (2, None), (6, None), (8, None), (3, 0), (3, n_word - 1), (4, 0), (4, n_sym - 1), (5, 0), (5, n_pos - 1), (7, 0.0), (7, 1.0000001),
                   (7, float("nan")), (6, C.c_void_p(good.data_ptr() + 4))):
        _lib_refuses("sy11_sync_peaks", lib2(items), pos, v)
    for kw, what in entry:
        with pytest.raises(E_, match="sync_correlate: item 0.*" + what):
            _lib.call("sy11_sync_correlate", *lib1(one(items, 2, **kw)))
        with pytest.raises(E_, match="sync_peaks: item 0.*" + what):
            _lib.call("sy11_sync_peaks", *lib2(one(items, 2, **kw)))
    for bad_items, what in ((short_first, "not a tile"), (twice, "writes position"), (overlap, "writes position")):
        with pytest.raises(E_, match=what):
            _lib.call("sy11_sync_correlate", *lib1(bad_items))
        with pytest.raises(E_, match=what):
            _lib.call("sy11_sync_peaks", *lib2(bad_items))
    torch.cuda.synchronize()
    assert bool((rho2 == -7.0).all()) and bool((q == 7).all()) and bool((hit == 7).all())                   # no refused call wrote anything
    # ---- launch 3: two frames, the second the order-4 clip's, at the clip's last position
    fr = np.zeros(2, dtype=FRAME)
    fr["sym_off"], fr["n_sym"], fr["word_off"], fr["p"], fr["L"], fr["order"], fr["q"], fr["payload"], fr["row"] = [0, 300], [300, 40], [0, 16], [20, 32], [16, 8], [2, 4], \
        [0, 1], 10, [0, 1]
    rows = torch.full((2, 3), -7, dtype=torch.int32, device=DEV)
    pay = torch.full((2, 3), 7, dtype=torch.uint8, device=DEV)
    g_rows, g_pay = ops.sync_frames(sym, fr, wbuf, torch.zeros_like(rows), torch.zeros_like(pay))           # the table itself is good
    assert g_rows.cpu().tolist() == [[0, 0, 10], [F.frames(clips[1], F.decisions(bits, 4), 4, 32, 1, 10, 3)[0], F.frames(clips[1], F.decisions(bits, 4), 4, 32, 1, 10, 3)[1], 0]]
    entry3 = ((dict(order=0), "order"), (dict(order=3), "order"), (dict(q=4), "rotation"), (dict(q=-1), "rotation"), (dict(order=2, q=2), "rotation"),
              (dict(sym_off=-1), "packed symbols"), (dict(sym_off=301), "packed symbols"), (dict(n_sym=41), "packed symbols"), (dict(L=7), "word of"), (dict(L=257), "word of"),
              (dict(word_off=-1), "word symbols"), (dict(word_off=17), "word symbols"), (dict(p=33), "ends after"), (dict(p=-1), "ends after"),
              (dict(payload=13), "payload symbols"), (dict(payload=2 ** 20), "payload symbols"), (dict(payload=-1), "payload symbols"),
              (dict(row=-1), "writes row"), (dict(row=2), "writes row"))
    for kw, what in entry3:
        with pytest.raises(E_, match="sync_frames: frame 0.*" + what):
            ops.sync_frames(sym, one(fr, 1, **kw), wbuf, rows, pay)
    with pytest.raises(E_, match="a row takes one frame"):
        ops.sync_frames(sym, np.concatenate((one(fr, 0), one(fr, 1, row=0))), wbuf, rows, pay)
    with pytest.raises(E_, match="payload symbols"):
        ops.sync_frames(sym, fr, wbuf, rows, pay[:, :2].contiguous())           # 20 bits need 3 bytes
    for bad in (dict(sym=sym.to(torch.complex128)), dict(sym=sym.cpu()), dict(words=wbuf.to(torch.int32)), dict(words=wbuf[:0]), dict(rows=rows.to(torch.int64)),
                dict(rows=rows[:, :2]), dict(rows=rows[:0]), dict(bits=pay[:1]), dict(bits=pay.to(torch.int32)), dict(bits=pay[:, ::2]), dict(bits=pay.cpu()),
                dict(frames=fr[:0]), dict(frames=np.zeros((2, 7), dtype=np.int64))):
        a = dict(sym=sym, words=wbuf, rows=rows, bits=pay, frames=fr)
        a.update(bad)
        with pytest.raises(E_):
            ops.sync_frames(a["sym"], a["frames"], a["words"], a["rows"], a["bits"])

    def lib3(host_frames):
        return table(host_frames) + [n_word, p(wbuf), n_sym, p(sym), 2, p(rows), 3, p(pay), None]
    for pos, v in ((0, 0), (1, None), (2, None), (4, None), (6, None), (8, None), (10, None), (3, 0), (3, n_word - 1), (5, 0), (5, n_sym - 1), (7, 0), (7, 1), (9, -1),
                   (9, 2), (9, 2 ** 18 + 1), (6, C.c_void_p(sym.data_ptr() + 4)), (8, C.c_void_p(rows.data_ptr() + 2))):
        _lib_refuses("sy11_sync_frames", lib3(fr), pos, v)
    for kw, what in entry3:
        with pytest.raises(E_, match="sync_frames: frame 0.*" + what):
            _lib.call("sy11_sync_frames", *lib3(one(fr, 1, **kw)))
    with pytest.raises(E_, match="an earlier frame"):
        _lib.call("sy11_sync_frames", *lib3(np.concatenate((one(fr, 0), one(fr, 1, row=0)))))
    torch.cuda.synchronize()
    assert bool((rows == -7).all()) and bool((pay == 7).all())


# ------------------------------------------------------------------------------------------------------------- end to end
def _extraction(clips, D, fs=F.FS, fc=FC):
    """A real ``Extraction`` around the given clips (numpy complex64), packed one after the other; clip i starts 1 000 i decimated samples
    into the capture, so that ``t0`` differs from clip to clip."""
    from sy11.data.extract import Extraction, ExtractPlan
    n = len(clips)
    D = np.asarray(D, dtype=np.int64)
    M = np.array([len(c) for c in clips], dtype=np.int64)
    plan = ExtractPlan(int(M.sum()) * 64, fs, fc, np.arange(n, dtype=np.int64), np.zeros((n, 4)), D, np.zeros(n, dtype=np.int64),
                       1000 * np.arange(n, dtype=np.int64), M)
    packed = torch.from_numpy(np.concatenate(clips) if clips else np.zeros(0, dtype=np.complex64)).to(DEV)
    return Extraction(plan, packed, cls=np.arange(n) % 2, conf=np.linspace(0.5, 0.9, n), names={0: "a", 1: "b"})


@pytest.fixture(scope="module")
def chain():
    """``demodulate`` -> ``find_frames`` of the four shared clips with all four words, once; shared and left unchanged."""
    from sy11 import _lib
    from sy11.engine.model import YOLO
    cs = F.case_clips()
    ext = _extraction([c["x"] for c in cs], [c["D"] for c in cs])
    y = YOLO.__new__(YOLO)
    y.device = DEV
    d = y.demodulate(ext, symbol_rate=[c["rate"] for c in cs], offset=[c["offset"] for c in cs], order=[c["order"] for c in cs], span=F.SPAN)
    words = [list(c["bits"]) for c in cs]
    _lib.PROFILE = []
    try:
        f = y.find_frames(d, words, payload=F.PAYLOAD, t0=ext.t0)
        calls = [k[0] for k in _lib.PROFILE]
    finally:
        _lib.PROFILE = None
    assert calls == ["sy11_sync_correlate", "sy11_sync_peaks", "sy11_sync_frames"]                         # three launches, whatever the number of clips and words
    return cs, ext, d, words, f, y


def test_demodulate_then_find_frames_reads_the_embedded_frames(chain):
    from sy11.data.frames import Frames
    cs, ext, d, words, f, y = chain
    assert isinstance(f, Frames) and d.valid.all() and ext.t0.tolist() == [0.0, 1.0e-3, 4.0e-3, 3.0e-3]
    assert f.cls.tolist() == ext.cls.tolist() and f.names == ext.names and f.rows.tolist() == [0, 1, 2, 3] and f.conf.tolist() == ext.conf.tolist()
    order = np.lexsort((f.position, f.word, f.clip))
    assert order.tolist() == list(range(len(f)))                              # sorted by (clip, word, position)
    k = 0
    for i, (c, (ref, found, m0)) in enumerate(zip(cs, F.case_reference())):
        r = d.symbols[i].cpu().numpy()
        for j, b in enumerate(words):
            why = F.pair_reason(len(r), c["order"], len(b))
            assert f.pairs["reason"][i, j] == why and bool(f.pairs["valid"][i, j]) == (why == "")
            if why:
                continue
            got = F.find(r, b, c["order"], 0.8, F.PAYLOAD)                    # the reference on the device's own symbols: every pair, exactly
            sl = slice(int(f.raw["pos0"][i * 4 + j]), int(f.raw["pos0"][i * 4 + j + 1]))
            assert _same(f.raw["rho2"][sl].cpu().numpy(), got["rho2"]) and np.array_equal(f.raw["q"][sl].cpu().numpy(), got["q"])
            assert np.array_equal(f.raw["hit"][sl].cpu().numpy(), got["hit"])
            for h, p in enumerate(got["position"]):
                assert (int(f.clip[k]), int(f.word[k]), int(f.position[k]), int(f.rotation[k])) == (i, j, int(p), got["rotation"][h])
                assert (int(f.errors[k]), int(f.bit_errors[k]), int(f.n_payload[k])) == (got["errors"][h], got["bit_errors"][h], got["n_payload"][h])
                assert f.rho[k] == math.sqrt(got["rho2"][p]) and np.array_equal(f.payload_bits(k), got["payload"][h]) and f.payload_bits(k).dtype == np.uint8
                # from the demodulation's integers, exactly; then one rounding each
                sample = (d.raw["T0"][i] + (d.raw["i_first"][i] + int(p)) * d.raw["STEP"][i]) / 2.0 ** 32
                time = sample / c["fs"] + float(ext.t0[i])
                assert abs(f.sample[k] - sample) <= 1e-12 * sample and abs(f.time[k] - time) <= 1e-12 * time
                k += 1
        # the clip's own word: the frames the reference alone finds (tests/test_frames_cpu.py), where they were embedded, and what was sent after them
        L = len(F.decisions(c["bits"], c["order"]))
        own = np.flatnonzero((f.clip == i) & (f.word == i))
        m0_dev = F.stream_index(d.raw["T0"][i], d.raw["STEP"][i], d.raw["i_first"][i], c["sps"], c["u0"], F.SPAN)
        assert f.position[own].tolist() == [j - m0_dev for j in c["at"]] == found["position"].tolist()
        assert not f.errors[own].any() and not f.bit_errors[own].any() and f.n_payload[own].tolist() == [F.PAYLOAD] * len(own) and f.rho[own].min() >= 0.98
        for h, at in zip(own, c["at"]):
            assert np.array_equal(f.payload_bits(int(h)), F.bits_of(c["d"][at + L:at + L + F.PAYLOAD], c["order"]))
        assert f.rotation[own].tolist() == found["rotation"]
        # the rotation of tests/_demod_ref.errors turns r FORWARD onto what was sent: it undoes ours
        a = R.point(c["d"], c["order"])
        k0 = (d.raw["T0"][i] + d.raw["i_first"][i] * d.raw["STEP"][i]) / 2.0 ** 32
        bad, rot, shift = R.errors(r, c["order"], k0, c["sps"], a, c["u0"], F.SPAN)
        print(f"find_frames[{c['label']}]: {len(own)} frames of its word at {f.position[own].tolist()}, rho {np.round(f.rho[own], 4).tolist()}, rotation {int(f.clip_rotation[i])}; "
              f"the stream has {bad} symbol errors at the reference's rotation {rot}, shift {shift}")
        assert (bad, shift) == (0, 0) and int(f.clip_rotation[i]) == (c["order"] - rot) % c["order"]
        assert int(f.n_frames[i]) == int((f.clip == i).sum()) >= len(own)
    assert k == len(f) and f.payload.shape == (len(f), 10) and f.payload.device.type == "cuda"
    assert f[0]["clip"] == 0 and f[0]["errors"] == int(f.errors[0])


def test_max_errors_save_round_trip_and_the_empty_demodulation(chain, tmp_path):
    from sy11 import _lib
    from sy11.engine.predictor import DetectionPredictor
    cs, ext, d, words, f, y = chain
    pred = DetectionPredictor.__new__(DetectionPredictor)
    pred.device = DEV
    f0 = pred.find_frames(d, words, payload=F.PAYLOAD, max_errors=0, t0=ext.t0)
    keep = f.errors <= 0
    assert len(f0) == int(keep.sum()) >= 11 and np.array_equal(f0.position, f.position[keep]) and np.array_equal(f0.time, f.time[keep])
    assert torch.equal(f0.payload, f.payload[torch.from_numpy(keep).to(DEV)])
    no_t0 = y.find_frames(d, words[:1])
    assert np.array_equal(no_t0.time, no_t0.sample / np.asarray(d.sample_rate)[no_t0.clip]) and no_t0.payload.shape == (len(no_t0), 0) and no_t0.payload_bits(0).shape == (0,)
    out = f.save(tmp_path / "f")
    z = np.load(tmp_path / "f" / "frames.npz")
    index = json.loads((tmp_path / "f" / "frames.json").read_text())
    assert out == str(tmp_path / "f")
    for key in f.COLUMNS + ("clip_rotation", "n_frames"):
        assert np.array_equal(z[key], getattr(f, key)), key
    assert np.array_equal(z["payload"], f.payload.cpu().numpy()) and np.array_equal(z["pair_valid"], f.pairs["valid"])
    assert index["words"] == words and index["payload"] == F.PAYLOAD and index["threshold"] == 0.8 and len(index["frames"]) == len(f)
    assert index["frames"][0]["position"] == int(f.position[0]) and index["frames"][0]["time"] == float(f.time[0]) and index["frames"][0]["name"] == "a"
    # argument errors come before the device; an empty demodulation launches nothing
    with pytest.raises(ValueError, match="threshold"):
        y.find_frames(d, words, threshold=0.0)
    with pytest.raises(ValueError, match="t0"):
        y.find_frames(d, words, t0=[0.0])
    none = _extraction([], [])
    _lib.PROFILE = []
    try:
        e = y.find_frames(y.demodulate(none, symbol_rate=[], offset=[], order=[]), words, payload=8)
        short = y.find_frames(d, [[0, 1, 1, 0]])                                 # no valid pair: four symbols at the most
        calls = [k[0] for k in _lib.PROFILE]
    finally:
        _lib.PROFILE = None
    assert calls == [] and len(e) == 0 and e.position.shape == (0,) and e.payload.shape == (0, 0) and e.clip_rotation.shape == (0,) and e.n_frames.shape == (0,)
    assert len(short) == 0 and short.clip_rotation.tolist() == [-1] * 4 and short.n_frames.tolist() == [0] * 4 and not short.pairs["valid"].any() and short.raw["rho2"] is None
