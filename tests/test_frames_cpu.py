"""CPU: the frame search's preconditions from the reference alone (tests/_frames_ref.py on the reference demodulation of four clips with
embedded sync words: every frame found at its place at threshold 0.8 and nothing else, no word error, the 40 payload symbols as sent, one
rotation per clip), the tie rule, and the host plan of sy11/data/frames.py: every ``ValueError`` of ``plan_frames``, the pair-skipping reasons,
the item table and the record layouts.  Nothing here touches a device."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from tests import _frames_ref as F

ROOT = Path(__file__).resolve().parents[1]


# ------------------------------------------------------------------------------------------------------------- preconditions
def test_reference_finds_every_embedded_frame_and_nothing_else():
    for c, (ref, found, m0) in zip(F.case_clips(), F.case_reference()):
        w = F.decisions(c["bits"], c["order"])
        L = len(w)
        want = [j - m0 for j in c["at"]]
        rho = np.sqrt(found["rho2"])
        apart = np.ones(rho.shape[0], dtype=bool)
        for p in want:
            apart[max(p - L + 1, 0):p + L] = False
        print(f"frames[{c['label']}]: {ref['n_symbols']} symbols, L = {L}; frames at {found['position'].tolist()} (embedded at {want}), rho {np.round(found['rho'], 4).tolist()}, "
              f"rotation {found['rotation']}, word errors {found['errors']}; best position apart from a frame {rho[apart].max():.4f}")
        assert found["position"].tolist() == want                           # every frame, at its place, and nothing else
        assert min(found["rho"]) >= 0.98 and rho[apart].max() < 0.75        # the margin on both sides of the default threshold of 0.8
        assert found["errors"] == [0] * len(want) and found["bit_errors"] == [0] * len(want)
        assert len(set(found["rotation"])) == 1                             # one rotation per clip
        assert found["n_payload"] == [F.PAYLOAD] * len(want)
        for k, j in enumerate(c["at"]):
            sent = F.bits_of(c["d"][j + L:j + L + F.PAYLOAD], c["order"])
            assert sent.shape == (F.PAYLOAD * c["order"] // 2,) and np.array_equal(found["payload"][k], sent)
        # the rotation is the one that turns the whole stream into what was sent
        d = F.decide(F.turn(ref["r"].astype(np.complex64), found["rotation"][0], c["order"]), c["order"])
        assert np.array_equal(d, c["d"][m0:m0 + d.shape[0]])


def test_of_equal_peaks_closer_than_the_word_the_earliest_wins():
    bits = [0, 0, 1, 0] * 4
    stream = F.points(np.array([0, 0, 1, 0] * 6), 2).astype(np.complex64)   # noiseless +-1: the pattern six times
    rho2, q = F.correlate(stream, F.decisions(bits, 2), 2)
    assert rho2.shape == (9,) and np.flatnonzero(rho2 == 1.0).tolist() == [0, 4, 8] and rho2.max() == 1.0 and not q.any()
    for thr in (0.8, 1.0):
        assert np.flatnonzero(F.peaks(rho2, 16, thr * thr)).tolist() == [0]
    rho2n, qn = F.correlate(-stream, F.decisions(bits, 2), 2)
    assert np.array_equal(rho2n, rho2) and qn.tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1]          # between the matches C = 0: not below 0
    # a NaN is never a hit and suppresses none; a zero run has rho2 = 0
    z = stream.copy()
    z[20] = np.nan
    r2, _ = F.correlate(z, F.decisions(bits, 2), 2)
    assert np.isnan(r2[5:]).all() and np.flatnonzero(F.peaks(r2, 16, 0.64)).tolist() == [0]
    assert F.correlate(np.zeros(20, dtype=np.complex64), F.decisions(bits, 2), 2)[0].tolist() == [0.0] * 5


def test_reference_rotations_and_payload_packing():
    g = np.random.default_rng(3)
    bits = g.integers(0, 2, 32)
    for order in (2, 4):
        w = F.decisions(bits, order)
        d = np.concatenate((g.integers(0, order, 5).astype(np.uint8), w, g.integers(0, order, 11).astype(np.uint8)))
        for q in range(order):
            r = (F.points(d, order) * np.exp(2j * np.pi * q / order)).astype(np.complex64)
            r = (np.round(r.real) + 1j * np.round(r.imag)).astype(np.complex64)
            found = F.find(r, bits, order, 1.0, payload=20)
            assert found["position"].tolist() == [5] and found["rotation"] == [q] and found["errors"] == [0] and found["n_payload"] == [11]
            assert np.array_equal(found["payload"][0], F.bits_of(d[5 + len(w):], order))
            e, be, n_pay, row = F.frames(r, w ^ 1, order, 5, q, 20, 6)       # every decision's last bit flipped
            assert (e, be, n_pay) == (len(w), len(w), 11) and row.shape == (6,) and not row[(11 * (order // 2) + 7) // 8:].any()


# ------------------------------------------------------------------------------------------------------------- the host plan
def test_plan_frames_raises_every_argument_error_as_value_error():
    from sy11.data.frames import plan_frames
    ok = ((np.array([100, 50]), np.array([2, 4])), [[0, 1] * 8])
    plan_frames(*ok)
    bad = [
        (dict(words=[]), "non-empty sequence"), (dict(words=()), "non-empty sequence"), (dict(words="0101"), "non-empty sequence"), (dict(words=None), "non-empty sequence"),
        (dict(words=[[0, 1, 2] * 4]), "word 0"), (dict(words=[[0, 1] * 8, [0.0, 1.0] * 8]), "word 1"), (dict(words=[[True, False] * 8]), "word 0"),
        (dict(words=[[]]), "word 0"), (dict(words=[[[0, 1] * 4] * 2]), "word 0"), (dict(words=[[0, -1] * 8]), "word 0"),
        (dict(payload=-1), "payload"), (dict(payload=2 ** 20), "payload"), (dict(payload=1.5), "payload"), (dict(payload=True), "payload"),
        (dict(threshold=0.0), "threshold"), (dict(threshold=1.0001), "threshold"), (dict(threshold=-0.5), "threshold"), (dict(threshold=float("nan")), "threshold"),
        (dict(threshold=float("inf")), "threshold"), (dict(threshold="0.8"), "threshold"),
        (dict(max_errors=-1), "max_errors"), (dict(max_errors=0.5), "max_errors"),
        (dict(t0=[0.0]), "t0"), (dict(t0=[0.0, 1.0, 2.0]), "t0"), (dict(t0=1.0), "t0"),
        (dict(demodulation=(np.array([1.5, 2.0]), 2)), "integers"), (dict(demodulation=(np.array([10, 20]), np.array([2, 4, 2]))), "order"),
        (dict(demodulation=7), "Demodulation"), (dict(demodulation=(np.array([2 ** 31]), 2)), "2\\^31"),
    ]
    for kw, what in bad:
        a = dict(demodulation=ok[0], words=ok[1], payload=0, threshold=0.8, max_errors=None, t0=None)
        a.update(kw)
        with pytest.raises(ValueError, match=what):
            plan_frames(a["demodulation"], a["words"], a["payload"], a["threshold"], max_errors=a["max_errors"], t0=a["t0"])
    p = plan_frames(ok[0], ok[1], 2 ** 20 - 1, 1.0, max_errors=0, t0=[0.5, 1.5])
    assert (p.payload, p.threshold, p.max_errors, p.t0.tolist()) == (2 ** 20 - 1, 1.0, 0, [0.5, 1.5])


def test_plan_frames_skips_pairs_with_a_reason_and_tiles_the_rest():
    from sy11.data.frames import ITEM, plan_frames, tile, word_decisions
    T = tile()
    assert T == F.TILE
    g = np.random.default_rng(9)
    words = [g.integers(0, 2, n).tolist() for n in (13, 16, 7, 514, 512)]
    n_sym = np.array([2 * T + 3 + 15, 12, 300, 0, 40, 256])
    order = np.array([2, 4, 4, 2, 3, 2])
    p = plan_frames((n_sym, order), words)
    want_valid = np.zeros((6, 5), dtype=bool)
    for i in range(6):
        for j, w in enumerate(words):
            why = F.pair_reason(int(n_sym[i]), int(order[i]), len(w))
            assert p.reason[i, j] == why, (i, j)
            want_valid[i, j] = why == ""
    assert np.array_equal(p.valid, want_valid)
    assert p.reason[0].tolist() == ["", "", "word outside [8, 256] symbols", "word outside [8, 256] symbols", "word outside [8, 256] symbols"]
    assert p.reason[1].tolist() == ["bit count not divisible by log2(order)", "", "bit count not divisible by log2(order)", "word outside [8, 256] symbols", "clip shorter than the word"]
    assert p.reason[2, 3] == "word outside [8, 256] symbols" and p.reason[2, 4] == "" and p.L[2, 4] == 256 and p.P[2, 4] == 45
    assert set(p.reason[3].tolist()) == {"clip not valid"} and set(p.reason[4].tolist()) == {"clip not valid"}
    assert p.reason[5, 4] == "word outside [8, 256] symbols" and p.valid[5, 0]
    assert p.sym_off.tolist() == [0, 530, 542, 842, 842, 842]               # the clips that are not valid hold no symbols
    assert np.array_equal(p.P[p.valid], (n_sym[:, None] - p.L + 1)[p.valid]) and not p.P[~p.valid].any()
    assert p.pos0.tolist() == np.concatenate(([0], np.cumsum(p.P.reshape(-1)))).tolist() and p.total_positions == int(p.P.sum())
    for j, w in enumerate(words):
        for o in (2, 4):
            d = F.decisions(w, o)
            mine = word_decisions(np.array(w), o)
            assert (d is None) == (mine is None) and (d is None or np.array_equal(d, mine))
    items, pair = p.items()
    assert items.dtype == ITEM and items.shape[0] == int((-(-p.P // T)).sum())
    seen = np.zeros(p.total_positions, dtype=np.int64)
    for it, k in zip(items, pair):
        i, j = divmod(int(k), 5)
        assert p.valid[i, j] and (int(it["sym_off"]), int(it["n_sym"]), int(it["L"]), int(it["order"])) == (int(p.sym_off[i]), int(n_sym[i]), int(p.L[i, j]), int(order[i]))
        assert int(it["p0"]) % T == 0 and 1 <= int(it["cnt"]) <= T and (int(it["cnt"]) == T or int(it["p0"]) + int(it["cnt"]) == int(p.P[i, j]))
        assert int(it["pos_off"]) == int(p.pos0[k])
        w = p.word_buf[int(it["word_off"]):int(it["word_off"]) + int(it["L"])]
        assert np.array_equal(w, F.decisions(words[j], int(order[i])))
        seen[int(it["pos_off"]) + int(it["p0"]):int(it["pos_off"]) + int(it["p0"]) + int(it["cnt"])] += 1
    assert (seen == 1).all()                                                # every position of every valid pair, once
    assert [int(c) for c in items["cnt"][pair == 0]] == [T, T, 6]           # P = 2 T + 6 at L = 13


def test_records_are_laid_out_as_the_header_declares_them():
    from sy11.data.frames import FRAME, ITEM
    header = (ROOT / "include" / "sy11.h").read_text()
    ctype = {"int64_t": C.c_int64, "int32_t": C.c_int32}
    for name, dt in (("sy11_sync_item", ITEM), ("sy11_sync_frame", FRAME)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S).group(1)
        fields = re.findall(r"^\s*(int64_t|int32_t)\s+(\w+);", body, re.M)
        assert [f[1] for f in fields] == list(dt.names)

        class S(C.Structure):
            _fields_ = [(n, ctype[t]) for t, n in fields]
        assert C.sizeof(S) == dt.itemsize and dt.itemsize % 8 == 0
        for t, n in fields:
            assert getattr(S, n).offset == dt.fields[n][1] and C.sizeof(ctype[t]) == dt.fields[n][0].itemsize


def test_the_library_refuses_bad_frame_search_calls_before_any_launch():
    """Without a GPU: every argument check of the three entries returns before anything is launched."""
    from sy11 import _lib
    from sy11.data.frames import FRAME, ITEM
    lib = _lib.load()
    assert lib.sy11_sync_tile() == F.TILE
    it = np.zeros(1, dtype=ITEM)
    it["n_sym"], it["L"], it["order"], it["cnt"] = 40, 16, 2, 25
    buf = np.zeros(1024, dtype=np.uint8)
    ptr, tab = C.c_void_p(buf.ctypes.data), C.c_void_p(it.ctypes.data)
    assert lib.sy11_sync_correlate(1, tab, tab, 16, None, 40, ptr, 25, ptr, ptr, None) == -1 and b"null" in lib.sy11_last_error()
    for kw, what in ((dict(order=3), b"order"), (dict(L=7), b"word of"), (dict(L=41), b"word of"), (dict(n_sym=41), b"packed symbols"), (dict(word_off=1), b"word symbols"),
                     (dict(cnt=24), b"not a tile"), (dict(cnt=26), b"not a tile"), (dict(p0=256), b"not a tile"), (dict(pos_off=1), b"packed positions")):
        bad = it.copy()
        for k, v in kw.items():
            bad[k] = v
        t = C.c_void_p(bad.ctypes.data)
        assert lib.sy11_sync_correlate(1, t, t, 16, ptr, 40, ptr, 25, ptr, ptr, None) == -1 and what in lib.sy11_last_error(), kw
        assert lib.sy11_sync_peaks(1, t, t, 16, 40, 25, ptr, 0.64, ptr, None) == -1 and what in lib.sy11_last_error(), kw
    for thr2 in (0.0, 1.5, float("nan")):
        assert lib.sy11_sync_peaks(1, tab, tab, 16, 40, 25, ptr, thr2, ptr, None) == -1 and b"threshold" in lib.sy11_last_error()
    fr = np.zeros(1, dtype=FRAME)
    fr["n_sym"], fr["L"], fr["order"], fr["p"], fr["payload"] = 40, 16, 4, 24, 8
    for kw, what in ((dict(q=4), b"rotation"), (dict(q=-1), b"rotation"), (dict(order=8), b"order"), (dict(p=25), b"ends after"), (dict(payload=9), b"payload symbols"),
                     (dict(payload=2 ** 20), b"payload symbols"), (dict(row=1), b"writes row"), (dict(L=300), b"word of")):
        bad = fr.copy()
        for k, v in kw.items():
            bad[k] = v
        t = C.c_void_p(bad.ctypes.data)
        assert lib.sy11_sync_frames(1, t, t, 16, ptr, 40, ptr, 1, ptr, 2, ptr, None) == -1 and what in lib.sy11_last_error(), kw
