"""GPU: the frame corrector's kernels (sy11_rs_decode, sy11_rs_check) against tests/_rs_ref.py.  Every comparison is ``np.array_equal``: the decoder is exact
integer arithmetic.  The kernel-level tests feed synthetic byte rows to ``ops.rs_*`` directly, for every preset and four more codes, every interleaving depth
and offset, with the outputs' slack and spare rows filled with sentinels that must survive; one call over all frames, one call per frame and a permuted
packing give the same bytes; the byte-serial CRC of ``rs_check`` and the bit-serial one of ``fec_check`` / ``ldpc_check`` agree on the same bytes; every refusal is raised by ``ops``
and by the library with the outputs untouched; and ``demodulate`` -> ``find_frames`` -> ``decode``
-> ``correct`` on two clips reads what was sent, through a burst the Viterbi decoder does not survive, in exactly two launches."""
import copy
import ctypes as C
import functools
import json

import numpy as np
import pytest
import torch

from tests import _fec_ref as FEC
from tests import _frames_ref as F
from tests import _rs_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FC = 2.4e9
CODES = dict(R.CODES, **{"40-36": R.code(40, 36), "60-55": R.code(60, 55, fcr=3, prim=7), "255-253": R.code(255, 253, fcr=1), "20-19": R.code(20, 19)})
MISCORRECTING = {"255-253": 100, "40-36": 100}                 # the codes that supply the miscorrected codewords, and the random words each setting adds for it
DATA_FILL, INFO_FILL, CW_FILL = 0xA5, 0x5A, -7


def _hit(g, word, at):
    word[at] ^= g.integers(1, 256, len(at)).astype(np.uint8)


def _words(cd, g, extra=0):
    """Received words of one setting -> (rx (words, n), sent (words, n), count: the byte errors put in, -1 where the word is not a damaged codeword, kinds)."""
    n, k = cd["n"], cd["k"]
    t = (n - k) // 2
    corners = [0, k - 1, n - 1]                                  # the first byte, the last information byte, the last parity byte
    plan = [(c, "random") for c in (0, 1, t, t + 1, t + 3)] + [(t, "burst")] + [(int(g.integers(0, t + 4)), "random") for _ in range(extra)]
    sent = R.encode(g.integers(0, 256, (len(plan), k)), cd)
    rx, count, kinds = sent.copy(), [], []
    for w, (c, kind) in enumerate(plan):
        if kind == "burst":
            at = np.arange(c) + int(g.integers(0, n - c + 1))
        else:
            first = [corners[(w + i) % 3] for i in range(min(c, 3))]
            rest = np.setdiff1d(np.arange(n), first)
            at = np.concatenate((first, g.choice(rest, c - len(first), replace=False))).astype(np.int64)
        _hit(g, rx[w], at)
        count.append(c), kinds.append(kind)
    more, kinds = [np.zeros(n, dtype=np.uint8), np.full(n, 0xFF, dtype=np.uint8)], kinds + ["zeros", "ones"]
    if n < 255 and t >= 1:
        # a codeword of the full-length code with ONE byte among those that are not transmitted: without that byte (and with t - 1 more errors) it lies
        # within t of the received word, but it is no word of the shortened code
        full = R.code(255, 255 - (n - k), cd["poly"], cd["fcr"], cd["prim"])
        m = np.concatenate((np.zeros(255 - n, dtype=np.int64), g.integers(0, 256, k)))
        m[int(g.integers(0, 255 - n))] = int(g.integers(1, 256))
        c = R.encode(m, full)
        assert np.count_nonzero(c[:255 - n]) == 1 and not R.syndromes(c[None], full).any()
        word = c[255 - n:].copy()
        _hit(g, word, g.choice(n, t - 1, replace=False))
        more.append(word), kinds.append("pad")
    count += [-1] * len(more)
    return np.concatenate((rx, np.stack(more))), np.concatenate((sent, np.zeros((len(more), n), dtype=np.uint8))), np.array(count), kinds


def _run(words, cd, I, offset, rows=None, n_rows=None, slack=3):
    """``words`` (frames, I, n) through ``ops.rs_decode`` -> (the data table, info, cw as numpy, sentinels and all)."""
    from sy11 import ops
    n, k, n_frame = cd["n"], cd["k"], len(words)
    rows = np.arange(n_frame) if rows is None else np.asarray(rows)
    n_rows = n_frame if n_rows is None else n_rows
    data = np.full((n_rows, offset + I * n + slack), DATA_FILL, dtype=np.uint8)
    for f in range(n_frame):
        data[rows[f], offset:offset + I * n] = R.interleave(words[f])
    dev = torch.from_numpy(data).to(DEV)
    info = torch.full((n_rows, I * k + slack), INFO_FILL, dtype=torch.uint8, device=DEV)
    cw = torch.full((n_rows, I, 2), CW_FILL, dtype=torch.int32, device=DEV)
    ops.rs_decode(dev, rows, cd, info, cw, interleave=I, offset=offset)
    assert np.array_equal(dev.cpu().numpy(), data)
    return data, info.cpu().numpy(), cw.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------- launch 1
@pytest.mark.parametrize("name", list(CODES))
def test_decode_every_depth_offset_and_error_count_equals_the_reference(name):
    cd = CODES[name]
    n, k = cd["n"], cd["k"]
    t = (n - k) // 2
    g = np.random.default_rng(41)
    seen = {"failed": 0, "miscorrected": 0, "corrected": 0, "pad": 0, "words": 0}
    for I in (1, 3, 8):
        for offset in (0, 5):
            rx, sent, count, kinds = _words(cd, g, MISCORRECTING.get(name, 0))
            fill = -len(rx) % I                                                # whole frames: more random words
            if fill:
                more = R.encode(g.integers(0, 256, (fill, k)), cd)
                for w in range(fill):
                    _hit(g, more[w], g.choice(n, int(g.integers(0, t + 1)), replace=False))
                rx, sent, count, kinds = np.concatenate((rx, more)), np.concatenate((sent, more)), np.concatenate((count, [-1] * fill)), kinds + ["fill"] * fill
            order = g.permutation(len(rx))                                     # the kinds spread over the frames and codewords
            rx, sent, count, kinds = rx[order], sent[order], count[order], [kinds[i] for i in order]
            n_frame = len(rx) // I
            rows = g.permutation(n_frame + 2)[:n_frame]                        # the frames' rows in another order, two rows of the table spare
            data, info, cw = _run(rx.reshape(n_frame, I, n), cd, I, offset, rows=rows, n_rows=n_frame + 2)
            want_info, want_cw = R.correct_rows(data, rows, cd, I, offset)
            assert np.array_equal(info[rows, :I * k], want_info), (name, I, offset)
            assert np.array_equal(cw[rows], want_cw), (name, I, offset)
            assert (info[rows, I * k:] == INFO_FILL).all()                      # the slack of a row, and the rows of no frame
            spare = np.setdiff1d(np.arange(n_frame + 2), rows)
            assert (info[spare] == INFO_FILL).all() and (cw[spare] == CW_FILL).all()
            e = want_cw.reshape(-1, 2)[:, 0]
            got = want_info.reshape(-1, k)
            for w in range(len(rx)):
                if 0 <= count[w] <= t:
                    assert e[w] == count[w] and np.array_equal(got[w], sent[w, :k]), (name, I, offset, w, kinds[w])
                    seen["corrected"] += 1
                elif count[w] > t:
                    assert e[w] == -1 or (e[w] <= t and not np.array_equal(got[w], sent[w, :k]))
                    seen["failed" if e[w] < 0 else "miscorrected"] += 1         # a miscorrection is one the reference accepts: it is a codeword within t
                elif kinds[w] == "pad":
                    assert e[w] == -1 and np.array_equal(got[w], rx[w, :k]), (name, I, offset, w)
                    seen["pad"] += 1
                elif kinds[w] == "zeros":
                    assert e[w] == 0 and not got[w].any()
            seen["words"] += len(rx)
    print(f"rs_decode[{name}]: {seen}")
    assert seen["failed"] >= 1 and seen["corrected"] >= 18
    if name in MISCORRECTING:
        assert seen["miscorrected"] >= 1
    if n < 255 and t >= 1:
        assert seen["pad"] == 6


def test_decode_largest_shape_64_frames_of_four_ccsds_codewords():
    cd = R.CODES["ccsds-255-223"]
    g = np.random.default_rng(42)
    sent = R.encode(g.integers(0, 256, (256, 223)), cd)
    rx = sent.copy()
    count = np.resize(np.arange(17), 256)
    for w in range(256):
        _hit(g, rx[w], g.choice(255, count[w], replace=False))
    data, info, cw = _run(rx.reshape(64, 4, 255), cd, 4, 0, slack=0)
    want_info, want_cw = R.correct_rows(data, np.arange(64), cd, 4, 0)
    assert np.array_equal(info, want_info) and np.array_equal(cw, want_cw)
    assert np.array_equal(info.reshape(256, 223), sent[:, :223]) and np.array_equal(cw.reshape(256, 2)[:, 0], count)
    assert np.array_equal(cw.reshape(256, 2)[:, 1], np.unpackbits(rx ^ sent, axis=1).sum(axis=1))


# ------------------------------------------------------------------------------------------------------------- batching
def test_one_call_per_frame_and_a_permuted_packing_give_the_same_bytes():
    cd, I, offset = CODES["60-55"], 3, 5
    g = np.random.default_rng(43)
    rx, _, _, _ = _words(cd, g, 9)
    n_frame = len(rx) // I
    words = rx[:n_frame * I].reshape(n_frame, I, cd["n"])
    _, info, cw = _run(words, cd, I, offset)
    perm = g.permutation(n_frame + 3)[:n_frame]                                # other rows, of a larger table, in another order
    order = g.permutation(n_frame)
    _, pi, pc = _run(words[order], cd, I, offset, rows=perm[order], n_rows=n_frame + 3)
    assert np.array_equal(pi[perm], info) and np.array_equal(pc[perm], cw)
    for f in range(n_frame):
        _, oi, oc = _run(words[f:f + 1], cd, I, offset)
        assert np.array_equal(oi[0], info[f]) and np.array_equal(oc[0], cw[f])
    assert (cw[:, :, 0] == -1).any() and (cw[:, :, 0] > 0).any()


# ------------------------------------------------------------------------------------------------------------- launch 2
SPECS = dict(FEC.CRCS, **{"none": None})


@pytest.mark.parametrize("name", list(SPECS))
def test_check_sums_and_crc_over_the_corrected_bytes(name):
    from sy11 import ops
    spec = SPECS[name]
    cd, I = CODES["40-36"], 3
    k, nb = cd["k"], (spec["width"] // 8 if spec else 0)
    g = np.random.default_rng(44)
    words, bodies = [], []
    for f in range(5):
        msg = g.integers(0, 256, I * k - nb).astype(np.uint8)
        check = [(FEC.crc(np.unpackbits(msg), spec) >> (8 * (nb - 1 - i))) & 255 for i in range(nb)] if spec else []
        body = np.concatenate((msg, check)).astype(np.uint8)
        if f == 3:
            body[5] ^= 1                                                        # a wrong message under a good check field
        cws = R.encode(body.reshape(I, k), cd)
        for w in range(I):
            _hit(g, cws[w], g.choice(cd["n"], (f + w) % 3, replace=False))      # 0 .. 2 errors: all corrected
        if f == 4:
            _hit(g, cws[1], np.arange(8, 13))                                   # one codeword of this frame beyond the code
        words.append(cws)
        bodies.append(body)
    data, info, cw = _run(np.stack(words), cd, I, 0)
    assert all(np.array_equal(info[f, :I * k], bodies[f]) for f in range(4))     # the corrected bytes are what the check runs over
    rows = torch.full((5, 6), CW_FILL, dtype=torch.int32, device=DEV)
    ops.rs_check(torch.from_numpy(info).to(DEV), torch.from_numpy(cw).to(DEV), np.arange(5), cd, rows, interleave=I, crc=spec)
    got = rows.cpu().numpy()
    for f in range(5):
        want = R.check(info[f, :I * k], cw[f], FEC.crc, spec)
        assert got[f, :3].tolist() == want[:3] and got[f, 3:5].view(np.uint32).tolist() == want[3:5] and got[f, 5] == want[5], (name, f)
        assert want[0] == (1 if f == 4 else 0) and want[5] == (-1 if spec is None else int(f < 3))
        assert want[1] == sum(int(e) for e in cw[f, :, 0] if e >= 0) and want[1] > 0


def test_bit_serial_and_byte_serial_crc_agree_in_the_three_check_launches():
    """The one CRC of csrc/frame_check.h in its two forms: ``ops.fec_check`` and ``ops.ldpc_check`` run it bit by bit, ``ops.rs_check`` byte by byte.  The same information
    bytes (a message and its check field) go to all three, for every whole-byte spec: the three (crc_calc, crc_recv, crc_ok) are identical and those of
    tests/_fec_ref.crc; one flipped message bit in frame 1 and all three say crc_ok = 0 there."""
    from sy11 import ops
    from sy11.data.decode import FECFRAME
    specs = dict(FEC.CRCS, **{"crc24-refin": dict(width=24, poly=0x864CFB, init=0xB704CE, refin=True, refout=False, xorout=0x000000)})
    msgs = [np.frombuffer(b"123456789", dtype=np.uint8).copy(), np.random.default_rng(45).integers(0, 256, 9).astype(np.uint8)]
    up = lambda a, dtype: torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(dtype)      # noqa: E731
    for name, spec in specs.items():
        W = spec["width"]
        k, n_info = 9 + W // 8, 8 * (9 + W // 8)
        for flip in (False, True):
            body = [m.copy() for m in msgs]
            field = [FEC.crc(np.unpackbits(m), spec) for m in msgs]             # the check field of the message as it was sent
            if flip:
                body[1][4] ^= 0x10
            info = np.stack([np.concatenate((m, [(c >> (W - 8 - 8 * i)) & 255 for i in range(W // 8)])).astype(np.uint8) for m, c in zip(body, field)])
            want = [[FEC.crc(np.unpackbits(m), spec), c, int(FEC.crc(np.unpackbits(m), spec) == c)] for m, c in zip(body, field)]
            got = {}
            # the Viterbi decoder's check: no tail, T = n_info steps, the decided bits are the information
            fr = np.zeros(2, dtype=FECFRAME)
            fr["T"], fr["order"], fr["row"], fr["scale"] = n_info, 2, np.arange(2), 1.0
            rows = torch.full((2, 5), CW_FILL, dtype=torch.int32, device=DEV)
            data = torch.full((2, k), DATA_FILL, dtype=torch.uint8, device=DEV)
            ops.fec_check(torch.zeros((2, 2 * n_info), dtype=torch.int8, device=DEV), up(info, torch.uint8), fr, FEC.POLYS, n_info, data, rows, crc=spec)
            got["fec_check"] = rows.cpu().numpy()[:, :3]
            assert np.array_equal(data.cpu().numpy(), info)
            # the LDPC decoder's check: N = K + 2, the first K decided bits are the information
            rows = torch.full((2, 5), CW_FILL, dtype=torch.int32, device=DEV)
            data = torch.full((2, k), DATA_FILL, dtype=torch.uint8, device=DEV)
            decided = np.concatenate((info, np.zeros((2, 1), dtype=np.uint8)), axis=1)
            ops.ldpc_check(torch.zeros((2, n_info + 2), dtype=torch.int8, device=DEV), up(decided, torch.uint8), np.arange(2), n_info + 2, n_info, data, rows, crc=spec)
            got["ldpc_check"] = rows.cpu().numpy()[:, :3]
            assert np.array_equal(data.cpu().numpy(), info)
            # the corrector's check: one codeword of k information bytes, nothing corrected
            rows = torch.full((2, 6), CW_FILL, dtype=torch.int32, device=DEV)
            ops.rs_check(up(info, torch.uint8), torch.zeros((2, 1, 2), dtype=torch.int32, device=DEV), np.arange(2), R.code(k + 2, k), rows, interleave=1, crc=spec)
            got["rs_check"] = rows.cpu().numpy()[:, 3:]
            for launch, r in got.items():
                calc, recv, ok = r[:, 0].copy().view(np.uint32).tolist(), r[:, 1].copy().view(np.uint32).tolist(), r[:, 2].tolist()
                assert [list(t) for t in zip(calc, recv, ok)] == want, (name, flip, launch)
            assert [w[2] for w in want] == [1, 0 if flip else 1], (name, flip)
    assert FEC.crc(np.unpackbits(msgs[0]), specs["crc32"]) == 0xCBF43926


# ------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_raise_and_write_nothing():
    from sy11 import _lib, ops
    cd, I = CODES["40-36"], 2
    p = lambda v: C.c_void_p(v.data_ptr())                                    # noqa: E731
    data = torch.full((2, 85), DATA_FILL, dtype=torch.uint8, device=DEV)
    info = torch.full((2, 72), INFO_FILL, dtype=torch.uint8, device=DEV)
    cw = torch.full((2, 2, 2), CW_FILL, dtype=torch.int32, device=DEV)
    rows = torch.full((2, 6), CW_FILL, dtype=torch.int32, device=DEV)
    fr = np.array([1, 0])
    crc16 = FEC.CRCS["crc16-ccitt-false"]
    # the arguments themselves are good: the same calls on copies go through
    ops.rs_decode(data, fr, cd, info.clone(), cw.clone(), interleave=I, offset=5)
    ops.rs_check(info.clone(), cw.clone().zero_(), fr, cd, rows.clone(), interleave=I, crc=crc16)
    good = dict(data=data, frames=fr, code=cd, info=info, cw=cw, interleave=I, offset=5)
    for bad in (dict(code=dict(cd, n=256)), dict(code=dict(cd, k=40)), dict(code=dict(cd, k=0)), dict(code=dict(cd, n=120, k=55)), dict(code=dict(cd, fcr=255)), dict(code=dict(cd, prim=3)),
                dict(code=dict(cd, prim=0)), dict(code=dict(cd, poly=0x11B)), dict(code=dict(cd, poly=0x1D)), dict(code="40-36"), dict(code=dict(n=40, k=36)), dict(interleave=0),
                dict(interleave=9), dict(interleave=3), dict(offset=-1), dict(offset=6), dict(offset=1.0), dict(frames=np.array([0, 2])), dict(frames=np.array([0, 0])),
                dict(frames=np.array([-1, 0])), dict(frames=np.zeros(0, dtype=np.int64)), dict(frames=np.array([0.0, 1.0])), dict(data=data.cpu()), dict(data=data[:, :84]),
                dict(data=data.to(torch.int8)), dict(info=info[:, :71]), dict(info=info[:1]), dict(info=info.to(torch.int8)), dict(cw=cw[:, :1]), dict(cw=cw.to(torch.int64)),
                dict(cw=cw[:1]), dict(cw=cw.cpu())):
        a = dict(good)
        a.update(bad)
        with pytest.raises(ValueError, match="rs_decode"):
            ops.rs_decode(a["data"], a["frames"], a["code"], a["info"], a["cw"], interleave=a["interleave"], offset=a["offset"])
    good = dict(info=info, cw=cw, frames=fr, code=cd, rows=rows, interleave=I, crc=crc16)
    for bad in (dict(code=dict(cd, prim=5)), dict(code=dict(cd, poly=0x11B)), dict(interleave=9), dict(interleave=3), dict(frames=np.array([0, 2])), dict(frames=np.array([1, 1])),
                dict(info=info[:, :71]), dict(info=info.cpu()), dict(cw=cw[:, :1]), dict(rows=rows[:, :5]), dict(rows=rows.to(torch.int64)), dict(rows=rows[:1]),
                dict(crc="crc8"), dict(crc=dict(width=8)), dict(crc=dict(crc16, width=12)), dict(crc=dict(crc16, width=40)), dict(crc=dict(crc16, poly=0x11021)),
                dict(crc=dict(crc16, refin=2))):
        a = dict(good)
        a.update(bad)
        with pytest.raises(ValueError, match="rs_check"):
            ops.rs_check(a["info"], a["cw"], a["frames"], a["code"], a["rows"], interleave=a["interleave"], crc=a["crc"])
    # the library itself
    keep = []

    def table(v):
        host = np.asarray(v, dtype=np.int32)
        t = torch.from_numpy(host.copy()).to(DEV)
        keep.extend((host, t))
        return [host.shape[0], C.c_void_p(host.ctypes.data), p(t)]

    def code(**kw):
        a = dict(n=40, k=36, fcr=0, prim=1, interleave=2, poly=0x11D)
        a.update(kw)
        c = _lib.RsCode(a["n"], a["k"], a["fcr"], a["prim"], a["interleave"], a["poly"])
        keep.append(c)
        return C.byref(c)
    spec = _lib.FecCrc(16, 0x1021, 0xFFFF, 0, 0, 0)
    lib1 = lambda r=(1, 0), **kw: table(r) + [code(**kw), 5, 2, 85, p(data), 72, p(info), p(cw), None]                 # noqa: E731
    lib2 = lambda r=(1, 0), s=spec, **kw: table(r) + [code(**kw), C.byref(s), 2, 72, p(info), p(cw), p(rows), None]      # noqa: E731
    codes = (dict(n=256), dict(n=36), dict(k=0), dict(n=120, k=55), dict(fcr=-1), dict(fcr=255), dict(prim=0), dict(prim=3), dict(interleave=0), dict(interleave=9), dict(interleave=3),
             dict(poly=0x11B), dict(poly=0x1D))
    for kw in codes:
        with pytest.raises(_lib.Sy11Error, match="rs_decode"):
            _lib.call("sy11_rs_decode", *lib1(**kw))
        if kw != dict(interleave=3):
            with pytest.raises(_lib.Sy11Error, match="rs_check"):
                _lib.call("sy11_rs_check", *lib2(**kw))
    for r in ((0, 2), (-1, 0), (1, 1)):
        with pytest.raises(_lib.Sy11Error, match="rs_decode: frame [01] reads row"):
            _lib.call("sy11_rs_decode", *lib1(r))
        with pytest.raises(_lib.Sy11Error, match="rs_check: frame [01] reads row"):
            _lib.call("sy11_rs_check", *lib2(r))
    for pos, v in ((0, 0), (1, None), (2, None), (3, None), (7, None), (9, None), (10, None), (4, -1), (4, 6), (5, 0), (5, 1), (6, 84), (8, 71), (10, C.c_void_p(cw.data_ptr() + 2))):
        a = lib1()
        a[pos] = v
        with pytest.raises(_lib.Sy11Error, match="rs_decode"):
            _lib.call("sy11_rs_decode", *a)
    for pos, v in ((0, 0), (1, None), (2, None), (3, None), (4, None), (7, None), (8, None), (9, None), (5, 0), (5, 1), (6, 71), (9, C.c_void_p(rows.data_ptr() + 2))):
        a = lib2()
        a[pos] = v
        with pytest.raises(_lib.Sy11Error, match="rs_check"):
            _lib.call("sy11_rs_check", *a)
    for bad in (_lib.FecCrc(7, 7, 0, 0, 0, 0), _lib.FecCrc(12, 7, 0, 0, 0, 0), _lib.FecCrc(40, 7, 0, 0, 0, 0), _lib.FecCrc(8, 0x107, 0, 0, 0, 0), _lib.FecCrc(8, 7, 0, 0, 2, 0)):
        with pytest.raises(_lib.Sy11Error, match="rs_check"):
            _lib.call("sy11_rs_check", *lib2(s=bad))
    torch.cuda.synchronize()
    assert bool((data == DATA_FILL).all()) and bool((info == INFO_FILL).all()) and bool((cw == CW_FILL).all()) and bool((rows == CW_FILL).all())


# ------------------------------------------------------------------------------------------------------------- end to end
E2E_CODE, E2E_I, E2E_CRC, N_INFO = R.code(40, 36), 2, "crc16-ccitt-false", 640
WHITEN = FEC.lfsr_bits((4, 7), [1, 1, 0, 1, 0, 0, 1], N_INFO)
# label, order, sps, M, offset (cycles / sample), snr_db, seed, stream index of the frame, the burst: (first payload symbol, symbols)
E2E = (("bpsk 3.3, clean", 2, 3.3, 4800, 5.3 / 64, 12.0, 61, 60, None), ("qpsk 2.5, burst", 4, 2.5, 2200, 0.02, 12.0, 62, 80, (300, 24)))


@functools.lru_cache(maxsize=None)
def e2e_clips():
    """The two clips: one frame each of 2 x (40, 36) codewords whose 72 information bytes end in a crc16-ccitt-false, whitened, with the tail; in the second, 24
    consecutive payload symbols are sent wrong.  With each the reference chain: what the reference Viterbi decoder makes of it and what the reference
    corrector makes of that (tests/test_correct_cpu.py asserts that the burst breaks the decoder and stays within t).  Computed once; leave it unchanged."""
    from tests._demod_ref import demodulate
    out = []
    for label, order, sps, M, off, snr, seed, at, burst in E2E:
        g = np.random.default_rng(2000 + seed)
        msg = g.integers(0, 256, 70).astype(np.uint8)
        check = FEC.crc(np.unpackbits(msg), FEC.CRCS[E2E_CRC])
        info = np.concatenate((msg, [check >> 8, check & 255])).astype(np.uint8)
        sent = R.interleave(R.encode(info.reshape(E2E_I, 36), E2E_CODE))
        c, _ = FEC.frame_bits(np.unpackbits(sent), None, FEC.POLYS, None, WHITEN, order)
        sym = F.decisions(c, order).copy()
        if burst:
            sym[burst[0]:burst[0] + burst[1]] ^= np.random.default_rng(7).integers(1, order, burst[1]).astype(np.uint8)
        bits = FEC.word_bits(order)
        x, d, u0 = F.clip(order, M, seed, sps, off, snr, {at: np.concatenate((F.decisions(bits, order), sym))}, span=FEC.SPAN)
        T = N_INFO + 6
        need = FEC.n_need(T, None, order)[1]
        case = {"label": label, "x": x, "u0": u0, "sps": sps, "rate": (1.0 / sps - 0.25 * FEC.BIN) * FEC.FS, "offset": (off + FEC.BIN / 16) * FEC.FS, "order": order,
                "bits": bits, "at": at, "msg": msg, "info": info, "sent": sent, "need": need, "burst": burst}
        ref = demodulate(x, FEC.FS, case["rate"], case["offset"], order, span=FEC.SPAN)
        r = ref["r"].astype(np.complex64)
        found = F.find(r, bits, order, FEC.THRESHOLD, need)
        m0 = F.stream_index(ref["T0"], ref["STEP"], ref["i_first"], sps, u0, FEC.SPAN)
        k = found["position"].tolist().index(at - m0)
        y = FEC.soft(r[at - m0 + 32:at - m0 + 32 + need], order, found["rotation"][k], FEC.scale_of(32.0, ref["gain"], order), None, T)
        dec = FEC.decode(y, N_INFO, FEC.POLYS, True, WHITEN, None)
        got, cw = R.correct_rows(dec["data"][None, :], [0], E2E_CODE, E2E_I, 0)
        case.update(ref_decoded=dec["data"], ref_info=got[0], ref_cw=cw[0])
        out.append(case)
    return tuple(out)


def _extraction(clips, fs=FEC.FS, fc=FC):
    from sy11.data.extract import Extraction, ExtractPlan
    n = len(clips)
    M = np.array([len(c) for c in clips], dtype=np.int64)
    plan = ExtractPlan(int(M.sum()) * 64, fs, fc, np.arange(n, dtype=np.int64), np.zeros((n, 4)), np.ones(n, dtype=np.int64), np.zeros(n, dtype=np.int64),
                       1000 * np.arange(n, dtype=np.int64), M)
    return Extraction(plan, torch.from_numpy(np.concatenate(clips)).to(DEV), cls=np.arange(n) % 2, conf=np.linspace(0.5, 0.9, n), names={0: "a", 1: "b"})


@pytest.fixture(scope="module")
def chain():
    """``demodulate`` -> ``find_frames`` -> ``decode`` -> ``correct`` of the two clips, once.  Shared and left unchanged."""
    from sy11 import _lib
    from sy11.engine.model import YOLO
    y = YOLO.__new__(YOLO)
    y.device = DEV
    out = []
    for c in e2e_clips():
        ext = _extraction([c["x"]])
        d = y.demodulate(ext, symbol_rate=[c["rate"]], offset=[c["offset"]], order=[c["order"]], span=FEC.SPAN)
        f = y.find_frames(d, [list(c["bits"])], payload=c["need"], threshold=FEC.THRESHOLD)
        dec = y.decode(f, d, n_info=N_INFO, whiten=WHITEN)
        _lib.PROFILE = []
        try:
            cor = y.correct(dec, code=E2E_CODE, interleave=E2E_I, crc=E2E_CRC)
            calls = [k[0] for k in _lib.PROFILE]
        finally:
            _lib.PROFILE = None
        assert calls == ["sy11_rs_decode", "sy11_rs_check"]                     # two launches, whatever the number of frames
        out.append((c, ext, d, f, dec, cor))
    return y, out


def test_demodulate_find_frames_decode_correct_reads_what_was_sent(chain):
    from sy11.data.correct import Corrected
    y, cases = chain
    for c, ext, d, f, dec, cor in cases:
        assert isinstance(cor, Corrected) and len(cor) == len(dec) >= 1 and cor.data.device.type == "cuda" and cor.data.shape == (len(dec), 72) and cor.errors.shape == (len(dec), 2)
        assert np.array_equal(cor.clip, dec.clip) and np.array_equal(cor.word, dec.word) and np.array_equal(cor.position, dec.position) and np.array_equal(cor.valid, dec.valid)
        assert cor.cls.tolist() == ext.cls.tolist() and cor.names == ext.names
        # the reference on the decoder's own bytes: every column, exactly
        v = np.flatnonzero(dec.valid)
        data = dec.data.cpu().numpy()
        want_info, want_cw = R.correct_rows(data, v, E2E_CODE, E2E_I, 0)
        got = cor.data.cpu().numpy()
        assert np.array_equal(got[v], want_info) and np.array_equal(cor.errors[v], want_cw[:, :, 0]) and not got[~dec.valid].any()
        for j, k in enumerate(v):
            want = R.check(want_info[j], want_cw[j], FEC.crc, FEC.CRCS[E2E_CRC])
            assert [int(getattr(cor, a)[k]) for a in ("n_failed", "byte_errors", "bit_errors", "crc_calc", "crc_recv")] == want[:5] and bool(cor.crc_ok[k]) == bool(want[5])
            assert bool(cor.ok[k]) == (want[0] == 0) and cor[int(k)]["errors"] == want_cw[j, :, 0].tolist() and cor.reason[k] == ""
        for k in np.flatnonzero(~dec.valid):
            assert cor.reason[k] == "undecoded" and not cor.ok[k] and not cor.crc_ok[k] and cor.errors[k].tolist() == [0, 0]
        # the embedded frame reads as it was sent
        m0 = F.stream_index(d.raw["T0"][0], d.raw["STEP"][0], d.raw["i_first"][0], c["sps"], c["u0"], FEC.SPAN)
        k = np.flatnonzero(f.position == c["at"] - m0)
        assert k.shape[0] == 1
        k = int(k[0])
        assert cor.valid[k] and cor.ok[k] and cor.crc_ok[k] and cor.message(k) == c["msg"].tobytes() and np.array_equal(got[k], c["info"])
        if c["burst"]:
            assert cor.byte_errors[k] > 0 and cor.bit_errors[k] >= cor.byte_errors[k] and not np.array_equal(data[k, :80], c["sent"]) and cor.errors[k].max() <= 2
        else:
            assert cor.byte_errors[k] == 0 and np.array_equal(data[k, :80], c["sent"])
        print(f"correct[{c['label']}]: {len(cor)} frames, {int(cor.valid.sum())} valid, the embedded frame's codewords had {cor.errors[k].tolist()} byte errors")


def test_save_round_trip_invalid_and_empty_decoded(chain, tmp_path):
    from sy11 import _lib
    from sy11.engine.predictor import DetectionPredictor
    y, cases = chain
    c, ext, d, f, dec, cor = cases[1]
    out = cor.save(tmp_path / "c")
    z = np.load(tmp_path / "c" / "correct.npz")
    index = json.loads((tmp_path / "c" / "correct.json").read_text())
    assert out == str(tmp_path / "c")
    for key in cor.COLUMNS:
        assert np.array_equal(z[key], getattr(cor, key)), key
    assert np.array_equal(z["data"], cor.data.cpu().numpy()) and np.array_equal(z["errors"], cor.errors) and z["reason"].tolist() == [str(r) for r in cor.reason]
    k = int(np.flatnonzero(cor.ok)[0])
    assert index["code"]["n"] == 40 and index["interleave"] == 2 and index["offset"] == 0 and index["crc"]["name"] == E2E_CRC and len(index["frames"]) == len(cor)
    assert index["frames"][k]["message"] == cor.message(k).hex() and index["frames"][k]["ok"] is True and index["frames"][k]["errors"] == cor.errors[k].tolist()
    # the predictor's method, without a check: crc_ok all True, the message is every byte
    pred = DetectionPredictor.__new__(DetectionPredictor)
    pred.device = DEV
    plain = pred.correct(dec, code=E2E_CODE, interleave=E2E_I)
    assert plain.crc_ok[plain.valid].all() and not plain.crc_calc.any() and np.array_equal(plain.data.cpu().numpy(), cor.data.cpu().numpy()) and plain.message(k) == c["info"].tobytes()
    # a Decoded with an invalid frame among valid ones: that row is zeros, the others are as before
    part = copy.copy(dec)
    part.valid = dec.valid.copy()
    part.valid[k] = False
    some = y.correct(part, code=E2E_CODE, interleave=E2E_I, crc=E2E_CRC)
    assert not some.valid[k] and some.reason[k] == "undecoded" and not some.data[k].any().item() and not some.ok[k] and some.errors[k].tolist() == [0, 0]
    rest = np.setdiff1d(np.arange(len(dec)), [k])
    assert np.array_equal(some.data.cpu().numpy()[rest], cor.data.cpu().numpy()[rest]) and np.array_equal(some.errors[rest], cor.errors[rest])
    # argument errors come before the device; an empty Decoded, or one without a valid frame, launches nothing
    none = y.find_frames(d, [[0, 1] * 40], payload=c["need"], threshold=0.9)
    empty = y.decode(none, d, n_info=N_INFO, whiten=WHITEN)
    deaf = copy.copy(dec)
    deaf.valid = np.zeros_like(dec.valid)
    _lib.PROFILE = []
    try:
        with pytest.raises(ValueError, match="beyond"):
            y.correct(dec, code=E2E_CODE, interleave=3)
        with pytest.raises(ValueError, match="not one of"):
            y.correct(dec, code="rs-nope")
        e = y.correct(empty, code=E2E_CODE, interleave=E2E_I, crc=E2E_CRC)
        g = y.correct(deaf, code=E2E_CODE, interleave=E2E_I, crc=E2E_CRC)
        calls = [k[0] for k in _lib.PROFILE]
    finally:
        _lib.PROFILE = None
    assert calls == [] and len(empty) == 0 and len(e) == 0 and e.data.shape == (0, 72) and e.errors.shape == (0, 2) and e.valid.shape == (0,) and e.raw["cw"] is None
    assert len(g) == len(dec) and not g.valid.any() and set(g.reason.tolist()) == {"undecoded"} and not g.data.any().item() and not g.ok.any() and g.raw["rows"] is None
