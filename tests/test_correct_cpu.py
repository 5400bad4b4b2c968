"""CPU: the Reed-Solomon reference (tests/_rs_ref.py) pinned to anchors that need no outside source and to the definition by brute force on a tiny code;
the package's host side (``sy11.data.correct``: presets, tables, generator, encoder, ``plan_correct``) against it; and the library's refusals, which all come
before a launch and so run without a device."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

from tests import _rs_ref as R

EXTRA = {"255-253": R.code(255, 253, fcr=1), "40-36": R.code(40, 36), "60-55": R.code(60, 55, fcr=3, prim=7), "20-19": R.code(20, 19)}


def _all_codes():
    return dict(R.CODES, **EXTRA)


# ------------------------------------------------------------------------------------------------------------- anchors
def test_presets_and_generators():
    from sy11.data import correct as K
    assert K.CODES == R.CODES and list(K.CODES) == ["dvb-204-188", "rs-255-239", "ccsds-255-223", "ccsds-255-239"]
    # DVB's published generator, x^16 + 59 x^15 + ... + 59
    dvb = [1, 59, 13, 104, 189, 68, 209, 30, 8, 163, 65, 41, 229, 98, 50, 36, 59]
    assert R.generator(R.CODES["rs-255-239"]) == dvb and K.rs_generator("rs-255-239").tolist() == dvb and K.rs_generator("dvb-204-188").tolist() == dvb
    g = R.generator(R.CODES["ccsds-255-223"])
    assert len(g) == 33 and g == g[::-1] and K.rs_generator("ccsds-255-223").tolist() == g          # palindromic
    for name, cd in _all_codes().items():
        assert K.rs_generator(name if name in R.CODES else cd).tolist() == R.generator(cd), name
        assert R.order_of_x(cd["poly"]) == 255
    assert K.rs_generator("ccsds-255-223").dtype == np.uint8


def test_field_tables_against_the_slow_product():
    from sy11.data.correct import gf_tables
    g = np.random.default_rng(2)
    for poly in (0x11D, 0x187):
        exp, log = gf_tables(poly)
        assert exp.shape == (512,) and log.shape == (256,) and exp.dtype == np.uint8 and sorted(exp[:255].tolist()) == list(range(1, 256))
        assert np.array_equal(exp[:255], exp[255:510]) and exp[0] == 1 and exp[1] == 2 and log[0] == 0 and log[1] == 0 and log[2] == 1
        a, b = g.integers(1, 256, 500), g.integers(1, 256, 500)
        assert np.array_equal(exp[log[a].astype(int) + log[b].astype(int)], R.gf_mul(a, b, poly))
        assert [R.mul(int(x), int(y), poly) for x, y in zip(a[:50], b[:50])] == R.gf_mul(a[:50], b[:50], poly).tolist()
    for bad, what in ((0x11B, "not primitive"), (0x100, "not primitive"), (0xFF, "9 bits"), (0x200, "9 bits"), (285.0, "9 bits"), (True, "9 bits")):
        with pytest.raises(ValueError, match=what):
            gf_tables(bad)


def test_encoders_agree_and_codewords_have_zero_syndromes():
    from sy11.data.correct import rs_encode
    g = np.random.default_rng(3)
    for name, cd in _all_codes().items():
        for I in (1, 3):
            msg = g.integers(0, 256, I * cd["k"]).astype(np.uint8)
            sent = rs_encode(msg, name if name in R.CODES else cd, I)
            cws = R.deinterleave(sent, I)
            assert sent.dtype == np.uint8 and sent.shape == (I * cd["n"],) and cws.shape == (I, cd["n"])
            assert np.array_equal(cws, R.encode(msg.reshape(I, cd["k"]), cd)) and np.array_equal(cws[:, :cd["k"]].reshape(-1), msg)     # systematic, codeword-major
            assert not R.syndromes(cws, cd).any(), name
            assert np.array_equal(R.interleave(cws), sent) and sent[1 % len(sent)] == cws[1 % I, 1 // I]
    assert np.array_equal(rs_encode(bytes(range(36)), EXTRA["40-36"]), rs_encode(np.arange(36), EXTRA["40-36"]))
    for bad in (dict(message_bytes=np.zeros(35, dtype=np.uint8)), dict(message_bytes=np.zeros((1, 36), dtype=np.uint8)), dict(message_bytes=np.full(36, 256)),
                dict(message_bytes=np.zeros(36)), dict(interleave=0), dict(interleave=9), dict(code="rs-1-2"), dict(code=dict(EXTRA["40-36"], k=40))):
        a = dict(message_bytes=np.zeros(36, dtype=np.uint8), code=EXTRA["40-36"], interleave=1)
        a.update(bad)
        with pytest.raises(ValueError, match="rs_encode"):
            rs_encode(**a)


# ------------------------------------------------------------------------------------------------------------- the reference against the definition
def test_reference_equals_nearest_codeword_search_on_a_tiny_code():
    """(15, 11) over GF(2^8), t = 2: whether a codeword lies within 2 bytes of r is decided by brute force over every error pattern of weight <= 2, through the
    syndromes of the patterns under the slow product (r ^ e is a codeword iff e has r's syndromes)."""
    cd = R.code(15, 11, fcr=1)
    n, poly = 15, cd["poly"]
    unit = np.zeros((n, n), dtype=np.uint8)
    unit[np.arange(n), np.arange(n)] = 1
    s1 = R.syndromes(unit, cd)                                                 # of the pattern with a 1 at byte i
    pack = lambda S: (np.asarray(S, dtype=np.int64) << (8 * np.arange(4))).sum(axis=-1)          # noqa: E731  (the four syndromes as one integer)
    keys = pack(R.gf_mul(s1[:, None, :], np.arange(1, 256)[None, :, None], poly))                # of value v at byte i: linear in v
    single = {int(keys[i, v - 1]): (i, v) for i in range(n) for v in range(1, 256)}
    assert len(single) == n * 255
    g = np.random.default_rng(4)
    msg = g.integers(0, 256, (300, 11))
    sent = R.encode(msg, cd)
    rx = sent.copy()
    count = g.integers(0, 6, 300)                                              # 0 .. 5 byte errors
    for w in range(300):
        at = g.choice(n, count[w], replace=False)
        rx[w, at] ^= g.integers(1, 256, count[w]).astype(np.uint8)
    info, cw = R.decode(rx, cd)
    S = R.syndromes(rx, cd)
    seen = {"exact": 0, "failed": 0, "other": 0}
    for w in range(300):
        want, s = None, int(pack(S[w]))
        if s == 0:
            want = {}
        elif s in single:
            i, v = single[s]
            want = {i: v}
        else:
            for key, (i, v) in single.items():
                other = single.get(s ^ key)
                if other is not None and other[0] != i:
                    want = {i: v, other[0]: other[1]}
                    break
        if want is None:
            assert cw[w].tolist() == [-1, 0] and np.array_equal(info[w], rx[w, :11]), w
            seen["failed"] += 1
            continue
        c = rx[w].copy()
        for i, v in want.items():
            c[i] ^= v
        assert cw[w].tolist() == [len(want), sum(bin(v).count("1") for v in want.values())] and np.array_equal(info[w], c[:11]), w
        seen["exact" if np.array_equal(c, sent[w]) else "other"] += 1
        if count[w] <= 2:
            assert np.array_equal(c, sent[w]) and len(want) == count[w]
    print(f"(15, 11): {seen}")
    assert seen["failed"] > 50 and seen["exact"] >= int((count <= 2).sum())


def test_reference_corrects_up_to_t_and_accepts_only_codewords():
    g = np.random.default_rng(5)
    for name, cd in _all_codes().items():
        n, k = cd["n"], cd["k"]
        t = (n - k) // 2
        W = 12 if n - k > 8 else 40
        msg = g.integers(0, 256, (W, k))
        sent = R.encode(msg, cd)
        rx = sent.copy()
        count = np.resize(np.arange(t + 4), W)
        for w in range(W):
            at = g.choice(n, count[w], replace=False)
            rx[w, at] ^= g.integers(1, 256, count[w]).astype(np.uint8)
        info, cw = R.decode(rx, cd)
        low = count <= t
        assert np.array_equal(info[low], msg[low]) and np.array_equal(cw[low, 0], count[low]), name
        assert np.array_equal(cw[low, 1], np.unpackbits(rx[low] ^ sent[low], axis=1).sum(axis=1))
        assert ((cw[~low, 0] == -1) | (cw[~low, 0] <= t)).all() and (cw[cw[:, 0] < 0, 1] == 0).all()
        if t == 0:
            assert np.array_equal(info, rx[:, :k])                             # detection only: nothing changes (a word may land on another codeword: 0 errors)


# ------------------------------------------------------------------------------------------------------------- the plan
def _decoded(n_info=8 * 100, valid=(True, False, True)):
    n = len(valid)
    return SimpleNamespace(plan=SimpleNamespace(n_info=n_info), valid=np.array(valid, dtype=bool), data=None, clip=np.arange(n), word=np.zeros(n, dtype=np.int64),
                           position=10 * np.arange(n), rows=None, cls=None, conf=None, names=None)


def test_plan_correct_columns_and_reasons():
    from sy11.data.correct import CorrectPlan, plan_correct
    p = plan_correct(_decoded(), code=EXTRA["40-36"], interleave=2, offset=3, crc="crc16-ccitt-false")
    assert isinstance(p, CorrectPlan) and len(p) == 3 and p.valid.tolist() == [True, False, True] and p.reason.tolist() == ["", "undecoded", ""]
    assert (p.n, p.k, p.nroots, p.t, p.interleave, p.offset, p.n_bytes) == (40, 36, 4, 2, 2, 3, 72) and p.code["name"] is None and p.crc["name"] == "crc16-ccitt-false"
    assert "2 x RS(40, 36)" in repr(p)
    q = plan_correct(_decoded(8 * 204, valid=()), interleave=1)
    assert len(q) == 0 and q.code == dict(R.CODES["dvb-204-188"], name="dvb-204-188") and q.crc is None and q.t == 8
    assert plan_correct(_decoded(8 * 1020 + 3), code="ccsds-255-223", interleave=4).n_bytes == 892
    assert plan_correct(_decoded(8 * 20), code=EXTRA["20-19"]).t == 0
    plan_correct(_decoded(8 * 100), code=EXTRA["40-36"], interleave=2, offset=20)      # the block ends with the frame


def test_plan_correct_argument_errors():
    from sy11.data.correct import plan_correct
    from sy11.data.decode import CRCS
    c = EXTRA["40-36"]
    good = dict(code=c, interleave=2, offset=0, crc=None)
    for kw, what in ((dict(code="rs-nope"), "not one of"), (dict(code=7), "name of CODES"), (dict(code=dict(n=40, k=36)), "holds n, k"), (dict(code=dict(c, extra=1)), "holds n, k"),
                     (dict(code=dict(c, poly=0x11B)), "not primitive"), (dict(code=dict(c, poly=0x1D)), "9 bits"), (dict(code=dict(c, prim=3)), "prim"),
                     (dict(code=dict(c, prim=0)), "prim"), (dict(code=dict(c, prim=255)), "prim"), (dict(code=dict(c, prim=85)), "prim"), (dict(code=dict(c, n=256)), "n and k"),
                     (dict(code=dict(c, k=40)), "n and k"), (dict(code=dict(c, k=0)), "n and k"), (dict(code=dict(c, k=41)), "n and k"), (dict(code=dict(c, n=40.0)), "integer"),
                     (dict(code=dict(c, n=120, k=55), interleave=1), "nroots"), (dict(code=dict(c, fcr=-1)), "fcr"), (dict(code=dict(c, fcr=255)), "fcr"),
                     (dict(code=dict(c, fcr=True)), "integer"), (dict(interleave=0), "interleave"), (dict(interleave=9), "interleave"), (dict(interleave=2.0), "interleave"),
                     (dict(offset=-1), "offset"), (dict(offset=1.0), "offset"), (dict(offset=21), "beyond"), (dict(interleave=3), "beyond"), (dict(code="dvb-204-188"), "beyond"),
                     (dict(crc="crc-nope"), "crc"), (dict(crc=dict(width=16)), "crc"), (dict(crc=dict(CRCS["crc8"], width=12, poly=7)), "whole bytes"),
                     (dict(crc=dict(CRCS["crc8"], width=33)), "width"), (dict(crc=dict(CRCS["crc8"], poly=0x107)), "poly"),
                     (dict(code=R.code(3, 2), interleave=1, crc="crc16-x25"), "not shorter"), (dict(code=R.code(5, 4), interleave=1, crc="crc32"), "not shorter")):
        a = dict(good)
        a.update(kw)
        with pytest.raises(ValueError, match=what):
            plan_correct(_decoded(), **a)
    plan_correct(_decoded(), code=R.code(5, 4), interleave=1, crc="crc16-x25")         # 32 information bits, a check of 16
    with pytest.raises(ValueError, match="Decoded"):
        plan_correct(SimpleNamespace(valid=np.ones(1, dtype=bool)), code=c)


# ------------------------------------------------------------------------------------------------------------- the library's refusals
def test_library_refuses_before_any_launch():
    """Every check of the two entry points returns -1 before a launch, so it runs without a device; the pointers are never followed."""
    from sy11 import _lib
    lib = _lib.load()
    row = np.array([1, 0], dtype=np.int32)
    host, fake = C.c_void_p(row.ctypes.data), C.c_void_p(0x1000)
    keep = []

    def table(*v):
        t = np.array(v, dtype=np.int32)
        keep.append(t)
        return C.c_void_p(t.ctypes.data)

    def code(**kw):
        a = dict(n=40, k=36, fcr=0, prim=1, interleave=2, poly=0x11D)
        a.update(kw)
        c = _lib.RsCode(a["n"], a["k"], a["fcr"], a["prim"], a["interleave"], a["poly"])
        keep.append(c)
        return C.byref(c)
    crc = _lib.FecCrc(16, 0x1021, 0xFFFF, 0, 0, 0)
    dec = lambda: [2, host, fake, code(), 5, 2, 85, fake, 72, fake, fake, None]                            # noqa: E731
    chk = lambda: [2, host, fake, code(), C.byref(crc), 2, 72, fake, fake, fake, None]                      # noqa: E731
    codes = (dict(n=256), dict(n=36), dict(k=0), dict(n=120, k=55), dict(fcr=-1), dict(fcr=255), dict(prim=0), dict(prim=3), dict(prim=255), dict(interleave=0),
             dict(interleave=9), dict(poly=0x11B), dict(poly=0x1D), dict(poly=0x31D))
    rows = ((2, 0), (-1, 0), (1, 1))
    cases = [("sy11_rs_decode", dec, [(0, 0), (1, None), (2, None), (3, None), (7, None), (9, None), (10, None), (4, -1), (4, 6), (5, 0), (5, 1), (6, 84), (6, 0), (8, 71),
                                     (2, C.c_void_p(0x1002)), (10, C.c_void_p(0x1002))]),
             ("sy11_rs_check", chk, [(0, 0), (1, None), (2, None), (3, None), (4, None), (7, None), (8, None), (9, None), (5, 0), (5, 1), (6, 71), (2, C.c_void_p(0x1001)),
                                    (8, C.c_void_p(0x1002)), (9, C.c_void_p(0x1002))])]
    for name, args, positional in cases:
        fn = getattr(lib, name)
        for pos, v in positional:
            a = args()
            a[pos] = v
            assert fn(*a) == -1, (name, pos, v)
            assert name[5:].encode() in lib.sy11_last_error()
        for kw in codes:
            a = args()
            a[3] = code(**kw)
            assert fn(*a) == -1, (name, kw)
        for r in rows:
            a = args()
            a[1] = table(*r)
            assert fn(*a) == -1 and b"row" in lib.sy11_last_error(), (name, r)
    for bad in (_lib.FecCrc(7, 7, 0, 0, 0, 0), _lib.FecCrc(12, 7, 0, 0, 0, 0), _lib.FecCrc(40, 7, 0, 0, 0, 0), _lib.FecCrc(8, 0x107, 0, 0, 0, 0), _lib.FecCrc(8, 7, 0x100, 0, 0, 0),
                _lib.FecCrc(8, 7, 0, 0x100, 0, 0), _lib.FecCrc(8, 7, 0, 0, 2, 0), _lib.FecCrc(8, 7, 0, 0, 0, -1)):
        a = chk()
        a[4] = C.byref(bad)
        assert lib.sy11_rs_check(*a) == -1 and b"rs_check" in lib.sy11_last_error(), (bad.width, bad.poly)
    a = chk()
    a[3], a[6], a[4] = code(n=3, k=2, interleave=1), 2, C.byref(_lib.FecCrc(16, 0x1021, 0, 0, 0, 0))       # 16 information bits do not exceed a check of 16
    assert lib.sy11_rs_check(*a) == -1 and b"do not exceed" in lib.sy11_last_error()


# ------------------------------------------------------------------------------------------------------------- end to end
def test_reference_chain_the_burst_breaks_the_viterbi_decoder_and_stays_within_t():
    """The two clips the GPU test runs on the device, on the reference chain: the clean frame decodes as sent; in the other the Viterbi decoder leaves
    wrong bytes, at most t = 2 of a codeword, and the outer code reads what was sent."""
    from tests.test_correct_gpu import E2E_I, e2e_clips
    clean, burst = e2e_clips()
    assert np.array_equal(clean["ref_decoded"], clean["sent"]) and clean["ref_cw"].tolist() == [[0, 0], [0, 0]]
    wrong = np.flatnonzero(burst["ref_decoded"] != burst["sent"])
    print(f"correct[{burst['label']}]: the reference decoder leaves bytes {wrong.tolist()} wrong, codeword errors {burst['ref_cw'][:, 0].tolist()}")
    assert wrong.tolist() == [37, 38, 39] and wrong.max() - wrong.min() < 2 * E2E_I and burst["ref_cw"][:, 0].tolist() == [1, 2]
    for c in (clean, burst):
        assert np.array_equal(c["ref_info"], c["info"]) and c["ref_info"][:70].tobytes() == c["msg"].tobytes()
