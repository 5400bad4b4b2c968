"""CPU: the frame decoder's definition from the reference alone (tests/_fec_ref.py: the anchors of the code, the checks and the scrambler; the
invariants of the Viterbi decoder at every trellis length that takes another path on the device; noiseless round trips through every option; the
three end-to-end clips through the reference demodulation and frame search), the host side of sy11/data/decode.py (``lfsr_bits``, ``CRCS``, every
``ValueError`` of ``plan_decode`` and every per-frame reason, the record layout) and the library's refusals, which return before any launch.  Nothing here
touches a device."""
import binascii
import ctypes as C
import zlib
from types import SimpleNamespace

import numpy as np
import pytest

from tests import _fec_ref as R
from tests import _frames_ref as F


# ------------------------------------------------------------------------------------------------------------- anchors
def test_anchors_impulse_response_crcs_and_scrambler():
    assert "".join(str(b) for b in R.encode([1])) == "11101111000111"          # 11 10 11 11 00 01 11
    msg = R.bits_of_bytes(b"123456789")
    got = {k: R.crc(msg, s) for k, s in R.CRCS.items()}
    assert got == {"crc32": 0xCBF43926, "crc16-ccitt-false": 0x29B1, "crc16-x25": 0x906E, "crc8": 0xF4}
    g = np.random.default_rng(5)
    for n in (1, 2, 33):
        b = g.integers(0, 256, n).astype(np.uint8).tobytes()
        assert R.crc(R.bits_of_bytes(b), R.CRCS["crc32"]) == zlib.crc32(b) and R.crc(R.bits_of_bytes(b), R.CRCS["crc16-ccitt-false"]) == binascii.crc_hqx(b, 0xFFFF)
    s = R.lfsr_bits((4, 7), [1] * 7, 254)
    assert "".join(str(b) for b in s[:32]) == "00001110111100101100100100000010" and np.array_equal(s[:127], s[127:]) and int(s[:127].sum()) == 64


def test_the_package_agrees_on_scrambler_and_crc_table():
    from sy11.data import decode as D
    assert np.array_equal(D.lfsr_bits((4, 7), [1] * 7, 200), R.lfsr_bits((4, 7), [1] * 7, 200)) and D.lfsr_bits((4, 7), [1] * 7, 3).dtype == np.uint8
    assert np.array_equal(D.lfsr_bits((3, 5), [1, 0, 0, 1, 0], 64), R.lfsr_bits((3, 5), [1, 0, 0, 1, 0], 64))
    for k, spec in R.CRCS.items():
        assert D.CRCS[k] == spec
    for bad in (((0,), [1, 1]), ((3,), [1, 1]), ((1,), []), ((1,), [2])):
        with pytest.raises(ValueError):
            D.lfsr_bits(*bad, 4)
    assert D.t_max() == R.T_MAX == 8192
    from sy11 import _lib
    assert D.FECFRAME.itemsize == 32 and C.sizeof(_lib.FecCrc) == 24


# ------------------------------------------------------------------------------------------------------------- invariants
def _inputs(T, tail, seed):
    g = np.random.default_rng(seed)
    u = g.integers(0, 2, T - 6 * tail)
    c = R.encode(u, R.POLYS, tail).astype(np.float64)
    noisy = R.quantize((1.0 - 2.0 * c) + 0.7 * g.standard_normal(2 * T), 32.0)
    return {"uniform": g.integers(-127, 128, 2 * T).astype(np.int8), "zero": np.zeros(2 * T, dtype=np.int8),
            "full": (127 * (1 - 2 * g.integers(0, 2, 2 * T))).astype(np.int8), "noisy": noisy}


@pytest.mark.parametrize("T", [1, 6, 7, 64, 65, 8192])
def test_viterbi_reference_invariants(T):
    for tail in (False, True):
        if tail and T < 7:
            continue
        for kind, y in _inputs(T, tail, 10 * T + tail).items():
            u, metric, end, start = R.viterbi(y, R.POLYS, tail, start=True)
            assert start == 0, (kind, tail)                                    # the traceback lands in the state the encoder starts in
            c = R.encode(u, R.POLYS, tail=False).astype(np.int64)
            assert metric == int(((1 - 2 * c) * y.astype(np.int64)).sum()), (kind, tail)
            if tail:
                assert end == 0 and not u[T - 6:].any()
            if kind == "zero":
                assert not u.any() and metric == 0 and end == 0               # every comparison ties: b = 0 throughout, the lowest state
            batch = R.viterbi(np.stack((y, y[::-1].copy())), R.POLYS, tail)
            assert np.array_equal(batch[0][0], u) and batch[1][0] == metric and batch[2][0] == end


# ------------------------------------------------------------------------------------------------------------- round trips
WHITEN = R.lfsr_bits((4, 7), [1, 0, 1, 1, 1, 0, 1], 400)


@pytest.mark.parametrize("crc", [None] + list(R.CRCS))
@pytest.mark.parametrize("pattern", [None, R.P64])
@pytest.mark.parametrize("whiten", [None, WHITEN], ids=["plain", "whitened"])
def test_noiseless_round_trip_and_one_flipped_bit(crc, pattern, whiten):
    spec = None if crc is None else R.CRCS[crc]
    u = np.random.default_rng(7).integers(0, 2, 96).astype(np.uint8)
    c, info = R.frame_bits(u, spec, R.POLYS, pattern, whiten, order=2)
    n_info = info.shape[0]
    assert n_info == 96 + (spec["width"] if spec else 0)
    y = R.depuncture(R.quantize(1.0 - 2.0 * c.astype(np.float32), 32.0), pattern, n_info + 6)
    d = R.decode(y, n_info, R.POLYS, True, whiten, spec)
    assert np.array_equal(d["v"], info) and d["channel_errors"] == 0 and d["n_channel"] == c.shape[0] and d["end_state"] == 0
    assert d["metric"] == 32 * c.shape[0] and np.array_equal(np.unpackbits(d["data"])[:n_info], info)
    assert d["crc_ok"] == (-1 if spec is None else 1)
    if spec is not None:
        bad = u.copy()
        bad[17] ^= 1
        info2 = np.concatenate((bad, info[96:]))                                # the message changed, the check field not
        sent = info2 ^ (whiten[:n_info] if whiten is not None else 0)
        y2 = R.depuncture(R.quantize(1.0 - 2.0 * R.puncture(R.encode(sent, R.POLYS, True), pattern).astype(np.float32), 32.0), pattern, n_info + 6)
        d2 = R.decode(y2, n_info, R.POLYS, True, whiten, spec)
        assert np.array_equal(d2["v"], info2) and d2["crc_ok"] == 0 and d2["crc_recv"] == d["crc_recv"] and d2["crc_calc"] != d["crc_calc"]


def test_quantizer_ties_saturation_and_nan():
    x = np.array([0.5, 1.5, 2.5, -0.5, -1.5, 126.5, 127.5, 1e9, -1e9, np.inf, -np.inf, np.nan, 0.49999997], dtype=np.float32)
    assert R.quantize(x, 1.0).tolist() == [0, 2, 2, 0, -2, 126, 127, 127, -127, 127, -127, 0, 0]


# ------------------------------------------------------------------------------------------------------------- the plan
def _frames(n_symbols, order, payload, clip, position, rotation=None, n_payload=None, bits=32):
    """A ``Frames`` stand-in over a real ``FramePlan``: what ``plan_decode`` reads of it."""
    from sy11.data.frames import plan_frames
    word = [int(b) for b in np.random.default_rng(1).integers(0, 2, bits)]
    plan = plan_frames((np.asarray(n_symbols), np.asarray(order)), [word], payload, 0.6)
    clip, position = np.asarray(clip, dtype=np.int64), np.asarray(position, dtype=np.int64)
    L = plan.L[clip, 0]
    n_pay = np.minimum(payload, plan.n_symbols[clip] - position - L) if n_payload is None else np.asarray(n_payload)
    return SimpleNamespace(plan=plan, clip=clip, word=np.zeros_like(clip), position=position, rotation=np.zeros_like(clip) if rotation is None else np.asarray(rotation),
                           n_payload=n_pay, rows=None, cls=None, conf=None, names=None)


def _demod(n_symbols, order, gain):
    return SimpleNamespace(n_symbols=np.asarray(n_symbols, dtype=np.int64), order=np.asarray(order, dtype=np.int64), gain=np.asarray(gain, dtype=np.float64),
                           valid=np.ones(len(gain), dtype=bool))


def test_plan_decode_columns_and_reasons():
    from sy11.data.decode import plan_decode
    ns, order = [600, 600, 600, 600, 600, 600], [2, 4, 2, 2, 2, 4]
    gain = [2.0, 1.5, 0.0, np.nan, -1.0, np.inf]
    f = _frames(ns, order, 212, clip=[0, 0, 1, 1, 2, 3, 4, 5], position=[10, 500, 3, 490, 0, 0, 0, 0])
    p = plan_decode(f, _demod(ns, order, gain), n_info=100, crc="crc16-ccitt-false")
    assert (p.T, p.n_coded, p.period, p.mask) == (106, 212, 2, 3) and p.n_need.tolist() == [212, 212, 106, 106, 212, 212, 212, 106]
    assert p.reason.tolist() == ["", "short", "", "short", "gain", "gain", "gain", "gain"] and p.valid.tolist() == [True, False, True, False, False, False, False, False]
    assert p.sym_off.tolist() == [10 + 32, 500 + 32, 600 + 3 + 16, 600 + 490 + 16, 1200 + 32, 1800 + 32, 2400 + 32, 3000 + 16]
    assert p.scale.dtype == np.float32 and p.scale[0] == np.float32(16.0) and p.scale[2] == R.scale_of(32.0, 1.5, 4) and p.scale[2] == np.float32(32.0 / (1.5 / np.sqrt(2.0)))
    assert p.crc["width"] == 16 and p.crc["name"] == "crc16-ccitt-false" and p.whiten is None and p.pattern is None
    fr, at = p.table(f.rotation, f.plan.order[f.clip])
    assert at.tolist() == [0, 2] and fr["row"].tolist() == [0, 2] and fr["T"].tolist() == [106, 106] and fr["tail"].tolist() == [1, 1] and fr["order"].tolist() == [2, 4]
    # punctured: 4 of every 6 mother bits; the 64-long pattern; no tail
    p = plan_decode(f, _demod(ns, order, gain), n_info=100, puncture=R.P64)
    assert (p.n_coded, p.period, p.mask) == (int(R.sent_mask(R.P64, 212).sum()), 6, 0b011011) and p.n_need[0] == p.n_coded and p.n_need[2] == -(-p.n_coded // 2)
    pat = np.random.default_rng(2).integers(0, 2, 64)
    p = plan_decode(f, _demod(ns, order, gain), n_info=100, puncture=pat, tail=False, whiten=np.ones(130, dtype=np.int64))
    assert (p.T, p.period) == (100, 64) and p.n_coded == int(np.resize(pat, 200).sum()) and p.mask == sum(int(b) << i for i, b in enumerate(pat)) and p.whiten.shape == (100,)
    empty = _frames(ns, order, 212, clip=[], position=[])
    p = plan_decode(empty, _demod(ns, order, gain), n_info=100)
    assert len(p) == 0 and p.valid.shape == (0,)


def test_plan_decode_argument_errors():
    from sy11.data.decode import plan_decode
    ns, order, gain = [600, 600], [2, 4], [1.0, 1.0]
    f, d = _frames(ns, order, 212, clip=[0, 1], position=[10, 10]), _demod(ns, order, gain)
    good = dict(n_info=100)
    for kw, what in ((dict(n_info=0), "n_info"), (dict(n_info=8187), "n_info"), (dict(n_info=8193, tail=False), "n_info"), (dict(n_info=10.0), "n_info"), (dict(n_info=True), "n_info"),
                     (dict(tail=1), "tail"), (dict(polys=(0o171,)), "polys"), (dict(polys=(0o171, 0o132)), "polys"), (dict(polys=(0o71, 0o133)), "polys"),
                     (dict(polys=(0o371, 0o133)), "polys"), (dict(polys=7), "polys"), (dict(polys=(0o171, 91.0)), "polys"),
                     (dict(puncture=(1, 1, 0)), "puncture"), (dict(puncture=(0, 0)), "puncture"), (dict(puncture=(1, 2)), "puncture"), (dict(puncture=[1] * 66), "puncture"),
                     (dict(puncture=()), "puncture"), (dict(puncture="11"), "puncture"), (dict(puncture=[[1, 1]]), "puncture"),
                     (dict(whiten=[1] * 99), "whiten"), (dict(whiten=[2] * 100), "whiten"), (dict(whiten=[0.0] * 100), "whiten"),
                     (dict(crc="crc-nope"), "crc"), (dict(crc=7), "crc"), (dict(crc=dict(width=16)), "crc"), (dict(crc=dict(R.CRCS["crc8"], width=7)), "width"),
                     (dict(crc=dict(R.CRCS["crc8"], width=33)), "width"), (dict(crc=dict(R.CRCS["crc8"], poly=0x107)), "poly"), (dict(crc=dict(R.CRCS["crc8"], init=-1)), "init"),
                     (dict(crc=dict(R.CRCS["crc8"], refin=2)), "refin"), (dict(crc=dict(R.CRCS["crc8"], xorout=256)), "xorout"),
                     (dict(n_info=16, crc="crc16-x25"), "exceed"), (dict(n_info=100, crc="crc16-x25"), "whole bytes"), (dict(n_info=100, crc="crc32"), "whole bytes"),
                     (dict(soft_scale=0.0), "soft_scale"), (dict(soft_scale=127.5), "soft_scale"), (dict(soft_scale=float("nan")), "soft_scale"), (dict(soft_scale=None), "soft_scale"),
                     (dict(soft_scale=-1), "soft_scale"), (dict(n_info=207), "could be decoded"), (dict(n_info=213, tail=False), "could be decoded")):
        a = dict(good)
        a.update(kw)
        with pytest.raises(ValueError, match=what):
            plan_decode(f, d, **a)
    plan_decode(f, d, n_info=104, crc="crc16-x25")                             # whole bytes before the check field
    plan_decode(f, d, n_info=106, tail=False)
    only2 = _frames(ns, order, 150, clip=[0], position=[10])                    # order 2 needs 212 symbols; an order-4 frame would have had enough
    with pytest.raises(ValueError, match="could be decoded"):
        plan_decode(only2, d, n_info=100)
    assert plan_decode(_frames(ns, order, 150, clip=[0, 1], position=[10, 10]), d, n_info=100).reason.tolist() == ["short", ""]
    # a Frames and a Demodulation that do not belong together
    for other in (_demod([600], [2], [1.0]), _demod([600, 601], order, gain), _demod(ns, [2, 2], gain), _demod(ns, [4, 2], gain)):
        with pytest.raises(ValueError, match="not found in this demodulation"):
            plan_decode(f, other, n_info=100)
    with pytest.raises(ValueError, match="Frames"):
        plan_decode(d, d, n_info=100)


# ------------------------------------------------------------------------------------------------------------- the library's refusals
def test_library_refuses_before_any_launch():
    """Every check of the three entry points returns -1 before a launch, so it runs without a device; the pointers are never followed."""
    from sy11 import _lib
    from sy11.data.decode import FECFRAME
    lib = _lib.load()
    fr = np.zeros(2, dtype=FECFRAME)
    fr["sym_off"], fr["T"], fr["order"], fr["q"], fr["tail"], fr["row"], fr["scale"] = [0, 50], [20, 14], [2, 4], [1, 3], [1, 0], [0, 1], [32.0, 16.0]
    host, fake = C.c_void_p(fr.ctypes.data), C.c_void_p(0x1000)

    def table(**kw):
        t = fr.copy()
        for k, v in kw.items():
            t[k][1] = v
        keep.append(t)
        return C.c_void_p(t.ctypes.data)
    keep = []
    crc = _lib.FecCrc(8, 0x07, 0, 0, 0, 0)
    soft = lambda: [2, host, fake, 2, 3, 100, fake, 2, 40, fake, None]                                   # noqa: E731
    vit = lambda: [2, host, fake, 0o171, 0o133, 2, 40, fake, 3, fake, fake, None]                         # noqa: E731
    chk = lambda: [2, host, fake, 0o171, 0o133, 14, None, C.byref(crc), 2, 40, fake, 3, fake, 2, fake, fake, None]      # noqa: E731
    entry = (dict(order=3), dict(order=0), dict(q=4), dict(q=-1), dict(tail=2), dict(T=0), dict(T=8193), dict(row=2), dict(row=-1), dict(row=0))
    cases = [("sy11_fec_soft", soft, [(0, 0), (1, None), (2, None), (6, None), (9, None), (3, 0), (3, 3), (3, 66), (4, 0), (4, 4), (5, 0), (5, 56), (7, 0), (8, 38), (8, 39),
                                     (8, 16386), (2, C.c_void_p(0x1004)), (6, C.c_void_p(0x1004)), (9, C.c_void_p(0x1001))],
              entry + (dict(sym_off=-1), dict(sym_off=94), dict(T=21), dict(scale=0.0), dict(scale=float("nan")), dict(scale=float("inf")))),
             ("sy11_fec_viterbi", vit, [(0, 0), (1, None), (2, None), (7, None), (9, None), (10, None), (3, 0o170), (3, 0o71), (3, 0o371), (4, 0o132), (5, 0), (6, 38), (6, 39),
                                        (8, 0), (8, 2), (8, 1025), (2, C.c_void_p(0x1004)), (7, C.c_void_p(0x1001)), (10, C.c_void_p(0x1002))], entry + (dict(T=21),)),
             ("sy11_fec_check", chk, [(0, 0), (1, None), (2, None), (7, None), (10, None), (12, None), (14, None), (15, None), (3, 0o170), (4, 0o32), (5, 0), (5, 17), (5, 13),
                                      (8, 0), (9, 38), (11, 2), (13, 1), (13, 0), (15, C.c_void_p(0x1002))], entry + (dict(T=15), dict(tail=1)))]
    for name, args, positional, entries in cases:
        fn = getattr(lib, name)
        for pos, v in positional:
            a = args()
            a[pos] = v
            assert fn(*a) == -1, (name, pos, v)
            assert name[5:].encode() in lib.sy11_last_error()
        for kw in entries:
            a = args()
            a[1] = table(**kw)
            assert fn(*a) == -1, (name, kw)
    # the frame of 14 steps has no tail: with one it would be legal (T >= 7), with T = 6 not
    a = vit()
    a[1] = table(T=6, tail=1)
    assert lib.sy11_fec_viterbi(*a) == -1 and b"trellis steps" in lib.sy11_last_error()
    for bad in (_lib.FecCrc(7, 7, 0, 0, 0, 0), _lib.FecCrc(33, 7, 0, 0, 0, 0), _lib.FecCrc(8, 0x107, 0, 0, 0, 0), _lib.FecCrc(8, 7, 0x100, 0, 0, 0), _lib.FecCrc(8, 7, 0, 0x100, 0, 0),
                _lib.FecCrc(8, 7, 0, 0, 2, 0), _lib.FecCrc(8, 7, 0, 0, 0, -1), _lib.FecCrc(16, 0x1021, 0, 0, 0, 0), _lib.FecCrc(8, 7, 0, 0, 1, 0)):
        a = chk()
        a[7] = C.byref(bad)
        assert lib.sy11_fec_check(*a) == -1, (bad.width, bad.poly)


# ------------------------------------------------------------------------------------------------------------- end to end
def test_reference_chain_decodes_the_embedded_frames_without_an_error():
    """The cases the GPU test runs on the device: both frames of every clip are found by the reference search at threshold 0.6 and decoded without a
    bit error, CRC ok, through a channel that did make errors.  The channel's hard errors (the sign of the received component against the bit sent,
    before the quantiser) are the figures the cases were chosen by; ``channel_errors`` counts the same where the soft value is not 0."""
    hard_want = {"a": [16, 16], "b": [4, 2], "c": [4, 3]}
    for c, (ref, found, dec, m0) in zip(R.case_clips(), R.case_reference()):
        want = [j - m0 for j in c["at"]]
        assert found["position"].tolist() == want and found["n_payload"] == [c["n_need"]] * 2 and len(set(found["rotation"])) == 1
        assert c["n_coded"] == {"a": 444, "b": 444, "c": 424}[c["label"][0]]
        r = ref["r"].astype(np.complex64)
        hard = []
        for k, (p, d) in enumerate(zip(want, dec)):
            assert d is not None and np.array_equal(d["v"], c["info"][k]) and np.array_equal(d["v"][:-16], c["u"][k]) and d["crc_ok"] == 1 and d["end_state"] == 0
            sent = R.frame_bits(c["u"][k], R.CRCS[R.CRC], R.POLYS, c["pattern"], None, c["order"])[0]
            x = R.received(r[p + 32:p + 32 + c["n_need"]], c["order"], found["rotation"][k])[:c["n_coded"]]
            hard.append(int(((x < 0) != sent[:c["n_coded"]].astype(bool)).sum()))
            zero = int((R.quantize(x, R.scale_of(32.0, ref["gain"], c["order"])) == 0).sum())
            assert d["n_channel"] == c["n_coded"] - zero and hard[-1] - zero <= d["channel_errors"] <= hard[-1] and d["channel_errors"] >= 1
        print(f"decode[{c['label']}]: frames at {want}, hard channel errors {hard} of {c['n_coded']}, channel_errors {[d['channel_errors'] for d in dec]} of "
              f"{[d['n_channel'] for d in dec]}, metric {[d['metric'] for d in dec]}")
        assert hard == hard_want[c["label"][0]] and min(hard) >= 2
