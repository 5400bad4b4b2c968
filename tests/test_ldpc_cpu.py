"""CPU: the LDPC reference (tests/_ldpc_ref.py) pinned by properties that need no outside source; the package's host side (``sy11.data.ldpc``: ``ldpc_code``,
``ldpc_staircase``, ``ldpc_encode``, ``plan_ldpc``, ``LdpcDecoded``) against it; and the library's refusals, which all come before a launch and so run without a device."""
import ctypes as C
import json
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

from tests import _fec_ref as FEC
from tests import _ldpc_ref as R
from tests.test_decode_cpu import _demod, _frames

ROOT = Path(__file__).resolve().parents[1]
# a base matrix with empty blocks, and one whose parity part has two equal block rows
LOOPED = np.array([[0, 2, 1, -1, 3], [4, -1, 0, 2, -1], [-1, 1, -1, 0, 1]])
SINGULAR = np.array([[1, 2, 0, 0], [3, 4, 0, 0]])


# ------------------------------------------------------------------------------------------------------------- the reference pinned by itself
@pytest.mark.parametrize("Z", [1, 3, 27])
def test_reference_returns_a_clean_codeword_in_one_iteration(Z):
    kb, mb, w = (2, 2, 2) if Z < 27 else (12, 12, 6)
    base = R.staircase_base(kb, mb, Z, 5 + Z, w)
    g = np.random.default_rng(Z)
    for _ in range(4):
        c = R.encode_staircase(g.integers(0, 2, kb * Z), base, Z)
        y = (16 * (1 - 2 * c.astype(np.int64))).astype(np.int8)
        out = R.decode(y, base, Z, 20, 12)
        assert out["iterations"].tolist() == [1] and out["unsat"].tolist() == [0] and np.array_equal(out["x"][0], c)
        assert np.array_equal(np.sign(out["post"][0]), np.sign(y)) and (np.abs(out["post"][0]) >= 16).all()


def test_reference_converges_only_on_codewords_of_a_code_of_12_bits():
    Z, base = 3, R.staircase_base(2, 2, 3, 9, 2)
    H = R.dense_h(base, Z).astype(np.int64)
    assert H.shape == (6, 12)
    g = np.random.default_rng(12)
    y = g.integers(-40, 41, (400, 12)).astype(np.int8)
    out = R.decode(y, base, Z, 10, 12)
    done = out["unsat"] == 0
    assert 40 < done.sum() and (~done).sum() > 0 and (out["iterations"][~done] == 10).all()
    assert not ((out["x"][done].astype(np.int64) @ H.T) & 1).any()
    assert (((out["x"][~done].astype(np.int64) @ H.T) & 1).sum(axis=1) == out["unsat"][~done]).all()
    one = R.decode(y[7], base, Z, 10, 12)                                       # a frame alone gives what it gives in the batch
    assert np.array_equal(one["x"][0], out["x"][7]) and np.array_equal(one["post"][0], out["post"][7]) and one["iterations"][0] == out["iterations"][7]


def test_reference_corrects_a_weak_flipped_bit_among_strong_ones():
    Z, base = 27, R.staircase_base(12, 12, 27, 3, 6)
    g = np.random.default_rng(4)
    c = R.encode_staircase(g.integers(0, 2, 12 * 27), base, Z)
    for at in (0, 100, 323, 324, 647):
        y = (100 * (1 - 2 * c.astype(np.int64))).astype(np.int8)
        y[at] = -np.sign(y[at]) * 3
        out = R.decode(y, base, Z, 20, 12)
        assert out["unsat"][0] == 0 and np.array_equal(out["x"][0], c) and out["iterations"][0] <= 2, at


# ------------------------------------------------------------------------------------------------------------- the code and the encoder
def test_ldpc_code_tables_and_staircase():
    from sy11.data.ldpc import LDPCENTRY, LdpcCode, ldpc_code, ldpc_staircase, n_max
    assert n_max() == R.N_MAX == 2 * FEC.T_MAX
    cd = ldpc_code(np.hstack((LOOPED, [[-1], [-1], [0]])), 5)
    assert isinstance(cd, LdpcCode) and (cd.Z, cd.mb, cd.nb, cd.N, cd.M, cd.K) == (5, 3, 6, 30, 15, 15)
    assert cd.layer.tolist() == [0, 4, 7, 11] and cd.layer.dtype == np.int32 and cd.entry.dtype == LDPCENTRY
    assert cd.entry["column"].tolist() == [0, 1, 2, 4, 0, 2, 3, 1, 3, 4, 5] and cd.entry["shift"].tolist() == [0, 2, 1, 3, 4, 0, 2, 1, 0, 1, 0]
    assert cd.spec() == {"Z": 5, "base": cd.base.tolist()} and "N=30" in repr(cd)
    for kb, mb, Z, w in ((12, 12, 27, 6), (2, 2, 1, 2), (4, 12, 40, 2), (5, 3, 3, 2)):
        a, b = ldpc_staircase(kb, mb, Z, 7, row_weight=w), ldpc_staircase(kb, mb, Z, 7, row_weight=w)
        assert np.array_equal(a.base, b.base) and a.base.shape == (mb, kb + mb) and ((a.base[:, :kb] >= 0).sum(axis=1) == w).all() and ((a.base >= 0).sum(axis=0) >= 1).all()
        par = a.base[:, kb:]
        want = np.full((mb, mb), -1)
        want[np.arange(mb), np.arange(mb)] = 0
        want[np.arange(1, mb), np.arange(mb - 1)] = 0
        assert np.array_equal(par, want) and (a.base < Z).all()
    assert not np.array_equal(ldpc_staircase(12, 12, 27, 7).base, ldpc_staircase(12, 12, 27, 8).base)


def test_ldpc_encode_both_paths_against_the_dense_matrix():
    from sy11.data.ldpc import ldpc_code, ldpc_encode, ldpc_staircase
    g = np.random.default_rng(8)
    stair = ldpc_staircase(12, 12, 27, 3)
    tri = ldpc_code(np.array([[1, 3, -1, 2, -1, -1], [0, -1, 4, 1, 3, -1], [-1, 2, 2, -1, 0, 4]]), 5)     # lower-triangular, shifts on the diagonal
    # an entry above the diagonal: the elimination.  The parity part's determinant over GF(2)[x] / (x^6 + 1) is x + x + 1 = 1, so it has an inverse
    loop = ldpc_code(np.array([[1, 4, 1, 0, -1], [2, -1, 0, 0, 0], [-1, 3, -1, 0, 0]]), 6)
    for cd, triangular in ((stair, True), (tri, True), (loop, False)):
        H = R.dense_h(cd.base, cd.Z).astype(np.int64)
        u = g.integers(0, 2, (6, cd.K))
        c = ldpc_encode(u, cd)
        assert c.shape == (6, cd.N) and c.dtype == np.uint8 and np.array_equal(c[:, :cd.K], u) and not ((c.astype(np.int64) @ H.T) & 1).any()
        one = ldpc_encode(u[2], {"Z": cd.Z, "base": cd.base})
        assert one.shape == (cd.N,) and np.array_equal(one, c[2])
        assert (cd._inverse is None) == triangular
    assert np.array_equal(ldpc_encode(np.ones(stair.K, dtype=np.int64), stair), R.encode_staircase(np.ones(stair.K), stair.base, 27))
    with pytest.raises(ValueError, match="not encodable"):
        ldpc_encode(np.zeros(10, dtype=np.int64), ldpc_code(SINGULAR, 5))
    for bad in (np.zeros(9, dtype=np.int64), np.zeros((2, 3, 10), dtype=np.int64), np.full(10, 2), np.zeros(10), np.zeros(10, dtype=bool)):
        with pytest.raises(ValueError, match="ldpc_encode: `bits`"):
            ldpc_encode(bad, ldpc_code(SINGULAR, 5))


def test_ldpc_code_argument_errors_name_the_row_column_or_entry():
    from sy11.data.ldpc import ldpc_code, ldpc_staircase
    good = np.array([[0, 1, 0, -1], [2, -1, 0, 0]])
    ldpc_code(good, 3)
    wide = np.zeros((2, 40), dtype=np.int64)
    for base, Z, what in ((good, 0, "Z must be"), (good, 513, "Z must be"), (good, 3.0, "Z must be"), (good, True, "Z must be"), (good[0], 3, "2-D array"), ("ab", 3, "2-D array"),
                          (good.astype(float), 3, "2-D array"), (good > 0, 3, "2-D array"), (np.zeros((2, 2), dtype=int), 3, "mb < nb"), (np.zeros((65, 70), dtype=int), 2, "mb <= 64"),
                          (np.zeros((2, 129), dtype=int), 2, "nb <= 128"), (np.zeros((2, 3), dtype=int), 3, "N = nb Z = 3 x 3 = 9 must be even"),
                          (np.zeros((2, 33), dtype=int), 512, "at most 16384"), (np.array([[0, 1, 3, -1], [2, -1, 0, 0]]), 3, r"entry \(0, 2\) of `base` is 3"),
                          (np.array([[0, 1, 0, -1], [2, -2, 0, 0]]), 3, r"entry \(1, 1\) of `base` is -2"), (np.array([[0, 1, 0, -1], [-1, -1, 0, -1]]), 3, "row 1 of `base` has weight 1"),
                          (wide, 2, "row 0 of `base` has weight 40"), (np.array([[0, -1, 0, -1], [2, -1, 0, 0]]), 3, "column 1 of `base` has no entry"),
                          (np.where((np.arange(64)[None, :] - np.arange(63)[:, None]) % 64 < 10, 0, -1), 256, "bytes of LDS")):
        with pytest.raises(ValueError, match="ldpc_code: .*" + what):
            ldpc_code(base, Z)
    for kw, what in ((dict(kb=0), "kb"), (dict(mb=0), "mb"), (dict(Z=0), "Z"), (dict(seed=-1), "seed"), (dict(row_weight=13), "row_weight"), (dict(kb=30, mb=2, row_weight=6), "row_weight"),
                     (dict(Z=2.0), "Z"), (dict(row_weight=32), "row_weight")):
        a = dict(kb=12, mb=12, Z=27, seed=1, row_weight=6)
        a.update(kw)
        with pytest.raises(ValueError, match="ldpc_staircase: .*" + what):
            ldpc_staircase(**a)


# ------------------------------------------------------------------------------------------------------------- the plan
def test_plan_ldpc_columns_and_reasons():
    from sy11.data.ldpc import LdpcPlan, ldpc_staircase, plan_ldpc
    cd = ldpc_staircase(4, 4, 25, 2, row_weight=3)                              # N = 200, K = 100
    ns, order = [600, 600, 600, 600], [2, 4, 2, 4]
    gain = [2.0, 1.5, 0.0, np.nan]
    f = _frames(ns, order, 200, clip=[0, 0, 1, 1, 2, 3], position=[10, 500, 3, 490, 0, 0])
    p = plan_ldpc(f, _demod(ns, order, gain), code=cd, crc="crc16-ccitt-false", whiten=[1, 0] * 60)
    assert isinstance(p, LdpcPlan) and (p.N, p.M, p.n_info, p.T, p.n_coded, p.period, p.mask, p.tail) == (200, 100, 100, 100, 200, 2, 3, False)
    assert p.n_need.tolist() == [200, 200, 100, 100, 200, 100] and p.reason.tolist() == ["", "short", "", "short", "gain", "gain"]
    assert p.scale.dtype == np.float32 and p.scale[0] == np.float32(8.0) and p.scale[2] == FEC.scale_of(16.0, 1.5, 4) and (p.iterations, p.scale16, p.soft_scale) == (20, 12, 16.0)
    assert p.crc["name"] == "crc16-ccitt-false" and p.whiten.tolist() == ([1, 0] * 50) and p.code is cd and "LdpcPlan(6 frames, 2 valid" in repr(p)
    fr, at = p.table(f.rotation, f.plan.order[f.clip])
    assert at.tolist() == [0, 2] and fr["T"].tolist() == [100, 100] and fr["tail"].tolist() == [0, 0] and fr["order"].tolist() == [2, 4]
    q = plan_ldpc(f, _demod(ns, order, gain), code={"Z": cd.Z, "base": cd.base.tolist()}, iterations=100, scale=16, soft_scale=127)
    assert q.code.N == 200 and q.crc is None and q.whiten is None and (q.iterations, q.scale16) == (100, 16)


def test_plan_ldpc_argument_errors():
    from sy11.data.ldpc import ldpc_staircase, plan_ldpc
    cd = ldpc_staircase(4, 4, 25, 2, row_weight=3)
    ns, order, gain = [600, 600], [2, 4], [1.0, 1.0]
    f, d = _frames(ns, order, 200, clip=[0, 1], position=[10, 10]), _demod(ns, order, gain)
    crc8 = FEC.CRCS["crc8"]
    for kw, what in ((dict(code=7), "code must be"), (dict(code={"Z": 25}), "code must be"), (dict(code={"Z": 25, "base": cd.base, "x": 1}), "code must be"),
                     (dict(code={"Z": 0, "base": cd.base}), "Z must be"), (dict(code={"Z": 25, "base": np.where(cd.base == 0, 25, cd.base)}), r"entry \(\d+, \d+\)"),
                     (dict(iterations=0), "iterations"), (dict(iterations=101), "iterations"), (dict(iterations=5.0), "iterations"), (dict(iterations=True), "iterations"),
                     (dict(scale=0), "scale"), (dict(scale=17), "scale"), (dict(scale=0.75), "scale"), (dict(whiten=[1] * 99), "whiten"), (dict(whiten=[2] * 100), "whiten"),
                     (dict(whiten="10"), "whiten"), (dict(crc="crc-nope"), "crc"), (dict(crc=7), "crc"), (dict(crc=dict(width=16)), "crc"), (dict(crc=dict(crc8, width=7)), "width"),
                     (dict(crc=dict(crc8, poly=0x107)), "poly"), (dict(crc=dict(crc8, refin=2)), "refin"), (dict(crc="crc16-x25"), "whole bytes"),
                     (dict(soft_scale=0.0), "soft_scale"), (dict(soft_scale=128), "soft_scale"), (dict(soft_scale=float("nan")), "soft_scale"), (dict(soft_scale=True), "soft_scale")):
        a = dict(code=cd)
        a.update(kw)
        with pytest.raises(ValueError, match="plan_ldpc: .*" + what):
            plan_ldpc(f, d, **a)
    with pytest.raises(ValueError, match="plan_ldpc: .*n_info = 8"):
        plan_ldpc(f, d, code=ldpc_staircase(1, 3, 8, 1, row_weight=1), crc="crc8")     # K = 8 does not exceed the 8 bits
    with pytest.raises(ValueError, match="Frames of find_frames"):
        plan_ldpc(SimpleNamespace(), d, code=cd)
    with pytest.raises(ValueError, match="not found in this demodulation"):
        plan_ldpc(f, _demod([600, 601], order, gain), code=cd)
    with pytest.raises(ValueError, match="payload = 99 symbols, but the code needs 100 at order 4"):
        plan_ldpc(_frames(ns, order, 99, clip=[0, 1], position=[10, 10]), d, code=cd)
    with pytest.raises(ValueError, match="payload = 150 symbols, but the code needs 200"):
        plan_ldpc(_frames(ns, order, 150, clip=[0], position=[10]), d, code=cd)


# ------------------------------------------------------------------------------------------------------------- the C-ABI
def test_header_declares_and_library_exports_the_new_symbols():
    from sy11 import _lib
    header = (ROOT / "include" / "sy11.h").read_text()
    lib = _lib.load()
    for name in ("sy11_ldpc_nmax", "sy11_ldpc_lds_bytes", "sy11_ldpc_decode", "sy11_ldpc_check"):
        assert re.search(rf"\b{name}\s*\(", header) and hasattr(lib, name), name
    assert "typedef struct sy11_ldpc_code" in header and "typedef struct sy11_ldpc_entry" in header
    assert lib.sy11_ldpc_nmax() == 16384
    assert lib.sy11_ldpc_lds_bytes(81, 12, 24, 88) == 3888 + 8 * 972 + 352 + 64 + 16 and lib.sy11_ldpc_lds_bytes(513, 2, 4, 8) == -1 and lib.sy11_ldpc_lds_bytes(27, 0, 4, 8) == -1
    assert C.sizeof(_lib.LdpcCode) == 16


def test_library_refuses_before_any_launch():
    """Every check of the two entry points returns -1 before a launch, so it runs without a device; the device pointers are never followed."""
    from sy11 import _lib
    from sy11.data.ldpc import LDPCENTRY
    lib = _lib.load()
    fake = C.c_void_p(0x1000)
    keep = []

    def i32(*v):
        t = np.array(v, dtype=np.int32)
        keep.append(t)
        return C.c_void_p(t.ctypes.data)

    def entries(v):
        t = np.array(v, dtype=LDPCENTRY)
        keep.append(t)
        return C.c_void_p(t.ctypes.data)

    def code(**kw):
        a = dict(Z=3, mb=2, nb=4, n_entry=6)
        a.update(kw)
        c = _lib.LdpcCode(a["Z"], a["mb"], a["nb"], a["n_entry"])
        keep.append(c)
        return C.byref(c)
    ENT = [(0, 0), (1, 1), (2, 0), (0, 2), (2, 0), (3, 0)]
    crc = _lib.FecCrc(0, 0, 0, 0, 0, 0)
    # n_frame, row_host, row, code, layer_host, layer, entry_host, entry, iterations, scale, n_rows, stride_soft, soft, stride_bits, bits, out, stride_post, post, stream
    dec = lambda: [2, i32(1, 0), fake, code(), i32(0, 3, 6), fake, entries(ENT), fake, 20, 12, 2, 12, fake, 2, fake, fake, 12, fake, None]       # noqa: E731
    # n_frame, row_host, row, N, K, whiten, crc, n_rows, stride_soft, soft, stride_bits, bits, stride_data, data, rows, stream
    chk = lambda: [2, i32(1, 0), fake, 40, 20, None, C.byref(crc), 2, 40, fake, 5, fake, 3, fake, fake, None]                                    # noqa: E731

    def refused(name, a, word):
        assert getattr(lib, name)(*a) == -1, (name, word)
        msg = lib.sy11_last_error()
        assert name[5:].encode() in msg and word.encode() in msg, (name, word, msg)

    def with_(args, **at):
        a = args()
        for pos, v in at.items():
            a[int(pos[1:])] = v
        return a
    odd = C.c_void_p(0x1002)
    for pos in (1, 2, 3, 4, 5, 6, 7, 12, 14, 15):
        refused("sy11_ldpc_decode", with_(dec, **{f"p{pos}": None}), "null")
    for pos in (2, 5, 7, 15):
        refused("sy11_ldpc_decode", with_(dec, **{f"p{pos}": odd}), "aligned")
    refused("sy11_ldpc_decode", with_(dec, p17=C.c_void_p(0x1001)), "aligned")
    for kw in (dict(Z=0), dict(Z=513), dict(mb=0), dict(mb=65, nb=70), dict(nb=2), dict(nb=129)):
        refused("sy11_ldpc_decode", with_(dec, p3=code(**kw)), "the code")
    refused("sy11_ldpc_decode", with_(dec, p3=code(nb=5)), "not even")
    refused("sy11_ldpc_decode", with_(dec, p3=code(Z=512, nb=34)), "at most 16384")
    refused("sy11_ldpc_decode", with_(dec, p3=code(n_entry=3)), "entries are not")
    refused("sy11_ldpc_decode", with_(dec, p3=code(n_entry=65)), "entries are not")
    for it in (0, 101, -1):
        refused("sy11_ldpc_decode", with_(dec, p8=it), "iterations")
    for sc in (0, 17):
        refused("sy11_ldpc_decode", with_(dec, p9=sc), "scale")
    refused("sy11_ldpc_decode", with_(dec, p4=i32(1, 3, 6)), "layer offsets run")
    refused("sy11_ldpc_decode", with_(dec, p4=i32(0, 3, 5)), "layer offsets run")
    refused("sy11_ldpc_decode", with_(dec, p4=i32(0, 0, 6)), "layer 0: the offsets")
    refused("sy11_ldpc_decode", with_(dec, p4=i32(0, 7, 6)), "layer 0: the offsets")
    refused("sy11_ldpc_decode", with_(dec, p4=i32(0, 1, 6)), "layer 0: a row weight of 1")
    refused("sy11_ldpc_decode", with_(dec, p3=code(mb=2, nb=40, Z=2, n_entry=35), p4=i32(0, 33, 35)), "a row weight of 33")
    for at, v, word in ((1, (4, 1), "column 4 is not in [0, 4)"), (1, (-1, 1), "column -1"), (4, (2, 3), "shift 3 is not in [0, 3)"), (0, (0, -1), "shift -1"),
                        (1, (0, 1), "layer 0 names column 0 twice"), (5, (0, 0), "layer 1 names column 0 twice")):
        e = list(ENT)
        e[at] = v
        refused("sy11_ldpc_decode", with_(dec, p6=entries(e)), word)
    e = list(ENT)
    e[1] = (3, 1)
    refused("sy11_ldpc_decode", with_(dec, p6=entries(e)), "column 1 of the code has no entry")
    lay = list(range(0, 631, 10))                                               # 63 x 64 blocks of 256 with ten entries a row: 2 N + 8 M + 4 entries beyond 160 KiB
    wide = [((i + k) % 64, 0) for i in range(63) for k in range(10)]
    refused("sy11_ldpc_decode", with_(dec, p3=code(Z=256, mb=63, nb=64, n_entry=630), p4=i32(*lay), p6=entries(wide), p11=16384, p13=2048, p16=16384), "bytes of LDS")
    for rows in ((2, 0), (-1, 0), (1, 1)):
        refused("sy11_ldpc_decode", with_(dec, p1=i32(*rows)), "reads row")
        refused("sy11_ldpc_check", with_(chk, p1=i32(*rows)), "reads row")
    for pos, v, word in ((0, 0, "need frames"), (10, 0, "need frames"), (11, 11, "soft bits leave"), (11, 16385, "soft bits leave"), (13, 1, "bits leave"), (13, 2049, "bits leave"),
                         (16, 11, "posteriors leave"), (16, 16385, "posteriors leave")):
        refused("sy11_ldpc_decode", with_(dec, **{f"p{pos}": v}), word)
    for pos in (1, 2, 6, 9, 11, 13, 14):
        refused("sy11_ldpc_check", with_(chk, **{f"p{pos}": None}), "null")
    for pos in (2, 14):
        refused("sy11_ldpc_check", with_(chk, **{f"p{pos}": odd}), "aligned")
    for pos, v, word in ((3, 41, "N = 41"), (3, 0, "N = 0"), (3, 16386, "N = 16386"), (4, 0, "K = 0"), (4, 40, "K = 40"), (8, 39, "leave a row"), (10, 4, "leave a row"),
                         (12, 2, "leave a row"), (12, 2049, "leave a row"), (0, 0, "need frames"), (7, 0, "need frames")):
        refused("sy11_ldpc_check", with_(chk, **{f"p{pos}": v}), word)
    for bad, word in ((_lib.FecCrc(7, 7, 0, 0, 0, 0), "CRC of 7 bits"), (_lib.FecCrc(33, 7, 0, 0, 0, 0), "CRC of 33 bits"), (_lib.FecCrc(8, 0x107, 0, 0, 0, 0), "beyond the CRC"),
                      (_lib.FecCrc(8, 7, 0x100, 0, 0, 0), "beyond the CRC"), (_lib.FecCrc(8, 7, 0, 0x100, 0, 0), "beyond the CRC"), (_lib.FecCrc(8, 7, 0, 0, 2, 0), "refin / refout"),
                      (_lib.FecCrc(8, 7, 0, 0, 0, -1), "refin / refout"), (_lib.FecCrc(24, 7, 0, 0, 0, 0), "do not exceed"), (_lib.FecCrc(32, 7, 0, 0, 0, 0), "do not exceed")):
        keep.append(bad)
        refused("sy11_ldpc_check", with_(chk, p6=C.byref(bad)), word)
    refin = _lib.FecCrc(8, 7, 0, 0, 1, 0)
    refused("sy11_ldpc_check", with_(chk, p6=C.byref(refin)), "whole bytes")


# ------------------------------------------------------------------------------------------------------------- the result
def test_ldpc_decoded_from_host_arrays_round_trips(tmp_path):
    import torch
    from sy11.data.ldpc import LdpcDecoded, ldpc_staircase, plan_ldpc
    cd = ldpc_staircase(4, 4, 25, 2, row_weight=3)
    ns, order, gain = [600, 600], [2, 4], [1.0, 0.0]
    f = _frames(ns, order, 200, clip=[0, 0, 1], position=[10, 300, 10])
    plan = plan_ldpc(f, _demod(ns, order, gain), code=cd, crc="crc16-ccitt-false")
    g = np.random.default_rng(3)
    msg = g.integers(0, 2, (3, 84)).astype(np.uint8)
    info = np.stack([np.concatenate((m, FEC.int_bits(FEC.crc(m, FEC.CRCS["crc16-ccitt-false"]), 16))) for m in msg])
    info[2] = 0
    n = 3
    cols = {"valid": plan.valid.copy(), "clip": f.clip.copy(), "word": f.word.copy(), "position": f.position.copy(), "iterations": np.array([3, 20, 0]),
            "unsatisfied": np.array([0, 7, 0]), "converged": np.array([True, False, False]), "channel_errors": np.array([11, 40, 0]), "n_channel": np.array([200, 199, 0]),
            "ber": np.array([11 / 200, 40 / 199, np.nan]), "crc_ok": np.array([True, False, False]), "crc_calc": np.array([1, 2, 0], dtype=np.uint32),
            "crc_recv": np.array([1, 3, 0], dtype=np.uint32)}
    raw = {"soft": None, "decided": None, "out": None, "post": None, "rows": None}
    dec = LdpcDecoded(plan, cols, plan.reason, torch.from_numpy(np.packbits(info, axis=1)), raw, cls=np.array([0, 1]), conf=np.array([0.5, 0.6]), names={0: "a", 1: "b"})
    assert len(dec) == n and dec.data.shape == (3, 13) and plan.valid.tolist() == [True, True, False] and dec.reason.tolist() == ["", "", "gain"]
    assert np.array_equal(dec.bits(0), info[0]) and dec.bits(1).shape == (100,) and isinstance(dec.message(0), np.ndarray) and np.array_equal(dec.message(0), msg[0])
    assert dec[0] == dict({k: cols[k][0].item() for k in dec.COLUMNS}, reason="") and dec[-1]["reason"] == "gain" and dec[1]["unsatisfied"] == 7
    assert dec.soft(0).shape == (200,) and dec.soft(0).dtype == torch.int8 and dec.posterior(1).shape == (200,) and dec.posterior(1).dtype == torch.int16 and not dec.posterior(1).any()
    out = dec.save(tmp_path / "l")
    z = np.load(tmp_path / "l" / "ldpc.npz")
    index = json.loads((tmp_path / "l" / "ldpc.json").read_text())
    assert out == str(tmp_path / "l")
    for key in dec.COLUMNS:
        assert np.array_equal(z[key], getattr(dec, key), equal_nan=True), key
    assert np.array_equal(z["data"], dec.data.numpy()) and z["reason"].tolist() == ["", "", "gain"]
    assert index["code"] == cd.spec() and (index["N"], index["K"], index["iterations"], index["scale"]) == (200, 100, 20, 12) and index["crc"]["name"] == "crc16-ccitt-false"
    assert len(index["frames"]) == 3 and index["frames"][0]["converged"] is True and index["frames"][2]["ber"] is None and index["frames"][0]["name"] == "a"
    # whole bytes before the check field: the message is bytes, and hex in the index
    cd2 = ldpc_staircase(4, 4, 26, 2, row_weight=3)                             # K = 104 = 88 + 16
    plan2 = plan_ldpc(_frames(ns, order, 208, clip=[0], position=[10]), _demod(ns, order, [1.0, 1.0]), code=cd2, crc="crc16-ccitt-false")
    body = g.integers(0, 256, 11).astype(np.uint8)
    bits = np.concatenate((np.unpackbits(body), np.zeros(16, dtype=np.uint8)))
    one = LdpcDecoded(plan2, {k: v[:1] for k, v in cols.items()}, plan2.reason, torch.from_numpy(np.packbits(bits)[None, :]), raw)
    assert one.message(0) == body.tobytes() and json.loads(Path(one.save(tmp_path / "m"), "ldpc.json").read_text())["frames"][0]["message"] == body.tobytes().hex()
    # what plan_correct reads of a Decoded
    from sy11.data.correct import plan_correct
    assert plan_correct(one, code=dict(n=13, k=11, poly=0x11D, fcr=0, prim=1)).valid.tolist() == [True]


# ------------------------------------------------------------------------------------------------------------- end to end
def test_reference_chain_reads_the_embedded_frames_through_channel_errors():
    """The three clips the GPU test runs on the device, on the reference chain: every embedded frame has raw bit errors and decodes, before iteration 20, to what
    was sent (tests/test_ldpc_gpu.py holds the clips and the assertions; the module needs no device to import)."""
    from tests import test_ldpc_gpu as G
    G.test_case_list_covers_the_weights_shifts_and_empty_blocks()
    G.test_reference_chain_reads_the_embedded_frames_through_channel_errors()
