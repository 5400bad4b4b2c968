"""GPU: the LDPC frame decoder's kernels (sy11_ldpc_decode, sy11_ldpc_check) against tests/_ldpc_ref.py.  Every comparison is ``np.array_equal``: everything after the
quantiser of launch 1 is integer arithmetic, so no tolerance is due.  The kernel-level tests feed synthetic int8 soft bits to ``ops.ldpc_*`` directly; one call over
all frames, one call per frame and a permuted packing give the same bytes; every refusal is raised by ``ops`` and by the library with the sentinel-filled outputs
untouched; and ``demodulate`` -> ``find_frames`` -> ``decode_ldpc`` on synthesised BPSK and QPSK clips reads the embedded frames as they were sent, in exactly three
launches, and hands a frame that carries a Reed-Solomon codeword on to ``correct``."""
import copy
import ctypes as C
import functools
import json

import numpy as np
import pytest
import torch

from tests import _fec_ref as FEC
from tests import _frames_ref as F
from tests import _ldpc_ref as R
from tests import _rs_ref as RS

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FC = 2.4e9
BITS_FILL, OUT_FILL, POST_FILL, DATA_FILL = 0xA5, -7, -12345, 0x5A


# ------------------------------------------------------------------------------------------------------------- the codes of the case list
def _random_base(mb, nb, Z, seed, fill):
    """A seeded base matrix with empty blocks: every block is kept with probability ``fill``, every row weight in [2, 32] and column weight >= 1 made good, the
    shifts random with 0 and Z - 1 among them."""
    g = np.random.default_rng(seed)
    on = g.random((mb, nb)) < fill
    for i in range(mb):
        while on[i].sum() < 2:
            on[i, g.integers(0, nb)] = True
        while on[i].sum() > 32:
            on[i, g.choice(np.flatnonzero(on[i]))] = False
    for j in np.flatnonzero(on.sum(axis=0) == 0):
        rows = np.flatnonzero(on.sum(axis=1) < 32)
        on[g.choice(rows), j] = True
    base = np.where(on, g.integers(0, Z, (mb, nb)), -1)
    i, j = np.nonzero(on)
    base[i[0], j[0]], base[i[-1], j[-1]] = 0, Z - 1
    return base


# Z, base, iterations, the note of the case list
CODES = {
    "Z1 2x4": (1, np.array([[0, -1, 0, -1], [-1, 0, 0, 0]]), 20),                                     # a row of weight 2
    "Z3 2x4": (3, np.array([[0, -1, 2, -1], [1, 2, 0, 1]]), 20),                                      # a row of weight 2; shifts 0 and Z - 1
    "Z27 12x24": (27, R.staircase_base(12, 12, 27, 1, 6), 20),
    "Z64 4x8": (64, _random_base(4, 8, 64, 2, 0.6), 20),
    "Z65 3x6": (65, _random_base(3, 6, 65, 3, 0.7), 20),                                              # a second wave with one live lane
    "Z300 2x6": (300, _random_base(2, 6, 300, 4, 0.8), 20),                                           # above one workgroup's width
    "Z5 1x32": (5, _random_base(1, 32, 5, 5, 1.0), 20),                                               # mb = 1, a row of weight 32
    "Z40 5x40": (40, _random_base(5, 40, 40, 6, 0.9), 7),                                             # five rows of weight 32
}
BIG = (512, _random_base(16, 32, 512, 7, 0.25), 3)                                                    # N = 16 384, one frame, 3 iterations


def _inputs(N, seed):
    """The frames of one case: all +127, all 0, two of +-127 with random signs (conflicts: the clip of R is hit), three of random values."""
    g = np.random.default_rng(seed)
    return np.stack([np.full(N, 127), np.zeros(N, dtype=np.int64)] + [127 * (1 - 2 * g.integers(0, 2, N)) for _ in range(2)] +
                    [g.integers(-127, 128, N) for _ in range(3)]).astype(np.int8)


def _run(base, Z, y, iterations=20, scale=12, rows=None, n_rows=None, post=True, slack=3):
    """``ops.ldpc_decode`` over the frames ``y`` (frames, N), frame k in row rows[k] of sentinel-filled tables with ``slack`` spare bytes / values a row -> (bits, out, post)."""
    from sy11 import ops
    n, N = y.shape
    rows = np.arange(n) if rows is None else np.asarray(rows)
    n_rows = n if n_rows is None else n_rows
    soft = np.zeros((n_rows, N), dtype=np.int8)
    soft[rows] = y
    bits = torch.full((n_rows, min((N + 7) // 8 + slack, R.N_MAX // 8)), BITS_FILL, dtype=torch.uint8, device=DEV)
    out = torch.full((n_rows, 2), OUT_FILL, dtype=torch.int32, device=DEV)
    pq = torch.full((n_rows, min(N + slack, R.N_MAX)), POST_FILL, dtype=torch.int16, device=DEV) if post else None
    ops.ldpc_decode(torch.from_numpy(soft).to(DEV), rows, {"Z": Z, "base": base}, bits, out, post=pq, iterations=iterations, scale=scale)
    return bits.cpu().numpy(), out.cpu().numpy(), pq.cpu().numpy() if post else None


def _assert_rows(got, want, N, rows=None):
    """The three tables against the reference's dict, frame k in row rows[k]; zeros after the N bits to the end of a row of bits, the sentinel after the N posteriors."""
    bits, out, post = got
    n = want["x"].shape[0]
    rows = np.arange(n) if rows is None else rows
    nb = (N + 7) // 8
    for k in range(n):
        r = rows[k]
        assert np.array_equal(np.unpackbits(bits[r, :nb])[:N], want["x"][k]), k
        assert not np.unpackbits(bits[r, :nb])[N:].any() and not bits[r, nb:].any(), k
        assert out[r].tolist() == [int(want["iterations"][k]), int(want["unsat"][k])], k
        if post is not None:
            assert np.array_equal(post[r, :N], want["post"][k]) and (post[r, N:] == POST_FILL).all(), k


# ------------------------------------------------------------------------------------------------------------- launch 2
@pytest.mark.parametrize("name", list(CODES))
def test_decode_every_code_of_the_case_list_equals_the_reference(name):
    Z, base, iterations = CODES[name]
    N = base.shape[1] * Z
    y = _inputs(N, 40 + Z)
    want = R.decode(y, base, Z, iterations, 12)
    weight = (base >= 0).sum(axis=1)
    print(f"ldpc[{name}]: row weights {sorted(set(weight.tolist()))}, iterations {want['iterations'].tolist()}, unsat {want['unsat'].tolist()}, largest |T| {want['t_max']}, "
          f"{want['n_clip']} minima clipped")
    assert want["iterations"][0] == 1 and want["unsat"][0] == 0 and not want["x"][0].any()                 # all +127: the zero word at once
    assert want["iterations"][1] == 1 and want["unsat"][1] == 0 and not want["x"][1].any() and not want["post"][1].any()     # all 0: the zero word, Q stays 0
    if base.shape[0] > 1:                                                                                   # with one layer T is y again in every iteration
        assert want["t_max"] > 127 and (Z == 1 or want["n_clip"] > 0)                                       # the reference itself meets |T| beyond 127 and clips R
    _assert_rows(_run(base, Z, y, iterations), want, N)


def test_case_list_covers_the_weights_shifts_and_empty_blocks():
    weights, shapes = set(), set()
    for Z, base, _ in list(CODES.values()) + [BIG]:
        weights |= set((base >= 0).sum(axis=1).tolist())
        shapes.add((Z,) + base.shape)
        live = base[base >= 0]
        assert 0 in live and Z - 1 in live and (Z == 1 or base.shape[0] == 1 or (base < 0).any())
    assert {2, 32} <= weights and shapes >= {(1, 2, 4), (3, 2, 4), (27, 12, 24), (64, 4, 8), (65, 3, 6), (300, 2, 6), (512, 16, 32)} and any(s[1] == 1 for s in shapes)


def test_decode_the_largest_code_one_frame_three_iterations():
    Z, base, iterations = BIG
    N = 32 * Z
    assert N == R.N_MAX
    y = np.random.default_rng(9).integers(-127, 128, (1, N)).astype(np.int8)
    want = R.decode(y, base, Z, iterations, 12)
    assert want["iterations"].tolist() == [3] and want["unsat"][0] > 0
    _assert_rows(_run(base, Z, y, iterations, slack=0), want, N)


@functools.lru_cache(maxsize=None)
def noisy():
    """48 seeded frames of the 12 x 24, Z = 27 code, half at Eb/N0 1 dB and half at 2 dB, with the reference's decoding at 20 iterations.  Computed once; leave it
    unchanged."""
    from sy11.data.ldpc import ldpc_encode
    Z, base, _ = CODES["Z27 12x24"]
    g = np.random.default_rng(77)
    c = ldpc_encode(g.integers(0, 2, (48, 12 * Z)), {"Z": Z, "base": base})
    assert not ((c.astype(np.int64) @ R.dense_h(base, Z).T.astype(np.int64)) & 1).any()
    y = np.concatenate((R.awgn_soft(c[:24], 1.0, 0.5, g), R.awgn_soft(c[24:], 2.0, 0.5, g)))
    return Z, base, c, y, R.decode(y, base, Z, 20, 12)


def test_decode_noisy_codewords_early_stop_and_full_run_in_one_launch():
    Z, base, c, y, want = noisy()
    early, full = (want["unsat"] == 0) & (want["iterations"] < 20), want["unsat"] > 0
    print(f"ldpc[noisy]: {int(early.sum())} of 48 frames converge before iteration 20, {int(full.sum())} do not; iterations {sorted(set(want['iterations'].tolist()))}; "
          f"{int((want['x'] == c).all(axis=1).sum())} decoded as sent")
    assert early.sum() >= 12 and full.sum() >= 12 and len(set(want["iterations"][early].tolist())) > 1      # on the reference alone
    assert (want["x"][early] == c[early]).all()
    _assert_rows(_run(base, Z, y, 20), want, 24 * Z)


def test_one_call_per_frame_and_a_permuted_packing_give_the_same_bytes():
    Z, base, c, y, want = noisy()
    N, n = 24 * Z, 48
    perm = np.random.default_rng(5).permutation(n + 3)[:n]                      # other rows, of a larger table, in another order
    order = np.random.default_rng(6).permutation(n)
    got = _run(base, Z, y[order], 20, rows=perm[order], n_rows=n + 3)
    _assert_rows(got, want, N, rows=perm)
    spare = np.setdiff1d(np.arange(n + 3), perm)
    assert (got[0][spare] == BITS_FILL).all() and (got[1][spare] == OUT_FILL).all() and (got[2][spare] == POST_FILL).all()     # rows of no frame stay untouched
    for k in (0, 7, 23, 24, 40, 47):
        one = {key: want[key][k:k + 1] for key in ("x", "iterations", "unsat", "post")}
        _assert_rows(_run(base, Z, y[k:k + 1], 20), one, N)


@pytest.mark.parametrize("scale, iterations", [(1, 20), (12, 1), (12, 100), (16, 20)])
def test_decode_scale_and_iterations(scale, iterations):
    Z, base, c, y, _ = noisy()
    y = y[::6]
    want = R.decode(y, base, Z, iterations, scale)
    assert iterations != 100 or (want["iterations"].max() == 100 and want["iterations"].min() < 20)
    got = _run(base, Z, y, iterations, scale, post=False)                        # post = None is accepted
    assert got[2] is None
    _assert_rows(got, want, 24 * Z)


# ------------------------------------------------------------------------------------------------------------- launch 3
def _run_check(xs, ys, N, K, whiten, spec):
    from sy11 import ops
    n = len(xs)
    bits = np.stack([np.packbits(x) for x in xs])
    data = torch.full((n, (K + 7) // 8 + 2), DATA_FILL, dtype=torch.uint8, device=DEV)
    rows = torch.full((n, 5), OUT_FILL, dtype=torch.int32, device=DEV)
    ops.ldpc_check(torch.from_numpy(np.stack(ys)).to(DEV), torch.from_numpy(bits).to(DEV), np.arange(n), N, K, data, rows,
                   whiten=None if whiten is None else torch.from_numpy(np.asarray(whiten[:K], dtype=np.uint8)).to(DEV), crc=spec)
    return data.cpu().numpy(), rows.cpu().numpy()


SPECS = dict(FEC.CRCS, **{"none": None, "in only": dict(width=12, poly=0x80F, init=0x5A5, refin=True, refout=False, xorout=0x0FF)})


@pytest.mark.parametrize("name", list(SPECS))
def test_check_crc_whitening_and_channel_errors(name):
    spec = SPECS[name]
    W = spec["width"] if spec else 0
    g = np.random.default_rng(31)
    whiten = FEC.lfsr_bits((4, 7), [1, 1, 0, 1, 0, 0, 1], 200)
    msg = FEC.bits_of_bytes(b"123456789")
    for extra, wh in ((30, None), (35, whiten)):                                # N = K + extra: the bits beyond K are counted against the channel, and not written
        K = 72 + W
        N = K + extra + (K + extra) % 2
        xs, ys = [], []
        for k in range(4):
            m = msg if k == 0 else g.integers(0, 2, 72).astype(np.uint8)
            info = np.concatenate((m, FEC.int_bits(FEC.crc(m, spec), W))) if spec else m
            if k == 3 and spec:
                info[5] ^= 1                                                    # a wrong message under a good check field
            x = np.concatenate((info ^ (wh[:K] if wh is not None else 0), g.integers(0, 2, N - K))).astype(np.uint8)
            y = (1 - 2 * x.astype(np.int64)) * g.integers(1, 128, N)
            y[g.random(N) < 0.2] = 0                                            # erasures
            flip = g.random(N) < 0.1
            y[flip] = -y[flip]
            xs.append(x), ys.append(y.astype(np.int8))
        data, rows = _run_check(xs, ys, N, K, wh, spec)
        for k in range(4):
            want = R.check(ys[k], xs[k], K, wh, spec)
            nb = (K + 7) // 8
            assert np.array_equal(data[k, :nb], want["data"]) and not data[k, nb:].any(), (name, extra, k)
            assert rows[k].view(np.uint32)[:2].tolist() == [want["crc_calc"], want["crc_recv"]], (name, extra, k)
            assert rows[k, 2:].tolist() == [want["crc_ok"], want["channel_errors"], want["n_channel"]], (name, extra, k)
            assert want["channel_errors"] > 0 and want["n_channel"] < N
            assert want["crc_ok"] == (-1 if spec is None else int(k != 3))
        if name in FEC.CRCS and wh is None:                                      # the anchors on the device
            assert int(rows[0].view(np.uint32)[0]) == {"crc32": 0xCBF43926, "crc16-ccitt-false": 0x29B1, "crc16-x25": 0x906E, "crc8": 0xF4}[name]


# ------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_raise_and_write_nothing():
    from sy11 import _lib, ops
    from sy11.data.ldpc import LDPCENTRY, ldpc_code
    E_ = _lib.Sy11Error
    p = lambda v: C.c_void_p(v.data_ptr())                                    # noqa: E731
    Z, base = 3, CODES["Z3 2x4"][1]
    cd = ldpc_code(base, Z)                                                     # N = 12, K = 6
    soft = torch.from_numpy(np.random.default_rng(1).integers(-127, 128, (2, 14)).astype(np.int8)).to(DEV)
    bits = torch.full((2, 3), BITS_FILL, dtype=torch.uint8, device=DEV)
    out = torch.full((2, 2), OUT_FILL, dtype=torch.int32, device=DEV)
    post = torch.full((2, 13), POST_FILL, dtype=torch.int16, device=DEV)
    data = torch.full((2, 2), DATA_FILL, dtype=torch.uint8, device=DEV)
    rows = torch.full((2, 5), OUT_FILL, dtype=torch.int32, device=DEV)
    fr = np.array([1, 0])
    # the arguments themselves are good: the same calls on copies go through
    ops.ldpc_decode(soft, fr, cd, bits.clone(), out.clone(), post=post.clone())
    ops.ldpc_check(soft, bits.clone().zero_(), fr, 12, 6, data.clone(), rows.clone())
    good = dict(soft=soft, frames=fr, code=cd, bits=bits, out=out, post=post, iterations=20, scale=12)
    for bad in (dict(code=7), dict(code={"Z": 3}), dict(code={"Z": 0, "base": base}), dict(code={"Z": 3, "base": np.where(base == 2, 3, base)}), dict(code={"Z": 3, "base": base[:, :3]}),
                dict(code={"Z": 3, "base": np.array([[0, -1, 2, -1], [1, -1, -1, -1]])}), dict(code={"Z": 4, "base": np.array([[0, 1, 2, 3], [1, 2, 3, 0]])}),
                dict(iterations=0), dict(iterations=101), dict(iterations=2.0), dict(scale=0), dict(scale=17), dict(scale=True), dict(frames=np.array([0, 2])),
                dict(frames=np.array([0, 0])), dict(frames=np.array([-1, 0])), dict(frames=np.zeros(0, dtype=np.int64)), dict(frames=np.array([0.0, 1.0])), dict(soft=soft.cpu()),
                dict(soft=soft[:, :11]), dict(soft=soft.to(torch.uint8)), dict(bits=bits[:, :1]), dict(bits=bits[:1]), dict(bits=bits.to(torch.int8)), dict(out=out[:, :1]),
                dict(out=out.to(torch.int64)), dict(out=out.cpu()), dict(post=post[:, :11]), dict(post=post.to(torch.int32)), dict(post=post[:1])):
        a = dict(good)
        a.update(bad)
        with pytest.raises(ValueError, match="ldpc_decode"):
            ops.ldpc_decode(a["soft"], a["frames"], a["code"], a["bits"], a["out"], post=a["post"], iterations=a["iterations"], scale=a["scale"])
    crc8 = FEC.CRCS["crc8"]
    wide = dict(soft=torch.zeros((2, 40), dtype=torch.int8, device=DEV), bits=torch.zeros((2, 5), dtype=torch.uint8, device=DEV), N=40, K=20,
                data=torch.full((2, 3), DATA_FILL, dtype=torch.uint8, device=DEV))
    ops.ldpc_check(wide["soft"], wide["bits"], fr, 40, 20, wide["data"].clone(), rows.clone(), crc=crc8)
    good = dict(soft=soft, bits=bits, frames=fr, N=12, K=6, data=data, rows=rows, whiten=None, crc=None)
    for bad in (dict(N=13), dict(N=0), dict(N=12.0), dict(K=0), dict(K=12), dict(N=16), dict(frames=np.array([0, 2])), dict(frames=np.array([1, 1])), dict(soft=soft.cpu()),
                dict(bits=bits[:, :1]), dict(data=data[:1]), dict(data=data.to(torch.int8)), dict(rows=rows[:, :4]), dict(rows=rows.to(torch.int64)),
                dict(whiten=torch.zeros(5, dtype=torch.uint8, device=DEV)), dict(whiten=torch.zeros(6, dtype=torch.int32, device=DEV)), dict(crc="crc8"), dict(crc=dict(width=8)),
                dict(crc=crc8), dict(wide, crc=dict(crc8, width=7)), dict(wide, crc=dict(crc8, poly=0x107)), dict(wide, crc=dict(crc8, refin=2)), dict(wide, crc=dict(crc8, refin=True)),
                dict(wide, crc=dict(crc8, width=33)), dict(wide, crc=dict(crc8, width=24, poly=7))):
        a = dict(good)
        a.update(bad)
        with pytest.raises(ValueError, match="ldpc_check"):
            ops.ldpc_check(a["soft"], a["bits"], a["frames"], a["N"], a["K"], a["data"], a["rows"], whiten=a["whiten"], crc=a["crc"])
    # the library itself
    keep = []

    def i32(v):
        host = np.asarray(v, dtype=np.int32)
        t = torch.from_numpy(host.copy()).to(DEV)
        keep.extend((host, t))
        return [C.c_void_p(host.ctypes.data), p(t)]

    def entries(v):
        host = np.array(v, dtype=LDPCENTRY)
        t = torch.from_numpy(host.view(np.int32).copy()).to(DEV)
        keep.extend((host, t))
        return [C.c_void_p(host.ctypes.data), p(t)]

    def code(**kw):
        a = dict(Z=3, mb=2, nb=4, n_entry=6)
        a.update(kw)
        c = _lib.LdpcCode(a["Z"], a["mb"], a["nb"], a["n_entry"])
        keep.append(c)
        return C.byref(c)
    ENT = [tuple(int(v) for v in e) for e in cd.entry]
    assert ENT == [(0, 0), (2, 2), (0, 1), (1, 2), (2, 0), (3, 1)] and cd.layer.tolist() == [0, 2, 6]

    def lib1(r=(1, 0), lay=(0, 2, 6), ent=ENT, it=20, sc=12, **kw):
        return [len(r)] + i32(r) + [code(**kw)] + i32(lay) + entries(ent) + [it, sc, 2, 14, p(soft), 3, p(bits), p(out), 13, p(post), None]
    spec0 = _lib.FecCrc()

    def lib2(r=(1, 0), N=12, K=6, s=spec0):
        return [len(r)] + i32(r) + [N, K, None, C.byref(s), 2, 14, p(soft), 3, p(bits), 2, p(data), p(rows), None]
    _lib.call("sy11_ldpc_decode", *(lib1()[:14] + [p(bits.clone()), p(out.clone()), 13, p(post.clone()), None]))     # the table of the library test is good
    for kw in (dict(Z=0), dict(Z=513), dict(mb=0), dict(nb=2), dict(nb=129), dict(nb=5), dict(n_entry=3), dict(n_entry=65)):
        with pytest.raises(E_, match="ldpc_decode"):
            _lib.call("sy11_ldpc_decode", *lib1(**kw))
    for kw in (dict(it=0), dict(it=101), dict(sc=0), dict(sc=17), dict(lay=(1, 2, 6)), dict(lay=(0, 2, 5)), dict(lay=(0, 0, 6)), dict(lay=(0, 1, 6)), dict(lay=(0, 5, 6))):
        with pytest.raises(E_, match="ldpc_decode"):
            _lib.call("sy11_ldpc_decode", *lib1(**kw))
    for at, v, what in ((1, (4, 1), "column 4"), (0, (-1, 0), "column -1"), (3, (1, 3), "shift 3"), (2, (0, -1), "shift -1"), (1, (0, 1), "names column 0 twice"),
                        (5, (0, 0), "names column 0 twice"), (3, (3, 2), "names column 3 twice")):
        e = list(ENT)
        e[at] = v
        with pytest.raises(E_, match="ldpc_decode: .*" + what):
            _lib.call("sy11_ldpc_decode", *lib1(ent=e))
    for r in ((0, 2), (-1, 0), (1, 1)):
        with pytest.raises(E_, match="ldpc_decode: frame [01] reads row"):
            _lib.call("sy11_ldpc_decode", *lib1(r))
        with pytest.raises(E_, match="ldpc_check: frame [01] reads row"):
            _lib.call("sy11_ldpc_check", *lib2(r))
    for pos, v in ((0, 0), (1, None), (2, None), (3, None), (4, None), (5, None), (6, None), (7, None), (12, None), (14, None), (15, None), (10, 0), (10, 1), (11, 11), (13, 1),
                   (16, 11), (15, C.c_void_p(out.data_ptr() + 2)), (17, C.c_void_p(post.data_ptr() + 1))):
        a = lib1()
        a[pos] = v
        with pytest.raises(E_, match="ldpc_decode"):
            _lib.call("sy11_ldpc_decode", *a)
    for pos, v in ((0, 0), (1, None), (2, None), (6, None), (9, None), (11, None), (13, None), (14, None), (3, 13), (3, 0), (4, 0), (4, 12), (7, 0), (7, 1), (8, 11), (10, 1),
                   (12, 0), (14, C.c_void_p(rows.data_ptr() + 2))):
        a = lib2()
        a[pos] = v
        with pytest.raises(E_, match="ldpc_check"):
            _lib.call("sy11_ldpc_check", *a)
    for bad in (_lib.FecCrc(7, 7, 0, 0, 0, 0), _lib.FecCrc(33, 7, 0, 0, 0, 0), _lib.FecCrc(8, 7, 0, 0, 0, 0)):
        with pytest.raises(E_, match="ldpc_check"):
            _lib.call("sy11_ldpc_check", *lib2(s=bad))
    torch.cuda.synchronize()
    assert bool((wide["data"] == DATA_FILL).all()) and bool((bits == BITS_FILL).all()) and bool((out == OUT_FILL).all()) and bool((post == POST_FILL).all()) and bool((data == DATA_FILL).all()) and bool((rows == OUT_FILL).all())


# ------------------------------------------------------------------------------------------------------------- end to end
E2E_Z, E2E_CRC = 27, "crc16-ccitt-false"
E2E_BASE = CODES["Z27 12x24"][1]                                                # N = 648, K = 324: 308 message bits and the check field
WHITEN = FEC.lfsr_bits((4, 7), [1, 1, 0, 1, 0, 0, 1], 324)
RS_CODE = RS.code(20, 16)                                                       # a shortened RS(20, 16) codeword is 160 bits
RS_Z, RS_BASE = 40, R.staircase_base(4, 4, 40, 11, 3)                            # K = 160, N = 320
# label, order, sps, M, offset (cycles / sample), snr_db, seed, stream indices of the two frames
E2E = (("bpsk 3.3, -3 dB", 2, 3.3, 5400, 5.3 / 64, -3.0, 61, (60, 820)), ("qpsk 2.5, 0 dB", 4, 2.5, 2400, 0.02, 0.0, 62, (80, 500)))
E2E_RS = ("bpsk 3.3, -2 dB, RS(20, 16) inside", 2, 3.3, 2900, 5.3 / 64, -2.0, 63, (60, 440))


def _reference_chain(c, N, base, Z, whiten, spec):
    """The reference demodulation, frame search and LDPC decoding of a clip's embedded frames -> list of dicts (of ``R.decode`` and ``R.check``, with ``soft``)."""
    from tests._demod_ref import demodulate
    ref = demodulate(c["x"], FEC.FS, c["rate"], c["offset"], c["order"], span=FEC.SPAN)
    r = ref["r"].astype(np.complex64)
    found = F.find(r, c["bits"], c["order"], FEC.THRESHOLD, c["need"])
    m0 = F.stream_index(ref["T0"], ref["STEP"], ref["i_first"], c["sps"], c["u0"], FEC.SPAN)
    out = []
    for at in c["at"]:
        k = found["position"].tolist().index(at - m0)
        L = len(c["bits"]) // (c["order"] // 2)
        y = FEC.soft(r[at - m0 + L:at - m0 + L + c["need"]], c["order"], found["rotation"][k], FEC.scale_of(16.0, ref["gain"], c["order"]), None, N // 2)
        dec = R.decode(y, base, Z, 20, 12)
        chk = R.check(y, dec["x"][0], N - base.shape[0] * Z, whiten, spec)
        chk.update(soft=y, iterations=int(dec["iterations"][0]), unsat=int(dec["unsat"][0]))
        out.append(chk)
    return out


def _clip(label, order, sps, M, off, snr, seed, at, sent):
    """A clip with the codewords ``sent`` (one per entry of ``at``) behind the sync word."""
    bits = FEC.word_bits(order)
    embed = {j: np.concatenate((F.decisions(bits, order), F.decisions(c, order))) for j, c in zip(at, sent)}
    x, d, u0 = F.clip(order, M, seed, sps, off, snr, embed, span=FEC.SPAN)
    N = len(sent[0])
    return {"label": label, "x": x, "u0": u0, "sps": sps, "rate": (1.0 / sps - 0.25 * FEC.BIN) * FEC.FS, "offset": (off + FEC.BIN / 16) * FEC.FS, "order": order, "bits": bits, "at": at,
            "need": -(-N // (order // 2))}


@functools.lru_cache(maxsize=None)
def e2e_clips():
    """The BPSK and the QPSK clip: two frames each of the 12 x 24, Z = 27 code, 308 message bits and a crc16-ccitt-false, whitened; and the clip whose two frames of
    the 4 x 8, Z = 40 code carry a shortened RS(20, 16) codeword each, one of them with two of its 20 bytes sent wrong.  With each the reference chain.  Computed
    once; leave it unchanged."""
    from sy11.data.ldpc import ldpc_encode
    out = []
    for label, order, sps, M, off, snr, seed, at in E2E:
        g = np.random.default_rng(3000 + seed)
        msgs = [g.integers(0, 2, 308).astype(np.uint8) for _ in at]
        infos = [np.concatenate((m, FEC.int_bits(FEC.crc(m, FEC.CRCS[E2E_CRC]), 16))) for m in msgs]
        sent = [ldpc_encode(i ^ WHITEN, {"Z": E2E_Z, "base": E2E_BASE}) for i in infos]
        c = _clip(label, order, sps, M, off, snr, seed, at, sent)
        c.update(msg=msgs, info=infos, sent=sent, ref=_reference_chain(c, 648, E2E_BASE, E2E_Z, WHITEN, FEC.CRCS[E2E_CRC]))
        out.append(c)
    label, order, sps, M, off, snr, seed, at = E2E_RS
    g = np.random.default_rng(3000 + seed)
    msgs = [g.integers(0, 256, 16).astype(np.uint8) for _ in at]
    words = [RS.encode(m[None, :], RS_CODE)[0].astype(np.uint8) for m in msgs]
    wrong = [w.copy() for w in words]
    wrong[1][[3, 17]] ^= np.array([0x41, 0x80], dtype=np.uint8)                  # what the LDPC code protects already holds two byte errors: the outer code's share
    sent = [ldpc_encode(np.unpackbits(w), {"Z": RS_Z, "base": RS_BASE}) for w in wrong]
    c = _clip(label, order, sps, M, off, snr, seed, at, sent)
    c.update(msg=msgs, words=words, wrong=wrong, sent=sent, ref=_reference_chain(c, 320, RS_BASE, RS_Z, None, None))
    out.append(c)
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
    """``demodulate`` -> ``find_frames`` -> ``decode_ldpc`` of the three clips, once.  Shared and left unchanged."""
    from sy11 import _lib
    from sy11.engine.model import YOLO
    y = YOLO.__new__(YOLO)
    y.device = DEV
    out = []
    for k, c in enumerate(e2e_clips()):
        ext = _extraction([c["x"]])
        d = y.demodulate(ext, symbol_rate=[c["rate"]], offset=[c["offset"]], order=[c["order"]], span=FEC.SPAN)
        f = y.find_frames(d, [list(c["bits"])], payload=c["need"], threshold=FEC.THRESHOLD)
        args = dict(code={"Z": E2E_Z, "base": E2E_BASE}, whiten=WHITEN, crc=E2E_CRC) if k < 2 else dict(code={"Z": RS_Z, "base": RS_BASE.tolist()})
        _lib.PROFILE = []
        try:
            dec = y.decode_ldpc(f, d, **args)
            calls = [k[0] for k in _lib.PROFILE]
        finally:
            _lib.PROFILE = None
        assert calls == ["sy11_fec_soft", "sy11_ldpc_decode", "sy11_ldpc_check"]    # three launches, whatever the number of frames
        out.append((c, ext, d, f, dec, args))
    return y, out


def _embedded(c, d, f):
    """The rows of the frames at the embedded positions."""
    m0 = F.stream_index(d.raw["T0"][0], d.raw["STEP"][0], d.raw["i_first"][0], c["sps"], c["u0"], FEC.SPAN)
    rows = []
    for at in c["at"]:
        k = np.flatnonzero(f.position == at - m0)
        assert k.shape[0] == 1
        rows.append(int(k[0]))
    return rows


def test_reference_chain_reads_the_embedded_frames_through_channel_errors():
    """On the reference alone: every embedded frame has raw bit errors and decodes, before iteration 20, to what was sent."""
    for k, c in enumerate(e2e_clips()):
        for j, ref in enumerate(c["ref"]):
            assert ref["unsat"] == 0 and ref["iterations"] < 20 and ref["channel_errors"] > 0, (c["label"], j, ref["iterations"], ref["channel_errors"])
            if k < 2:
                assert ref["crc_ok"] == 1 and np.array_equal(ref["v"], c["info"][j])
            else:
                assert np.array_equal(ref["data"], c["wrong"][j])
        print(f"ldpc[{c['label']}]: the reference needs {[r['iterations'] for r in c['ref']]} iterations against {[r['channel_errors'] for r in c['ref']]} channel errors")


def test_demodulate_find_frames_decode_ldpc_reads_what_was_sent(chain):
    from sy11.data.ldpc import LdpcDecoded
    y, cases = chain
    for c, ext, d, f, dec, args in cases[:2]:
        assert isinstance(dec, LdpcDecoded) and len(dec) == len(f) >= 2 and dec.data.device.type == "cuda" and dec.data.shape == (len(f), 41) and dec.plan.n_info == 324
        assert np.array_equal(dec.clip, f.clip) and np.array_equal(dec.word, f.word) and np.array_equal(dec.position, f.position) and dec.cls.tolist() == ext.cls.tolist()
        data = dec.data.cpu().numpy()
        r = d.symbols[0].cpu().numpy()
        L = len(c["bits"]) // (c["order"] // 2)
        for k in range(len(f)):
            p, q = int(f.position[k]), int(f.rotation[k])
            if int(f.n_payload[k]) < c["need"]:
                assert not dec.valid[k] and dec.reason[k] == "short" and not data[k].any() and not dec.soft(k).any().item() and not dec.posterior(k).any().item()
                assert np.isnan(dec.ber[k]) and not dec.crc_ok[k] and not dec.converged[k] and dec[k]["iterations"] == 0
                continue
            # the reference on the device's own symbols, gain and hit: every column, exactly
            soft = FEC.soft(r[p + L:p + L + c["need"]], c["order"], q, FEC.scale_of(16.0, d.gain[0], c["order"]), None, 324)
            ref = R.decode(soft, E2E_BASE, E2E_Z, 20, 12)
            want = R.check(soft, ref["x"][0], 324, WHITEN, FEC.CRCS[E2E_CRC])
            assert dec.valid[k] and dec.reason[k] == "" and np.array_equal(dec.soft(k).cpu().numpy(), soft) and np.array_equal(dec.posterior(k).cpu().numpy(), ref["post"][0])
            assert (int(dec.iterations[k]), int(dec.unsatisfied[k]), bool(dec.converged[k])) == (int(ref["iterations"][0]), int(ref["unsat"][0]), ref["unsat"][0] == 0)
            assert np.array_equal(data[k], want["data"]) and np.array_equal(dec.bits(k), want["v"]) and np.array_equal(dec.raw["decided"][k].cpu().numpy(), np.packbits(ref["x"][0]))
            assert (int(dec.channel_errors[k]), int(dec.n_channel[k]), dec.ber[k]) == (want["channel_errors"], want["n_channel"], want["channel_errors"] / want["n_channel"])
            assert (int(dec.crc_calc[k]), int(dec.crc_recv[k]), bool(dec.crc_ok[k])) == (want["crc_calc"], want["crc_recv"], bool(want["crc_ok"]))
        errs = []
        for j, k in enumerate(_embedded(c, d, f)):
            assert dec.valid[k] and dec.crc_ok[k] and dec.converged[k] and np.array_equal(dec.bits(k), c["info"][j]) and np.array_equal(dec.message(k), c["msg"][j])
            assert np.array_equal(np.unpackbits(dec.raw["decided"][k].cpu().numpy())[:648], c["sent"][j])
            errs.append(int(dec.channel_errors[k]))
        assert min(errs) > 0
        print(f"ldpc[{c['label']}]: {len(f)} frames, {int(dec.valid.sum())} decoded, {int(dec.converged.sum())} converged; the embedded frames had {errs} channel errors, "
              f"iterations {[int(dec.iterations[k]) for k in _embedded(c, d, f)]}")


def test_predictor_gives_the_same_rows_and_nothing_is_launched_without_a_valid_frame(chain, tmp_path):
    from sy11 import _lib
    from sy11.engine.predictor import DetectionPredictor
    y, cases = chain
    c, ext, d, f, dec, args = cases[1]
    pred = DetectionPredictor.__new__(DetectionPredictor)
    pred.device = DEV
    again = pred.decode_ldpc(f, d, **args)
    for key in dec.COLUMNS:
        assert np.array_equal(getattr(again, key), getattr(dec, key), equal_nan=True), key
    assert np.array_equal(again.data.cpu().numpy(), dec.data.cpu().numpy()) and again.reason.tolist() == dec.reason.tolist()
    out = dec.save(tmp_path / "l")
    z = np.load(tmp_path / "l" / "ldpc.npz")
    index = json.loads((tmp_path / "l" / "ldpc.json").read_text())
    k = _embedded(c, d, f)[0]
    assert out == str(tmp_path / "l") and np.array_equal(z["data"], dec.data.cpu().numpy()) and np.array_equal(z["iterations"], dec.iterations)
    assert index["code"]["Z"] == 27 and index["crc"]["name"] == E2E_CRC and len(index["frames"]) == len(dec) and index["frames"][k]["converged"] is True
    # argument errors come before the device; an empty Frames, or one without a valid frame, launches nothing
    none = y.find_frames(d, [[0, 1] * 40], payload=c["need"], threshold=0.9)
    deaf = copy.copy(d)
    deaf.gain = np.zeros_like(d.gain)
    _lib.PROFILE = []
    try:
        with pytest.raises(ValueError, match="iterations"):
            y.decode_ldpc(f, d, code=args["code"], iterations=0)
        with pytest.raises(ValueError, match="not found in this demodulation"):
            y.decode_ldpc(f, cases[0][2], code=args["code"])
        with pytest.raises(ValueError, match="could be decoded"):
            y.decode_ldpc(f, d, code={"Z": 54, "base": E2E_BASE})             # a longer code than the payload that was read
        e = y.decode_ldpc(none, d, **args)
        g = y.decode_ldpc(f, deaf, **args)
        calls = [k[0] for k in _lib.PROFILE]
    finally:
        _lib.PROFILE = None
    assert calls == [] and len(none) == 0 and len(e) == 0 and e.data.shape == (0, 41) and e.valid.shape == (0,) and e.raw["soft"] is None
    assert len(g) == len(f) and not g.valid.any() and set(g.reason.tolist()) <= {"gain", "short"} and "gain" in g.reason.tolist() and not g.data.any().item()
    assert not g.soft(0).any().item() and g.soft(0).shape == (648,) and g.posterior(0).shape == (648,) and not g.converged.any()


def test_a_frame_that_carries_a_reed_solomon_codeword_goes_on_through_correct(chain):
    y, cases = chain
    c, ext, d, f, dec, args = cases[2]
    assert dec.plan.n_info == 160 and dec.data.shape == (len(f), 20)
    cor = y.correct(dec, code=RS_CODE)
    assert len(cor) == len(dec) and np.array_equal(cor.valid, dec.valid)
    for j, k in enumerate(_embedded(c, d, f)):
        assert dec.valid[k] and dec.converged[k] and dec.channel_errors[k] > 0 and dec.data[k].cpu().numpy().tobytes() == c["wrong"][j].tobytes()
        assert cor.ok[k] and cor.message(k) == c["msg"][j].tobytes() and cor.errors[k].tolist() == [2 * j]
    print(f"ldpc[{c['label']}]: the outer code corrects {[cor.errors[k].tolist() for k in _embedded(c, d, f)]} byte errors")
