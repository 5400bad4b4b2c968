"""CPU: the result tables of the frame path (``Decoded``, ``LdpcDecoded``, ``Corrected``) built by hand from fixed small arrays and CPU tensors, no device and no
library: ``obj[k]``, ``bits``, ``message``, ``soft`` / ``posterior``, and what ``save`` writes (the arrays of the ``.npz`` by name, dtype and value; the ``.json`` with its key
order) against the literals of ``EXPECTED``.

THE LITERALS WERE PRODUCED BY RUNNING THIS SAME CONSTRUCTION (``_build`` and ``_observe`` below, unchanged) ON THE COMMIT BEFORE THE THREE CLASSES GOT THEIR COMMON BASE,
when each still carried its own ``__init__`` / ``__getitem__`` / ``message`` / ``save``; none comes from the code under test.  They pin every public attribute, the names and
dtypes of the saved arrays and the keys, key order and values of the JSON record.

A table has ONE plan, so whether the message before the check field is whole bytes is a property of the table, not of a frame: every class is therefore built twice,
three frames each (two valid, one invalid): once with a whole-byte message and classes / names set, once with a message that is not whole bytes (``Corrected``: without a
check; its messages are bytes always) and without classes.  The second frame of a ``Corrected`` has a codeword that could not be corrected."""
import json
import math
import os

import numpy as np
import pytest
import torch

from sy11.data.correct import Corrected, CorrectPlan
from sy11.data.decode import CRCS, Decoded, DecodePlan
from sy11.data.ldpc import LdpcCode, LdpcDecoded, LdpcPlan

DATA = [[0x31, 0x32, 0x5A, 0xC0], [0xDE, 0xAD, 0xBE, 0xE0], [0, 0, 0, 0]]
FRAME = dict(valid=np.array([True, True, False]), clip=np.array([0, 1, 1]), word=np.array([0, 0, 1]), position=np.array([17, 250, 3])).items()
CHECKED = dict(channel_errors=np.array([3, 0, 0]), n_channel=np.array([60, 0, 0]), ber=np.array([0.05, np.nan, np.nan]), crc_ok=np.array([True, False, False]),
               crc_calc=np.array([0x5A, 0xF00DFACE, 0], dtype=np.uint32), crc_recv=np.array([0x5A, 0xBE, 0], dtype=np.uint32)).items()
PER_FRAME = (np.array([2, 4, 2]), np.array([1.5, 2.0, 0.0]), np.array([49, 282, 35]), np.array([64, 64, 64]))         # order, gain, sym_off, n_payload: frame 2 has no gain
META = dict(rows=np.array([5, 9]), cls=np.array([1, 0]), conf=np.array([0.5, 0.75]), names={0: "a", 1: "b"})
WHITEN = np.array([1, 0, 1, 1, 0, 0, 1, 0] * 4, dtype=np.uint8)


def _build(case):
    kind, whole = case.split("-")
    whole = whole == "whole"
    meta = META if whole else {}
    reason = np.array(["", "", "gain"], dtype=object)
    data = torch.tensor(DATA, dtype=torch.uint8)
    n_info = 24 if whole else 28
    if kind == "decoded":
        plan = DecodePlan(n_info, (0o171, 0o133), True, n_info + 6, np.array([1, 1, 1, 0], dtype=np.uint8) if whole else None, None if whole else WHITEN[:n_info].copy(),
                          dict(CRCS["crc8"], name="crc8"), 32.0, *PER_FRAME)
        cols = dict(FRAME, metric=np.array([1234, -7, 0]), end_state=np.array([0, 63, 0]), **dict(CHECKED))
        soft = (torch.arange(3 * 2 * plan.T, dtype=torch.int32) % 251 - 125).to(torch.int8).reshape(3, 2 * plan.T)
        return Decoded(plan, cols, reason, data, {"soft": soft if whole else None, "decided": None, "out": None, "rows": None}, **meta)
    if kind == "ldpc":
        base = np.array([[1, -1, 0, 2, -1, 3, 0, -1], [-1, 2, 3, -1, 1, 0, 0, 0]] if whole else [[1, -1, 0, 2, -1, 3, 1, 0, -1], [-1, 2, 3, -1, 1, 0, -1, 0, 0]], dtype=np.int64)
        code = LdpcCode(base, 4)
        assert code.K == n_info
        plan = LdpcPlan(code, 20, 12, WHITEN[:n_info].copy() if whole else None, dict(CRCS["crc8"], name="crc8"), 16.0, *PER_FRAME)
        cols = dict(FRAME, iterations=np.array([3, 20, 0]), unsatisfied=np.array([0, 5, 0]), converged=np.array([True, False, False]), **dict(CHECKED))
        soft = (torch.arange(3 * code.N, dtype=torch.int32) % 251 - 125).to(torch.int8).reshape(3, code.N)
        post = (torch.arange(3 * code.N, dtype=torch.int32) * 37 % 4001 - 2000).to(torch.int16).reshape(3, code.N)
        raw = {"soft": soft if whole else None, "decided": None, "out": None, "post": post if whole else None, "rows": None}
        return LdpcDecoded(plan, cols, reason, data, raw, **meta)
    code = dict(n=6, k=4, poly=0x11D, fcr=0, prim=1, name=None)
    plan = CorrectPlan(code, 2, 1, dict(CRCS["crc16-ccitt-false"], name="crc16-ccitt-false") if whole else None, [True, True, False])
    cols = dict(FRAME, n_failed=np.array([0, 1, 0]), byte_errors=np.array([1, 1, 0]), bit_errors=np.array([3, 1, 0]), ok=np.array([True, False, False]),
                **{k: v for k, v in CHECKED if k.startswith("crc")})
    info = torch.tensor([row + row[::-1] for row in DATA], dtype=torch.uint8)
    return Corrected(plan, cols, plan.reason, np.array([[1, 0], [-1, 1], [0, 0]]), info, {"cw": None, "rows": None}, **meta)


def _plain(v):
    """NaN as the string "nan" (it equals itself), containers as lists / dicts of plain values."""
    if isinstance(v, dict):
        return {k: _plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    return "nan" if isinstance(v, float) and math.isnan(v) else v


def _observe(obj, directory):
    n = len(obj)
    out = {"len": n, "items": [_plain(obj[k]) for k in range(n)], "last_is_minus_one": _plain(obj[-1]) == _plain(obj[n - 1])}
    msg = [obj.message(k) for k in range(n)]
    out["message"] = [["bytes", m.hex()] if isinstance(m, bytes) else ["bits", str(m.dtype), m.tolist()] for m in msg]
    if hasattr(obj, "bits"):
        out["bits"] = [[str(b.dtype), "".join(str(v) for v in b.tolist())] for b in (obj.bits(k) for k in range(n))]
    for name in ("soft", "posterior"):                                          # device views: the dtype, the length and the first six values
        if hasattr(obj, name):
            out[name] = [[str(g.dtype), list(g.shape), g[:6].tolist()] for g in (getattr(obj, name)(k) for k in range(n))]
    out["returned"] = obj.save(directory) == os.fspath(directory)
    out["files"] = sorted(os.listdir(directory))
    stem = out["files"][0].split(".")[0]
    with np.load(os.path.join(directory, stem + ".npz")) as z:
        out["npz"] = [[k, str(z[k].dtype), _plain(z[k].tolist())] for k in z.files]
    with open(os.path.join(directory, stem + ".json")) as f:
        out["json"] = _plain(json.load(f, object_pairs_hook=list))
    return out


CASES = ("decoded-whole", "decoded-bits", "ldpc-whole", "ldpc-bits", "corrected-whole", "corrected-none")

# ---- the record of the commit before the common base.  ``obj[k]`` per class (the two builds of a class share their columns), in the order of its keys:
ITEMS = {
    "decoded": [
        {"valid": True, "clip": 0, "word": 0, "position": 17, "metric": 1234, "end_state": 0, "channel_errors": 3, "n_channel": 60, "ber": 0.05, "crc_ok": True, "crc_calc": 90, "crc_recv": 90, "reason": ""},
        {"valid": True, "clip": 1, "word": 0, "position": 250, "metric": -7, "end_state": 63, "channel_errors": 0, "n_channel": 0, "ber": "nan", "crc_ok": False, "crc_calc": 4027448014, "crc_recv": 190, "reason": ""},
        {"valid": False, "clip": 1, "word": 1, "position": 3, "metric": 0, "end_state": 0, "channel_errors": 0, "n_channel": 0, "ber": "nan", "crc_ok": False, "crc_calc": 0, "crc_recv": 0, "reason": "gain"},
    ],
    "ldpc": [
        {"valid": True, "clip": 0, "word": 0, "position": 17, "iterations": 3, "unsatisfied": 0, "converged": True, "channel_errors": 3, "n_channel": 60, "ber": 0.05, "crc_ok": True, "crc_calc": 90, "crc_recv": 90, "reason": ""},
        {"valid": True, "clip": 1, "word": 0, "position": 250, "iterations": 20, "unsatisfied": 5, "converged": False, "channel_errors": 0, "n_channel": 0, "ber": "nan", "crc_ok": False, "crc_calc": 4027448014, "crc_recv": 190, "reason": ""},
        {"valid": False, "clip": 1, "word": 1, "position": 3, "iterations": 0, "unsatisfied": 0, "converged": False, "channel_errors": 0, "n_channel": 0, "ber": "nan", "crc_ok": False, "crc_calc": 0, "crc_recv": 0, "reason": "gain"},
    ],
    "corrected": [
        {"valid": True, "clip": 0, "word": 0, "position": 17, "n_failed": 0, "byte_errors": 1, "bit_errors": 3, "ok": True, "crc_ok": True, "crc_calc": 90, "crc_recv": 90, "reason": "", "errors": [1, 0]},
        {"valid": True, "clip": 1, "word": 0, "position": 250, "n_failed": 1, "byte_errors": 1, "bit_errors": 1, "ok": False, "crc_ok": False, "crc_calc": 4027448014, "crc_recv": 190, "reason": "", "errors": [-1, 1]},
        {"valid": False, "clip": 1, "word": 1, "position": 3, "n_failed": 0, "byte_errors": 0, "bit_errors": 0, "ok": False, "crc_ok": False, "crc_calc": 0, "crc_recv": 0, "reason": "undecoded", "errors": [0, 0]},
    ],
}
# the saved arrays: a column under its own name with this dtype, in the order of ``ITEMS``; then these, in this order
DTYPES = {"valid": "bool", "converged": "bool", "ok": "bool", "crc_ok": "bool", "ber": "float64", "crc_calc": "uint32", "crc_recv": "uint32"}      # every other column: int64
DATA8 = [[49, 50, 90, 192, 192, 90, 50, 49], [222, 173, 190, 224, 224, 190, 173, 222], [0, 0, 0, 0, 0, 0, 0, 0]]
AFTER = {"decoded": [["data", "uint8", DATA], ["reason", "<U4", ["", "", "gain"]]], "ldpc": [["data", "uint8", DATA], ["reason", "<U4", ["", "", "gain"]]],
         "corrected": [["data", "uint8", DATA8], ["errors", "int64", [[1, 0], [-1, 1], [0, 0]]], ["reason", "<U9", ["", "", "undecoded"]]]}
CRC8 = [["width", 8], ["poly", 7], ["init", 0], ["refin", False], ["refout", False], ["xorout", 0], ["name", "crc8"]]
CRC16 = [["width", 16], ["poly", 4129], ["init", 65535], ["refin", False], ["refout", False], ["xorout", 0], ["name", "crc16-ccitt-false"]]
RS64 = [["n", 6], ["k", 4], ["poly", 285], ["fcr", 0], ["prim", 1], ["name", None]]
BITS24, BITS28 = ["001100010011001001011010", "110111101010110110111110", "0" * 24], ["0011000100110010010110101100", "1101111010101101101111101110", "0" * 28]
# per build: message(k); soft(k) and posterior(k) as (length, the first six values); the files; the JSON header before "frames"; a frame's (message, name, class) after
# its columns
BUILDS = {
    "decoded-whole": dict(
        message=[["bytes", "3132"], ["bytes", "dead"], ["bytes", "0000"]], bits=BITS24,
        soft=[[60, [-125, -124, -123, -122, -121, -120]], [60, [-65, -64, -63, -62, -61, -60]], [60, [-5, -4, -3, -2, -1, 0]]], files=["decode.json", "decode.npz"],
        header=[["n_info", 24], ["polys", [121, 91]], ["tail", True], ["puncture", [1, 1, 1, 0]], ["whiten", None], ["crc", CRC8], ["soft_scale", 32.0], ["file", "decode.npz"]],
        tails=[["3132", "b", 1], ["dead", "a", 0], [None, "a", 0]]),
    "decoded-bits": dict(
        message=[["bits", "uint8", [int(c) for c in b[:20]]] for b in BITS28], bits=BITS28, soft=[[68, [0] * 6]] * 3, files=["decode.json", "decode.npz"],
        header=[["n_info", 28], ["polys", [121, 91]], ["tail", True], ["puncture", None], ["whiten", [1, 0, 1, 1, 0, 0, 1, 0] * 3 + [1, 0, 1, 1]], ["crc", CRC8], ["soft_scale", 32.0],
                ["file", "decode.npz"]],
        tails=[[None, None, None]] * 3),
    "ldpc-whole": dict(
        message=[["bytes", "3132"], ["bytes", "dead"], ["bytes", "0000"]], bits=BITS24,
        soft=[[32, [-125, -124, -123, -122, -121, -120]], [32, [-93, -92, -91, -90, -89, -88]], [32, [-61, -60, -59, -58, -57, -56]]],
        posterior=[[32, [-2000, -1963, -1926, -1889, -1852, -1815]], [32, [-816, -779, -742, -705, -668, -631]], [32, [368, 405, 442, 479, 516, 553]]], files=["ldpc.json", "ldpc.npz"],
        header=[["code", [["Z", 4], ["base", [[1, -1, 0, 2, -1, 3, 0, -1], [-1, 2, 3, -1, 1, 0, 0, 0]]]]], ["N", 32], ["K", 24], ["iterations", 20], ["scale", 12],
                ["whiten", [1, 0, 1, 1, 0, 0, 1, 0] * 3], ["crc", CRC8], ["soft_scale", 16.0], ["file", "ldpc.npz"]],
        tails=[["3132", "b", 1], ["dead", "a", 0], [None, "a", 0]]),
    "ldpc-bits": dict(
        message=[["bits", "uint8", [int(c) for c in b[:20]]] for b in BITS28], bits=BITS28, soft=[[36, [0] * 6]] * 3, posterior=[[36, [0] * 6]] * 3, files=["ldpc.json", "ldpc.npz"],
        header=[["code", [["Z", 4], ["base", [[1, -1, 0, 2, -1, 3, 1, 0, -1], [-1, 2, 3, -1, 1, 0, -1, 0, 0]]]]], ["N", 36], ["K", 28], ["iterations", 20], ["scale", 12], ["whiten", None],
                ["crc", CRC8], ["soft_scale", 16.0], ["file", "ldpc.npz"]],
        tails=[[None, None, None]] * 3),
    "corrected-whole": dict(
        message=[["bytes", "31325ac0c05a"], ["bytes", "deadbee0e0be"], ["bytes", "000000000000"]], files=["correct.json", "correct.npz"],
        header=[["code", RS64], ["interleave", 2], ["offset", 1], ["crc", CRC16], ["file", "correct.npz"]],
        tails=[["31325ac0c05a", "b", 1], ["deadbee0e0be", "a", 0], [None, "a", 0]]),
    "corrected-none": dict(
        message=[["bytes", "31325ac0c05a3231"], ["bytes", "deadbee0e0beadde"], ["bytes", "0000000000000000"]], files=["correct.json", "correct.npz"],
        header=[["code", RS64], ["interleave", 2], ["offset", 1], ["crc", None], ["file", "correct.npz"]],
        tails=[["31325ac0c05a3231", None, None], ["deadbee0e0beadde", None, None], [None, None, None]]),
}


def _expected(case):
    """The record of a build, laid out as ``_observe`` lays out what it sees.  A frame of the JSON is its ``obj[k]`` (NaN as null), then message, name and class."""
    kind, b, items = case.split("-")[0], BUILDS[case], ITEMS[case.split("-")[0]]
    out = {"len": 3, "items": items, "last_is_minus_one": True, "message": b["message"], "returned": True, "files": b["files"]}
    if "bits" in b:
        out["bits"] = [["uint8", s] for s in b["bits"]]
    for name, dtype in (("soft", "torch.int8"), ("posterior", "torch.int16")):
        if name in b:
            out[name] = [[dtype, [n], head] for n, head in b[name]]
    out["npz"] = [[c, DTYPES.get(c, "int64"), [it[c] for it in items]] for c in items[0] if c not in ("reason", "errors")] + AFTER[kind]
    frames = [[[c, None if v == "nan" else v] for c, v in it.items()] + [["message", m], ["name", n], ["class", cls]] for it, (m, n, cls) in zip(items, b["tails"])]
    out["json"] = b["header"] + [["frames", frames]]
    return out


EXPECTED = {case: _expected(case) for case in CASES}


@pytest.mark.parametrize("case", CASES)
def test_table_items_bits_message_and_saved_files_are_the_recorded_ones(case, tmp_path):
    got = _observe(_build(case), tmp_path / "out")
    want = EXPECTED[case]
    assert sorted(got) == sorted(want)
    for key in want:
        assert got[key] == want[key], (case, key)


def test_a_table_is_its_columns_and_takes_no_other_index():
    for case in CASES:
        obj = _build(case)
        assert len(obj) == 3 and all(getattr(obj, c).shape == (3,) for c in obj.COLUMNS) and obj.valid.tolist() == [True, True, False]
        assert obj.names == (META["names"] if case.endswith("whole") else None) and obj.data.shape[0] == 3
        with pytest.raises(IndexError):
            obj[3]
        with pytest.raises(IndexError):
            obj.message(-4)
