"""The result table of a stage of the frame path, defined ONCE: ``FrameTable`` is what ``Decoded`` (decode.py), ``LdpcDecoded`` (ldpc.py) and ``Corrected`` (correct.py)
share — the columns, ``obj[k]``, ``message`` and ``save`` with its ``.npz`` / ``.json`` layout — and ``BitTable`` what the two bit-oriented decoders share on top of it.
``frame_columns`` and ``unpack_check`` are the drivers' side: the empty columns of a result and the CRC triple / channel counts of the one host copy."""
from __future__ import annotations

import json
import math
import os

import numpy as np
import torch


class FrameTable:
    """One row per frame, each column of ``COLUMNS`` a numpy array over the frames and an attribute; ``reason`` ("" for a valid frame); ``data`` (frames, bytes) uint8
    on the DEVICE; ``plan``; ``raw`` (the device buffers); ``rows`` / ``cls`` / ``conf`` / ``names`` from the frames.  A subclass sets ``COLUMNS``, ``STEM`` (the files' name),
    ``EXTRA`` (further per-frame arrays that ``obj[k]`` and ``save`` carry) and defines ``_header`` and ``_message``."""

    COLUMNS, EXTRA, STEM = (), (), ""

    def __init__(self, plan, cols, reason, data, raw, rows=None, cls=None, conf=None, names=None):
        self.plan, self.raw, self.data, self.reason = plan, raw, data, reason
        self.rows, self.cls, self.conf, self.names = rows, cls, conf, names
        for k in self.COLUMNS:
            setattr(self, k, cols[k])

    def __len__(self):
        return self.valid.shape[0]

    def __getitem__(self, k):
        """Frame k as a dict of its scalars."""
        k = range(len(self))[k]
        d = {c: getattr(self, c)[k].item() for c in self.COLUMNS}
        d["reason"] = str(self.reason[k])
        d.update({c: getattr(self, c)[k].tolist() for c in self.EXTRA})
        return d

    def _header(self):
        """The arguments, as the JSON file opens with them."""
        raise NotImplementedError

    def _message(self, row):
        """What a host row of ``data`` carries before the check field: ``bytes``, or the uint8 bit array where it is not whole bytes."""
        raise NotImplementedError

    def message(self, k):
        """What frame ``k`` carries before the check field: ``bytes`` (MSB first), or the uint8 bit array where the bits are not a multiple of 8."""
        k = range(len(self))[k]
        return self._message(self.data[k].cpu().numpy())

    def save(self, directory):
        """Write ``<STEM>.npz`` (every column, the packed data, the ``EXTRA`` arrays and the reasons) and ``<STEM>.json`` (the arguments and one record per frame: ``obj[k]``
        with NaN as null, the message of a valid frame as hex where it is whole bytes, the clip's name and class).  -> the directory."""
        directory = os.fspath(directory)
        os.makedirs(directory, exist_ok=True)
        arrays = {k: getattr(self, k) for k in self.COLUMNS}
        arrays["data"] = self.data.cpu().numpy()
        arrays.update({k: getattr(self, k) for k in self.EXTRA}, reason=np.asarray([str(r) for r in self.reason], dtype=str))
        np.savez(os.path.join(directory, self.STEM + ".npz"), **arrays)
        out = []
        for k in range(len(self)):
            rec = {c: None if isinstance(v, float) and not math.isfinite(v) else v for c, v in self[k].items()}
            m = self._message(arrays["data"][k])
            cls = None if self.cls is None else int(self.cls[int(self.clip[k])])
            rec.update(message=m.hex() if self.valid[k] and isinstance(m, bytes) else None, name=None if cls is None or not self.names else self.names.get(cls))
            rec["class"] = cls
            out.append(rec)
        with open(os.path.join(directory, self.STEM + ".json"), "w") as f:
            json.dump(dict(self._header(), file=self.STEM + ".npz", frames=out), f, indent=1)
        return directory


class BitTable(FrameTable):
    """A decoder's table: ``data`` holds the ``plan.n_info`` de-whitened information bits of a frame packed MSB first, the check field last; ``raw["soft"]`` its
    ``2 plan.T`` soft bits."""

    def bits(self, k):
        """The ``n_info`` de-whitened information bits of frame ``k`` on the host, uint8, the first bit first."""
        k = range(len(self))[k]
        return np.unpackbits(self.data[k].cpu().numpy())[:self.plan.n_info].astype(np.uint8)

    def _message(self, row):
        b = np.unpackbits(row)[:self.plan.n_info]
        b = b[:b.shape[0] - (self.plan.crc["width"] if self.plan.crc else 0)]
        return np.packbits(b).tobytes() if b.shape[0] % 8 == 0 else b

    def soft(self, k):
        """The ``2T`` soft bits of frame ``k`` (an LDPC frame's N), int8, a view of the device buffer (zeros for an invalid frame)."""
        k = range(len(self))[k]
        if self.raw["soft"] is None:
            return torch.zeros(2 * self.plan.T, dtype=torch.int8, device=self.data.device)
        return self.raw["soft"][k, :2 * self.plan.T]


def frame_columns(valid, source, ints, bools=(), channel=False):
    """The columns of a result before anything is launched: ``valid``; ``clip`` / ``word`` / ``position`` copied from ``source`` (the ``Frames``, or the table before); the
    stage's own ``ints`` (int64) and ``bools``, and the CRC triple, zero; with ``channel`` the channel counts, zero, and ``ber``, NaN."""
    n = valid.shape[0]
    cols = {"valid": valid.copy()}
    cols.update({k: np.asarray(getattr(source, k), dtype=np.int64).copy() for k in ("clip", "word", "position")})
    cols.update({k: np.zeros(n, dtype=np.int64) for k in tuple(ints) + (("channel_errors", "n_channel") if channel else ())})
    cols.update({k: np.zeros(n, dtype=bool) for k in tuple(bools) + ("crc_ok",)})
    cols.update(crc_calc=np.zeros(n, dtype=np.uint32), crc_recv=np.zeros(n, dtype=np.uint32))
    if channel:
        cols["ber"] = np.full(n, np.nan)
    return cols


def unpack_check(cols, v, h, at, channel=False):
    """The valid frames' crc_calc, crc_recv, crc_ok from columns ``at`` .. ``at + 2`` of the host copy ``h`` of a check launch's rows; with ``channel`` channel_errors and
    n_channel from the two after them, and their ratio ``ber``."""
    cols["crc_calc"][v], cols["crc_recv"][v] = h[v, at].astype(np.int32).view(np.uint32), h[v, at + 1].astype(np.int32).view(np.uint32)
    cols["crc_ok"][v] = h[v, at + 2] != 0                                       # -1 without a crc: True
    if channel:
        cols["channel_errors"][v], cols["n_channel"][v] = h[v, at + 3], h[v, at + 4]
        some = v & (cols["n_channel"] > 0)
        cols["ber"][some] = cols["channel_errors"][some] / cols["n_channel"][some]
