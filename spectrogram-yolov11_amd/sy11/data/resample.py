"""Resample and retune a capture on the GPU: the plan of the digital down-converter (mix -> low-pass -> rational resample,
``csrc/ddc.hip``) and ``ResampledCapture``, which presents a capture at another rate / tuning as something a scan can slice.

Definition, zero delay by construction, with ``P / Q = fs_out / fs_in`` in lowest terms:

    y[m] = sum_k h[k] u[m Q + c - k],   u[i P] = x[i] e^{j 2 pi frac(i dphi / 2^32)},   u = 0 elsewhere and outside the capture

``h``: ``N = 2 Z R + 1`` taps at the P-times up-sampled rate (``R = max(P, Q)``, ``Z = 16``), ``sinc((k - c) / R) kaiser(N, 8)[k]``
scaled to ``sum h = P``, centre ``c = Z R``.  Output ``m`` sits at exactly ``m / fs_out`` seconds of the capture and there are
``M = floor((n - 1) P / Q) + 1`` outputs.  Only the taps ``k = phi + j P`` with ``phi = (m Q + c) mod P`` meet a sample, so the taps are
stored as a polyphase table ``(P, T)``, ``T = ceil(N / P)``, entry ``[phi, j] = h[phi + j P]``, and

    y[m] = sum_{j < T} table[phi, j] xm[i0 - j],   i0 = floor((m Q + c) / P),   xm = the mixed samples.

There is no filter state: every slice re-reads its ``T``-sample skirt, so a value depends on ``(m, capture)`` alone and chunked
reads are bit-identical to one pass.
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np
import torch

ZERO_CROSSINGS = 16          # Z: one-sided length of the prototype in zero crossings of the sinc
KAISER_BETA = 8.0
# The part of a decimated band that is clean: a property of prototype(1, D) above (Z = 16, beta = 8), not a knob.  In float64, for
# every D = 2 .. 64, its response stays within 0.01 dB up to 0.427 fs_out and is at or below -80 dB from 0.5795 fs_out upward, so
# whatever folds into |f| <= 0.42 fs_out (from 0.58 fs_out and beyond) is at least 80 dB down: 0.84 fs_out of every decimated band
# is flat and alias-free (tests/test_extract_cpu.py pins both figures; sy11/data/extract.py picks D with it).
USABLE_BAND = 0.84
MAX_PQ = 4096
MAX_RATIO = 64


def _nearest_ratio(r):
    """The admissible ratio (P, Q <= 4096, 1/64 <= P/Q <= 64) nearest to the positive Fraction ``r``."""
    r = min(max(r, Fraction(1, MAX_RATIO)), Fraction(MAX_RATIO))
    return r.limit_denominator(MAX_PQ) if r <= 1 else 1 / (1 / r).limit_denominator(MAX_PQ)


def prototype(P, Q):
    """-> (h float64 (N,), c): the low-pass at the P-times up-sampled rate, cut at min(fs_in, fs_out) / 2, sum h = P."""
    R = max(P, Q)
    c = ZERO_CROSSINGS * R
    N = 2 * c + 1
    h = np.sinc((np.arange(N, dtype=np.float64) - c) / R) * np.kaiser(N, KAISER_BETA)
    return h * (P / h.sum()), c


class ResamplePlan:
    """What one (fs_in, fs_out, shift) needs: the ratio, the polyphase table, the mixer step and the index maps."""

    def __init__(self, fs_in, fs_out, P, Q, dphi):
        self.fs_in, self.fs_out, self.P, self.Q, self.dphi = fs_in, fs_out, int(P), int(Q), int(dphi)
        h, self.c = prototype(self.P, self.Q)
        self.N = h.shape[0]
        self.T = -(-self.N // self.P)
        pad = np.zeros(self.P * self.T, dtype=np.float64)
        pad[:self.N] = h
        self.h = h
        self.taps = np.ascontiguousarray(pad.reshape(self.T, self.P).T.astype(np.float32))        # [phi, j] = h[phi + j P]
        self._dev = {}

    @property
    def shift_hz(self):
        """The shift really applied: the step is a whole number of 2^-32 cycles per input sample."""
        signed = self.dphi - (1 << 32) if self.dphi >= 1 << 31 else self.dphi
        return -signed / 2.0 ** 32 * float(self.fs_in)

    @property
    def filters(self):
        return self.P != self.Q

    @property
    def identity(self):
        """Nothing to do: the source is passed through untouched, with no launch."""
        return self.P == self.Q and self.dphi == 0

    def n_out(self, n_in):
        n_in = int(n_in)
        if n_in <= 0:
            return 0
        return n_in if not self.filters else (n_in - 1) * self.P // self.Q + 1

    def support(self, m0, m1):
        """Input index range [a, b) that the outputs [m0, m1) read (before clipping to the capture; a may be negative)."""
        m0, m1 = int(m0), int(m1)
        if m1 <= m0:
            raise ValueError(f"support: empty output range [{m0}, {m1})")
        if not self.filters:
            return m0, m1
        return (m0 * self.Q + self.c) // self.P - (self.T - 1), ((m1 - 1) * self.Q + self.c) // self.P + 1

    def taps_on(self, device):
        device = torch.device(device)
        if device not in self._dev:
            self._dev[device] = torch.from_numpy(self.taps).to(device)
        return self._dev[device]

    def __repr__(self):
        return (f"ResamplePlan({self.fs_in} -> {self.fs_out} Hz, P/Q = {self.P}/{self.Q}, T = {self.T}, "
                f"shift {self.shift_hz} Hz (dphi = {self.dphi}))")


def plan_resample(fs_in, fs_out, shift_hz=0.0):
    """Plan of a DDC from ``fs_in`` to ``fs_out`` (Hz; floats, ints or Fractions) that moves ``shift_hz`` to 0 Hz.  The ratio must be
    exactly ``P / Q`` with ``P, Q <= 4096`` and ``1/64 <= P/Q <= 64``: anything else is a ``ValueError`` that names the nearest
    admissible ratio, never a silent rounding."""
    try:
        fi, fo = Fraction(fs_in), Fraction(fs_out)
    except (TypeError, ValueError, OverflowError) as e:
        raise ValueError(f"plan_resample: sample rates must be finite numbers, got {fs_in!r} -> {fs_out!r}") from e
    if fi <= 0 or fo <= 0:
        raise ValueError(f"plan_resample: sample rates must be positive, got {fs_in!r} -> {fs_out!r}")
    r = fo / fi
    P, Q = r.numerator, r.denominator
    if P > MAX_PQ or Q > MAX_PQ or r > MAX_RATIO or r < Fraction(1, MAX_RATIO):
        near = _nearest_ratio(r)
        raise ValueError(f"plan_resample: fs_out / fs_in = {float(r)!r} is not P/Q with P, Q <= {MAX_PQ} and 1/{MAX_RATIO} <= P/Q <= "
                         f"{MAX_RATIO}; the nearest admissible ratio is {near.numerator}/{near.denominator} "
                         f"(fs_out = {float(fi * near)!r} Hz)")
    shift = float(shift_hz)
    if not math.isfinite(shift) or abs(shift) > float(fi) / 2:
        raise ValueError(f"plan_resample: shift_hz = {shift_hz!r} must be finite and within +- fs_in / 2")
    dphi = int(round(-shift / float(fi) * 2.0 ** 32)) % (1 << 32)
    return ResamplePlan(fs_in, fs_out, P, Q, dphi)


class ResampledCapture:
    """An opened capture (``open_iq``) seen through a DDC: ``len()`` outputs, ``cap[lo:hi]`` -> complex64 device tensor of the
    outputs [lo, hi).  A slice reads only ``plan.support(lo, hi)`` of the source (an ``np.memmap`` far larger than memory keeps
    working), sends it host -> device through a pinned staging buffer unless the source is a device tensor, and is ONE launch."""

    yields_device = True                                       # SpectrogramProducer.scan: slices need no staging

    def __init__(self, src, plan, device="cuda"):
        self.src, self.plan, self.device = src, plan, torch.device(device)
        self.n_in = len(src)
        self.n_out = plan.n_out(self.n_in)
        self._stage, self._copied = None, None

    def __len__(self):
        return self.n_out

    def _to_device(self, a, b):
        """Source samples [a, b) as a contiguous complex64 device tensor."""
        if isinstance(self.src, torch.Tensor) and self.src.is_cuda:
            return self.src[a:b]
        from .spectrogram import read_samples
        n = b - a
        if self._copied is not None:
            self._copied.synchronize()                         # the staging buffer is free once the previous copy is done
        if self._stage is None or self._stage.shape[0] < n:
            self._stage = torch.empty((n,), dtype=torch.complex64).pin_memory()
        self._stage.numpy()[:n] = read_samples(self.src, a, b)
        dev = torch.empty((n,), dtype=torch.complex64, device=self.device)
        dev.copy_(self._stage[:n], non_blocking=True)
        self._copied = torch.cuda.Event()
        self._copied.record()
        return dev

    def __getitem__(self, sl):
        if not isinstance(sl, slice) or sl.step not in (None, 1):
            raise TypeError("a ResampledCapture takes plain slices cap[lo:hi]")
        lo, hi, _ = sl.indices(self.n_out)
        if hi <= lo:
            return torch.empty((0,), dtype=torch.complex64, device=self.device)
        if self.plan.identity:
            return self._to_device(lo, hi)
        from .. import ops
        a, b = self.plan.support(lo, hi)
        a, b = max(a, 0), min(b, self.n_in)
        return ops.iq_resample(self._to_device(a, b), self.plan, a, lo, hi - lo, n_total=self.n_in)
