"""Channelise a wideband capture on the GPU: the plan of the polyphase analysis filter bank (``csrc/pfb.hip``),
``ChannelizedCapture``, which presents every band of a capture as something a scan can slice, and the cross-channel merge of a
channelised scan.

Definition: ``K`` channels (a power of two, 2 .. 64), ``oversample`` r in {1, 2}, decimation ``D = K / r``,
``fs_out = fs_in / D``, channel ``k`` centred at ``k fs_in / K`` (``(k - K) fs_in / K`` for ``k > K / 2``; ``k = K / 2`` sits on
+- fs_in / 2).  With ``h, c = resample.prototype(1, D)`` (``N = 32 D + 1`` taps, float32):

    y_k[m] = sum_n h[n] x[m D + c - n] e^{-j 2 pi k (m D + c - n) / K},     x = 0 outside the capture
           = sum_{r < K} e^{-j 2 pi k r / K} v_m[r],     v_m[r] = sum_{i = r (mod K)} h[m D + c - i] x[i]

``i`` is the absolute sample index, so the fold needs no circular shift.  Channel ``k`` is, by definition, the DDC of
``resample.py`` with ``P = 1``, ``Q = D`` and ``dphi = (-k 2^32 / K) mod 2^32`` (``ChannelPlan.ddc_plan``).  There are
``M = (n - 1) // D + 1`` time steps, output ``m`` sits at exactly ``m / fs_out`` seconds, and there is no filter state: every block
re-reads its skirt, so a value depends on ``(k, m, capture)`` alone and chunked reads are bit-identical to one pass.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np
import torch

from .resample import ResamplePlan, prototype

CHANNELS = (2, 4, 8, 16, 32, 64)
OVERSAMPLE = (1, 2)


class ChannelPlan:
    """What one (fs_in, K, oversample) needs: the decimation, the prototype, the FFT's twiddles and the index maps."""

    def __init__(self, fs_in, K, oversample=2):
        if isinstance(K, bool) or not isinstance(K, (int, np.integer)) or int(K) not in CHANNELS:
            raise ValueError(f"plan_channels: channels = {K!r} must be one of {CHANNELS} (a power of two)")
        if isinstance(oversample, bool) or not isinstance(oversample, (int, np.integer)) or int(oversample) not in OVERSAMPLE:
            raise ValueError(f"plan_channels: oversample = {oversample!r} must be one of {OVERSAMPLE}")
        try:
            ok = Fraction(fs_in) > 0
        except (TypeError, ValueError, OverflowError):
            ok = False
        if not ok:
            raise ValueError(f"plan_channels: the sample rate must be a positive finite number, got {fs_in!r}")
        self.fs_in, self.K, self.oversample = fs_in, int(K), int(oversample)
        self.D = self.K // self.oversample
        self.fs_out = fs_in / self.D
        self.h, self.c = prototype(1, self.D)
        self.N = self.h.shape[0]
        self.taps = np.ascontiguousarray(self.h.astype(np.float32))
        t = np.arange(max(self.K // 2, 1), dtype=np.float64)
        self.twiddle = np.exp(-2j * np.pi * t / self.K).astype(np.complex64)        # float64 on the host, rounded once
        k = np.arange(self.K, dtype=np.float64)
        self.offset_hz = np.where(k > self.K // 2, k - self.K, k) / self.K * float(fs_in)
        self._dev = {}

    def n_out(self, n_in):
        n_in = int(n_in)
        return 0 if n_in <= 0 else (n_in - 1) // self.D + 1

    def support(self, m0, m1):
        """Input index range [a, b) that the time steps [m0, m1) read (before clipping to the capture; a may be negative)."""
        m0, m1 = int(m0), int(m1)
        if m1 <= m0:
            raise ValueError(f"support: empty output range [{m0}, {m1})")
        return m0 * self.D + self.c - self.N + 1, (m1 - 1) * self.D + self.c + 1

    def ddc_plan(self, k):
        """The ``ResamplePlan`` that produces channel ``k`` alone (built directly: ``plan_resample`` refuses the shift of k = K/2)."""
        k = int(k)
        if not 0 <= k < self.K:
            raise ValueError(f"ddc_plan: channel {k} is not in [0, {self.K})")
        return ResamplePlan(self.fs_in, self.fs_out, 1, self.D, (-k * ((1 << 32) // self.K)) % (1 << 32))

    def default_select(self):
        """Every channel but K/2, whose band straddles the capture's edge and wraps (with oversample = 2 it is redundant)."""
        return [k for k in range(self.K) if k != self.K // 2]

    def on(self, device):
        """(taps, twiddle) on ``device``."""
        device = torch.device(device)
        if device not in self._dev:
            self._dev[device] = (torch.from_numpy(self.taps).to(device), torch.from_numpy(self.twiddle).to(device))
        return self._dev[device]

    def __repr__(self):
        return (f"ChannelPlan({self.fs_in} Hz -> {self.K} channels of {self.fs_out} Hz, oversample {self.oversample}, "
                f"D = {self.D}, N = {self.N})")


def plan_channels(fs_in, channels, oversample=2):
    """Plan of a ``channels``-band polyphase filter bank over a capture at ``fs_in`` Hz.  A bad ``channels`` or ``oversample`` is a
    ``ValueError`` that names the admissible values."""
    return ChannelPlan(fs_in, channels, oversample)


def plan_scan_channels(sample_rate, channels, oversample=2, select=None, trained=None, resample_to=None, tune_to=None):
    """-> (ChannelPlan, sorted list of selected channels) of ``scan(..., channels, oversample, select)``; every argument error of
    the three keywords is raised here.  ``trained``: the checkpoint's ``train_args`` (what ``"model"`` refers to)."""
    if resample_to is not None or tune_to is not None:
        raise ValueError("channels cannot be combined with resample_to / tune_to: the filter bank fixes every band's rate and centre")
    if isinstance(channels, ChannelPlan):
        plan = channels
    elif isinstance(channels, str):
        if channels != "model":
            raise ValueError(f"channels takes a channel count, a ChannelPlan or 'model', got {channels!r}")
        rate = (trained or {}).get("sample_rate")
        if not rate:
            raise ValueError("channels='model': this checkpoint records no sample_rate (it was not trained from IQ captures)")
        if isinstance(oversample, bool) or oversample not in OVERSAMPLE:
            raise ValueError(f"plan_channels: oversample = {oversample!r} must be one of {OVERSAMPLE}")
        ratio = Fraction(sample_rate) / Fraction(rate)
        D = ratio.numerator
        if ratio.denominator != 1 or D & (D - 1) or oversample * D not in CHANNELS:
            raise ValueError(f"channels='model': the capture's rate over the checkpoint's ({float(sample_rate)!r} / {float(rate)!r} = "
                             f"{float(ratio)!r}) must be a power of two D with K = {oversample} D <= {CHANNELS[-1]}")
        plan = ChannelPlan(sample_rate, oversample * D, oversample)
    else:
        plan = ChannelPlan(sample_rate, channels, oversample)
    if select is None:
        select = plan.default_select()
    else:
        try:
            select = sorted({int(k) for k in select})
        except (TypeError, ValueError) as e:
            raise ValueError(f"select must be a list of channel numbers, got {select!r}") from e
        if not select or select[0] < 0 or select[-1] >= plan.K:
            raise ValueError(f"select must name channels in [0, {plan.K}), got {select!r}")
    return plan, select


class _Channel:
    """Row ``k`` of a ``ChannelizedCapture`` as a capture of its own: ``len()`` time steps, ``ch[lo:hi]`` -> device tensor."""

    yields_device = True                                       # SpectrogramProducer.scan: slices need no staging

    def __init__(self, cap, k):
        self.cap, self.k = cap, k

    def __len__(self):
        return len(self.cap)

    def __getitem__(self, sl):
        if not isinstance(sl, slice) or sl.step not in (None, 1):
            raise TypeError("a channel takes plain slices ch[lo:hi]")
        lo, hi, _ = sl.indices(len(self.cap))
        if hi <= lo:
            return torch.empty((0,), dtype=torch.complex64, device=self.cap.device)
        return self.cap.block(lo, hi)[self.k]


class ChannelizedCapture:
    """An opened capture (``open_iq``) seen through the filter bank: ``len()`` time steps, ``block(lo, hi)`` -> (K, hi - lo)
    complex64 device tensor.  A block reads only ``plan.support(lo, hi)`` of the source (an ``np.memmap`` far larger than memory
    keeps working), sends it host -> device through a pinned staging buffer unless the source is a device tensor, and is ONE
    launch.  The last block is kept, so the K channel views of a scan that ask for the same range in turn share it."""

    def __init__(self, src, plan, device="cuda"):
        self.src, self.plan, self.device = src, plan, torch.device(device)
        self.n_in = len(src)
        self.n_out = plan.n_out(self.n_in)
        self._stage, self._copied, self._last = None, None, None

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

    def block(self, lo, hi):
        lo, hi = int(lo), int(hi)
        if not 0 <= lo < hi <= self.n_out:
            raise ValueError(f"block: time steps [{lo}, {hi}) are not among the capture's {self.n_out}")
        if self._last is not None and self._last[:2] == (lo, hi):
            return self._last[2]
        from .. import ops
        a, b = self.plan.support(lo, hi)
        a, b = max(a, 0), min(b, self.n_in)
        y = ops.iq_channelize(self._to_device(a, b), self.plan, a, lo, hi - lo, n_total=self.n_in)
        self._last = (lo, hi, y)
        return y

    def channel(self, k):
        k = int(k)
        if not 0 <= k < self.plan.K:
            raise ValueError(f"channel {k} is not in [0, {self.plan.K})")
        return _Channel(self, k)


def merge_channels(tf, score, cls, channel, metric="ios", thres=0.5, agnostic=False):
    """Cross-channel merge of a channelised scan -> bool keep mask (n,).  ``tf`` (n, 4) [t0_s, f_lo_hz, t1_s, f_hi_hz] (the image
    rows are a warped frequency axis, so boxes of different channels are only comparable in Hz), ``score`` (n,), ``cls`` (n,),
    ``channel`` (n,).  Greedy in float64 by (score descending, row ascending): a box is dropped when an already-kept box of ANOTHER
    channel (of its class unless ``agnostic``) has ``metric`` > ``thres`` with it; "ios" = intersection over the smaller area,
    "iou" = over the union, as in the seam merge.  Boxes are swept in order of t0, so only those that overlap in time are ever
    compared: there is no n x n matrix."""
    if metric not in ("ios", "iou"):
        raise ValueError(f"merge_channels: metric must be 'ios' or 'iou', got {metric!r}")
    tf = np.asarray(tf, dtype=np.float64).reshape(-1, 4)
    n = tf.shape[0]
    score, cls, channel = (np.asarray(v).reshape(-1) for v in (score, cls, channel))
    if not score.shape[0] == cls.shape[0] == channel.shape[0] == n:
        raise ValueError("merge_channels: expected tf (n, 4), score (n,), cls (n,) and channel (n,)")
    keep = np.zeros(n, dtype=bool)
    if n == 0:
        return keep
    by_t0 = np.argsort(tf[:, 0], kind="stable")                # sweep order
    st = tf[by_t0]
    s_cls, s_ch = cls[by_t0], channel[by_t0]
    area = (st[:, 2] - st[:, 0]) * (st[:, 3] - st[:, 1])
    longest = float((st[:, 2] - st[:, 0]).max())
    pos = np.empty(n, dtype=np.int64)
    pos[by_t0] = np.arange(n)
    kept = np.zeros(n, dtype=bool)                             # in sweep order
    for i in np.lexsort((np.arange(n), -score.astype(np.float64))):
        q = pos[i]
        b = st[q]
        lo = np.searchsorted(st[:, 0], b[0] - longest, side="left")       # earlier boxes that can still reach b's t0
        hi = np.searchsorted(st[:, 0], b[2], side="left")                 # boxes that start before b ends
        c = st[lo:hi]
        inter = np.maximum(0.0, np.minimum(b[2], c[:, 2]) - np.maximum(b[0], c[:, 0])) * \
            np.maximum(0.0, np.minimum(b[3], c[:, 3]) - np.maximum(b[1], c[:, 1]))
        with np.errstate(divide="ignore", invalid="ignore"):
            m = inter / np.minimum(area[q], area[lo:hi]) if metric == "ios" else inter / (area[q] + area[lo:hi] - inter)
        hit = kept[lo:hi] & (s_ch[lo:hi] != s_ch[q]) & (m > thres)
        if not agnostic:
            hit &= s_cls[lo:hi] == s_cls[q]
        if not hit.any():
            kept[q] = True
            keep[i] = True
    return keep
