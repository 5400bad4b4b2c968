"""IQ-domain augmentation recipes (no reference counterpart: the reference augments rendered images).  The host DRAWS — a few
numbers per sample — and maps the labels; the samples themselves are touched once, by ``ops.iq_gather_augment``.

Hyper-parameters (``IQ_HYP``, all augmentations default 0 = off): ``iq_jitter`` probability of jittering the window's first frame by
up to +-n_frames // 2; ``iq_shift`` frequency shift ~ U(-s, +s) * sample_rate; ``iq_conj`` probability of conjugating (mirrors the
spectrum about the centre frequency); ``iq_gain_db`` gain ~ U(-g, +g) dB; ``iq_noise_db`` with probability 0.5 white noise
U(0, n) dB above the window's median-chunk power; ``iq_mixup`` probability of summing a second window in before the STFT.

Draw order per item, all from Python's ``random`` (a seeded run repeats; each group is drawn only when its hyper-parameter is on):
  1. window  : random() < iq_jitter, then randint(-J, J)                    (train mode only)
  2. shift   : uniform(-iq_shift, iq_shift), then getrandbits(32) for phase 0
  3. conj    : random() < iq_conj
  4. gain    : uniform(-iq_gain_db, iq_gain_db)
  5. noise   : random() < 0.5, then uniform(0, iq_noise_db), then getrandbits(64) for the seed
  6. mix     : random() < iq_mixup, then randint(0, len - 1) = the partner item, then the partner's own groups 1 - 4.
The validation loader draws nothing."""
from __future__ import annotations

import math
import random
from dataclasses import dataclass, field

import numpy as np

from .spectrogram import freq_to_rows, rows_to_freq, time_to_cols

IQ_HYP = dict(iq_jitter=1.0, iq_shift=0.0, iq_conj=0.0, iq_gain_db=0.0, iq_noise_db=0.0, iq_mixup=0.0, iq_cache_bytes=8 << 30)
WH_THR, AREA_THR = 2.0, 0.1          # box_candidates' thresholds (data/augment.py): both sides > 2 px, clipped / unclipped area > 0.1
NOISE_PROBE = (16, 256)              # the noise estimator reads 16 chunks of 256 samples = 4096 samples of the window


@dataclass
class Geometry:
    """What maps seconds / Hz to pixels of one window image."""
    sample_rate: float
    center_freq: float = 0.0
    n_fft: int = 1024
    hop: int = 256
    n_frames: int = 640
    n_mel: int = 640
    warp_alpha: float = 1.25

    @property
    def n_samples(self):
        return self.n_fft + (self.n_frames - 1) * self.hop

    def band(self):
        """(f_min, f_max): the absolute frequencies of the image's bottom and top pixel edges (pixel coordinate 0 and n_mel)."""
        f = rows_to_freq(np.array([-0.5, self.n_mel - 0.5]), self.sample_rate, self.center_freq, self.n_fft, self.n_mel, self.warp_alpha)
        return float(f[0]), float(f[1])


@dataclass
class IQSource:
    """One window of one capture and what is done to it: the kernel's per-source fields plus the label-side values."""
    cap: int
    first: int                       # first sample
    dphi: int = 0                    # uint32 phase step (2^-32 cycles per sample)
    phi0: int = 0
    conj: bool = False
    gain: float = 1.0
    shift_hz: float = 0.0            # the QUANTISED shift dphi stands for


@dataclass
class IQRecipe:
    a: IQSource
    b: IQSource = None               # the MixUp partner, or None
    sigma: float = 0.0
    seed: int = 0
    labels: np.ndarray = field(default_factory=lambda: np.zeros((0, 5), np.float32))


def quantise_shift(delta_hz, sample_rate):
    """Hz -> (dphi uint32, the shift dphi stands for exactly).  Truncation towards zero: the quantised shift never exceeds the
    clamped one, so a box the clamp kept in the band stays there."""
    k = int(delta_hz / float(sample_rate) * 4294967296.0)
    k = max(min(k, 2 ** 31 - 1), -(2 ** 31))
    return k & 0xFFFFFFFF, k / 4294967296.0 * float(sample_rate)


def map_freq(f, g, shift_hz=0.0, conj=False):
    """Absolute Hz of the capture -> absolute Hz after the optional conjugate (f -> 2 fc - f) and the shift."""
    f = np.asarray(f, dtype=np.float64)
    return (2.0 * g.center_freq - f if conj else f) + shift_hz


def boxes_in_time(rows, first, g):
    """The rows (cls t0 t1 f_lo f_hi) whose time extent overlaps the window that starts at sample ``first``."""
    if not len(rows):
        return rows
    t_lo, t_hi = first / g.sample_rate, (first + g.n_samples) / g.sample_rate
    return rows[(rows[:, 2] > t_lo) & (rows[:, 1] < t_hi)]


def shift_limits(rows, first, g, conj=False):
    """(lo, hi) Hz: the shifts that keep every emission overlapping the window in time inside the band, so that nothing wraps around
    Nyquist and shows up unlabelled.  Emissions are clipped to the band first (what lies outside was never visible)."""
    f_min, f_max = g.band()
    rows = boxes_in_time(rows, first, g)
    if not len(rows):
        return f_min - f_max, f_max - f_min
    e = map_freq(rows[:, 3:5], g, 0.0, conj)
    lo, hi = np.clip(e.min(1), f_min, f_max), np.clip(e.max(1), f_min, f_max)
    return min(f_min - float(lo.min()), 0.0), max(f_max - float(hi.max()), 0.0)


def window_labels(rows, src, g):
    """Sidecar rows (cls t0 t1 f_lo f_hi; seconds from the capture's first sample, absolute Hz) -> (n, 5) float32 normalised
    cls cx cy w h of the window ``src`` describes.  A box edge at time t / frequency f sits at pixel ``col + 0.5`` / ``row + 0.5``
    (``time_to_cols`` / ``freq_to_rows``; the convention ``scan_boxes_to_tf`` uses in the other direction).  Boxes are clipped to the
    image; a box is kept when both sides exceed 2 px and its clipped area exceeds 0.1 of its unclipped area."""
    if not len(rows):
        return np.zeros((0, 5), np.float32)
    rows = np.asarray(rows, dtype=np.float64)
    x = time_to_cols(rows[:, 1:3] - src.first / g.sample_rate, g.sample_rate, g.n_fft, g.hop) + 0.5
    f = map_freq(rows[:, 3:5], g, src.shift_hz, src.conj)
    y = freq_to_rows(f, g.sample_rate, g.center_freq, g.n_fft, g.n_mel, g.warp_alpha) + 0.5
    y = np.sort(y, axis=1)                                                     # a conjugate swaps the low and the high edge
    W, H = float(g.n_frames), float(g.n_mel)
    xc, yc = np.clip(x, 0.0, W), np.clip(y, 0.0, H)
    w0, h0 = x[:, 1] - x[:, 0], y[:, 1] - y[:, 0]
    w, h = xc[:, 1] - xc[:, 0], yc[:, 1] - yc[:, 0]
    keep = (w > WH_THR) & (h > WH_THR) & (w * h > AREA_THR * w0 * h0)
    out = np.stack((rows[:, 0], (xc[:, 0] + xc[:, 1]) / 2 / W, (yc[:, 0] + yc[:, 1]) / 2 / H, w / W, h / H), 1)
    return out[keep].astype(np.float32)


def noise_reference_power(capture, first, n_samples):
    """Median over 16 evenly spread chunks of 256 samples of the chunk's mean |x|^2: 4096 samples of the window, read on the host.
    A JUDGEMENT, not a measured optimum: the median of short chunks follows the noise floor under bursty emissions (a mean would
    follow the bursts) and costs a few microseconds; it is not the per-frame power of the STFT."""
    n_chunks, size = NOISE_PROBE
    step = (n_samples - size) // (n_chunks - 1)
    p = [float(np.mean(np.abs(np.asarray(capture[first + k * step:first + k * step + size], dtype=np.complex64)).astype(np.float64) ** 2))
         for k in range(n_chunks)]
    return float(np.median(p))


def draw_source(ds, index, augment):
    """Groups 1 - 4 of the draw order for item ``index`` of ``ds`` (an ``IQDataset``) -> IQSource."""
    cap, frame = ds.items[index]
    g, hyp = ds.geometry, ds.hyp
    if augment and hyp.iq_jitter > 0 and random.random() < hyp.iq_jitter:
        j = g.n_frames // 2
        frame = min(max(frame + random.randint(-j, j), 0), ds.last_frame[cap])
    src = IQSource(cap, int(frame) * g.hop)
    if not augment:
        return src
    rows = ds.rows[cap]
    delta, phi0 = 0.0, 0
    if hyp.iq_shift > 0:
        delta = random.uniform(-hyp.iq_shift, hyp.iq_shift) * g.sample_rate
        phi0 = random.getrandbits(32)
    if hyp.iq_conj > 0:
        src.conj = random.random() < hyp.iq_conj
    if hyp.iq_shift > 0:
        lo, hi = shift_limits(rows, src.first, g, src.conj)
        src.dphi, src.shift_hz = quantise_shift(min(max(delta, lo), hi), g.sample_rate)
        src.phi0 = phi0
    if hyp.iq_gain_db > 0:
        src.gain = float(10.0 ** (random.uniform(-hyp.iq_gain_db, hyp.iq_gain_db) / 20.0))
    return src


def draw_recipe(ds, index):
    """The whole recipe of item ``index``: source, noise, partner, labels.  Validation datasets draw nothing."""
    augment = ds.augment
    g, hyp = ds.geometry, ds.hyp
    a = draw_source(ds, index, augment)
    rec = IQRecipe(a)
    if augment and hyp.iq_noise_db > 0:
        if random.random() < 0.5:
            db = random.uniform(0.0, hyp.iq_noise_db)
            rec.seed = random.getrandbits(64)
            p = noise_reference_power(ds.captures[a.cap], a.first, g.n_samples) * a.gain ** 2
            rec.sigma = float(math.sqrt(p * 10.0 ** (db / 10.0)))
    labels = [window_labels(ds.rows[a.cap], a, g)]
    if augment and hyp.iq_mixup > 0 and random.random() < hyp.iq_mixup:
        rec.b = draw_source(ds, random.randint(0, len(ds) - 1), True)
        labels.append(window_labels(ds.rows[rec.b.cap], rec.b, g))
    rec.labels = np.concatenate(labels, 0)
    return rec


def pack_recipes(recipes):
    """[IQRecipe] -> the kernel's record array (``ops.IQ_RECIPE``; the partner's address is filled in by ``ops.iq_gather_augment``)."""
    from ..ops import iq_recipes
    from .._lib import IQ_CONJ, IQ_CONJ2
    rec = iq_recipes(len(recipes))
    for i, r in enumerate(recipes):
        a, b = r.a, r.b
        rec[i]["dphi"], rec[i]["phi0"], rec[i]["gain"], rec[i]["sigma"], rec[i]["seed"] = a.dphi, a.phi0, a.gain, r.sigma, r.seed
        flags = IQ_CONJ if a.conj else 0
        if b is not None:
            rec[i]["dphi2"], rec[i]["phi02"], rec[i]["gain2"] = b.dphi, b.phi0, b.gain
            flags |= IQ_CONJ2 if b.conj else 0
        rec[i]["flags"] = flags
    return rec
