"""IQ -> STFT -> power -> triangular "mel" bank -> dB -> min-max -> (B, 3, 640, 640) image producer on the MI355X.

The reference contains NO implementation of this stage (README.md:7 prose only); it plugs in where
``DetectionTrainer.preprocess_batch`` (models/yolo/detect/train.py:57-74) / ``BasePredictor.preprocess``
(engine/predictor.py:118-136) produce the float image.  Spec (build-defined): n_fft 1024, hop 256,
periodic Hann, two-sided (complex IQ), 640 frames, fftshift, |X|^2, 640 triangular filters on a log-warped
two-sided axis (<= 8 bins per filter), 10*log10(p + 1e-10), per-image min-max, 3 identical channels.

Long captures (``plan_windows`` / ``SpectrogramProducer.scan``): a recording of any length is cut into windows of ``n_frames``
frames on a regular frame grid.  Per chunk of windows the frames they cover are transformed ONCE into a dB strip, whatever the
overlap, and every window image is cut from the strip with its own min-max (``ops.stft_windows``).  ``rows_to_freq`` /
``cols_to_time`` map image rows to Hz and strip columns to seconds.
"""
from __future__ import annotations

import math
import os

import numpy as np
import torch

from .. import ops


RAW_IQ_SUFFIXES = (".cf32", ".fc32", ".iq")


def plan_windows(n_samples, overlap=0.5, stride_frames=None, n_fft=1024, hop=256, n_frames=640):
    """First frame (int64) of every window of a capture of ``n_samples`` samples: 0, s, 2s, ... while the window fits, plus one
    last window aligned to the last full frame when the capture does not end on that grid (never a padded window).
    ``s = stride_frames`` or ``round(n_frames * (1 - overlap))``."""
    need = n_fft + (n_frames - 1) * hop
    if n_samples < need:
        raise ValueError(f"need >= {need} IQ samples per image, got {n_samples}")
    stride = int(stride_frames) if stride_frames is not None else int(round(n_frames * (1.0 - float(overlap))))
    if not 1 <= stride <= n_frames:
        raise ValueError(f"window stride must be in [1, {n_frames}] frames, got {stride} (overlap={overlap}, stride_frames={stride_frames})")
    last = (n_samples - n_fft) // hop + 1 - n_frames             # first frame of the last window that fits
    start = np.arange(0, last + 1, stride, dtype=np.int64)
    if start[-1] != last:
        start = np.append(start, np.int64(last))
    return start


def plan_chunks(start, chunk_windows=64, n_fft=1024, hop=256, n_frames=640):
    """Chunks of a scan: [(w0, w1, sample_lo, sample_hi)] — windows w0 .. w1-1 are cut from the strip of the frames
    start[w0] .. start[w1-1] + n_frames - 1, which needs the samples [sample_lo, sample_hi).  A chunk holds at most
    ``chunk_windows`` windows and ends early where the next window would leave a gap of frames nobody asked for."""
    start = np.asarray(start, dtype=np.int64).reshape(-1)
    if chunk_windows < 1:
        raise ValueError("chunk_windows must be >= 1")
    if (chunk_windows * n_frames) * hop + n_fft >= 2 ** 31:
        raise ValueError(f"chunk_windows={chunk_windows}: the chunk's sample count must stay below 2^31")
    if start.size and (start[0] < 0 or np.any(np.diff(start) < 0)):
        raise ValueError("window starts must be non-negative and non-decreasing")
    chunks, w0 = [], 0
    while w0 < start.size:
        w1 = w0 + 1
        while w1 < start.size and w1 - w0 < chunk_windows and start[w1] <= start[w1 - 1] + n_frames:
            w1 += 1
        chunks.append((w0, w1, int(start[w0]) * hop, (int(start[w1 - 1]) + n_frames - 1) * hop + n_fft))
        w0 = w1
    return chunks


def open_iq(source):
    """A capture as something that has ``len()`` and yields complex64 samples for ``source[lo:hi]``: a 1-D complex64 tensor or
    array as it is, a ``.npy`` of complex64 or a raw interleaved-float32 file (``.cf32`` / ``.fc32`` / ``.iq``) as ``np.memmap``
    (a recording may be far larger than memory: only the slices a scan asks for are ever read)."""
    if isinstance(source, (str, os.PathLike)):
        path = os.fspath(source)
        if path.lower().endswith(".npy"):
            arr = np.load(path, mmap_mode="r")
            if arr.dtype != np.complex64 or arr.ndim != 1:
                raise ValueError(f"{path}: expected a 1-D complex64 array, got {arr.dtype} {arr.shape}")
            return arr
        if path.lower().endswith(RAW_IQ_SUFFIXES):
            n_bytes = os.path.getsize(path)
            if n_bytes == 0 or n_bytes % 8:
                raise ValueError(f"{path}: {n_bytes} bytes is not a whole number of interleaved float32 I/Q pairs")
            return np.memmap(path, dtype=np.complex64, mode="r")
        raise ValueError(f"{path}: an IQ file must be .npy (complex64) or raw interleaved float32 ({' / '.join(RAW_IQ_SUFFIXES)})")
    if isinstance(source, torch.Tensor):
        if source.dim() != 1 or source.dtype != torch.complex64:
            raise ValueError(f"expected a 1-D complex64 tensor, got {source.dtype} {tuple(source.shape)}")
        return source if source.is_cuda else source.detach().contiguous().numpy()
    if isinstance(source, np.ndarray) and (source.ndim != 1 or source.dtype != np.complex64):
        raise ValueError(f"expected a 1-D complex64 array, got {source.dtype} {source.shape}")
    return source


def read_samples(src, lo, hi):
    """Samples [lo, hi) of an opened capture as a contiguous complex64 host array (the only read a scan makes of its source)."""
    out = np.ascontiguousarray(src[lo:hi], dtype=np.complex64)
    if out.shape != (hi - lo,):
        raise ValueError(f"the capture ends before sample {hi} (got {out.shape[0]} of {hi - lo} samples from {lo})")
    return out


def rows_to_freq(r, sample_rate, center_freq=0.0, n_fft=1024, n_mel=640, warp_alpha=1.25):
    """Image row -> Hz (float64).  Integer ``r`` is the centre of image row ``r`` (the peak of filter ``r``); a box edge at pixel
    coordinate ``y`` is ``r = y - 0.5``.  Inverse of the bank's warped axis (``filter_bank``): edge index e = r + 1,
    m = 2e / (n_mel + 1) - 1, u = sign(m) expm1(|m| log1p(alpha)) / alpha, bin = (1 + u) (n_fft / 2) (n_fft - 1) / n_fft,
    Hz = (bin / n_fft - 0.5) * sample_rate + center_freq."""
    e = np.asarray(r, dtype=np.float64) + 1.0
    m = 2.0 * e / (n_mel + 1) - 1.0
    u = np.sign(m) * np.expm1(np.abs(m) * math.log1p(warp_alpha)) / warp_alpha
    b = (1.0 + u) * (n_fft / 2) * (n_fft - 1) / n_fft
    return (b / n_fft - 0.5) * float(sample_rate) + float(center_freq)


def cols_to_time(X, sample_rate, n_fft=1024, hop=256):
    """Strip column (frame index, float64; a box edge at pixel coordinate ``x`` is column ``x - 0.5``) -> seconds from the first
    sample of the capture: the centre of that frame's n_fft-sample support."""
    return (np.asarray(X, dtype=np.float64) * hop + n_fft / 2) / float(sample_rate)


def freq_to_rows(hz, sample_rate, center_freq=0.0, n_fft=1024, n_mel=640, warp_alpha=1.25):
    """Hz -> image row (float64), the inverse of ``rows_to_freq``: a frequency that is the low / high edge of a box sits at pixel
    coordinate ``row + 0.5``.  Frequencies outside the band map outside [-1, n_mel] (the warp is continued, nothing is clipped)."""
    b = ((np.asarray(hz, dtype=np.float64) - float(center_freq)) / float(sample_rate) + 0.5) * n_fft
    u = b / ((n_fft / 2) * (n_fft - 1) / n_fft) - 1.0
    m = np.sign(u) * np.log1p(np.abs(u) * warp_alpha) / math.log1p(warp_alpha)
    return (m + 1.0) * (n_mel + 1) / 2.0 - 1.0


def time_to_cols(t, sample_rate, n_fft=1024, hop=256):
    """Seconds from the first sample of the capture -> strip column (float64), the inverse of ``cols_to_time``; a box edge at that
    time sits at pixel coordinate ``col + 0.5``."""
    return (np.asarray(t, dtype=np.float64) * float(sample_rate) - n_fft / 2) / hop


class SpectrogramProducer:
    def __init__(self, device="cuda", n_fft=1024, hop=256, n_frames=640, n_mel=640, warp_alpha=1.25, mel_taps=8):
        self.n_fft, self.hop, self.n_frames, self.n_mel, self.mel_taps = n_fft, hop, n_frames, n_mel, mel_taps
        self.warp_alpha = warp_alpha
        self.n_samples = n_fft + (n_frames - 1) * hop
        start, wts = self.filter_bank(n_mel, n_fft, warp_alpha, mel_taps)
        self.device = torch.device(device)
        self.window = torch.hann_window(n_fft, periodic=True, dtype=torch.float32).to(self.device)
        self.mel_start = torch.from_numpy(start).to(self.device)
        self.mel_w = torch.from_numpy(wts).to(self.device)

    @staticmethod
    def filter_bank(n_mel, n_fft, alpha, taps):
        """Gather-form triangular bank: first FFT bin and `taps` weights per filter (zero padded)."""
        m = np.linspace(-1.0, 1.0, n_mel + 2, dtype=np.float64)
        u = np.sign(m) * np.expm1(np.abs(m) * math.log1p(alpha)) / alpha
        p = (n_fft / 2) * (1.0 + u) * (n_fft - 1) / n_fft
        start = np.zeros(n_mel, dtype=np.int32)
        wts = np.zeros((n_mel, taps), dtype=np.float32)
        for j in range(1, n_mel + 1):
            lo, c, hi = p[j - 1], p[j], p[j + 1]
            ks = [k for k in range(int(math.ceil(lo)), int(math.floor(hi)) + 1) if 0 <= k < n_fft]
            if len(ks) > taps:
                raise ValueError(f"filter {j} spans {len(ks)} bins > mel_taps={taps}")
            start[j - 1] = ks[0] if ks else 0
            for t, k in enumerate(ks):
                wts[j - 1, t] = max((k - lo) / (c - lo) if k <= c else (hi - k) / (hi - c), 0.0)
        return start, wts

    def logmel_db(self, iq: torch.Tensor):
        """(B, n_samples) complex64 on device -> (db (B, frames, n_mel), minmax (B, 2))."""
        if iq.shape[1] < self.n_samples:
            raise ValueError(f"need >= {self.n_samples} IQ samples per image, got {iq.shape[1]}")
        return ops.stft_logmel(iq, self.window, self.mel_start, self.mel_w, self.n_fft, self.hop, self.n_frames, self.n_mel)

    def __call__(self, iq: torch.Tensor, out: torch.Tensor = None) -> torch.Tensor:
        """(B, n_samples) complex64 -> (B, 3, n_mel, n_frames) f32 in [0, 1] (NCHW, what the model's stem reads).
        ``out``: write the image there (the trainer passes the captured graph's static input: no 315 MB copy per step)."""
        db, mm = self.logmel_db(iq)
        return ops.stft_normalize(db, mm, out)

    def scan(self, iq, start, chunk_windows=64, out=None):
        """Window images of a long capture, chunk by chunk: yields ``(images (w, 3, n_mel, n_frames) f32 on the device,
        start[w0:w1])``.  ``iq``: an opened capture (``open_iq``; anything with ``iq[lo:hi]`` -> complex64, e.g. an ``np.memmap``
        far larger than device memory); ``start``: first frame of every window (``plan_windows``).  Per chunk the samples its
        windows cover go host -> device through a pinned staging buffer, ONE strip ``logmel`` call transforms every frame once
        and one ``stft_windows`` call cuts and normalises the windows, so strip memory is bounded by the chunk.  A capture whose
        slices are device tensors already (it says so with ``yields_device = True``: ``resample.ResampledCapture``) is used as it
        is, with no staging.  ``out``: an
        optional (chunk_windows, 3, n_mel, n_frames) f32 buffer to write every chunk's images into (valid until the next chunk)."""
        start = np.asarray(start, dtype=np.int64).reshape(-1)
        chunks = plan_chunks(start, chunk_windows, self.n_fft, self.hop, self.n_frames)
        on_device = isinstance(iq, torch.Tensor) and iq.is_cuda
        yields_device = bool(getattr(iq, "yields_device", False))        # e.g. a ResampledCapture: iq[lo:hi] is a device tensor already
        stage, copied = None, None
        if chunks and not on_device and not yields_device:
            stage = torch.empty((max(hi - lo for _, _, lo, hi in chunks),), dtype=torch.complex64).pin_memory()
        for w0, w1, lo, hi in chunks:
            L = hi - lo
            if on_device:
                if hi > iq.shape[0]:
                    raise ValueError(f"the capture ends before sample {hi}")
                dev_iq = iq[lo:hi].contiguous()
            elif yields_device:
                dev_iq = iq[lo:hi]
                if not (isinstance(dev_iq, torch.Tensor) and dev_iq.is_cuda and dev_iq.dtype == torch.complex64):
                    raise ValueError("a capture that declares `yields_device` must return complex64 device tensors")
                if dev_iq.shape != (L,):
                    raise ValueError(f"the capture ends before sample {hi} (got {dev_iq.shape[0]} of {L} samples from {lo})")
                dev_iq = dev_iq.contiguous()
            else:
                if copied is not None:
                    copied.synchronize()                       # the staging buffer is free once the previous chunk's copy is done
                stage.numpy()[:L] = read_samples(iq, lo, hi)
                dev_iq = torch.empty((L,), dtype=torch.complex64, device=self.device)
                dev_iq.copy_(stage[:L], non_blocking=True)
                copied = torch.cuda.Event()
                copied.record()
            F = (L - self.n_fft) // self.hop + 1
            db, _ = ops.stft_logmel(dev_iq.view(1, L), self.window, self.mel_start, self.mel_w, self.n_fft, self.hop, F, self.n_mel)
            rel = torch.from_numpy((start[w0:w1] - start[w0]).astype(np.int32)).to(self.device)
            img, _ = ops.stft_windows(db[0], rel, self.n_frames, None if out is None else out[:w1 - w0])
            yield img, start[w0:w1]
