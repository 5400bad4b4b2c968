"""Prediction path with the reference's contract (ultralytics/engine/predictor.py:66-167,222-306 and
models/yolo/detect/predict.py:23-73; results containers engine/results.py:187,1015-1122), hot path only:
preprocess (a list of raw HWC BGR uint8 images, uint8/float image tensors, or raw IQ) -> inference (fused DetectionModel
on libsy11) -> postprocess (non_max_suppression on the HIP bit-matrix NMS, scale_boxes) -> Results(boxes=(n,6)
[x1,y1,x2,y2,conf,cls]).  pre_transform's LetterBox and preprocess's BGR->RGB / HWC->CHW / /255 (predictor.py:118-163)
are one HIP launch per image writing into the batch tensor; only file decoding stays outside."""
from __future__ import annotations

import threading

import numpy as np
import torch

from ..utils import ops


class Boxes:
    """(n, 6) detections in original-image pixels (results.py:1015): xyxy, conf, cls accessors."""

    def __init__(self, boxes: torch.Tensor, orig_shape):
        assert boxes.shape[-1] == 6
        self.data = boxes
        self.orig_shape = orig_shape

    @property
    def xyxy(self):
        return self.data[:, :4]

    @property
    def conf(self):
        return self.data[:, -2]

    @property
    def cls(self):
        return self.data[:, -1]

    @property
    def xywh(self):
        return ops.xyxy2xywh(self.xyxy)

    def __len__(self):
        return self.data.shape[0]


class Results:
    def __init__(self, orig_img, path, names, boxes=None, orig_shape=None):
        self.orig_img = orig_img
        self.orig_shape = orig_shape or (tuple(orig_img.shape[-2:]) if orig_img is not None else None)
        self.boxes = Boxes(boxes, self.orig_shape) if boxes is not None else None
        self.names = names
        self.path = path

    def __len__(self):
        return len(self.boxes) if self.boxes is not None else 0


class ScanResults:
    """Detections of a long-capture scan (``DetectionPredictor.scan``), one row per box:
    ``boxes`` (n, 6) float64 [X1, y1, X2, y2, conf, cls] — X in strip frames (window start + window-local x), y in image rows;
    ``window`` (n,) int64 the window a box was found in; ``tf`` (n, 4) float64 [t0_s, f_lo_hz, t1_s, f_hi_hz];
    ``start`` (W,) int64 first frame of every window.  After a resampled / retuned scan ``sample_rate`` / ``center_freq`` are those
    of the DDC's output (frames, ``boxes`` and ``start`` count its samples), ``tf`` stays in seconds of the original capture and in
    absolute Hz, and ``resample`` is the plan that was used.  After a channelised scan ``channel`` (n,) int64 is the band every
    row was found in and ``channelizer`` the ``ChannelPlan``: ``sample_rate`` is the bands' rate (frames, ``boxes`` and ``start`` count
    a band's samples; all bands share ``start``), ``center_freq`` stays the capture's (band k is centred at ``center_freq +
    channelizer.offset_hz[k]``), ``tf`` is in seconds of the capture and absolute Hz; rows are ordered by channel.
    ``hop`` is the STFT hop of the scan (None on a hand-built result).  ``track`` (n,) int64 — the track of every row — and
    ``tracks`` (``sy11.data.link.Tracks``) are set by ``link`` / ``scan(link=...)`` and None on every other result."""

    def __init__(self, boxes, window, tf, names, start, sample_rate, center_freq, resample=None, channel=None, channelizer=None):
        self.boxes, self.window, self.tf, self.names = boxes, window, tf, names
        self.start, self.sample_rate, self.center_freq = start, sample_rate, center_freq
        self.resample = resample                            # the ResamplePlan of a resampled / retuned scan, else None
        self.channel, self.channelizer = channel, channelizer       # a channelised scan's band per row and its ChannelPlan, else None
        self.hop = None                                     # the scan's STFT hop: what gap_t="auto" of link counts in
        self.track, self.tracks = None, None                # set by link: the track of every row and the Tracks table

    def __len__(self):
        return self.boxes.shape[0]


class DetectionPredictor:
    """conf / iou / max_det defaults follow cfg/default.yaml (0.25 / 0.7 / 300)."""

    def __init__(self, model, device="cuda", conf=0.25, iou=0.7, max_det=300, classes=None, agnostic_nms=False, half=False,
                 producer=None, imgsz=640, graphs=True):
        self.device = torch.device(device)
        self.model = model.to(self.device).eval()
        self.model.fuse()                                   # predictor.setup_model -> AutoBackend(fuse=True)
        self.model._sy11_dtype = torch.float16 if half else torch.float32
        self.args = dict(conf=conf, iou=iou, max_det=max_det, classes=classes, agnostic_nms=agnostic_nms)
        self.producer = producer
        if graphs:                                          # batches of one shape replay a captured forward graph after 2 eager calls
            from . import enable_graphs
            enable_graphs(self.model)
        self.imgsz = (imgsz, imgsz) if isinstance(imgsz, int) else tuple(imgsz)
        self.trained = None                                 # the checkpoint's train_args (YOLO.scan sets it): what "model" means in scan
        self._lock = threading.Lock()                       # predictor.py:115: one inference at a time per predictor

    def pre_transform(self, im, out_dtype=None):
        """predictor.py:147-163 + :127-135 — [(h, w, 3) BGR uint8] * B -> (B, 3, H, W) RGB float/half in [0, 1] on the
        device.  LetterBox(imgsz, auto = all shapes equal, stride = model stride), as the reference's `pt` path."""
        from ..data.augment import LetterBox
        shapes = {tuple(x.shape) for x in im}
        stride = int(max(self.model.stride)) if hasattr(self.model, "stride") else 32
        lb = LetterBox(self.imgsz, auto=len(shapes) == 1, stride=stride, device=self.device)
        sizes = []
        for x in im:
            new_unpad, _, top, bottom, left, right = lb.geometry(x.shape[:2])
            sizes.append((new_unpad[1] + top + bottom, new_unpad[0] + left + right))
        if len(set(sizes)) != 1:                               # np.stack of the reference fails the same way
            raise ValueError(f"all input arrays must have the same shape after LetterBox, got {sorted(set(sizes))}")
        H, W = sizes[0]
        dtype = out_dtype or torch.float32                       # the stem kernel takes f32 NCHW and rounds for itself
        batch = torch.empty((len(im), 3, H, W), dtype=dtype, device=self.device)
        for i, x in enumerate(im):
            lb.into(x, batch[i], reverse_c=True)
        return batch

    def preprocess(self, im):
        """A list of raw (h, w, 3) BGR uint8 images (numpy or device tensors), a (B,3,H,W) uint8/float tensor (already
        letterboxed, RGB), or complex IQ (B, L) -> float image in [0, 1]."""
        if isinstance(im, (list, tuple)):
            return self.pre_transform(im)
        if torch.is_complex(im):
            if self.producer is None:
                raise ValueError("raw IQ input needs a SpectrogramProducer")
            return self.producer(im.to(self.device))
        im = im.to(self.device)
        return im.float() / 255 if im.dtype == torch.uint8 else im.float()

    @torch.no_grad()
    def inference(self, im):
        return self.model(im.contiguous())

    def postprocess(self, preds, img, orig_imgs=None, paths=None):
        a = self.args
        preds = ops.non_max_suppression(preds, a["conf"], a["iou"], classes=a["classes"], agnostic=a["agnostic_nms"],
                                        max_det=a["max_det"])
        out = []
        for i, pred in enumerate(preds):
            orig = orig_imgs[i] if orig_imgs is not None else img[i]
            hw = tuple(orig.shape[:2]) if orig.shape[-1] == 3 and orig.ndim == 3 else tuple(orig.shape[-2:])   # HWC raw | CHW tensor
            pred = pred.clone()
            pred[:, :4] = ops.scale_boxes(img.shape[2:], pred[:, :4], hw)
            out.append(Results(orig, paths[i] if paths else None, self.model.names, boxes=pred[:, :6], orig_shape=hw))
        return out

    def __call__(self, source, orig_imgs=None, paths=None):
        with self._lock:
            if isinstance(source, (list, tuple)) and orig_imgs is None:
                orig_imgs = source
            im = self.preprocess(source)
            preds = self.inference(im)
            return self.postprocess(preds, im, orig_imgs, paths)

    @torch.no_grad()
    def scan(self, iq, sample_rate, center_freq=0.0, overlap=0.5, batch=64, merge="ios", merge_thres=0.5, stride_frames=None,
             start=None, resample_to=None, tune_to=None, channels=None, oversample=2, select=None, link=None):
        """Run the model over a capture of any length -> ``ScanResults``.  ``iq``: what ``sy11.data.spectrogram.open_iq`` returns
        (1-D complex64 samples: array, tensor or ``np.memmap``).  Windows come from ``plan_windows(len(iq), overlap | stride_frames)``
        (or ``start``); per chunk of ``batch`` windows: the producer's strip images -> ``inference`` (graph replay for full chunks,
        a second signature for the ragged last one) -> ``non_max_suppression`` with this predictor's conf / iou / max_det.  After
        the last chunk ONE seam merge (``ops.scan_merge``) suppresses, in strip coordinates, the boxes that overlapping windows
        found twice: ``merge`` = "ios" (intersection over the smaller area: a box cut by a window edge matches its full twin from
        the neighbouring window, which IoU does not), "iou", or None for the unmerged rows.  ``merge_thres`` = 0.5 for "ios" is a
        default chosen by judgement, not a measured optimum.

        ``resample_to`` / ``tune_to`` put a DDC (``sy11.data.resample``) in front: the capture is low-passed and resampled to
        ``resample_to`` Hz and ``tune_to`` Hz becomes the new centre, chunk by chunk on the device.  ``"model"`` stands for the rate
        (and, for ``tune_to``, the centre) the checkpoint records; a ready ``ResamplePlan`` (``plan_scan_ddc``) is taken as it is.
        The results then carry the output rate, the centre really tuned to (the shift is a whole number of 2^-32 cycles per
        sample) and the plan; seconds and Hz stay those of the capture.

        ``channels`` puts a polyphase filter bank (``sy11.data.channelize``) in front instead and scans every band of a wideband
        capture from one read of it: K (a power of two, 2 .. 64), a ready ``ChannelPlan``, or ``"model"`` (K = ``oversample`` x the
        capture's rate over the checkpoint's, which must be a power of two).  ``oversample`` = 2 lets neighbouring bands share half
        their width, so an emission cut by one band's edge is whole in the next; ``select`` = the bands to scan (default: all but
        K/2, which wraps round the capture's edge).  Per chunk there is ONE channelise launch, then the usual steps per band; after
        the per-band seam merges a cross-band merge (``channelize.merge_channels``, in seconds / Hz) runs when ``oversample`` is 2
        and ``merge`` is not None.  ``channels`` excludes ``resample_to`` / ``tune_to``.

        ``link`` = True, or a dict of ``link``'s keywords, runs ``link`` on the result before it is returned (``results.track`` /
        ``results.tracks``); None changes nothing."""
        from .. import ops as kops
        from ..data import spectrogram as sp
        if self.producer is None:
            raise ValueError("scan needs a SpectrogramProducer")
        if merge not in (None, "ios", "iou"):
            raise ValueError(f"merge must be 'ios', 'iou' or None, got {merge!r}")
        link = link_keywords(link)
        p = self.producer
        if channels is not None:
            res = self._scan_channels(iq, sample_rate, center_freq, overlap, batch, merge, merge_thres, stride_frames, start,
                                      resample_to, tune_to, channels, oversample, select)
            res.hop = p.hop
            return res if link is None else self.link(res, **link)
        plan = None
        if resample_to is not None or tune_to is not None:
            from ..data.resample import ResampledCapture, ResamplePlan
            plan = resample_to if isinstance(resample_to, ResamplePlan) else plan_scan_ddc(sample_rate, center_freq, resample_to, tune_to,
                                                                                           self.trained)
            iq = ResampledCapture(iq, plan, self.device)
            sample_rate, center_freq = plan.fs_out, float(center_freq) + plan.shift_hz
        if (p.n_mel, p.n_frames) != tuple(self.imgsz):
            raise ValueError(f"the producer's {p.n_mel} x {p.n_frames} images do not match imgsz={self.imgsz}")
        if start is None:
            start = sp.plan_windows(len(iq), overlap, stride_frames, p.n_fft, p.hop, p.n_frames)
        start = np.asarray(start, dtype=np.int64).reshape(-1)
        a = self.args
        rows, wins = [], []
        with self._lock:
            buf = torch.empty((min(batch, max(start.size, 1)), 3, p.n_mel, p.n_frames), dtype=torch.float32, device=self.device)
            w0 = 0
            for img, st in p.scan(iq, start, chunk_windows=batch, out=buf):
                preds = ops.non_max_suppression(self.inference(img), a["conf"], a["iou"], classes=a["classes"], agnostic=a["agnostic_nms"],
                                                max_det=a["max_det"])
                for k, pr in enumerate(preds):
                    pr = pr[:, :6].float().clone()
                    ops.clip_boxes(pr[:, :4], img.shape[2:])                 # what postprocess's scale_boxes comes to at gain 1
                    rows.append(pr)
                    wins.append(torch.full((pr.shape[0],), w0 + k, dtype=torch.int32, device=pr.device))
                w0 += len(st)
            rows = torch.cat(rows) if rows else torch.zeros((0, 6), dtype=torch.float32, device=self.device)
            wins = torch.cat(wins) if wins else torch.zeros((0,), dtype=torch.int32, device=self.device)
            if merge is not None and rows.shape[0]:
                keep = kops.scan_merge(wins, rows[:, :4].contiguous(), rows[:, 4].contiguous(), rows[:, 5].to(torch.int32), start, p.n_frames,
                                       metric=merge, thres=merge_thres, agnostic=a["agnostic_nms"])
                rows, wins = rows[keep], wins[keep]
        rows, wins = rows.cpu(), wins.cpu().to(torch.int64)
        boxes = rows.to(torch.float64)
        off = torch.from_numpy(start)[wins].to(torch.float64)
        boxes[:, 0] += off
        boxes[:, 2] += off
        tf = scan_boxes_to_tf(boxes, sample_rate, center_freq, p)
        res = ScanResults(boxes, wins, tf, getattr(self.model, "names", None), start, float(sample_rate), float(center_freq), plan)
        res.hop = p.hop
        return res if link is None else self.link(res, **link)

    def link(self, results, gap_t="auto", gap_f="auto", align=0.5, agnostic=False, hop=None):
        """Link the boxes of one emission — the pieces that windows shorter than it, or bands narrower than it, cut it into —
        into tracks (``sy11.data.link``, ``csrc/link.hip``) -> the same ``results``, with ``results.track`` (n,) int64 the track of
        every row and ``results.tracks`` the ``Tracks`` table (union rectangle, best class, confidence, member rows), which
        ``extract`` takes in place of the results to cut one clip per emission.  Rows of one class (``agnostic``: of any) are linked
        when they continue each other in time — at most ``gap_t`` seconds apart ("auto": 8 STFT hops of the scanned rate) and
        sharing ``align`` of the narrower one's bandwidth — or, with ``gap_f`` (Hz; "auto": 0.0 behind a filter bank with
        ``oversample`` 2, else None = off), in frequency; a track is a connected component.  The defaults are judgements, not
        measurements.  Argument errors are ``ValueError``s raised before anything touches the device; an empty ``results`` gives an
        empty ``Tracks`` with no launch."""
        from ..data.link import link_results
        tracks = link_results(results, self.device, gap_t, gap_f, align, agnostic, hop)
        results.track, results.tracks = tracks.track, tracks
        return results

    def extract(self, iq, results, sample_rate, center_freq=0.0, rows=None, pad_t=0.0, pad_f=0.1, decimate="auto", chunk_samples=1 << 24):
        """Every detection of ``results`` (a ``ScanResults`` of this capture) as baseband IQ -> ``sy11.data.extract.Extraction``: per row
        the band of the box (widened by ``pad_f`` on both sides) is shifted to 0 Hz, low-passed, decimated by a power of two and cut to
        the box's time span (widened by ``pad_t`` seconds), all clips of a staged chunk in ONE launch (``csrc/extract.hip``).  ``iq``: what
        ``open_iq`` returns.  ``sample_rate`` / ``center_freq`` are the CAPTURE's own, always passed explicitly: after a resampled or
        channelised scan ``results.sample_rate`` is the output rate, while ``results.tf`` — the only thing read here — is in seconds
        and absolute Hz of the capture, so extraction works the same behind ``scan``, ``scan(resample_to=)`` and ``scan(channels=)``.
        ``rows``: the rows to extract (default: all); ``decimate``: "auto" (the largest power of two <= 64 that keeps the padded band
        inside the flat, alias-free 84 % of the output rate) or one power of two for all rows.  Argument errors are ``ValueError``s
        raised before anything touches the device; an empty ``results`` gives an empty ``Extraction`` with no launch."""
        from ..data.extract import extract_results
        return extract_results(iq, results, sample_rate, center_freq, self.device, rows, pad_t, pad_f, decimate, chunk_samples)

    def measure(self, iq, results, sample_rate, center_freq=0.0, rows=None, n_fft=1024, pad_f=0.25, beta=0.99, noise_band=0.8,
                envelope=True, chunk_samples=1 << 24):
        """Measure every detection of ``results`` (a ``ScanResults`` of this capture, or its ``Tracks``) -> ``sy11.data.measure.Measurement``:
        the Welch power spectrum of the box's time span (periodic Hann, ``n_fft`` in {64 .. 1024}, half-overlapped frames anchored at
        sample 0), all boxes of a staged chunk in ONE launch and one reduction launch at the end (``csrc/measure.hip``).  From it: the
        power inside the box's bins, the noise density (the median of the bins outside the box widened by ``pad_f`` on both sides, within
        the central ``noise_band`` of the capture, corrected to a mean), the SNR, the ``beta`` occupied bandwidth and the power-weighted
        centre over the widened span, and with ``envelope`` the in-box power of every frame.  ``iq``, ``sample_rate`` / ``center_freq`` and
        ``rows`` as in ``extract``.  Argument errors are ``ValueError``s raised before anything touches the device; an empty ``results``
        gives an empty ``Measurement`` with no launch."""
        from ..data.measure import measure_results
        return measure_results(iq, results, sample_rate, center_freq, self.device, rows, n_fft, pad_f, beta, noise_band, envelope,
                               chunk_samples)

    def characterize(self, extraction, n_fft=1024, min_rate=None, line_db=13.0):
        """Say what kind of signal every clip of ``extraction`` (what ``extract`` returned) holds ->
        ``sy11.data.characterize.Characterization``: per clip the Welch spectra (periodic Hann, ``n_fft`` in {64 .. 1024}, half-overlapped
        frames from the clip's first sample) of |x|^2, x^2 and x^4, all clips in ONE launch and one reduction launch (``csrc/cyclo.hip``).
        The line of |x|^2 gives the ``symbol_rate`` (searched from ``min_rate`` Hz up; ``keyed`` when it stands ``line_db`` dB above the median
        floor), the lines of x^2 and x^4 the carrier's offset from the clip's centre at ``order`` 2 (BPSK, a bare carrier) or 4 (a
        four-phase constellation), hence ``carrier``; ``c42`` is the normalised fourth-order cumulant and ``power`` the mean |x|^2.  The 13 dB
        default of ``line_db`` is a judgement, not a measurement.  A clip shorter than ``n_fft`` is marked invalid.  Argument errors are
        ``ValueError``s raised before anything touches the device; an empty extraction gives an empty ``Characterization`` with no launch."""
        from ..data.characterize import characterize_extraction
        return characterize_extraction(extraction, n_fft, min_rate, line_db)

    def demodulate(self, extraction, characterization=None, *, symbol_rate=None, offset=None, order=None, beta=0.35, span=8, block=32):
        """Say what every clip of ``extraction`` (what ``extract`` returned) sent and how clean it was -> ``sy11.data.demodulate.Demodulation``:
        per clip the corrected symbols, the decisions (``bits(i)``) and ``evm`` / ``mer_db``, feed-forward (``csrc/demod.hip``).  The symbol rate,
        the carrier offset and the order (2: BPSK, 4: four-phase) of every clip come from ``characterization`` (what ``characterize``
        returned for the same extraction) OR from ``symbol_rate`` / ``offset`` (Hz from the clip's centre) / ``order`` (scalars broadcast).  All
        clips go through THREE launches: de-rotation, the root-raised-cosine matched filter (roll-off ``beta``, ``span`` symbols each side) and
        the timing partials of every 512-sample tile; the symbols, interpolated at the instants of a line fitted through the tiles' timing
        phases, with the sums of s^order per ``block`` symbols; the symbols turned back by the carrier phase tracked over the blocks, and
        the decisions.  The stream is right up to a rotation by 2 pi / order (``phase_ambiguity``).  A clip that cannot be demodulated
        (order not 2 or 4, not keyed, 2.5 <= fs / symbol_rate <= 16 violated, too short) is a row with ``valid`` False and a ``reason``.  Argument
        errors are ``ValueError``s raised before anything touches the device; without a valid clip nothing is launched."""
        from ..data.demodulate import demodulate_extraction
        return demodulate_extraction(extraction, characterization, symbol_rate=symbol_rate, offset=offset, order=order, beta=beta, span=span,
                                     block=block)

    def demodulate_fsk(self, extraction, *, symbol_rate, offset=0.0, pulse="gauss", bt=0.5, span=2, block=32):
        """Read every frequency-keyed clip (2-FSK, GFSK, GMSK) of ``extraction`` (what ``extract`` returned) by its discriminator ->
        ``sy11.data.demodulate_fsk.FskDemodulation``, a ``Demodulation`` at order 2 that ``find_frames``, ``equalize``, ``decode``, ``decode_ldpc`` and ``correct`` take as it is
        (``csrc/demod_fsk.hip``).  ``symbol_rate`` and ``offset`` (Hz from the clip's centre, a first guess of the midpoint of the two tones) come from the
        caller, per clip or as scalars, as do ``pulse``, ``bt`` and ``span``.  All clips go through THREE launches: the instantaneous frequency ``arg(x[n] conj(x[n - 1])) / 2 pi`` of every
        sample, filtered by a Gaussian of bandwidth-time product ``bt`` over ``span`` symbols each side (``pulse="gauss"``) or by an integrate-and-dump
        over one symbol (``pulse="rect"``), with the timing partials of every 512-sample tile; the symbols, interpolated at the instants of a line
        fitted through the tiles' timing phases, with the sums of the two levels per ``block`` symbols; the symbols scaled so that the two tones
        sit at +-1, and the decisions.  ``carrier_fit`` is the midpoint of the two tones, ``deviation`` half their distance (Hz), ``mod_index`` their
        distance over the symbol rate.  Which tone is "1" is not known (``phase_ambiguity`` 2): ``find_frames``' rotation 1 is the inverted polarity.
        A clip that cannot be demodulated (2.5 <= fs / symbol_rate <= 16 violated, |offset| >= fs / 2, too short, one tone only) is a row with
        ``valid`` False and a ``reason``.  Not done here: a pre-detection filter (``extract``'s low-pass is the one), 4-FSK, estimating the symbol rate
        (``characterize`` calls a constant-envelope clip "not keyed"), coherent MSK detection, a carrier that drifts over the clip.  Argument errors
        are ``ValueError``s raised before anything touches the device; without a valid clip nothing is launched."""
        from ..data.demodulate_fsk import demodulate_fsk_extraction
        return demodulate_fsk_extraction(extraction, symbol_rate=symbol_rate, offset=offset, pulse=pulse, bt=bt, span=span, block=block)

    def demodulate_ofdm(self, extraction, *, n_fft, cp, carriers, pilots, order=4, offset=0.0, spacing=None, advance=None):
        """Read every cyclic-prefix OFDM clip of ``extraction`` (what ``extract`` returned) -> ``sy11.data.demodulate_ofdm.OfdmDemodulation``, a ``Demodulation`` at the clips'
        ``order`` that ``find_frames``, ``equalize``, ``decode``, ``decode_ldpc`` and ``correct`` take as it is (``csrc/demod_ofdm.hip``).  The clip must be sampled at ``n_fft`` carrier
        spacings (a capture at another rate goes through the resampler in front of the scan, or through ``extract(decimate=)``); ``cp`` is the prefix in samples, ``carriers`` the
        data carriers (signed), ``pilots`` a mapping k -> +-1 or a pair ``(k_p, c_p)``: at least 2, uniformly spaced, the same in every OFDM symbol.  ``order`` (2 or 4) and ``offset``
        (Hz from the clip's centre, right to within half a carrier spacing) are per clip or scalars; ``n_fft``, ``cp``, ``carriers``, ``pilots`` and ``advance`` may be given per clip as
        lists.  All clips go through THREE launches: the prefix correlation ``x[n + n_fft] conj(x[n])`` folded over the period, whose peak gives where the OFDM symbols start
        (``timing``) and the fractional carrier offset (``cfo``, ``carrier_fit``, ``cp_corr``); the FFT of every OFDM symbol, its window started ``advance`` samples inside the prefix,
        with the pilots' values and the power; the data carriers turned by the pilots' common phase and slope (``slope``) and scaled by their amplitude, and the decisions.  OFDM symbols
        whose pilots are weaker than half the strongest are not ``active``: they stay in ``symbols`` so that a position maps to a time, and stay out of ``gain``, ``evm`` and ``mer_db``.
        The pilots fix the phase (``phase_ambiguity`` 1).  A clip that cannot be demodulated (order, ``spacing`` against the clip's rate, |offset| >= fs / 2, fewer than 2 whole periods)
        is a row with ``valid`` False and a ``reason``.  Not done here: pilots that change from symbol to symbol, non-uniform pilots, a per-carrier channel estimate, a search over
        whole carrier spacings, sampling-clock offset, 16-QAM and above, interleaver and scrambler, n_fft above 1024.  Argument errors are ``ValueError``s raised before anything
        touches the device; without a valid clip nothing is launched."""
        from ..data.demodulate_ofdm import demodulate_ofdm_extraction
        return demodulate_ofdm_extraction(extraction, n_fft=n_fft, cp=cp, carriers=carriers, pilots=pilots, order=order, offset=offset, spacing=spacing, advance=advance)

    def find_frames(self, demodulation, words, *, payload=0, threshold=0.8, max_errors=None, t0=None):
        """Say where framed data starts in every clip of ``demodulation`` (what ``demodulate`` returned) and at which of the ``order`` rotations the
        demodulator landed -> ``sy11.data.frames.Frames``, one row per frame sorted by (clip, word, position) (``csrc/framesync.hip``).  ``words``: the
        sync words, each a sequence of 0/1 bits, first bit first, mapped to symbols as ``Demodulation.bits`` maps them.  All clips and words go
        through THREE launches: the normalised correlation ``rho`` of the corrected symbols with every word at every position, in float64
        and one fixed order; its peaks at or above ``threshold`` (of equal peaks closer than a word the earliest); and, for every peak, the
        word's symbol and bit errors after turning the symbols back by the peak's rotation and ``payload`` symbols' bits after the word,
        packed on the device (``Frames.payload_bits(k)``).  ``max_errors`` drops frames with more word symbol errors; ``t0`` (per clip, seconds:
        ``extraction.t0``) is added to ``time``.  A pair (clip, word) that cannot be searched (clip not valid, bit count not divisible by
        log2(order), word outside 8 .. 256 symbols or longer than the clip) is listed in ``Frames.pairs`` with a reason.  Argument errors are
        ``ValueError``s raised before anything touches the device; without a valid pair nothing is launched."""
        from ..data.frames import find_frames
        return find_frames(demodulation, words, payload=payload, threshold=threshold, max_errors=max_errors, t0=t0)

    def equalize(self, frames, demodulation, *, taps=7, reg=1e-3, refine=0):
        """Undo the multipath of every frame of ``frames`` (what ``find_frames`` returned for ``demodulation``) -> ``sy11.data.equalize.Equalized``, which ``find_frames`` and
        ``decode`` take in place of the demodulation (``csrc/equalize.hip``).  The frame search says where each known word sits and at which rotation, so the
        equaliser is feed-forward, in TWO launches over all frames and clips: per frame, one wavefront solves the regularised least-squares problem
        (``reg``, relative to the mean diagonal) for the ``taps`` (odd, 3 .. 15) taps of a symbol-spaced FIR that maps the received word onto the word as sent,
        by a Cholesky factorisation in float64; then the taps of each frame filter the symbols it owns, from its word to the end of its payload, of
        overlapping frames the later one, in float64 and one fixed order, and every other symbol is copied bit for bit.  With ``refine`` beyond the word's
        length both launches run again, trained on ``refine`` symbols of which those after the word are the first pass's decisions.  The symbols keep
        the clip's rotation and gain.  Per frame ``Equalized.frames`` lists ``mse_before`` / ``mse_after`` over the word and the smallest pivot; a frame whose word is
        shorter than twice the taps ("word"), whose clip has no positive gain ("gain") or is not valid ("clip"), or whose system is singular ("singular")
        is a row with ``valid`` False and its symbols pass through.  Argument errors are ``ValueError``s raised before anything touches the device; without a
        valid frame nothing is launched."""
        from ..data.equalize import equalize_frames
        return equalize_frames(frames, demodulation, taps=taps, reg=reg, refine=refine)

    def decode(self, frames, demodulation, *, n_info, polys=(0o171, 0o133), puncture=None, tail=True, whiten=None, crc=None, soft_scale=32.0):
        """Turn the channel bits of every frame of ``frames`` (what ``find_frames`` returned for ``demodulation``) into a checked message ->
        ``sy11.data.decode.Decoded``, one row per frame in the frames' order (``csrc/fec.hip``).  The frames are coded with the rate 1/2, K = 7
        convolutional code of the generators ``polys``, ``n_info`` information bits (the check field included) followed by six zero bits when ``tail``,
        punctured by the 0/1 pattern ``puncture`` (1 = sent), whitened by the 0/1 sequence ``whiten`` (``sy11.data.decode.lfsr_bits``) and protected by
        ``crc`` (a name of ``sy11.data.decode.CRCS`` or a Rocksoft dict).  All frames go through THREE launches: the payload symbols turned back by
        the frame's rotation, scaled so that a clean component is ``soft_scale``, quantised to int8 and depunctured; the Viterbi decoder, one
        wavefront per frame and one lane per state, in exact integer arithmetic; and the decision encoded again and compared with the
        received signs (``channel_errors`` of ``n_channel``, ``ber``), the information bits de-whitened and packed on the device (``Decoded.bits(k)``,
        ``message(k)``) and their CRC (``crc_ok``).  ``find_frames`` must have read ``payload`` symbols enough for the code; a frame cut short by the
        clip's end is a row with ``valid`` False and the reason "short", one of a clip without a positive gain has the reason "gain".
        Argument errors are ``ValueError``s raised before anything touches the device; without a valid frame nothing is launched."""
        from ..data.decode import decode_frames
        return decode_frames(frames, demodulation, n_info=n_info, polys=polys, puncture=puncture, tail=tail, whiten=whiten, crc=crc, soft_scale=soft_scale)

    def decode_ldpc(self, frames, demodulation, *, code, iterations=20, scale=12, whiten=None, crc=None, soft_scale=16.0):
        """Turn the channel bits of every frame of ``frames`` (what ``find_frames`` returned for ``demodulation``) into a checked message when the frames are
        block-coded with a quasi-cyclic LDPC code -> ``sy11.data.ldpc.LdpcDecoded``, one row per frame in the frames' order (``csrc/ldpc.hip``).  ``code``: an
        ``LdpcCode`` (``sy11.data.ldpc.ldpc_code`` of a standard's base matrix typed in, or the seeded test code ``ldpc_staircase``) or a dict ``{"Z": ..., "base": ...}``
        with -1 for an empty block and the circulant's shift otherwise; N = nb Z received bits carry K = N - mb Z information bits, the first K of the
        codeword, whitened by the 0/1 sequence ``whiten`` (``sy11.data.decode.lfsr_bits``) and protected by ``crc`` (a name of ``sy11.data.decode.CRCS`` or a Rocksoft
        dict), the check field their last bits.  All frames go through THREE launches: the payload symbols turned back by the frame's rotation, scaled so
        that a clean component is ``soft_scale`` and quantised to int8 (the first launch of ``decode``, unchanged); the layered normalised min-sum decoder,
        one workgroup per frame with the posteriors in LDS, at most ``iterations`` sweeps with the check messages scaled by ``scale`` sixteenths, in exact
        integer arithmetic, a frame stopping at the first sweep that satisfies every check (``iterations``, ``unsatisfied``, ``converged``); and the decision
        compared with the received signs (``channel_errors`` of ``n_channel``, ``ber``), the information bits de-whitened and packed on the device
        (``LdpcDecoded.bits(k)``, ``message(k)``, ``posterior(k)``) and their CRC (``crc_ok``).  ``find_frames`` must have read ``payload`` symbols enough for the N
        bits; a frame cut short by the clip's end is a row with ``valid`` False and the reason "short", one of a clip without a positive gain has the reason
        "gain".  The result goes on to ``correct`` as a ``Decoded`` does.  Shortened or punctured codes and named presets are out of scope.  Argument errors
        are ``ValueError``s raised before anything touches the device; without a valid frame nothing is launched."""
        from ..data.ldpc import decode_ldpc_frames
        return decode_ldpc_frames(frames, demodulation, code=code, iterations=iterations, scale=scale, whiten=whiten, crc=crc, soft_scale=soft_scale)

    def correct(self, decoded, *, code="dvb-204-188", interleave=1, offset=0, crc=None):
        """Remove the byte errors the Viterbi decoder left in every frame of ``decoded`` (what ``decode`` returned) with the Reed-Solomon outer code ->
        ``sy11.data.correct.Corrected``, one row per frame in the frames' order (``csrc/rs.hip``).  ``code``: a name of ``sy11.data.correct.CODES``
        ("dvb-204-188", "rs-255-239", "ccsds-255-223", "ccsds-255-239") or a dict n, k, poly, fcr, prim over GF(2^8); the CCSDS presets use the
        conventional basis, the dual basis is out of scope.  A frame holds ``interleave`` codewords (1 .. 8), interleaved byte by byte from byte
        ``offset`` of its de-whitened bytes.  All frames and codewords go through TWO launches: every codeword, one wavefront each, is de-interleaved
        and corrected by up to ``(n - k) // 2`` byte errors in exact integer arithmetic (syndromes, Berlekamp-Massey, a Chien search, Forney's
        formula) - a codeword beyond that is reported in ``errors`` as -1 and passes through; then per frame the failed codewords, the corrected
        byte and bit errors and, with ``crc`` (a name of ``sy11.data.decode.CRCS`` or a Rocksoft dict of whole bytes), the check over the information
        bytes (``crc_ok``; ``message(k)`` is what precedes the check field).  A frame the decoder left out is a row with ``valid`` False and the reason
        "undecoded".  Argument errors are ``ValueError``s raised before anything touches the device; without a valid frame nothing is launched."""
        from ..data.correct import correct_decoded
        return correct_decoded(decoded, code=code, interleave=interleave, offset=offset, crc=crc)

    def _scan_channels(self, iq, sample_rate, center_freq, overlap, batch, merge, merge_thres, stride_frames, start, resample_to,
                       tune_to, channels, oversample, select):
        """``scan`` through the filter bank.  Chunks are outermost: the selected bands' strip generators advance in lock-step over
        one ``ChannelizedCapture``, whose first slice of a chunk is the chunk's one channelise launch and whose other slices are
        rows of that block; every band's chunk is consumed (inference + NMS) before the next band's is produced, so one image
        buffer serves all of them."""
        from .. import ops as kops
        from ..data import spectrogram as sp
        from ..data.channelize import ChannelizedCapture, merge_channels, plan_scan_channels
        p = self.producer
        plan, select = plan_scan_channels(sample_rate, channels, oversample, select, self.trained, resample_to, tune_to)
        if (p.n_mel, p.n_frames) != tuple(self.imgsz):
            raise ValueError(f"the producer's {p.n_mel} x {p.n_frames} images do not match imgsz={self.imgsz}")
        cap = ChannelizedCapture(iq, plan, self.device)
        if start is None:
            start = sp.plan_windows(len(cap), overlap, stride_frames, p.n_fft, p.hop, p.n_frames)
        start = np.asarray(start, dtype=np.int64).reshape(-1)
        a = self.args
        fs_out = plan.fs_out
        rows, wins = {k: [] for k in select}, {k: [] for k in select}
        out_b, out_w, out_c = [], [], []
        with self._lock:
            buf = torch.empty((min(batch, max(start.size, 1)), 3, p.n_mel, p.n_frames), dtype=torch.float32, device=self.device)
            gens = [(k, p.scan(cap.channel(k), start, chunk_windows=batch, out=buf)) for k in select]
            w0 = 0
            for _ in sp.plan_chunks(start, batch, p.n_fft, p.hop, p.n_frames):
                n_st = 0
                for k, gen in gens:
                    img, st = next(gen)
                    preds = ops.non_max_suppression(self.inference(img), a["conf"], a["iou"], classes=a["classes"],
                                                    agnostic=a["agnostic_nms"], max_det=a["max_det"])
                    for j, pr in enumerate(preds):
                        pr = pr[:, :6].float().clone()
                        ops.clip_boxes(pr[:, :4], img.shape[2:])
                        rows[k].append(pr)
                        wins[k].append(torch.full((pr.shape[0],), w0 + j, dtype=torch.int32, device=pr.device))
                    n_st = len(st)
                w0 += n_st
            for k in select:
                r = torch.cat(rows[k]) if rows[k] else torch.zeros((0, 6), dtype=torch.float32, device=self.device)
                w = torch.cat(wins[k]) if wins[k] else torch.zeros((0,), dtype=torch.int32, device=self.device)
                if merge is not None and r.shape[0]:
                    keep = kops.scan_merge(w, r[:, :4].contiguous(), r[:, 4].contiguous(), r[:, 5].to(torch.int32), start, p.n_frames,
                                           metric=merge, thres=merge_thres, agnostic=a["agnostic_nms"])
                    r, w = r[keep], w[keep]
                out_b.append(r.cpu())
                out_w.append(w.cpu().to(torch.int64))
                out_c.append(torch.full((r.shape[0],), k, dtype=torch.int64))
        tfs = []
        for k, r, w in zip(select, out_b, out_w):
            b = r.to(torch.float64)
            off = torch.from_numpy(start)[w].to(torch.float64)
            b[:, 0] += off
            b[:, 2] += off
            tfs.append(scan_boxes_to_tf(b, fs_out, float(center_freq) + float(plan.offset_hz[k]), p))
        boxes = torch.cat([r.to(torch.float64) for r in out_b])
        wins, chan, tf = torch.cat(out_w), torch.cat(out_c), torch.cat(tfs)
        off = torch.from_numpy(start)[wins].to(torch.float64)
        boxes[:, 0] += off
        boxes[:, 2] += off
        if merge is not None and plan.oversample == 2 and boxes.shape[0]:
            keep = torch.from_numpy(merge_channels(tf.numpy(), boxes[:, 4].numpy(), boxes[:, 5].numpy(), chan.numpy(), merge, merge_thres,
                                                   a["agnostic_nms"]))
            boxes, wins, chan, tf = boxes[keep], wins[keep], chan[keep], tf[keep]
        return ScanResults(boxes, wins, tf, getattr(self.model, "names", None), start, float(fs_out), float(center_freq), None, chan, plan)


def link_keywords(link):
    """``scan(link=...)`` -> the keywords of ``link`` or None; their argument errors are raised here, before the scan starts."""
    if link is None or link is False:
        return None
    if link is not True and not isinstance(link, dict):
        raise ValueError(f"link must be None, True or a dict of link's keywords, got {link!r}")
    from ..data.link import check_link_args
    kw = {} if link is True else dict(link)
    unknown = set(kw) - {"gap_t", "gap_f", "align", "agnostic", "hop"}
    if unknown:
        raise ValueError(f"link: unknown keywords {sorted(unknown)}")
    check_link_args(**kw)
    return kw


def plan_scan_ddc(sample_rate, center_freq, resample_to=None, tune_to=None, trained=None):
    """The ``ResamplePlan`` of ``scan(..., resample_to, tune_to)``; every argument error of the two keywords is raised here.
    ``trained``: the checkpoint's ``train_args`` (what ``"model"`` refers to)."""
    from ..data.resample import plan_resample
    trained = trained or {}
    if isinstance(resample_to, str) or isinstance(tune_to, str):
        if any(isinstance(v, str) and v != "model" for v in (resample_to, tune_to)):
            raise ValueError(f"resample_to / tune_to take Hz or 'model', got {resample_to!r} / {tune_to!r}")
        if resample_to == "model":
            if not trained.get("sample_rate"):
                raise ValueError("resample_to='model': this checkpoint records no sample_rate (it was not trained from IQ captures)")
            resample_to = float(trained["sample_rate"])
            if tune_to is None and trained.get("center_freq"):       # a recorded centre of 0 is "baseband, untuned": nothing to tune to
                tune_to = "model"
        if tune_to == "model":
            if "center_freq" not in trained:
                raise ValueError("tune_to='model': this checkpoint records no center_freq")
            tune_to = float(trained["center_freq"])
    fs_in = sample_rate
    fs_out = fs_in if resample_to is None else resample_to
    shift = 0.0 if tune_to is None else float(tune_to) - float(center_freq)
    if shift != 0.0 and abs(shift) + float(fs_out) / 2 > float(fs_in) / 2:
        raise ValueError(f"the kept band {float(tune_to)!r} +- {float(fs_out) / 2!r} Hz is not inside the capture's "
                         f"{float(center_freq)!r} +- {float(fs_in) / 2!r} Hz")
    return plan_resample(fs_in, fs_out, shift)


def scan_boxes_to_tf(boxes, sample_rate, center_freq, producer):
    """(n, >= 4) float64 [X1, y1, X2, y2] in strip frames / image rows -> (n, 4) float64 [t0_s, f_lo_hz, t1_s, f_hi_hz]; a pixel
    edge at coordinate c is row / column c - 0.5.  Rows grow with frequency, so y1 is the low edge."""
    from ..data.spectrogram import cols_to_time, rows_to_freq
    b = boxes[:, :4].to(torch.float64).numpy()
    alpha = getattr(producer, "warp_alpha", 1.25)
    t0, t1 = (cols_to_time(b[:, i] - 0.5, sample_rate, producer.n_fft, producer.hop) for i in (0, 2))
    f0, f1 = (rows_to_freq(b[:, i] - 0.5, sample_rate, center_freq, producer.n_fft, producer.n_mel, alpha) for i in (1, 3))
    return torch.from_numpy(np.stack((t0, f0, t1, f1), 1))
