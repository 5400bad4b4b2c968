"""Which layers take the fused 1x1 backward (sy11.nn.modules.conv.fused_dwgrad_applies, a pure function of the layer's geometry,
the dtype, the pixel count and two switches) and how the entry point cuts a filter into column blocks
(sy11_dgrad_wgrad_1x1_plan, host arithmetic of include/sy11.h).  No GPU."""
import itertools

import pytest
import torch

from sy11 import _lib, ops
from sy11.nn.modules import conv as conv_mod

T = conv_mod._DWGRAD_FUSED_MIN_PIXELS


def test_threshold_is_the_measured_one():
    assert T == 409600          # 80 x 80 x 64: every 1x1 layer of the 160^2 and 80^2 maps at batch 64


def test_truth_table():
    """Every combination of the eight inputs: true exactly for dense 1x1 stride-1 undilated 16-bit layers at or above the threshold,
    ordered mode off, not on the zero-padded-channel path."""
    dtypes = [torch.float16, torch.bfloat16, torch.float32]
    n_true = 0
    for k, s, g, d, dt, M, det, padded in itertools.product([1, 3], [1, 2], [1, 2], [1, 2], dtypes, [T - 1, T, 4 * T], [False, True], [False, True]):
        want = k == 1 and s == 1 and g == 1 and d == 1 and dt != torch.float32 and M >= T and not det and not padded
        assert conv_mod.fused_dwgrad_applies(k, s, g, d, dt, M, det, padded, 64, 64) == want, (k, s, g, d, dt, M, det, padded)
        n_true += want
    assert n_true == 4          # two dtypes x two pixel counts


@pytest.mark.parametrize("C,N,want", [(16, 16, True), (256, 256, True), (96, 128, True), (128, 80, True), (8, 64, False), (64, 8, False),
                                      (72, 64, False), (64, 72, False), (512, 128, False), (128, 272, False)])
def test_channel_counts(C, N, want):
    assert conv_mod.fused_dwgrad_applies(1, 1, 1, 1, torch.float16, T, False, False, C, N) == want


def test_threshold_argument_and_module_constant(monkeypatch):
    assert not conv_mod.fused_dwgrad_applies(1, 1, 1, 1, torch.float16, 512, False, False, 32, 32)
    assert conv_mod.fused_dwgrad_applies(1, 1, 1, 1, torch.float16, 512, False, False, 32, 32, threshold=512)
    monkeypatch.setattr(conv_mod, "_DWGRAD_FUSED_MIN_PIXELS", 512)
    assert conv_mod.fused_dwgrad_applies(1, 1, 1, 1, torch.float16, 512, False, False, 32, 32)
    assert not conv_mod.fused_dwgrad_applies(1, 1, 1, 1, torch.float16, 511, False, False, 32, 32)


def plan_ref(C, N, lds):
    """include/sy11.h, sy11_dgrad_wgrad_1x1_plan, in Python."""
    pad = lambda v: 64 if v <= 64 else 128 if v <= 128 else 256
    np_ = pad(N)
    fits = [c for c in (256, 128, 64) if np_ * c <= 32768 and 256 * (np_ + c) + 2 * np_ * c <= lds]
    if not fits:
        return None
    nb = -(-C // fits[0])
    cb = -(-(-(-C // nb)) // 16) * 16
    return np_, pad(cb), cb, -(-C // cb)


@pytest.mark.parametrize("lds", [160 * 1024, 64 * 1024])
def test_plan_covers_every_channel_once(lds):
    for C, N in itertools.product(range(16, 257, 16), repeat=2):
        if plan_ref(C, N, lds) is None:                                       # 64 KB: no tile for N > 128
            with pytest.raises(_lib.Sy11Error):
                ops.dgrad_wgrad_1x1_plan(C, N, lds)
            continue
        np_, cp, cb, blocks = ops.dgrad_wgrad_1x1_plan(C, N, lds)
        assert (np_, cp, cb, blocks) == plan_ref(C, N, lds), (C, N)
        assert N <= np_ and cb <= cp and np_ * cp <= 32768 and 256 * (np_ + cp) + 2 * np_ * cp <= lds
        assert cb % 16 == 0 and (blocks - 1) * cb < C <= blocks * cb          # the blocks tile 0 .. C, none is empty


def test_plan_of_the_model_shapes():
    """The qualifying layers of yolo11s at 160 KB of LDS: one column block unless the filter is 192 x 256."""
    want = {(64, 64): (64, 64, 64, 1), (96, 128): (128, 128, 96, 1), (128, 128): (128, 128, 128, 1), (128, 80): (128, 128, 128, 1),
            (192, 128): (128, 256, 192, 1), (192, 256): (256, 128, 96, 2), (256, 256): (256, 128, 128, 2)}
    for (C, N), p in want.items():
        assert ops.dgrad_wgrad_1x1_plan(C, N) == p, (C, N)


def test_plan_refusals():
    L = _lib.load()
    assert L.sy11_dgrad_wgrad_1x1_plan(64, 64, 160 * 1024, None, None, None, None) == -1          # SY11_EINVAL
    for C, N, lds in [(8, 64, 160 * 1024), (64, 24, 160 * 1024), (512, 64, 160 * 1024), (64, 64, 1024)]:
        with pytest.raises(_lib.Sy11Error):
            ops.dgrad_wgrad_1x1_plan(C, N, lds)


def test_wrapper_is_declared_and_profiled():
    assert "sy11_conv2d_dgrad_wgrad_1x1" in _lib.SIGNATURES and len(_lib.SIGNATURES["sy11_conv2d_dgrad_wgrad_1x1"]) == 14
    assert _lib.CFG_DWGRAD_1X1 == 101
    assert _lib.get_option("dwgrad_fused") in (0, 1) and _lib.get_option("dwgrad_wg") >= 0
