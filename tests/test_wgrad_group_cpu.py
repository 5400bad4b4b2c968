"""CPU: the grouped filter-gradient entry point (sy11_conv2d_wgrad_group) refuses what it must before anything is launched, and
its host work split (sy11_wgrad_group_plan, the formula in include/sy11.h) hands every pixel of every tile of every problem to
exactly one workgroup."""
import ctypes as C
import math

import pytest

ALIGNED = 0x10000            # never dereferenced: every call here returns before the first launch


def lib():
    from sy11 import _lib
    return _lib


def problem(dtype=1, B=2, H=6, W=6, Cn=16, N=16, k=1, s=1, p=0, d=1, groups=1, x_ld=None, dy_ld=None, x=ALIGNED, dy=ALIGNED, dw=ALIGNED):
    L = lib()
    OH, OW = (H + 2 * p - d * (k - 1) - 1) // s + 1, (W + 2 * p - d * (k - 1) - 1) // s + 1
    x_ld, dy_ld = Cn if x_ld is None else x_ld, N if dy_ld is None else dy_ld
    q = L.WgradProblem()
    q.desc = L.ConvDesc(dtype, B, H, W, Cn, x_ld, OH, OW, N, dy_ld, k, k, s, s, p, p, d, d, groups, 0, 1)
    q.x, q.dy, q.dw, q.dy_ld = x, dy, dw, dy_ld
    return q


def group_call(problems, dtype=1, count=None, target=0):
    L = lib()
    arr = (L.WgradProblem * max(len(problems), 1))(*problems)
    rc = L.load().sy11_conv2d_wgrad_group(dtype, len(problems) if count is None else count, arr, target, None)
    return rc, L.load().sy11_last_error().decode()


EINVAL, EUNSUPPORTED = -1, -2


def test_constants_agree_with_the_header_and_the_kernel_file():
    import re
    from pathlib import Path
    root = Path(__file__).resolve().parents[1]
    L = lib()
    assert int(re.search(r"#define SY11_WGRAD_GROUP_MAX (\d+)", (root / "include" / "sy11.h").read_text()).group(1)) == L.WGRAD_GROUP_MAX
    tune_h = (root / "spectrogram-yolov11_amd" / "csrc" / "tune.h").read_text()
    assert int(re.search(r"SY11_CFG_WGRAD_GROUP = (\d+);", tune_h).group(1)) == L.CFG_WGRAD_GROUP
    assert int(re.search(r"SY11_WGRAD_NCFG = (\d+);", tune_h).group(1)) == 20 and not 0 <= L.CFG_WGRAD_GROUP < 20


def test_refuses_a_null_list_and_bad_counts():
    L = lib()
    rc = L.load().sy11_conv2d_wgrad_group(1, 1, None, 0, None)
    assert rc == EINVAL and "null" in L.load().sy11_last_error().decode()
    rc, msg = group_call([problem()], count=0)
    assert rc == EINVAL and "count 0" in msg
    many = [problem() for _ in range(L.WGRAD_GROUP_MAX + 1)]
    rc, msg = group_call(many)
    assert rc == EINVAL and f"count {L.WGRAD_GROUP_MAX + 1}" in msg


def test_refuses_f32_and_grouped_problems_as_unsupported():
    rc, msg = group_call([problem(dtype=0)], dtype=0)
    assert rc == EUNSUPPORTED and "16-bit" in msg
    rc, msg = group_call([problem(dtype=7)], dtype=7)
    assert rc == EINVAL and "dtype" in msg
    rc, msg = group_call([problem(), problem(dtype=2)])            # bf16 problem in an f16 group
    assert rc == EINVAL and "problem 1" in msg and "dtype" in msg
    rc, msg = group_call([problem(), problem(groups=2)])
    assert rc == EUNSUPPORTED and "problem 1" in msg and "groups=2" in msg
    rc, msg = group_call([problem(Cn=16, N=16, groups=16)])        # depthwise
    assert rc == EUNSUPPORTED and "groups=16" in msg


def test_refuses_bad_strides_pointers_and_geometry():
    rc, msg = group_call([problem(x_ld=20)])                       # >= C but not a multiple of 8
    assert rc == EINVAL and "pixel strides" in msg
    rc, msg = group_call([problem(), problem(dy_ld=12)])
    assert rc == EINVAL and "problem 1" in msg and "pixel strides" in msg
    rc, msg = group_call([problem(x=ALIGNED + 8)])
    assert rc == EINVAL and "misaligned" in msg
    rc, msg = group_call([problem(dy=ALIGNED + 2)])
    assert rc == EINVAL and "misaligned" in msg
    rc, msg = group_call([problem(dw=ALIGNED + 2)])
    assert rc == EINVAL and "misaligned" in msg
    rc, msg = group_call([problem(dw=None)])
    assert rc == EINVAL and "null" in msg
    rc, msg = group_call([problem(Cn=12)])
    assert rc == EINVAL and "multiples of 8" in msg
    q = problem()
    q.desc.OH += 1
    rc, msg = group_call([q])
    assert rc == EINVAL and "OH/OW" in msg
    rc, msg = group_call([problem()], target=-1)
    assert rc == EINVAL and "target_workgroups" in msg


def test_refuses_ordered_mode_with_valid_arguments():
    L = lib()
    old = L.get_option("deterministic")
    try:
        L.set_option("deterministic", 1)
        rc, msg = group_call([problem(), problem(k=3, p=1)], target=8)
        assert rc == EUNSUPPORTED and "ordered" in msg
        rc, msg = group_call([problem(x_ld=20)], target=8)          # an invalid argument is still reported as such
        assert rc == EINVAL
    finally:
        L.set_option("deterministic", old)


# ------------------------------------------------------------------------------------------------------------ work split
def plan_mirror(M, N, K, G):
    """include/sy11.h, sy11_wgrad_group_plan, in Python."""
    cd = lambda a, b: -(-a // b)
    tiles = [cd(n, 128) * cd(k, 128) for n, k in zip(N, K)]
    stages = [cd(m, 64) for m in M]
    chunk = max(8, cd(sum(t * s for t, s in zip(tiles, stages)), G))
    pps, start = [], [0]
    for m, t, s in zip(M, tiles, stages):
        splits = cd(s, chunk)
        pps.append(64 * cd(s, splits))
        start.append(start[-1] + t * cd(m, pps[-1]))
    return pps, start


YOLO_20 = [(25600, 512, 512)] * 3 + [(25600, 256, 256), (25600, 128, 1152), (25600, 512, 768), (25600, 64, 4608)]
PLAN_TABLE = [
    ([(70, 40, 32)], 1), ([(70, 40, 32)], 512),                                   # one tiny problem: one workgroup whatever G
    ([(63, 8, 8), (64, 8, 8), (65, 8, 8)], 4),                                    # around one stage
    ([(70, 40, 32), (72, 136, 576), (50, 8, 144), (98, 16, 24), (98, 16, 24), (18, 8, 8)], 1),
    ([(70, 40, 32), (72, 136, 576), (50, 8, 144), (98, 16, 24), (98, 16, 24), (18, 8, 8)], 1000),
    (YOLO_20, 512), (YOLO_20, 256), (YOLO_20, 1024),
    ([(102400, 256, 384)] * 4 + [(102400, 64, 576)] * 5 + YOLO_20 * 3, 512),      # a full fork of 30
    ([(1000003, 129, 129), (5, 8, 8)], 7),                                        # a ragged large one beside a tiny one
    ([(131072, 128, 128)] * 32, 512),
]


@pytest.mark.parametrize("probs,G", PLAN_TABLE, ids=lambda v: str(v) if isinstance(v, int) else f"n{len(v)}")
def test_work_split_covers_every_pixel_of_every_tile_once(probs, G):
    from sy11 import ops
    M, N, K = ([q[i] for q in probs] for i in range(3))
    pps, start = ops.wgrad_group_plan(M, N, K, G)
    assert (pps, start) == plan_mirror(M, N, K, G)
    assert start[0] == 0 and len(start) == len(probs) + 1 and all(b > a for a, b in zip(start, start[1:]))
    total = start[-1]
    seen = {}                                                  # (problem, tile) -> list of pixel ranges
    vids = range(total) if total <= 20000 else list(range(0, total, 97)) + [total - 1]
    for vid in vids:
        pi = sum(1 for i in range(1, len(probs)) if vid >= start[i])          # the kernel's scan
        assert start[pi] <= vid < start[pi + 1]
        tiles = math.ceil(N[pi] / 128) * math.ceil(K[pi] / 128)
        split, tile = divmod(vid - start[pi], tiles)
        lo, hi = split * pps[pi], min(M[pi], (split + 1) * pps[pi])
        assert pps[pi] % 64 == 0 and 1 <= hi - lo <= pps[pi], (vid, pi, split, lo, hi)
        seen.setdefault((pi, tile), []).append((lo, hi))
    if total <= 20000:
        for pi in range(len(probs)):
            tiles = math.ceil(N[pi] / 128) * math.ceil(K[pi] / 128)
            for t in range(tiles):
                r = sorted(seen[(pi, t)])
                assert r[0][0] == 0 and r[-1][1] == M[pi] and all(a[1] == b[0] for a, b in zip(r, r[1:])), (pi, t, r)
    # the split follows the target: sum tiles_i * ceil(stages_i / chunk) <= sum tiles_i * stages_i / chunk + sum tiles_i <= G + sum tiles_i
    assert total <= G + sum(math.ceil(n / 128) * math.ceil(k / 128) for n, k in zip(N, K))


def test_plan_refuses_bad_arguments():
    from sy11 import ops
    L = lib()
    for M, N, K, G in (([], [], [], 8), ([64] * 33, [8] * 33, [8] * 33, 8), ([64], [8], [8], 0), ([0], [8], [8], 8), ([64], [8], [-8], 8)):
        with pytest.raises(L.Sy11Error):
            ops.wgrad_group_plan(M, N, K, G)
    assert L.load().sy11_wgrad_group_plan(1, None, None, None, 8, None, None) == EINVAL


def test_engine_switch_and_small_rule_are_functions_of_the_shapes():
    import torch
    from sy11 import engine
    assert engine._WGRAD_GROUP in (True, False)
    small = lambda B, OH, OW: engine._wgrad_is_small((None, torch.empty(B, OH, OW, 0), None, 1, 1, 0, 1))
    lim = engine._WGRAD_GROUP_MAX_PIXELS
    assert small(1, 1, lim) and not small(1, 1, lim + 1)
