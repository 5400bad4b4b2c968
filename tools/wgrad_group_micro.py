"""The small-map dense filter gradients of yolo11s (640x640, batch 64, f16; output map <= 40x40, M <= 102 400), with their
multiplicities, timed inside replayed hipGraphs in two ways:
  (a) one launch per layer with the tuner on, as `conv_sweep.py wgrad` runs them;
  (b) as the engine issues them: the layers it calls small (M <= --group-m) in grouped launches (ops.conv2d_wgrad_group), in backward
      order, 32 per launch; the rest one launch per layer.
Prints a per-launch table and both totals.   python tools/wgrad_group_micro.py [--target G] [--group-m M] [--m-max M] [--per-group N] [-v]
--target: workgroups per grouped launch (default: the engine's, three per CU); --group-m: largest M that joins a group (default: the
engine's); --m-max: largest M the table covers."""
import sys
from pathlib import Path
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "spectrogram-yolov11_amd"))
sys.path.insert(0, str(ROOT / "tools"))
import torch
from sy11 import _lib, ops
from bn_sweep import timed
from conv_sweep import LAYERS


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def main():
    from sy11 import engine
    target = arg("--target", engine._wgrad_group_target("cuda"))          # the engine's: three workgroups per CU
    group_m = arg("--group-m", engine._WGRAD_GROUP_MAX_PIXELS)            # the engine's "small": larger layers stay one launch each in (b)
    m_max, per_group, verbose = arg("--m-max", 102400), arg("--per-group", _lib.WGRAD_GROUP_MAX), "-v" in sys.argv
    B, dt, reps = 64, torch.float16, 10
    layers = []
    for (H, W, C, N, k, s, g, cnt) in LAYERS:
        OH, OW = ops.conv_out_hw(H, W, k, s, k // 2)
        if g == 1 and B * OH * OW <= m_max:
            layers.append((H, W, C, N, k, s, cnt, OH, OW))
    print(f"{len(layers)} shapes, {sum(l[6] for l in layers)} layers, M <= {m_max}")
    probs, total_a, rows = [], 0.0, []
    for (H, W, C, N, k, s, cnt, OH, OW) in layers:
        x = torch.randn(B, H, W, C, device="cuda", dtype=dt)
        dy = torch.randn(B, OH, OW, N, device="cuda", dtype=dt)
        dw = torch.zeros(N, k, k, C, device="cuda")
        ms = timed(lambda: ops.conv2d_wgrad(x, dy, dw, k, s, k // 2), reps, False)      # the first call measures the candidates
        cfg = _lib.get_option("wgrad_last_cfg")
        total_a += ms * cnt
        rows.append(f"  {H:3d}x{W:<3d} {C:4d}->{N:<4d} k{k} s{s} x{cnt}  M={B * OH * OW:6d}  cfg {cfg:2d}  {ms * 1e3:7.1f} us")
        probs += [(x, dy, torch.zeros_like(dw), k, s, k // 2, 1) for _ in range(cnt)]
    probs.reverse()                                                                     # the backward pass meets the last layer first
    one_by_one = timed(lambda: [ops.conv2d_wgrad(*p[:6]) for p in probs], 3, False)
    print("(a) per layer, tuner on:")
    print("\n".join(rows))
    total_b, rows = 0.0, []
    pixels = lambda p: p[1].shape[0] * p[1].shape[1] * p[1].shape[2]
    large = [p for p in probs if pixels(p) > group_m]
    probs = [p for p in probs if pixels(p) <= group_m]
    if large:
        ms = timed(lambda: [ops.conv2d_wgrad(*p[:6]) for p in large], 3, False)
        total_b += ms
        rows.append(f"  {len(large)} layers with M > {group_m}: one launch each  {ms * 1e3:7.1f} us")
    groups = [probs[i:i + per_group] for i in range(0, len(probs), per_group)]
    for i, grp in enumerate(groups):
        ms = timed(lambda: ops.conv2d_wgrad_group(grp, target), reps, False)
        assert _lib.get_option("wgrad_last_cfg") == _lib.CFG_WGRAD_GROUP
        M, N, K = ([p[1].shape[0] * p[1].shape[1] * p[1].shape[2] for p in grp], [p[1].shape[3] for p in grp],
                   [p[3] * p[3] * p[0].shape[3] for p in grp])
        pps, start = ops.wgrad_group_plan(M, N, K, target)
        total_b += ms
        rows.append(f"  group {i}: {len(grp):2d} problems, {start[-1]:4d} workgroups, splits {min(-(-m // q) for m, q in zip(M, pps))}.."
                    f"{max(-(-m // q) for m, q in zip(M, pps))}  {ms * 1e3:7.1f} us")
        if verbose:
            rows += [f"      M={m:6d} N={n:4d} K={kk:5d} pix_per_split {q:6d} workgroups {b - a}" for m, n, kk, q, a, b in zip(M, N, K, pps, start, start[1:])]
    all_groups = timed(lambda: [ops.conv2d_wgrad_group(grp, target) for grp in groups], 3, False)
    print(f"(b) grouped, target {target}:")
    print("\n".join(rows))
    print(f"TOTAL ms/step: per layer {total_a:.3f} (sum of the table), {one_by_one:.3f} (all layers back to back in one graph);  "
          f"grouped {total_b:.3f} (sum of the table), {all_groups:.3f} (all groups back to back in one graph)")


if __name__ == "__main__":
    main()
