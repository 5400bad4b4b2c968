"""The dense 1x1 stride-1 layers of yolo11s and of the fusion variant (640x640, batch 64, f16) whose backward may take the fused input +
filter gradient (ops.conv2d_dgrad_wgrad_1x1, csrc/dwgrad1x1.hip), timed inside replayed hipGraphs of 10 calls:
  pair   ops.conv2d_dgrad then ops.conv2d_wgrad, tuner on (the first call measures the candidates) — each alone and back to back;
  fused  the one launch;
  floor  dy + x + dx once each at 5.5 TB/s.
python tools/dwgrad1x1_micro.py [--m-min M] [--wg G] [--bf16]     --m-min: smallest M = B*H*W the table covers (default 102 400: one
map size below the engine's threshold); --wg: force the fused launch to G workgroups per column block (default: occupancy API)."""
import sys
from pathlib import Path
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "spectrogram-yolov11_amd"))
sys.path.insert(0, str(ROOT / "tools"))
import torch
from sy11 import _lib, ops
from bn_sweep import timed
from conv_sweep import LAYERS

# 1x1 layers the fusion variant (yolo11_fusion_sand3_new.yaml, scale s) adds on the large maps: (H, W, C, N, count)
FUSION_EXTRA = [(80, 80, 256, 128, 1)]


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def main():
    m_min, wg = arg("--m-min", 102400), arg("--wg", 0)
    B, dt, reps = 64, torch.bfloat16 if "--bf16" in sys.argv else torch.float16, 10
    shapes = [(H, W, C, N, cnt) for (H, W, C, N, k, s, g, cnt) in LAYERS if k == 1 and s == 1 and g == 1] + FUSION_EXTRA
    shapes = [sh for sh in shapes if B * sh[0] * sh[1] >= m_min and sh[2] <= 256 and sh[3] <= 256 and sh[2] % 16 == 0 and sh[3] % 16 == 0]
    _lib.set_option("dwgrad_wg", wg)
    print(f"{len(shapes)} shapes, {sum(sh[4] for sh in shapes)} layers, M >= {m_min}, {str(dt)[6:]}, fused workgroups {'by occupancy' if wg == 0 else wg}")
    tot = {"pair": 0.0, "fused": 0.0, "floor": 0.0}
    for (H, W, C, N, cnt) in shapes:
        M = B * H * W
        x = torch.randn(B, H, W, C, device="cuda", dtype=dt)
        dy = torch.randn(B, H, W, N, device="cuda", dtype=dt)
        w = (torch.randn(N, 1, 1, C, device="cuda") / C ** 0.5).to(dt)
        wt = ops.weight_transpose(w)
        dx, dw = torch.empty_like(x), torch.zeros(N, 1, 1, C, device="cuda")
        dgrad = lambda: ops.conv2d_dgrad(dy, wt, dx, (B, H, W, N), 1, 1, 0)
        wgrad = lambda: ops.conv2d_wgrad(x, dy, dw, 1, 1, 0)
        t_d = timed(dgrad, reps, False)
        cfg_d = _lib.get_option("igemm_last_cfg")
        t_w = timed(wgrad, reps, False)
        cfg_w = _lib.get_option("wgrad_last_cfg")
        t_p = timed(lambda: (dgrad(), wgrad()), reps, False)
        t_f = timed(lambda: ops.conv2d_dgrad_wgrad_1x1(dy, x, wt, dx, dw), reps, False)
        assert _lib.get_option("wgrad_last_cfg") == _lib.CFG_DWGRAD_1X1
        floor = (M * N + 2 * M * C) * 2 / 5.5e12 * 1e3
        np_, cp, cb, blocks = ops.dgrad_wgrad_1x1_plan(C, N)
        for k, v in (("pair", t_p), ("fused", t_f), ("floor", floor)):
            tot[k] += v * cnt
        print(f"  {H:3d}x{W:<3d} {C:4d}->{N:<4d} x{cnt}  M={M:7d}  dgrad {t_d * 1e3:6.1f} (cfg {cfg_d:2d})  wgrad {t_w * 1e3:6.1f} (cfg {cfg_w:2d})  "
              f"pair {t_p * 1e3:6.1f} us  fused {t_f * 1e3:6.1f} us (tile {np_}x{cp}, {blocks} block{'s' if blocks > 1 else ''})  "
              f"floor {floor * 1e3:6.1f} us  fused/pair {t_f / t_p:4.2f}")
    print(f"TOTAL ms/step: pair {tot['pair']:.3f}  fused {tot['fused']:.3f}  floor {tot['floor']:.3f}")


if __name__ == "__main__":
    main()
