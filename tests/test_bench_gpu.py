"""GPU: a plain `bench.py` run (no --full) reports none of the --full legs; with --dump-outputs it writes what its last timed step
computed, two such runs with the same arguments dump bit-identical arrays, and the dumped loss is the loss of step 3 + W + N of the
bench's own workload (three set-up steps, W warm-up, N timed).  The runs start from the default environment (atomic reductions,
measuring tuner), not from this suite's ordered settings (tests/conftest.py): a dump run switches to ordered reductions with the
heuristic tiles itself, a plain run does not."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
FULL_ONLY = ("roofline", "peaks", "cpu_baseline", "forward_only", "extra", "gradient_exchange")
ARGS = ["--steps", "3", "--warmup", "1", "--batch", "4", "--imgsz", "256", "--no-stft"]


def _run(out_dir=None):
    env = dict(os.environ, SY11_DETERMINISTIC="0", SY11_TUNE="1", OMP_NUM_THREADS="2")
    dump = ["--dump-outputs", str(out_dir)] if out_dir else []
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", *ARGS, *dump], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.split("\n") if ln.strip()]
    assert len(lines) == 1, r.stdout[:2000]
    return json.loads(lines[0])


def _losses_of_the_bench_workload(n):
    """The bench's workload built by bench.make_workload as rank 0 builds it, in the ordered mode with the heuristic tiles: the dumped
    loss and model state after each of the first n steps."""
    import torch
    sys.path.insert(0, str(ROOT))
    import bench
    from sy11.utils.torch_utils import set_deterministic
    set_deterministic(True)
    a = bench.parse_args(ARGS)
    torch.manual_seed(1)
    tr, data, labels = bench.make_workload(a, torch.device("cuda", 0), 0, a.model, a.nc, a.dtype, not a.no_stft)
    losses, states = [], []
    for _ in range(n):
        out = tr.train_step({**data, **labels})
        arrays = bench.step_outputs(tr, out, "train")
        losses.append(bench.flat_sample("loss", arrays["loss"]))
        states.append(bench.flat_sample("model_state", arrays["model_state"]))      # BatchNorm running statistics move every step
    return losses, states


def test_dump_run_is_the_last_timed_step_and_repeats_it(tmp_path):
    out = _run(tmp_path / "a")
    assert out["steps"] == 3 and out["warmup"] == 1 and out["ms_per_step"] > 0 and out["value"] > 0
    assert out["unit"] == "spectrogram-images/s" and out["higher_is_better"] is True and out["dtype"] == "f16"
    assert all(out[k] is None for k in FULL_ONLY) and out["deterministic"] is True and out["tile_tuner"] is False
    names = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert names == ["ema_state.npy", "loss.npy", "loss_items.npy", "model_state.npy"]
    a = {Path(n).stem: np.load(tmp_path / "a" / n) for n in names}
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert a["loss"].shape == (1,) and a["loss"][0] > 0 and a["loss_items"].shape == (3,)
    _run(tmp_path / "b")
    for n, v in a.items():
        assert np.array_equal(v, np.load(tmp_path / "b" / f"{n}.npy")), n
    losses, states = _losses_of_the_bench_workload(3 + 1 + 3 + 1)         # set-up, warm-up, timed, and one step more
    assert np.array_equal(a["loss"], losses[6]) and np.array_equal(a["model_state"], states[6]), (a["loss"], losses)
    assert not np.array_equal(a["model_state"], states[5]) and not np.array_equal(a["model_state"], states[7])


def test_plain_run_keeps_the_default_reductions():
    out = _run()
    assert out["steps"] == 3 and out["ms_per_step"] > 0 and out["deterministic"] is False and out["tile_tuner"] is True
