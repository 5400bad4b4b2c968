"""`bench.py --dump-outputs DIR`: the sampling and writing helpers on the host (what the last timed step computed, as float32 .npy files
that two builds can compare position for position; at most 64 MB in all)."""
import importlib
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]


def _bench():
    sys.path.insert(0, str(ROOT))
    return importlib.import_module("bench")


def test_small_outputs_are_dumped_whole_in_float32():
    bench = _bench()
    a, b = torch.arange(6, dtype=torch.float64).view(2, 3), torch.tensor([7.5], dtype=torch.float16)
    got = bench.flat_sample("x", [a, b])
    assert got.dtype == np.float32 and got.tolist() == [0, 1, 2, 3, 4, 5, 7.5]


def test_large_outputs_are_a_fixed_seeded_sample():
    bench = _bench()
    t = torch.arange(10_000, dtype=torch.float32)
    s1, s2 = bench.flat_sample("x", [t], limit=100), bench.flat_sample("x", [t.clone()], limit=100)
    assert s1.shape == (100,) and np.array_equal(s1, s2)                     # same name and length: same positions
    assert np.all(np.diff(s1) >= 0) and s1.min() >= 0 and s1.max() < 10_000   # positions sorted, values are the elements there
    assert not np.array_equal(s1, bench.flat_sample("y", [t], limit=100))


def test_dump_writes_one_npy_per_name_and_refuses_more_than_the_limit(tmp_path, monkeypatch):
    bench = _bench()
    n = bench.dump_outputs(tmp_path / "out", {"loss": [torch.tensor(2.0)], "items": [torch.ones(3)]})
    assert n == 16 and sorted(p.name for p in (tmp_path / "out").iterdir()) == ["items.npy", "loss.npy"]
    assert np.load(tmp_path / "out" / "loss.npy").tolist() == [2.0]
    monkeypatch.setattr(bench, "DUMP_BYTES", 8)
    with pytest.raises(ValueError):
        bench.dump_outputs(tmp_path / "big", {"items": [torch.ones(3)]})


def test_step_outputs_of_a_train_step_hold_the_returned_loss_and_the_updated_state():
    bench = _bench()
    model, ema = torch.nn.BatchNorm2d(2), torch.nn.BatchNorm2d(2)
    tr = SimpleNamespace(model=model, ema=SimpleNamespace(ema=ema))
    out = bench.step_outputs(tr, (torch.tensor(3.0), torch.ones(3)), "train")
    assert sorted(out) == ["ema_state", "loss", "loss_items", "model_state"]
    assert len(out["model_state"]) == 4                                       # weight, bias, running mean / var; the int counter is left out
    assert bench.step_outputs(tr, [torch.ones(2), torch.zeros(3)], "fwd").keys() == {"head_outputs"}


def test_full_is_off_by_default_and_dump_outputs_takes_a_directory(monkeypatch):
    """The parser as a plain run sees it; the parent of `--gpus N` hands every option on to its ranks unchanged."""
    bench = _bench()
    a = bench.parse_args(["--gpus", "1", "--steps", "4", "--warmup", "2"])
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 4, 2)
    a = bench.parse_args(["--full", "--dump-outputs", "out"])
    assert a.full and a.dump_outputs == "out"
    from sy11.engine import ddp
    seen = {}
    monkeypatch.setattr(ddp, "launch", lambda args, n, env=None, timeout=None: seen.setdefault("args", list(args)) and [0] * n)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    argv = ["bench.py", "--gpus", "2", "--steps", "3", "--warmup", "1", "--dump-outputs", "d", "--full"]
    monkeypatch.setattr(sys, "argv", argv)
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 0 and seen["args"][1:] == argv[1:]
