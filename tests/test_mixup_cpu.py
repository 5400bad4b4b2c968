"""CPU: MixUp on the host side.  The product's MixUp runs lazily (a partner recipe and r are recorded, no pixel is rendered, so no
GPU is needed) on the generator's in-memory dataset under the same seeds: boxes, classes and both consumed RNG streams must equal
what the REFERENCE's own v8_transforms(mixup > 0) produced (tests/golden/mixup.npz), a sample carries a partner exactly when the
reference mixed it, with the recorded r, and the recorded recipe executed in numpy gives the reference's pixels.  Plus the
DeviceImage folding rules, the worker-process contract (a worker ships a recipe, never pixels) and the front door."""
import ctypes as C
import math
import pickle
import random
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests._golden import load
from tests._mixup_util import BASE, CONFIGS, IMGSZ, N_SAMPLES, FakeDataset, oracle_render, run_pipeline


def test_fixture_exercises_both_kinds():
    gold = load("mixup.npz")
    assert list(gold["configs"]) == list(CONFIGS) and int(gold["n_samples"]) == N_SAMPLES == 8
    mixed = {n: sum(bool(gold[f"{n}.{k}.mixed"]) for k in range(N_SAMPLES)) for n in CONFIGS}
    assert mixed == {"mix_always": 8, "mix_half": 3, "mix_nomosaic": 8, "mix_halfmosaic": 5}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_labels_partner_and_rng_streams_match_reference(name):
    from sy11.data.augment import DeviceImage
    gold = load("mixup.npz")
    n = 0
    # lazy source images (as in a loader worker): the LetterBox of the non-mosaic samples is recorded too, nothing launches
    for k, out in run_pipeline(gold, name, "cpu", lazy=True):
        if k is None:
            assert np.array_equal(out, gold[f"{name}.rng_after"])              # same number of draws from both streams
            continue
        assert np.array_equal(out["bboxes"].numpy(), gold[f"{name}.{k}.bboxes"])
        assert np.array_equal(out["cls"].numpy(), gold[f"{name}.{k}.cls"])
        di = out["img"]
        assert isinstance(di, DeviceImage) and di.shape == (IMGSZ, IMGSZ, 3)
        assert (di.partner is not None) == bool(gold[f"{name}.{k}.mixed"])
        if di.partner is not None:
            assert di.mix_r == float(gold[f"{name}.{k}.r"])                    # the very double the reference drew
            p = di.partner
            assert p.out_hw == di.out_hw and p.lut is None and not p.flip_ud and not p.flip_lr and p.partner is None
            assert 1 <= len(p.tiles) <= 4
        else:
            assert di.mix_r is None and math.isnan(float(gold[f"{name}.{k}.r"]))
        assert di.lut is not None                                              # HSV recorded after the mix folded into the recipe
        n += 1
    assert n == N_SAMPLES


def test_recipes_reproduce_golden_pixels_through_the_oracle():
    """Both sides of every mix_half recipe through the oracle's numpy functions, blended with the reference's numpy expression."""
    gold = load("mixup.npz")
    seen = set()
    for k, out in run_pipeline(gold, "mix_half", "cpu"):
        if k is None:
            break
        seen.add(out["img"].partner is not None)
        assert np.array_equal(oracle_render(out["img"]), gold[f"mix_half.{k}.img"])
    assert seen == {True, False}


def test_device_image_mix_rules():
    """What folds into the one launch and what has to become pixels first (a LazyImage "render" node on CPU tensors would need the
    GPU, so the flattening cases are observed through LazyImage tiles, which defer the render as a worker process does)."""
    from sy11.data.augment import DeviceImage
    from sy11.data.recipe import LazyImage, file_image
    M = np.array([[1, 0, 2], [0, 1, 3]], np.float32)

    def fresh(i=0, hw=(8, 6)):
        return DeviceImage.wrap(file_image(i, hw))

    a, b = fresh(0).warp(M, (10, 12)), fresh(1).warp(M, (10, 12))
    assert a.mix(b, 0.25) is a and a.partner is not None and a.mix_r == 0.25 and a.pending and a.plain_tensor() is None
    assert a.partner is not b and a.partner.minv == b.minv and a.minv is not None          # two geometry recipes: folded, nothing rendered
    assert a.tiles[0][0].op == ("file", 0) and a.partner.tiles[0][0].op == ("file", 1) and a.has_lazy()
    assert [t[0].op for t in a.source_tiles()] == [("file", 0), ("file", 1)]
    # hsv and flips after a mix fold
    lut = tuple(np.arange(256, dtype=np.uint8) for _ in range(3))
    a.hsv(lut).flip(ud=True).flip(lr=True)
    assert a.partner is not None and a.lut is not None and a.flip_ud and a.flip_lr and a.tiles[0][0].op == ("file", 0)
    # frozen / pickled copies keep the partner; resolved() turns both sides' nodes into tensors
    c = pickle.loads(pickle.dumps(a.frozen()))
    assert c.partner is not None and c.mix_r == 0.25 and c.partner.tiles[0][0].op == ("file", 1)
    res = a.resolved(lambda node: torch.zeros(node.shape, dtype=torch.uint8))
    assert not res.has_lazy() and torch.is_tensor(res.tiles[0][0]) and torch.is_tensor(res.partner.tiles[0][0]) and a.has_lazy()
    # a warp after a mix flattens: the blend comes before the second warp
    a.warp(M, (10, 12))
    assert a.partner is None and a.mix_r is None and a.lut is None and len(a.tiles) == 1
    node = a.tiles[0][0]
    assert isinstance(node, LazyImage) and node.op[0] == "render" and node.op[1].partner is not None and node.op[1].mix_r == 0.25
    # a side with HSV / flips pending, or already carrying a partner, is flattened first
    s, o = fresh(0, (12, 10)).hsv(lut), fresh(1, (12, 10)).flip(lr=True)
    s.mix(o, 0.5)
    assert s.lut is None and s.tiles[0][0].op[0] == "render" and s.tiles[0][0].op[1].lut is not None
    assert s.partner.tiles[0][0].op[0] == "render" and s.partner.tiles[0][0].op[1].flip_lr and not s.partner.flip_lr
    assert o.flip_lr and o.tiles[0][0].op == ("file", 1)                                   # the caller's partner object is left alone
    s2 = fresh(2, (12, 10))
    s2.mix(s, 0.75)                                                                        # partner already mixed: its blend renders first
    assert s2.partner.partner is None and s2.partner.tiles[0][0].op[0] == "render" and s2.partner.tiles[0][0].op[1].mix_r == 0.5
    s.mix(fresh(3, (12, 10)), 0.1)                                                         # self already mixed: the same
    assert s.mix_r == 0.1 and s.tiles[0][0].op[0] == "render" and s.tiles[0][0].op[1].mix_r == 0.5
    # sizes must agree, r must be a weight
    with pytest.raises(ValueError):
        fresh(0, (8, 6)).mix(fresh(1, (8, 7)), 0.5)
    for bad in (1.5, -0.1, float("nan")):
        with pytest.raises(ValueError):
            fresh(0).mix(fresh(1), bad)
    # plain tensors: a mixed recipe is no longer "one untouched image"
    t = torch.zeros((8, 6, 3), dtype=torch.uint8)
    d = DeviceImage.wrap(t)
    assert d.plain_tensor() is t
    d.mix(DeviceImage.wrap(torch.ones((8, 6, 3), dtype=torch.uint8)), 0.5)
    assert d.plain_tensor() is None and d.pending


def test_mixup_at_p0_draws_one_number_and_changes_nothing():
    from sy11.data.augment import MixUp

    class Never:
        def __len__(self):
            raise AssertionError("p = 0 must not look at the dataset")
    m = MixUp(Never(), pre_transform=None, p=0.0)
    random.seed(7)
    labels = {"img": object()}
    assert m(labels) is labels
    after = random.random()
    random.seed(7)
    random.uniform(0, 1)
    assert after == random.random()


def test_front_door_accepts_mixup_and_still_refuses_copy_paste():
    from sy11.data.augment import MixUp, v8_transforms
    gold = load("mixup.npz")
    tf = v8_transforms(FakeDataset(gold, "cpu"), IMGSZ, SimpleNamespace(**{**BASE, "mixup": 0.3}))
    mix = tf.transforms[1]
    assert isinstance(mix, MixUp) and mix.p == 0.3 and mix.pre_transform is tf.transforms[0]   # the SAME geometry Compose as the sample's
    with pytest.raises(NotImplementedError):
        v8_transforms(FakeDataset(gold, "cpu"), IMGSZ, SimpleNamespace(**{**BASE, "copy_paste": 0.1}))


def test_dataset_zeroes_mixup_for_rect_and_close_mosaic(tmp_path):
    from sy11.data.augment import MixUp
    from sy11.data.dataset import DEFAULT_HYP, YOLODataset
    from tests.test_loader_workers_cpu import make_dataset as _md  # noqa: F401  (the dataset files)
    _md(tmp_path)
    hyp = SimpleNamespace(**{**DEFAULT_HYP, "mixup": 0.4})
    ds = YOLODataset(str(tmp_path / "images"), imgsz=64, augment=True, batch_size=4, data={"nc": 2}, device="cpu", hyp=hyp)
    assert [t.p for t in ds.transforms.transforms if isinstance(t, MixUp)] == [0.4]
    ds.close_mosaic(ds.hyp)
    assert [t.p for t in ds.transforms.transforms if isinstance(t, MixUp)] == [0.0]
    rect = YOLODataset(str(tmp_path / "images"), imgsz=64, augment=True, rect=True, batch_size=4, stride=8, data={"nc": 2}, device="cpu",
                       hyp=SimpleNamespace(**{**DEFAULT_HYP, "mixup": 0.4}))
    assert [t.p for t in rect.transforms.transforms if isinstance(t, MixUp)] == [0.0]


def _node_sig(node):
    return node.op if node.op[0] == "file" else (node.op[0], node.op[1].op, *node.op[2:])


def _tiles_sig(tiles):
    return [(_node_sig(t[0]), t[0].shape, *t[1:]) for t in tiles]


def recipe_signature(sample):
    """tests/test_loader_workers_cpu.py's signature, extended by the partner's tiles, map and r."""
    img = sample["img"]
    p = img.partner
    partner = None if p is None else (_tiles_sig(p.tiles), p.canvas_hw, p.out_hw, None if p.minv is None else tuple(p.minv), img.mix_r)
    return (_tiles_sig(img.tiles), img.canvas_hw, img.out_hw, None if img.minv is None else tuple(img.minv),
            None if img.lut is None else img.lut.tobytes(), img.flip_ud, img.flip_lr, img.final_reverse_c, partner,
            sample["bboxes"].numpy().tobytes(), sample["cls"].numpy().tobytes())


def test_one_worker_with_mixup_reproduces_the_in_process_recipes_and_close_mosaic_reaches_it(tmp_path):
    from sy11.data.dataset import DEFAULT_HYP, WorkerLoader, YOLODataset
    from sy11.data.recipe import LazyImage
    from tests.test_loader_workers_cpu import make_dataset
    make_dataset(tmp_path)
    ds = YOLODataset(str(tmp_path / "images"), imgsz=64, augment=True, batch_size=4, data={"nc": 2}, device="cpu",
                     hyp=SimpleNamespace(**{**DEFAULT_HYP, "mixup": 1.0}))
    dl = WorkerLoader(ds, 4, procs=1, shuffle=False, seed=3)
    try:
        it = dl._recipes()
        got = [next(it) for _ in range(4)]
        twin = pickle.loads(pickle.dumps(ds))
        twin.recipe_mode = True
        seed = 1000003 * (3 + 1)
        random.seed(seed); np.random.seed(seed % 2**32); torch.manual_seed(seed)
        want = [[twin[i] for i in range(k, k + 4)] for k in (0, 4, 8)] + [[twin[i] for i in range(0, 4)]]
        for a, b in zip(got, want):
            assert [recipe_signature(x) for x in a] == [recipe_signature(x) for x in b]
        for batch in got:
            for s in batch:
                img = s["img"]
                assert img.partner is not None and 0.0 < img.mix_r < 1.0 and img.lut is not None
                assert all(isinstance(t[0], LazyImage) for t in img.source_tiles()) and len(img.partner.tiles) >= 1
                assert len(s["bboxes"]) == len(s["cls"])
        assert len(pickle.dumps(got[0][0])) < 16000                  # two recipes, still not an image
        with pytest.raises(RuntimeError):
            got[0][0]["img"].render(chw=True)                        # a worker never renders: pixels only after resolved()
        ds.close_mosaic(ds.hyp)                                      # mixup off in the worker too, stale batches dropped
        it = dl._recipes()
        batch = next(it)
        assert all(s["img"].partner is None and len(s["img"].tiles) == 1 for s in batch)
    finally:
        dl.close()
    assert all(not p.is_alive() for p in dl.workers)


def test_mixup_warp_rejects_bad_weights_before_any_launch():
    """The C entry's own checks return the library's error code before anything is launched, so they run without a GPU: pointers
    are never dereferenced on these paths (host arrays stand in for the device images)."""
    from sy11 import _lib
    lib = _lib.load()
    src = (C.c_void_p * 1)(0x1000)
    geom = (C.c_int32 * 8)(8, 8, 0, 0, 8, 8, 0, 0)
    dst = C.c_void_p(0x2000)

    def call(r, s, geom_b=geom, n_b=1, canvas_b=8):
        return lib.sy11_image_mixup_warp(_lib.U8, 1, src, geom, 8, 8, None, n_b, src, geom_b, canvas_b, canvas_b, None, r, s, 8, 8, None,
                                         0, 0, 114, 0, 1, dst, None)
    for r, s in ((1.5, -0.5), (float("nan"), 0.5), (0.5, float("nan")), (float("inf"), 0.0), (-0.25, 1.25)):
        assert call(r, s) == -1 and b"blend weights" in lib.sy11_last_error()
    assert call(0.5, 0.5, n_b=5) == -1 and b"partner" in lib.sy11_last_error() and b"tiles" in lib.sy11_last_error()
    assert call(0.5, 0.5, canvas_b=16) == -1 and b"partner" in lib.sy11_last_error()           # un-warped partner of another size
    outside = (C.c_int32 * 8)(8, 8, 0, 0, 9, 8, 0, 0)
    assert call(0.5, 0.5, geom_b=outside) == -1 and b"partner" in lib.sy11_last_error()
