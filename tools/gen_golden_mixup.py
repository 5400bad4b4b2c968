"""TEST INFRASTRUCTURE ONLY.  Golden vectors for MixUp in the training augmentation chain.

Runs the REFERENCE's own v8_transforms + Format (ultralytics/data/augment.py: Mosaic -> RandomPerspective -> MixUp ->
RandomHSV -> RandomFlip x2) with mixup > 0 on the in-memory dataset of oracle.gen_golden_augment, seeded the same way, and
stores per sample the final image / boxes / classes plus whether MixUp fired and with which r (taken by wrapping
MixUp._mix_transform here).  As for augment.npz the reference's cv2 pixel calls are bound to oracle.image_ref's
restatements (opencv-python is not installed); the blend itself is plain numpy in the reference, so that step is the
reference proper.  Needs the reference checkout (dev container only); tests read the .npz only.

Run:  python tools/gen_golden_mixup.py   ->  tests/golden/mixup.npz
"""
from __future__ import annotations

import random
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from oracle.gen_golden import OUT, import_reference  # noqa: E402
from oracle.gen_golden_augment import BASE, IMGSZ, bind_cv2, make_dataset_arrays  # noqa: E402

CONFIGS = {
    "mix_always": dict(mixup=1.0),
    "mix_half": dict(mixup=0.5, degrees=10.0, shear=2.0, flipud=0.5),
    "mix_nomosaic": dict(mixup=1.0, mosaic=0.0, degrees=5.0),
    "mix_halfmosaic": dict(mixup=0.5, mosaic=0.5),
}
HALF = ("mix_half", "mix_halfmosaic")
N_SAMPLES = 8


def main():
    import_reference()
    bind_cv2()
    from ultralytics.data import augment as A
    from ultralytics.utils import IterableSimpleNamespace
    from ultralytics.utils.instance import Instances

    imgs, boxes, clss = make_dataset_arrays()

    class FakeDataset:
        """The four things the transforms touch: buffer, len, get_image_and_label, data / use_keypoints."""
        data, use_keypoints = {}, False

        def __init__(self):
            self.buffer = list(range(len(imgs)))

        def __len__(self):
            return len(imgs)

        def get_image_and_label(self, i):
            h, w = imgs[i].shape[:2]
            return {"im_file": f"im{i}", "ori_shape": (h, w), "resized_shape": (h, w), "img": imgs[i].copy(), "cls": clss[i].copy(),
                    "ratio_pad": (1.0, 1.0), "instances": Instances(boxes[i].copy(), np.zeros((0, 1000, 2), np.float32), None, "xywh", True)}

    fired = []                                                   # one r per MixUp that actually mixed, in call order
    inner = A.MixUp._mix_transform

    def recording(self, labels):
        state = np.random.get_state()
        fired.append(float(np.random.beta(32.0, 32.0)))          # the draw _mix_transform is about to make ...
        np.random.set_state(state)                               # ... left for it to make
        return inner(self, labels)
    A.MixUp._mix_transform = recording

    store = {"n_images": np.asarray(len(imgs)), "configs": np.array(list(CONFIGS)), "n_samples": np.asarray(N_SAMPLES)}
    for i, (im, b, c) in enumerate(zip(imgs, boxes, clss)):
        store[f"in.{i}.img"], store[f"in.{i}.boxes"], store[f"in.{i}.cls"] = im, b, c
    for name, over in CONFIGS.items():
        hyp = IterableSimpleNamespace(**{**BASE, **over})
        ds = FakeDataset()
        tf = A.v8_transforms(ds, IMGSZ, hyp)
        tf.append(A.Format(bbox_format="xywh", normalize=True, batch_idx=True, bgr=hyp.bgr))
        random.seed(1234)
        np.random.seed(1234)
        n_mixed = 0
        for k in range(N_SAMPLES):
            del fired[:]
            out = tf(ds.get_image_and_label(k % len(imgs)))
            assert len(fired) <= 1
            store[f"{name}.{k}.img"] = out["img"].numpy()
            store[f"{name}.{k}.bboxes"] = out["bboxes"].numpy()
            store[f"{name}.{k}.cls"] = out["cls"].numpy()
            store[f"{name}.{k}.mixed"] = np.asarray(bool(fired))
            store[f"{name}.{k}.r"] = np.asarray(fired[0] if fired else np.nan, np.float64)
            n_mixed += bool(fired)
        store[f"{name}.rng_after"] = np.asarray([random.random(), np.random.uniform()])     # both streams consumed identically
        print(f"{name}: {n_mixed} of {N_SAMPLES} samples mixed")
        # a fixture that exercises nothing must not be written
        assert n_mixed >= 3, (name, n_mixed)
        assert name not in HALF or N_SAMPLES - n_mixed >= 2, (name, n_mixed)
    np.savez_compressed(OUT / "mixup.npz", **store)
    print("wrote", OUT / "mixup.npz", sum(v.nbytes for v in store.values()), "bytes raw")


if __name__ == "__main__":
    main()
