"""Golden records of the centroid crop: the reference's own RandomHorizontalFlip, ColorJitter, RandomSizeAndCrop(..., centroid=), Resize
and RandomGaussianBlur (dataloaders.py), run in transform_tr's order (main.py:410-419) on tiny seeded pairs.

    python tests/golden/make_golden_class_uniform.py <reference checkout>   ->  tests/golden/class_uniform.npz  (~40 KB)

The cases are tests/class_uniform_common.py::golden_templates (four source sizes, crop 16, centroids at 0, at w - 1 and inside).  For
every case python's `random` and numpy's global stream are seeded with the same number; RandomSizeAndCrop is given the centroid
mirrored (w - 1 - c_x) when the flip fired -- this build's rule, the reference's transform_tr hands no centroid on -- and, while the
crop runs, Image.resize, Image.crop and random.randint are wrapped to record what the reference did: the scaled size, the padded size
the crop was taken from (hence the padding), the crop origin, and how many randint calls were made.  One random.random() after the
pipeline records the stream position.  Stored: the records, the seeds, the cropped label and image bytes, the source pairs.

A seed whose ColorJitter draws a negative hue factor is passed over: `np.uint8(hue_factor * 255)` of dataloaders.py:589 raises under
numpy 2 (the wrap-around of the numpy 1.x the reference pins is covered by tests/golden/input_pipeline.npz).  The next seed that
runs is taken, and the coverage the CPU test asks for (early return, padding in one axis and in both, both flips) is asserted here."""
import os
import random
import sys
import types
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import class_uniform_common as cu  # noqa: E402
from make_golden_relaxed import save_npz  # noqa: E402


def import_reference_dataloaders(ref):
    """dataloaders.py imports torchvision.transforms for Lambda and Compose only: two one-line stand-ins when it is not installed."""
    class Lambda:
        def __init__(self, fn):
            self.fn = fn

        def __call__(self, x):
            return self.fn(x)

    class Compose:
        def __init__(self, transforms):
            self.transforms = transforms

        def __call__(self, x):
            for t in self.transforms:
                x = t(x)
            return x
    try:
        import torchvision.transforms  # noqa: F401
    except ImportError:
        tv = types.ModuleType("torchvision")
        tv.transforms = types.ModuleType("torchvision.transforms")
        tv.transforms.Lambda, tv.transforms.Compose = Lambda, Compose
        sys.modules["torchvision"], sys.modules["torchvision.transforms"] = tv, tv.transforms
    sys.path.insert(0, ref)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        import dataloaders
    return dataloaders


def run_case(dl, Image, img, lab, seed, smin, smax, centroid):
    """-> (record dict, cropped image uint8 [T,T,3], cropped label uint8 [T,T]); raises what the reference raises."""
    h, w = lab.shape
    T = cu.GOLDEN_CROP
    random.seed(seed)
    np.random.seed(seed)
    state = random.getstate()
    flip = random.random() < 0.5                 # what RandomHorizontalFlip is about to draw
    random.setstate(state)
    sample = {"image": Image.fromarray(img), "label": Image.fromarray(lab)}
    sample = dl.RandomHorizontalFlip()(sample)
    sample = dl.ColorJitter(**cu.JITTER)(sample)
    given = (w - 1 - centroid[0] if flip else centroid[0], centroid[1])
    log = {"resize": [], "crop": [], "randint": 0}
    real_resize, real_crop, real_randint = Image.Image.resize, Image.Image.crop, random.randint

    def resize(self, size, *a, **k):
        log["resize"].append(tuple(size))
        return real_resize(self, size, *a, **k)

    def crop(self, box=None):
        log["crop"].append((self.size, tuple(box)))
        return real_crop(self, box)

    def randint(a, b):
        log["randint"] += 1
        return real_randint(a, b)
    Image.Image.resize, Image.Image.crop, random.randint = resize, crop, randint
    try:
        sample = dl.RandomSizeAndCrop(T, False, scale_min=smin, scale_max=smax, ignore_index=255)(sample, centroid=given)
    finally:
        Image.Image.resize, Image.Image.crop, random.randint = real_resize, real_crop, real_randint
    sw, sh = log["resize"][0]
    if log["crop"]:
        (W2, H2), (x1, y1, x2, y2) = log["crop"][0]
        assert (x2 - x1, y2 - y1) == (T, T) and (W2 - sw) % 2 == 0 and (H2 - sh) % 2 == 0
        pad = ((W2 - sw) // 2, (H2 - sh) // 2)
    else:                                        # the early return of RandomCrop: nothing padded, nothing cropped
        assert (sw, sh) == (T, T) and log["randint"] == 0
        pad, x1, y1 = (0, 0), 0, 0
    sample = dl.Resize(T, T)(sample)
    sample = dl.RandomGaussianBlur()(sample)
    probe = random.random()
    rec = dict(flip=int(flip), sw=sw, sh=sh, pad_w=pad[0], pad_h=pad[1], x1=x1, y1=y1, nrandint=log["randint"], probe=probe)
    out_img, out_lab = np.array(sample["image"], dtype=np.uint8), np.array(sample["label"], dtype=np.uint8)
    assert out_img.shape == (T, T, 3) and out_lab.shape == (T, T)
    return rec, out_img, out_lab


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    from PIL import Image
    dl = import_reference_dataloaders(sys.argv[1])
    templates = cu.golden_templates()
    out = {}
    for si in range(len(cu.GOLDEN_SIZES)):
        out["src_img_%d" % si], out["src_lab_%d" % si] = cu.golden_source(si)
    keys = ("flip", "sw", "sh", "pad_w", "pad_h", "x1", "y1", "nrandint")
    recs, probes, seeds, imgs, labs, params = [], [], [], [], [], []
    seed = 100
    for si, smin, smax, cen in templates:
        img, lab = out["src_img_%d" % si], out["src_lab_%d" % si]
        while True:
            seed += 1
            try:
                rec, oi, ol = run_case(dl, Image, img, lab, seed, smin, smax, cen)
                break
            except OverflowError:                # a negative hue factor under numpy 2
                continue
        recs.append([rec[k] for k in keys])
        probes.append(rec["probe"])
        seeds.append(seed)
        imgs.append(oi)
        labs.append(ol)
        params.append([si, cen[0], cen[1]])
    rec = np.array(recs, dtype=np.int32)
    T = cu.GOLDEN_CROP
    early = (rec[:, 7] == 0)
    padded_x, padded_y = rec[:, 3] > 0, rec[:, 4] > 0
    assert early.any() and (padded_x & padded_y).any() and (padded_x ^ padded_y).any() and set(rec[:, 0].tolist()) == {0, 1}
    assert (~early & (rec[:, 7] == 2)).sum() == (~early).sum()          # two randint calls wherever the crop ran
    out.update(records=rec, record_keys=np.array(keys), probes=np.array(probes, dtype=np.float64), seeds=np.array(seeds, dtype=np.int64),
               params=np.array(params, dtype=np.int32), scales=np.array([[t[1], t[2]] for t in templates], dtype=np.float64),
               out_img=np.stack(imgs), out_lab=np.stack(labs))
    path = cu.GOLDEN
    save_npz(path, out)
    print("written", path, os.path.getsize(path), "bytes;", int(early.sum()), "early returns,", int((padded_x & padded_y).sum()),
          "padded in both axes,", int((padded_x ^ padded_y).sum()), "in one,", int(rec[:, 0].sum()), "flipped, T =", T)


if __name__ == "__main__":
    main()
