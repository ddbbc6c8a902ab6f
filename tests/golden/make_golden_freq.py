"""Golden vectors of the frequency filters: outputs of the reference's own HPF, LPF and PHOT classes (dataloaders.py:24-79)
on small seeded images.

    python tests/golden/make_golden_freq.py <reference checkout>   ->  tests/golden/freq_filters.npz

The three classes use only numpy and PIL; dataloaders.py imports torchvision at module level (for ColorJitter's Lambda), so a
stub stands in for it before the import.  Stored per case: the uint8 [H,W,3] input and the float32 [H,W,3] outputs exactly as
the classes return them (before ToTensor).  Cases: an even size, an odd size, a size below the 33x33 band box, and a grey image
(R = G = B: every channel-frequency 1 and 2 bin is exactly zero, so PHOT returns NaN everywhere)."""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "tests", "golden", "freq_filters.npz")

# name -> (H, W, grey)
CASES = {"even": (32, 40, False), "odd": (45, 75, False), "tiny": (24, 20, False), "grey": (20, 30, True)}


def case_image(name):
    H, W, grey = CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    img = rng.integers(0, 256, (H, W, 1 if grey else 3), dtype=np.uint8)
    return np.ascontiguousarray(np.repeat(img, 3, -1) if grey else img)


def import_reference_dataloaders(ref):
    tv = types.ModuleType("torchvision")
    tr = types.ModuleType("torchvision.transforms")
    tr.Lambda = lambda f: f
    tr.Compose = lambda ts: ts
    tv.transforms = tr
    sys.modules.setdefault("torchvision", tv)
    sys.modules.setdefault("torchvision.transforms", tr)
    sys.path.insert(0, ref)
    import dataloaders
    return dataloaders


def main():
    import warnings
    from PIL import Image
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    dl = import_reference_dataloaders(sys.argv[1])
    out = {}
    for name in CASES:
        img = case_image(name)
        out[name + "_img"] = img
        for filt in ("HPF", "LPF", "PHOT"):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")          # ComplexWarning of astype(float32); 0/0 of a zero bin
                y = getattr(dl, filt)()({"image": Image.fromarray(img), "label": None})["image"]
            assert y.dtype == np.float32 and y.shape == img.shape, (filt, y.dtype, y.shape)
            out["%s_%s" % (name, filt.lower())] = y
    np.savez_compressed(OUT, **out)
    print("written", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
