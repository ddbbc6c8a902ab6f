"""Golden vectors of boundary label relaxation: outputs of the reference's own RelaxedBoundaryLossToTensor
(transforms/transforms.py:75-124) on small label maps, packed to one word per pixel (bit c = plane c of its uint8 [C+1,H,W] output).

    python tests/golden/make_golden_relaxed.py <reference checkout>   ->  tests/golden/relaxed.npz

transforms.py imports scikit-image and torchvision at module level; neither is needed by the class (find_boundaries is reached only
with REDUCE_BORDER_ITER != -1, which stays at its default -1), so stubs stand in for them before the import.  scipy is the real one:
the (2 border + 1)^2 scipy.ndimage.shift calls at spline order 3 are what is recorded.

Label maps (C = 19, each <= 48 x 64): blocky regions; one-pixel-wide lines; 255 runs touching each edge; an all-255 map.  Each with
BORDER_WINDOW 0, 1, 2 and STRICTBORDERCLASS None and [5, 11].  One 5 x 7 case is stored as the raw multi-hot bytes as well.
The archive is written with fixed member dates: two runs give the same bytes."""
import io
import os
import sys
import types
import warnings
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import relaxed_common as rc  # noqa: E402

C = rc.GOLDEN_C


def label_maps():
    rng = np.random.default_rng(19)
    blocky = np.repeat(np.repeat(rng.integers(0, C, (8, 8)), 5, 0), 7, 1)[:40, :56].astype(np.uint8)
    blocky[12:20, 30:44] = 5
    blocky[25:33, 3:12] = 11
    blocky[18:22, 40:48] = 255
    lines = np.full((33, 47), 2, dtype=np.uint8)
    lines[:, 10] = 5            # vertical, strict class
    lines[16, :] = 7            # horizontal
    lines[5, 20:40] = 11        # strict class
    for i in range(20):
        lines[6 + i, 22 + i] = 13          # diagonal
    lines[30, 1:46:2] = 255     # dotted ignore
    edges = rng.integers(0, C, (24, 31)).astype(np.uint8)
    edges[0, 3:12] = 255
    edges[-1, 15:31] = 255
    edges[5:18, 0] = 255
    edges[0:9, -1] = 255
    all255 = np.full((16, 20), 255, dtype=np.uint8)
    tiny = np.array([[0, 0, 1, 1, 255, 2, 2],
                     [0, 5, 5, 1, 1, 2, 2],
                     [3, 3, 5, 11, 11, 2, 18],
                     [3, 3, 3, 11, 255, 255, 18],
                     [4, 4, 3, 3, 17, 17, 18]], dtype=np.uint8)
    return {"blocky": blocky, "lines": lines, "edges": edges, "all255": all255, "tiny": tiny}


def import_reference_transform(ref):
    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules.setdefault(name, m)
        return sys.modules[name]

    def absent(*a, **k):
        raise RuntimeError("a stubbed scikit-image / torchvision function was called")
    sk = stub("skimage")
    sk.filters = stub("skimage.filters", gaussian=absent)
    sk.restoration = stub("skimage.restoration", denoise_bilateral=absent)
    sk.segmentation = stub("skimage.segmentation", find_boundaries=absent)
    sk.util = stub("skimage.util", random_noise=absent)
    tv = stub("torchvision")
    tv.transforms = stub("torchvision.transforms")
    sys.path.insert(0, ref)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # scipy.ndimage.interpolation is a deprecated namespace
        from transforms import transforms as ref_tr
    from config import cfg
    return ref_tr, cfg


def pack(onehot):
    """uint8 [C+1,H,W] of 0 / 1 -> int32 [H,W]."""
    assert onehot.dtype == np.uint8 and onehot.shape[0] == C + 1 and onehot.max() <= 1
    bits = np.arange(C + 1, dtype=np.uint32).reshape(-1, 1, 1)
    return (onehot.astype(np.uint32) << bits).sum(0).astype(np.uint32).view(np.int32)


def save_npz(path, arrays):
    """np.savez_compressed with fixed member dates and a fixed member order."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref_tr, cfg = import_reference_transform(sys.argv[1])
    assert cfg.REDUCE_BORDER_ITER == -1
    tr = ref_tr.RelaxedBoundaryLossToTensor(255, C)
    maps = label_maps()
    out = {}
    for name in rc.GOLDEN_MAPS + ("tiny",):
        out[name + "_lab"] = maps[name]
        for border in rc.GOLDEN_BORDERS:
            for sname, strict in rc.GOLDEN_STRICT.items():
                cfg.BORDER_WINDOW, cfg.STRICTBORDERCLASS = border, strict
                onehot = tr(maps[name].copy()).numpy()
                out[rc.golden_key(name, border, sname)] = pack(onehot)
                if name == "tiny" and border == 1 and strict is None:
                    out["tiny_multihot"] = onehot
    path = os.path.join(ROOT, "tests", "golden", "relaxed.npz")
    save_npz(path, out)
    print("written", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
