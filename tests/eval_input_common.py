"""Numpy restatement of the evaluation input path (mrfp_amd/input_pipeline.py: LabelEncoder, EvalTransform,
ResizeHeightCenterCropPad), the PIL form of the same steps in the reference's order, the deterministic samples and the cases
that tests/test_eval_input_cpu.py, tests/test_eval_input_gpu.py and tests/golden/make_golden_eval_input.py share.

The samples come from integer arithmetic alone (no random generator whose stream could differ between numpy versions): the
fixture tests/golden/eval_input.npz records only what PIL made of them."""
import os

import numpy as np

from oracle import input_oracle as io

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "eval_input.npz")

DATASETS = ("CityscapesSegmentation", "RainyCityscapesSegmentation", "Foggy_CityscapesSegmentation", "GTAVSegmentation",
            "BDD100kSegmentation", "SynthiaSegmentation", "MapillarySegmentation")

EVAL_SIZE = 16
# (name, source width, source height) at eval_size 16: w' = int(w / h * 16), x1 = int(round((w' - 16) / 2.))
CASES = (
    ("half_even", 40, 30),      # w' = 21, w' - tw = 5, x1 = round(2.5) = 2
    ("diff3", 36, 30),          # w' = 19, x1 = round(1.5) = 2
    ("diff1", 32, 30),          # w' = 17, x1 = round(0.5) = 0
    ("exact", 30, 30),          # w' = tw
    ("narrow", 30, 40),         # w' = 12, pad 4 + 4, x1 = -2: 2 outside columns, 4 pad columns, 10 content columns
    ("pad_only", 29, 30),       # w' = 15, pad 1 + 1, x1 = round(-0.5) = 0: no outside column
    ("upscale", 13, 10),        # h < 16: w' = 20, x1 = 2
    ("down16", 300, 256),       # 16x down in height: w' = 18, x1 = 1, bicubic support of 64 source rows
    ("same_height", 20, 16),    # h = 16 and w' = w: PIL copies, only the crop remains
)
VARIANTS = ((True, 0), (True, 255), (False, 0), (False, 255))      # (Mapillary encoder applied, ignore_index)


def sample(w: int, h: int, seed: int = 0, ids: int = 66):
    """-> (uint8 [h,w,3] image, uint8 [h,w] label map): a multiplicative hash of the coordinates; labels below `ids`, except a
    sprinkle of 255 and of ids, ids + 1 (values a table leaves unchanged or treats specially)."""
    y, x = np.meshgrid(np.arange(h, dtype=np.uint64), np.arange(w, dtype=np.uint64), indexing="ij")
    def mix(c):
        v = (y * np.uint64(7919) + x * np.uint64(104729) + np.uint64(c * 1299709 + seed * 15485863 + 12345)) * np.uint64(2654435761)
        v ^= v >> np.uint64(15)
        v = (v * np.uint64(2246822519)) & np.uint64(0xFFFFFFFF)
        return v ^ (v >> np.uint64(13))
    img = np.stack([(mix(c) & np.uint64(255)).astype(np.uint8) for c in range(3)], -1)
    m = mix(3)
    lab = ((m >> np.uint64(8)) % np.uint64(ids)).astype(np.uint8)
    sel = (m & np.uint64(31)).astype(np.int64)
    lab[sel == 0] = 255
    lab[sel == 1] = min(ids, 255)
    lab[sel == 2] = min(ids + 1, 255)
    return np.ascontiguousarray(img), np.ascontiguousarray(lab)


def all_values_map(h: int = 32, w: int = 48, seed: int = 0) -> np.ndarray:
    """uint8 [h,w] holding every one of the 256 values (h * w >= 256), in hashed order."""
    _, lab = sample(w, h, seed)
    flat = lab.reshape(-1).copy()
    order = np.argsort(sample(w, h, seed + 1)[0][..., 0].reshape(-1), kind="stable")
    flat[order[:256]] = np.arange(256, dtype=np.uint8)
    return flat.reshape(h, w)


def encode_lists(mask: np.ndarray, void_classes, valid_classes, ignore_index: int = 255) -> np.ndarray:
    """The in-place loops over a uint8 map, literally: voids first, then valids in list order (valid_classes[i] -> i)."""
    mask = mask.copy()
    class_map = dict(zip(valid_classes, range(len(valid_classes))))
    for c in void_classes:
        mask[mask == c] = ignore_index
    for c in valid_classes:
        mask[mask == c] = class_map[c]
    return mask


def encode_map(mask: np.ndarray, class_map: dict, default=None) -> np.ndarray:
    """The copy-based loops: out starts as a copy (default None) or as an all-`default` map, out[mask == k] = v."""
    out = mask.copy() if default is None else np.full(mask.shape, default, dtype=mask.dtype)
    for k, v in class_map.items():
        out[mask == k] = v
    return out


def to_tensor(img_u8: np.ndarray, lab_u8: np.ndarray):
    """ToTensor: float32 [3,H,W] in 0..255 and the label map as int64."""
    return np.ascontiguousarray(img_u8.astype(np.float32).transpose(2, 0, 1)), lab_u8.astype(np.int64)


def eval_transform(img_u8: np.ndarray, lab_u8: np.ndarray, table=None):
    return to_tensor(img_u8, lab_u8 if table is None else table[lab_u8])


def geometry(w: int, h: int, eval_size: int):
    tw = int(w / h * eval_size)
    return tw, (eval_size - tw if tw < eval_size else 0), int(round((tw - eval_size) / 2.))


def _crop(a: np.ndarray, x1: int, y1: int, tw: int, th: int) -> np.ndarray:
    """Image.crop: pixels outside the image are 0."""
    out = np.zeros((th, tw) + a.shape[2:], a.dtype)
    H, W = a.shape[:2]
    ys = [(o, y1 + o) for o in range(th) if 0 <= y1 + o < H]
    xs = [(o, x1 + o) for o in range(tw) if 0 <= x1 + o < W]
    if ys and xs:
        out[np.ix_([o for o, _ in ys], [o for o, _ in xs])] = a[np.ix_([s for _, s in ys], [s for _, s in xs])]
    return out


def rhccp_numpy(img_u8: np.ndarray, lab_u8: np.ndarray, eval_size: int, ignore_index: int = 0, table=None):
    """ResizeHeight(eval_size) -> CenterCropPad(eval_size, ignore_index) on arrays -> (uint8 [t,t,3], uint8 [t,t]); the label is
    encoded first, as the reference's __getitem__ does."""
    h, w = lab_u8.shape
    t = eval_size
    tw, pad_x, x1 = geometry(w, h, t)
    lab = lab_u8 if table is None else table[lab_u8]
    simg = io.resample_u8(img_u8, tw, t, "bicubic")
    ty, tx = io.nearest_table(h, t), io.nearest_table(w, tw)
    slab = lab[np.ix_(ty, tx)]
    if pad_x:                                                        # the full deficit on both sides; the height needs none
        simg = np.pad(simg, ((0, 0), (pad_x, pad_x), (0, 0)), constant_values=0)
        slab = np.pad(slab, ((0, 0), (pad_x, pad_x)), constant_values=ignore_index)
    return _crop(simg, x1, 0, t, t), _crop(slab, x1, 0, t, t)        # x1 from the width before padding


def rhccp_pil(img_u8: np.ndarray, lab_u8: np.ndarray, eval_size: int, ignore_index: int = 0, table=None):
    """The same steps by PIL itself, in the reference's order: Image.resize, ImageOps.expand, Image.crop."""
    from PIL import Image, ImageOps
    t = eval_size
    h, w = lab_u8.shape
    tw, pad_x, x1 = geometry(w, h, t)
    img = Image.fromarray(img_u8).resize((tw, t), Image.BICUBIC)
    mask = Image.fromarray(lab_u8 if table is None else table[lab_u8]).resize((tw, t), Image.NEAREST)
    if pad_x:                                                        # (left, top, right, bottom)
        img = ImageOps.expand(img, border=(pad_x, 0, pad_x, 0), fill=0)
        mask = ImageOps.expand(mask, border=(pad_x, 0, pad_x, 0), fill=ignore_index)
    box = (x1, 0, x1 + t, t)
    return np.array(img.crop(box), dtype=np.uint8), np.array(mask.crop(box), dtype=np.uint8)


def case_sample(i: int):
    name, w, h = CASES[i]
    return sample(w, h, seed=i + 1)


_fixture = None


def fixture():
    global _fixture
    if _fixture is None:
        with np.load(FIXTURE) as z:
            _fixture = {k: z[k] for k in z.files}
    return _fixture
