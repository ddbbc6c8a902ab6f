"""What a user looks at or hands in: colour images of a prediction (reference utils_main.py:28-103, decode_segmap and
get_cityscapes_labels, which main.py:15 star-imports) on the device.  The label maps themselves come from harness.predict
(ops.upsample_argmax); the way back from train ids to a dataset's own ids is input_pipeline.LabelEncoder.inverse()."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from .input_pipeline import _cached, _dev

# the public Cityscapes colour coding of the 19 train ids, in the order of reference utils_main.py:83-103
_CITYSCAPES = (
    (128, 64, 128), (244, 35, 232), (70, 70, 70), (102, 102, 156), (190, 153, 153), (153, 153, 153), (250, 170, 30), (220, 220, 0),
    (107, 142, 35), (152, 251, 152), (70, 130, 180), (220, 20, 60), (255, 0, 0), (0, 0, 142), (0, 0, 70), (0, 60, 100), (0, 80, 100),
    (0, 0, 230), (119, 11, 32))


class Palette:
    """A colour coding as one uint8 [256,3] table, applied on the device (csrc/predict.hip: colorize_u8).  The device copy is
    cached per device, as LabelEncoder's table."""

    def __init__(self, table):
        table = np.asarray(table)
        if table.shape != (256, 3) or table.min() < 0 or table.max() > 255:
            raise ValueError("Palette: a [256,3] table of values in 0..255 expected")
        self.table = np.ascontiguousarray(table.astype(np.uint8))
        self.table.setflags(write=False)
        self._dev_tables = {}

    @classmethod
    def cityscapes(cls) -> "Palette":
        """The 19 Cityscapes colours; every index >= 19 maps to (i, i, i), which is what the reference's decode_segmap leaves for a
        label outside 0..18 (it copies the label into all three channels: 255 comes out white)."""
        t = np.repeat(np.arange(256, dtype=np.int64)[:, None], 3, axis=1)
        t[:len(_CITYSCAPES)] = np.asarray(_CITYSCAPES, dtype=np.int64)
        return cls(t)

    def device_table(self, dev) -> torch.Tensor:
        return _cached(self._dev_tables, str(dev), lambda: _dev(dev, self.table.copy())[0])

    def __call__(self, pred_u8: torch.Tensor, image_u8=None, alpha: float = 0.5, out=None) -> torch.Tensor:
        """uint8 label map [...] on the device -> uint8 [..., 3]; with image_u8 the blend of ops.colorize."""
        from . import ops
        if not (isinstance(pred_u8, torch.Tensor) and pred_u8.is_cuda):
            raise _lib.MrfpHipError("Palette: a uint8 CUDA tensor expected (there is no CPU path)")
        return ops.colorize(pred_u8, self.device_table(pred_u8.device), image_u8, alpha, out)


_PALETTES = {}


def decode_segmap(label_u8: torch.Tensor, dataset: str = "cityscapes") -> np.ndarray:
    """reference utils_main.py:28-63 on a device tensor: uint8 label map [H,W] -> the float64 [H,W,3] array the reference function
    returns (the uint8 colours divided by 255.0 on the host).  Only 'cityscapes' is built: the reference's 'pascal' / 'coco' branch
    indexes its 19-row table with 21 classes and cannot run."""
    if dataset != "cityscapes":
        raise NotImplementedError("decode_segmap: dataset %r (only 'cityscapes' is built)" % (dataset,))
    pal = _cached(_PALETTES, dataset, Palette.cityscapes)
    return pal(label_u8).cpu().numpy() / 255.0
