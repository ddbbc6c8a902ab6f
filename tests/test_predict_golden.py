"""The colour coding against the reference's own output (tests/golden/predict.npz, written by tests/golden/make_golden_predict.py
from the reference's decode_segmap / get_cityscapes_labels).  No GPU: the table and the look-up rule; the device kernel is held to
the same array in test_predict_gpu.py."""
import numpy as np
import pytest

from mrfp_amd import predict

import predict_common as pc


@pytest.fixture(scope="module")
def golden():
    return np.load(pc.FIXTURE)


def test_fixture_covers_every_label_the_issue_names(golden):
    mask = golden["mask"]
    assert mask.dtype == np.uint8 and mask.shape == (6, 8)
    assert set(range(19)) | {19, 20, 200, 255} == set(mask.reshape(-1).tolist())
    assert golden["rgb"].dtype == np.float64 and golden["rgb"].shape == (6, 8, 3)


def test_cityscapes_table_is_the_reference_table(golden):
    pal = predict.Palette.cityscapes()
    assert pal.table.dtype == np.uint8 and pal.table.shape == (256, 3)
    assert np.array_equal(pal.table[:19], golden["table"])
    i = np.arange(19, 256)
    assert np.array_equal(pal.table[19:], np.stack([i, i, i], axis=1))      # labels outside 0..18: the label in all three channels


def test_lookup_divided_by_255_is_the_reference_array(golden):
    pal = predict.Palette.cityscapes()
    got = pc.np_colorize(golden["mask"], pal.table) / 255.0
    assert got.dtype == np.float64 and np.array_equal(got, golden["rgb"])
    assert np.array_equal(got[golden["mask"] == 255], np.ones((int((golden["mask"] == 255).sum()), 3)))     # 255 comes out white


def test_other_datasets_are_not_built():
    with pytest.raises(NotImplementedError):
        predict.decode_segmap(None, "pascal")
    with pytest.raises(NotImplementedError):
        predict.decode_segmap(None, "coco")
