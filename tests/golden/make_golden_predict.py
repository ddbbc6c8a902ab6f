"""Writes tests/golden/predict.npz: what the reference's own colour coding gives.

    python tests/golden/make_golden_predict.py /path/to/reference/utils_main.py

Needs the reference tree; no GPU.  utils_main.py imports matplotlib, torchmetrics and skimage at module level and runs code on
import, so it is parsed with `ast` and only its two functions get_cityscapes_labels and decode_segmap are compiled and run, as they
stand, with numpy.  Recorded:
  mask [6,8] uint8       every label 0..18, plus 19, 20, 200 and 255
  rgb  [6,8,3] float64   decode_segmap(mask, 'cityscapes') as the reference returns it
  table [19,3] int64     get_cityscapes_labels()"""
import ast
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "predict.npz")
WANTED = ("get_cityscapes_labels", "decode_segmap")


def golden_mask():
    vals = list(range(19)) + [19, 20, 200, 255]
    return np.array([vals[(3 * i) % len(vals)] if i >= len(vals) else vals[i] for i in range(48)], dtype=np.uint8).reshape(6, 8)


def main(path):
    tree = ast.parse(open(path).read())
    funcs = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in WANTED]
    assert sorted(f.name for f in funcs) == sorted(WANTED)
    mod = ast.Module(body=funcs, type_ignores=[])
    ast.fix_missing_locations(mod)
    env = {"np": np}
    exec(compile(mod, "<reference utils_main.py>", "exec"), env)
    mask = golden_mask()
    assert set(range(19)) | {19, 20, 200, 255} == set(mask.reshape(-1).tolist())
    rgb = env["decode_segmap"](mask, "cityscapes")
    table = np.asarray(env["get_cityscapes_labels"]())
    assert rgb.dtype == np.float64 and rgb.shape == (6, 8, 3) and table.shape == (19, 3)
    np.savez_compressed(FIXTURE, mask=mask, rgb=rgb, table=table.astype(np.int64))
    print(FIXTURE, os.path.getsize(FIXTURE), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
