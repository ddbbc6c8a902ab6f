"""Writes tests/golden/eval_input.npz: what the reference and PIL themselves give for the evaluation input path.

    python tests/golden/make_golden_eval_input.py /path/to/reference/main.py

Needs the reference tree and Pillow; no GPU.  Recorded:
  names, tables [7,256]   per dataset class of main.py: what that class's own label-encoding statements leave of arange(256).
                          main.py cannot be imported (it parses arguments and opens datasets at import), so it is parsed
                          with `ast`: from __init__ the assignments of void_classes / valid_classes / ignore_index /
                          class_map (the loops that fill class_map included), from __getitem__ the statements between the
                          one that reads the label file into `_tmp` and the one that wraps the result in Image.fromarray --
                          those statements are then run, as they stand, on _tmp = arange(256).
  img_<case> [16,16,3], lab_<case> [4,16,16]
                          PIL's output (Image.resize, ImageOps.expand, Image.crop in the reference's order) for the cases and
                          variants of tests/eval_input_common.py, whose samples are generated, not stored."""
import ast
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                      # tests/
sys.path.insert(1, os.path.dirname(os.path.dirname(HERE)))     # the repository root (oracle/)
import eval_input_common as eic  # noqa: E402

ENCODING_ATTRS = {"void_classes", "valid_classes", "ignore_index", "class_map"}


def _self_attr(node):
    """the attribute name when `node` is self.<name> or self.<name>[...]"""
    if isinstance(node, ast.Subscript):
        node = node.value
    if isinstance(node, ast.Attribute) and isinstance(node.value, ast.Name) and node.value.id == "self":
        return node.attr
    return None


def _sets_encoding_attr(stmt) -> bool:
    if isinstance(stmt, ast.Assign):
        return all(_self_attr(t) in ENCODING_ATTRS for t in stmt.targets)
    if isinstance(stmt, ast.For):
        return bool(stmt.body) and all(_sets_encoding_attr(s) for s in stmt.body)
    return False


def _run(stmts, env):
    mod = ast.Module(body=list(stmts), type_ignores=[])
    ast.fix_missing_locations(mod)
    exec(compile(mod, "<reference main.py>", "exec"), env)


def _assigns_name(stmt, name) -> bool:
    return isinstance(stmt, ast.Assign) and any(isinstance(t, ast.Name) and t.id == name for t in stmt.targets)


def class_table(cls: ast.ClassDef) -> np.ndarray:
    funcs = {f.name: f for f in cls.body if isinstance(f, ast.FunctionDef)}
    me = types.SimpleNamespace()
    for s in cls.body:                                          # NUM_CLASSES = 19
        if isinstance(s, ast.Assign) and all(isinstance(t, ast.Name) for t in s.targets):
            for t in s.targets:
                setattr(me, t.id, ast.literal_eval(s.value))
    env = {"self": me, "np": np}
    _run([s for s in funcs["__init__"].body if _sets_encoding_attr(s)], env)
    if "encode_segmap" in funcs:
        _run([funcs["encode_segmap"]], env)
        me.encode_segmap = types.MethodType(env["encode_segmap"], me)
    body = funcs["__getitem__"].body
    first = next(i for i, s in enumerate(body) if _assigns_name(s, "_tmp"))
    last = next(i for i, s in enumerate(body) if _assigns_name(s, "_target"))
    wrap = body[last].value                                     # Image.fromarray(<the encoded map>)
    assert isinstance(wrap, ast.Call) and ast.unparse(wrap.func) == "Image.fromarray" and len(wrap.args) == 1, ast.unparse(wrap)
    env["_tmp"] = np.arange(256, dtype=np.uint8)
    _run(body[first + 1:last], env)
    out = eval(compile(ast.Expression(wrap.args[0]), "<reference main.py>", "eval"), env)
    out = np.asarray(out)
    assert out.shape == (256,) and out.min() >= 0 and out.max() <= 255, cls.name
    return out.astype(np.uint8)


def main(path: str):
    tree = ast.parse(open(path).read())
    classes = {c.name: c for c in tree.body if isinstance(c, ast.ClassDef)}
    rec = {"names": np.array(eic.DATASETS), "tables": np.stack([class_table(classes[n]) for n in eic.DATASETS])}
    mapillary = rec["tables"][eic.DATASETS.index("MapillarySegmentation")]
    for i, (name, w, h) in enumerate(eic.CASES):
        img, lab = eic.case_sample(i)
        outs = [eic.rhccp_pil(img, lab, eic.EVAL_SIZE, ign, mapillary if enc else None) for enc, ign in eic.VARIANTS]
        assert all(np.array_equal(o[0], outs[0][0]) for o in outs)
        rec["img_" + name] = outs[0][0]
        rec["lab_" + name] = np.stack([o[1] for o in outs])
    np.savez_compressed(eic.FIXTURE, **rec)
    print(eic.FIXTURE, os.path.getsize(eic.FIXTURE), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
