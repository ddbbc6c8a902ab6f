"""Poisoned fresh memory: every uninitialised buffer the Python layer obtains is laid between two guard bands and filled with one byte.

Host-only Python (it runs on CPU tensors as well as on the device; tests/test_poison_cpu.py proves it there).

The library uses no floating-point atomics and fixed-order finalizes, so the result of an operator must not depend on what its fresh
memory held -- not in one bit.  A fresh pytest process almost always hands out zero pages; training hands out last step's
activations.  `poisoned(byte)` replaces torch.empty, torch.empty_like, torch.empty_strided and torch.Tensor.new_empty for its duration
(ops.empty_cl and ops.wgrad_workspace go through torch.empty): each call is made for real to learn dtype, shape and strides, then
G + nbytes + G bytes of uint8 are allocated, filled with `byte`, and a tensor of the requested dtype, shape and strides over the middle
nbytes is returned.  Host allocations (pinned, or device cpu) pass through; poisoned(byte, host=True) fills unpinned CPU tensors too,
which is how the helper is tested without a device.

Three fills, each for a reason:
  0x00  what fresh pages look like: the baseline, not "the truth";
  0xFF  NaN in fp32, bf16 and f16; -1 in the integer types; 255 in uint8;
  0x7B  finite and huge in every float type (fp32 and bf16 about 1.3e36, f16 61280), 123 in uint8 -- NaN is swallowed by an
        fmaxf(x, 0) ReLU epilogue, and 255 is this project's ignore label and would hide a stale label or mask byte.

run_three(fn) runs fn under the three fills and asserts that the guard bands are intact, that every float result is finite and that
the three result tuples are equal bit for bit.  What is compared is what fn returns: what a caller may read.

inventory() walks the AST of EVERY module of the package for the functions that call one of the allocating names; tests/test_poison_cpu.py
holds the case table of tests/test_poison_gpu.py to it.
"""
import ast
import contextlib
import os
import sys

import torch

G = 4096                                  # guard band, bytes, on either side of the body (keeps 16- and 256-byte alignment)
FILLS = (0x00, 0xFF, 0x7B)
PATCHED = ("empty", "empty_like", "empty_strided")         # of torch; plus torch.Tensor.new_empty
HELPERS = ("ops.empty_cl", "ops.wgrad_workspace")          # they call torch.empty for their caller: both are recorded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mrfp_amd")
TORCH_NAMES = {"empty", "empty_like", "empty_strided"}          # counted as torch.<name>(...) only: numpy has the same names
OWN_NAMES = {"new_empty", "empty_cl", "wgrad_workspace"}       # a Tensor method and the package's two helpers, however they are reached
ALLOC_NAMES = TORCH_NAMES | OWN_NAMES


def package_modules(pkg=PKG):
    """Every Python module under the package, as dotted names relative to it: an operator that allocates in a module nobody thought of
    (inference.py, predict.py, network/...) is found too."""
    mods = []
    for base, dirs, files in os.walk(pkg):
        dirs[:] = sorted(d for d in dirs if d != "__pycache__")
        for f in sorted(files):
            if f.endswith(".py"):
                mods.append(os.path.relpath(os.path.join(base, f), pkg)[:-3].replace(os.sep, "."))
    return tuple(mods)


MODULES = package_modules()

_REAL = {n: getattr(torch, n) for n in PATCHED}
_REAL_NEW_EMPTY = torch.Tensor.new_empty
_ACTIVE = [None]                          # the fill byte while a poisoned() block is open
REGISTRY = []                             # (buffer uint8 [G + nbytes + G], nbytes, byte, call site)
SITES = set()                             # every module.qualname of mrfp_amd that obtained a poisoned buffer (helpers AND their callers)


# ---- call sites: module.qualname of the frames inside mrfp_amd -----------------------------------------------------------------
def _walk_functions(tree):
    """(qualname, node) of every function of a module, nested ones as outer.inner, methods as Class.method."""
    out = []

    def visit(node, qual):
        for ch in ast.iter_child_nodes(node):
            if isinstance(ch, (ast.FunctionDef, ast.AsyncFunctionDef, ast.ClassDef)):
                q = qual + [ch.name]
                if not isinstance(ch, ast.ClassDef):
                    out.append((".".join(q), ch))
                visit(ch, q)
            else:
                visit(ch, qual)
    visit(tree, [])
    return out


def _own_calls(fn):
    """The calls in fn's own body: not those of the functions and classes nested in it."""
    stack = list(ast.iter_child_nodes(fn))
    while stack:
        n = stack.pop()
        if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef, ast.ClassDef)):
            continue
        if isinstance(n, ast.Call):
            yield n
        stack.extend(ast.iter_child_nodes(n))


def _called_name(call):
    """The allocating name a call uses, or None: torch.empty / torch.empty_like / torch.empty_strided (np.empty and the like are host
    arrays), x.new_empty, and empty_cl / wgrad_workspace bare or through a module."""
    f = call.func
    if isinstance(f, ast.Name):
        return f.id if f.id in OWN_NAMES else None
    if not isinstance(f, ast.Attribute):
        return None
    if f.attr in OWN_NAMES:
        return f.attr
    if f.attr in TORCH_NAMES and isinstance(f.value, ast.Name) and f.value.id == "torch":
        return f.attr
    return None


def inventory(modules=MODULES, pkg=PKG):
    """{module.qualname: [(line, name, is_pinned)]} of every function of the package's allocating modules whose own body calls one of
    ALLOC_NAMES."""
    found = {}
    for m in modules:
        with open(os.path.join(pkg, *m.split(".")) + ".py") as f:
            tree = ast.parse(f.read())
        for qual, fn in _walk_functions(tree):
            for c in _own_calls(fn):
                n = _called_name(c)
                if n is not None:
                    pinned = any(k.arg == "pin_memory" for k in c.keywords)
                    found.setdefault(m + "." + qual, []).append((c.lineno, n, pinned))
    return found


_QUALNAMES = {}                           # file name -> {first line of a code object -> qualname}


def _qualnames(filename):
    tab = _QUALNAMES.get(filename)
    if tab is None:
        tab = {}
        with open(filename) as f:
            tree = ast.parse(f.read())
        for qual, fn in _walk_functions(tree):
            first = min([fn.lineno] + [d.lineno for d in fn.decorator_list])      # co_firstlineno is the first decorator's line
            tab[first] = qual
            tab[fn.lineno] = qual
        _QUALNAMES[filename] = tab
    return tab


def _frame_name(frame, pkg):
    fn = frame.f_code.co_filename
    if not fn.startswith(pkg + os.sep) or not fn.endswith(".py"):
        return None
    mod = os.path.relpath(fn, pkg)[:-3].replace(os.sep, ".")
    qual = _qualnames(fn).get(frame.f_code.co_firstlineno)
    return mod + "." + (qual if qual is not None else frame.f_code.co_name)


def call_site(depth=2, pkg=PKG):
    """-> (site, every name to record): the first frame inside the package above the patched call; when that frame is one of the
    HELPERS, its caller inside the package is the site and both are recorded.  None outside the package."""
    f = sys._getframe(depth)
    names = []
    while f is not None:
        n = _frame_name(f, pkg)
        if n is not None:
            names.append(n)
            if n not in HELPERS:
                break
        elif names:
            break                          # a helper called from outside the package
        f = f.f_back
    return (names[-1] if names else None), names


# ---- the poisoner ------------------------------------------------------------------------------------------------------------------
_HOST_TOO = [False]                       # poisoned(host=True): unpinned CPU tensors are filled too


def _guarded(proto, byte):
    """proto: the tensor the real call returned (dense or expanded from fewer elements: its storage is what is rebuilt)."""
    if proto.device.type == "cpu" and (not _HOST_TOO[0] or proto.is_pinned()):
        return proto                       # host memory
    if proto.layout != torch.strided or proto.is_quantized:
        return proto
    n = proto.untyped_storage().nbytes()
    es = proto.element_size()
    buf = _REAL["empty"](G + n + G, dtype=torch.uint8, device=proto.device)
    buf.fill_(byte)
    t = _REAL["empty"](0, dtype=proto.dtype, device=proto.device)
    t.set_(buf.untyped_storage(), G // es + proto.storage_offset(), proto.shape, proto.stride())
    if proto.requires_grad:
        t.requires_grad_(True)
    site, names = call_site(3)
    REGISTRY.append((buf, n, byte, site))
    SITES.update(names)
    return t


def _wrap(real):
    def patched(*a, **k):
        out = real(*a, **k)
        byte = _ACTIVE[0]
        if byte is None or k.get("pin_memory") or k.get("out") is not None:
            return out
        return _guarded(out, byte)
    patched.__name__ = getattr(real, "__name__", "patched")
    patched._poison_real = real
    return patched


@contextlib.contextmanager
def poisoned(byte, host=False):
    """For the duration: torch.empty / empty_like / empty_strided / Tensor.new_empty return guarded, `byte`-filled memory."""
    if _ACTIVE[0] is not None:
        raise RuntimeError("poisoned() does not nest (a block with fill 0x%02X is open)" % _ACTIVE[0])
    if not (isinstance(byte, int) and 0 <= byte <= 255):
        raise ValueError("poisoned(byte): 0 <= byte <= 255, got %r" % (byte,))
    _ACTIVE[0], _HOST_TOO[0] = byte, bool(host)
    try:
        for n, real in _REAL.items():
            setattr(torch, n, _wrap(real))
        torch.Tensor.new_empty = _wrap(_REAL_NEW_EMPTY)
        yield
    finally:
        for n, real in _REAL.items():
            setattr(torch, n, real)
        torch.Tensor.new_empty = _REAL_NEW_EMPTY
        _ACTIVE[0], _HOST_TOO[0] = None, False


def reset():
    """Forgets the recorded buffers and call sites."""
    del REGISTRY[:]
    SITES.clear()


def guard_report():
    """[] when every recorded front and back band still holds its fill byte everywhere; else one line per damaged band: the call
    site and the offset of the first changed byte relative to the END OF THE BODY (>= 0: behind the body; a front band reports
    -(nbytes + distance before the body's first byte))."""
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    bad = []
    for buf, n, byte, site in REGISTRY:
        for name, band, base in (("front", buf[:G], -n - G), ("back", buf[G + n:], 0)):
            ne = band != byte
            if bool(ne.any()):
                first = int(ne.nonzero()[0])
                bad.append("%s: %s guard of a %d-byte buffer (fill 0x%02X) changed, first at offset %+d from the end of the body, %d "
                           "bytes in all" % (site, name, n, byte, base + first, int(ne.sum())))
    return bad


def guards_intact():
    return not guard_report()


# ---- the comparison ----------------------------------------------------------------------------------------------------------------
_INT_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def bits(t):
    """t's elements as integers of the same width, so that NaN compares equal to itself and -0.0 differs from 0.0."""
    t = t.detach()
    if t.dtype == torch.bool:
        return t.to(torch.uint8)
    if not t.is_floating_point() and not t.is_complex():
        return t
    if t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last) and not t.is_contiguous():
        return t.permute(0, 2, 3, 1).view(_INT_VIEW[t.element_size()]).permute(0, 3, 1, 2)
    return t.contiguous().view(_INT_VIEW[t.element_size()])


class Named(tuple):
    """A result tuple that knows what its members are called (run_three's reports use the names)."""
    names = ()


def named(*pairs, **kw):
    """named(("y", y), ("dx", dx)) or named(y=y, dx=dx) -> the tuple (y, dx) with .names."""
    pairs = list(pairs) + list(kw.items())
    out = Named(t for _, t in pairs)
    out.names = tuple(n for n, _ in pairs)
    return out


def row_trip(C, dtype):
    """Pixels of a line one trip of a row kernel's 256 threads covers (csrc/common.hpp pick_vec / make_lanes: a 16-byte vector when it
    divides C, else scalars; colthreads x rowthreads over (channel vector, pixel); four pixels per row thread and trip)."""
    full = 16 // torch.empty((), dtype=dtype).element_size()
    vec = full if C % full == 0 else 1
    col = min(C // vec, 256)
    return 4 * (256 // col)


def describe_mismatch(name, a, b, fa, fb, first=6):
    ne = (bits(a) != bits(b))
    idx = ne.nonzero()[:first].tolist()
    lines = ["%s: fill 0x%02X and fill 0x%02X differ in %d of %d elements (%s %s)" % (name, fa, fb, int(ne.sum()), ne.numel(), a.dtype,
                                                                                   tuple(a.shape))]
    for i in idx:
        va, vb = a[tuple(i)].item(), b[tuple(i)].item()
        if a.dim() == 4:
            bb, c, y, x = i
            H, W, C = a.shape[2], a.shape[3], a.shape[1]
            trip = row_trip(C, a.dtype) if a.is_floating_point() else W
            lines.append("    (b, y, x, c) = (%d, %d, %d, %d); y = H - %d, x = W - %d, c = C - %d; in its line: trip %d of %d pixels, pixel "
                         "%d of it, line pixel %d mod 64 = %d: %r vs %r" % (bb, y, x, c, H - y, W - x, C - c, x // trip, trip, x % trip, x, x % 64,
                                                                            va, vb))
        else:
            lines.append("    %s (of %s): %r vs %r" % (tuple(i), tuple(a.shape), va, vb))
    return "\n".join(lines)


def run_three(fn, names=None, host=False):
    """fn() -> a flat tuple of result tensors (None members allowed; a Named tuple gives the reports their names).  Runs it under each of FILLS, with the weight packs invalidated
    first so that they are rebuilt under that fill; asserts intact guards, finite float results and bitwise equality of the three
    tuples.  -> the set of call sites recorded over the three runs."""
    from mrfp_amd import conv
    results, sites = [], set()
    for byte in FILLS:
        reset()
        conv.invalidate_packs()
        with poisoned(byte, host=host):
            out = fn()
        names = getattr(out, "names", None) or names
        out = tuple(out) if isinstance(out, (tuple, list)) else (out,)
        bad = guard_report()
        assert not bad, "fill 0x%02X: a store left its buffer\n%s" % (byte, "\n".join(bad))
        results.append(tuple(None if t is None else t.detach().clone() for t in out))
        sites |= SITES
        reset()
    base = results[0]
    nm = lambda i: names[i] if names is not None and i < len(names) else "result[%d]" % i
    for byte, res in zip(FILLS, results):
        assert len(res) == len(base), "fill 0x%02X returned %d results, fill 0x00 %d" % (byte, len(res), len(base))
        for i, t in enumerate(res):
            assert (t is None) == (base[i] is None), "%s: None under one fill only" % nm(i)
            if t is not None and t.is_floating_point():
                bad = ~torch.isfinite(t)
                assert not bool(bad.any()), "%s: %d non-finite values under fill 0x%02X, first at %s" % (
                    nm(i), int(bad.sum()), byte, tuple(bad.nonzero()[0].tolist()))
    problems = []
    for byte, res in zip(FILLS[1:], results[1:]):
        for i, (a, b) in enumerate(zip(base, res)):
            if a is None:
                continue
            assert a.shape == b.shape and a.dtype == b.dtype, "%s: %s %s vs %s %s" % (nm(i), a.dtype, tuple(a.shape), b.dtype, tuple(b.shape))
            if not torch.equal(bits(a), bits(b)):
                problems.append(describe_mismatch(nm(i), a, b, FILLS[0], byte))
    assert not problems, "the result depends on what fresh memory held:\n" + "\n".join(problems)
    return sites
