"""Times the centroid pass of class-uniform sampling: on the device, and the published host loop on the cores of the same machine.
profiles/class_uniform.md is one run of

    timeout -k 10 600 python tools/class_uniform_micro.py host && timeout -k 10 300 python tools/class_uniform_micro.py device && \
    python tools/class_uniform_micro.py report

Every step writes out/class_uniform_<step>.json (MRFP_OUT names another directory); `report` joins them into
profiles/class_uniform.md (MRFP_PROFILE names another file).
  host    the published form: per label map `for tile: for class: scipy.ndimage.center_of_mass(patch == c)`, the id -> train id table
          applied first, the maps spread over a pool of 16 worker processes (the maps are in memory: no PNG decoding is timed);
          wall clock, median of 3; needs no GPU
  device  mrfp_tile_class_sums over 16 x 1024 x 2048 label maps at tile 1024, 19 classes, with and without the table, and
          mrfp_label_lut_u8 over the same maps -- a pure streaming pass (one byte read, one written per label): device-event median
          of single calls and of bursts of 20, label bytes per second in a burst.  Checked against the host result before anything
          is timed.  Needs a GPU: there is no fallback."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.environ.get("MRFP_OUT", os.path.join(ROOT, "out"))
PROFILE = os.environ.get("MRFP_PROFILE", os.path.join(ROOT, "profiles", "class_uniform.md"))
B, H, W, TILE, C, WORKERS = 16, 1024, 2048, 1024, 19, 16


def _maps():
    """16 label maps of Cityscapes label ids 0..33 in 32 x 32 patches of one id with 1 % noise on top: piecewise constant, as label
    maps are, with every id present."""
    rng = np.random.default_rng(16)
    blocks = rng.integers(0, 34, (B, H // 32, W // 32), dtype=np.uint8)
    lab = np.repeat(np.repeat(blocks, 32, 1), 32, 2)
    noise = rng.random((B, H, W)) < 0.01
    lab[noise] = rng.integers(0, 34, int(noise.sum()), dtype=np.uint8)
    return lab


def _table():
    from mrfp_amd import input_pipeline as ip
    return ip.label_encoder("Cityscapes").table.copy()


def _save(step, rows):
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "class_uniform_%s.json" % step)
    json.dump(rows, open(path, "w"), indent=1)
    for r in rows:
        print(json.dumps(r))
    print(path)


def _published(args):
    """One label map the published way -> [(ty, tx, c, cx, cy)]."""
    from scipy import ndimage
    lab, table = args
    m = table[lab]
    out = []
    for ty in range(H // TILE):
        for tx in range(W // TILE):
            y0, x0 = ty * TILE, tx * TILE
            patch = m[y0:y0 + TILE, x0:x0 + TILE]
            for c in range(C):
                mask = patch == c
                if mask.any():
                    cy, cx = ndimage.center_of_mass(mask)
                    out.append((ty, tx, c, int(cx) + x0, int(cy) + y0))
    return out


def host():
    import multiprocessing as mp
    lab, table = _maps(), _table()
    jobs = [(lab[b], table) for b in range(B)]
    ts = []
    with mp.get_context("fork").Pool(WORKERS) as pool:
        pool.map(_published, jobs[:WORKERS])                     # workers started and scipy imported before the clock runs
        for _ in range(3):
            t0 = time.perf_counter()
            res = pool.map(_published, jobs, chunksize=1)
            ts.append((time.perf_counter() - t0) * 1e3)
    ms = sorted(ts)[1]
    cent = np.full((B, H // TILE, W // TILE, C, 2), -1, dtype=np.int32)
    for b, lst in enumerate(res):
        for ty, tx, c, cx, cy in lst:
            cent[b, ty, tx, c] = (cx, cy)
    os.makedirs(OUT, exist_ok=True)
    np.save(os.path.join(OUT, "class_uniform_host_cent.npy"), cent)
    _save("host", [dict(what="published host loop (table, then center_of_mass per tile and class), %d worker processes" % WORKERS,
                        ms=ms, bytes=B * H * W, GBps=B * H * W / ms / 1e6)])


def _dev_median(fn, calls=20, load_s=1.0):
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.time()
    while time.time() - t0 < load_s:           # clocks and caches in their loaded state before anything is read
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
    ts = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2]


def device():
    import torch
    from mrfp_amd import input_pipeline as ip
    from mrfp_amd._lib import call, ptr, stream
    lab, table = _maps(), _table()
    x = torch.from_numpy(lab).cuda()
    enc = ip.LabelEncoder(table)
    t = enc.device_table(x.device)
    encoded = enc(x)
    sums, cent = ip.tile_class_centroids(x, C, TILE, t)
    plain_sums, plain_cent = ip.tile_class_centroids(encoded, C, TILE)
    assert torch.equal(sums, plain_sums) and torch.equal(cent, plain_cent)
    ref = os.path.join(OUT, "class_uniform_host_cent.npy")
    checked = os.path.exists(ref)
    if checked:
        assert np.array_equal(np.load(ref), cent.cpu().numpy()), "the device centroids differ from the published host loop's"
    o8 = torch.zeros_like(x)
    n = x.numel()
    nty, ntx = H // TILE, W // TILE
    rows = []
    for what, fn in (
            ("mrfp_tile_class_sums, table fused", lambda: call("mrfp_tile_class_sums", ptr(x), ptr(t), B, H, W, C, TILE, 0, ptr(sums), ptr(cent), stream())),
            ("mrfp_tile_class_sums, no table", lambda: call("mrfp_tile_class_sums", ptr(encoded), None, B, H, W, C, TILE, 0, ptr(sums), ptr(cent), stream())),
            ("mrfp_label_lut_u8 (streaming pass)", lambda: enc(x, out=o8))):
        ms = _dev_median(fn)

        def burst(fn=fn):                       # 20 calls between one pair of events: the per-call time without the pair's own floor
            for _ in range(20):
                fn()
        ms20 = _dev_median(burst, calls=10, load_s=0.5) / 20
        rows.append(dict(what=what, ms=ms, ms_in_burst=ms20, bytes=n, GBps=n / ms20 / 1e6, tiles=B * nty * ntx,
                         equals_host_loop=checked))
    _save("device", rows)


def report():
    dev = json.load(open(os.path.join(OUT, "class_uniform_device.json")))
    hst = json.load(open(os.path.join(OUT, "class_uniform_host.json")))
    stream_ms = [r for r in dev if "lut" in r["what"]][0]["ms_in_burst"]
    lines = ["# Class-uniform sampling: the centroid pass", "",
             "`tools/class_uniform_micro.py` (host, device, report) on one MI355X machine: %d label maps of %d x %d, tile %d, %d classes, "
             "label ids through the Cityscapes table.  GB/s counts the label bytes (%.1f MB) once, whatever a pass writes besides; "
             "the streaming pass `mrfp_label_lut_u8` reads and writes every one of them.  The device centroids were compared with the "
             "host loop's before timing: %s." % (B, H, W, TILE, C, B * H * W / 1e6, "equal" if all(r["equals_host_loop"] for r in dev)
                                                  else "NOT COMPARED (no host result in the output directory)"), "",
             "| what | ms per call | ms in a burst of 20 | GB/s of label bytes | time / streaming pass |", "|---|---|---|---|---|"]
    for r in dev:
        lines.append("| %s | %.4f | %.4f | %.0f | %.2f |" % (r["what"], r["ms"], r["ms_in_burst"], r["GBps"], r["ms_in_burst"] / stream_ms))
    for r in hst:
        lines.append("| %s | %.1f | | %.3f | %.0f |" % (r["what"], r["ms"], r["GBps"], r["ms"] / stream_ms))
    lines += ["", "No test asserts a time: these are the first measurements of either side."]
    os.makedirs(os.path.dirname(PROFILE), exist_ok=True)
    open(PROFILE, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print(PROFILE)


if __name__ == "__main__":
    {"host": host, "device": device, "report": report}[sys.argv[1]]()
