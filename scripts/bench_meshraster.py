"""Time the GPU rasteriser (neuraludf_amd/meshrender.py, csrc/meshraster.hip) with HIP events per stage, on the mesh of
scripts/bench_chamfer.py -- the radius-280 sphere at 512^3 in a 600 mm box (1.07 M vertices, 2.14 M faces) -- and the rig
of scripts/bench_meshclean.py: 64 views of 1600 x 1200.

    project      the (view, vertex) projections, summed over the chunks of 8 views
    bounds       the pixel count of every (view, face)
    split        torch: nonzero and the two compactions into the small and the large list
    draw_small   one thread per entry
    draw_large   one wavefront per entry
    resolve      depth, face and barycentrics per pixel
    rasterize / visibility / colour     the three public calls, whole (buffers, fills and the host side included)

With --thresholds a,b,c the draws (split + draw_small + draw_large) are timed again for each large_threshold; with
--cpu-reference N the numpy restatement (tests/meshraster_ref.py) draws the first N views, wall time in seconds, and its
buffers are compared with the GPU's.

    python scripts/bench_meshraster.py [--reps 3] [--views 64] [--thresholds 0,16,64,256,1024,1000000000] [--cpu-reference 1]
                                       [--grid 512]

--grid N meshes the same sphere on an N^3 grid: its faces, and so their pixel boxes, grow as 512 / N, which is how the
large path gets work (at 512 no box holds more than 16 pixels).

Run it under a time limit of its own.  Prints one JSON line: median milliseconds per stage over --reps timed runs after
one warm-up run."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

CHUNK = 8


def staged(pos, faces, proj, H, W, thr, ms, counts):
    """rasterize's steps one by one (meshrender._draw_chunk + resolve), adding each stage's milliseconds to `ms`"""
    import torch
    from neuraludf_amd import _lib
    from neuraludf_amd._lib import call, ptr
    dev, n_verts, n_faces = pos.device, pos.shape[0], faces.shape[0]
    pending = []

    def timed(name, fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = fn()
        b.record()
        pending.append((name, a, b))
        return r

    for s in range(0, proj.shape[0], CHUNK):
        pr = proj[s:s + CHUNK].contiguous()
        c = pr.shape[0]
        scr = torch.empty((c, n_verts, 3), dtype=torch.float64, device=dev)
        npix = torch.empty((c, n_faces), dtype=torch.int32, device=dev)
        zbuf = torch.full((c, H, W), -1, dtype=torch.int64, device=dev)
        depth = torch.empty((c, H, W), dtype=torch.float32, device=dev)
        face = torch.empty((c, H, W), dtype=torch.int32, device=dev)
        bary = torch.empty((c, H, W, 3), dtype=torch.float32, device=dev)
        d = _lib.MeshRaster(pos=ptr(pos), faces=ptr(faces), proj=ptr(pr), scr=ptr(scr), npix=ptr(npix), zbuf=ptr(zbuf),
                            depth=ptr(depth), face=ptr(face), bary=ptr(bary), n_faces=n_faces, n_verts=n_verts, n_views=c,
                            H=H, W=W)
        timed("project", lambda: call("nudf_meshraster_project", d))
        timed("bounds", lambda: call("nudf_meshraster_bounds", d))

        def split():
            flat = npix.reshape(-1)
            entries = torch.nonzero(flat).reshape(-1)
            big = flat[entries] > thr
            return entries[~big].contiguous(), entries[big].contiguous()
        small, large = timed("split", split)
        for name, lst in (("draw_small", small), ("draw_large", large)):
            if lst.numel():
                d.entries, d.n_entries = ptr(lst), lst.numel()
                timed(name, lambda: call("nudf_meshraster_" + name, d))
        timed("resolve", lambda: call("nudf_meshraster_resolve", d))
        counts["small"] += small.numel()
        counts["large"] += large.numel()
        counts["covered"] += int((face >= 0).sum())
        torch.cuda.synchronize()
        for name, a, b in pending:
            ms[name] = ms.get(name, 0.0) + a.elapsed_time(b)
        pending.clear()


def median_ms(runs):
    keys = sorted({k for r in runs for k in r})
    return {k: round(statistics.median(r.get(k, 0.0) for r in runs), 3) for k in keys}


def bench(reps, n_views, thresholds, cpu_views, grid):
    import numpy as np
    import torch
    from neuraludf_amd import meshclean, meshrender
    import bench_chamfer
    import bench_meshclean
    dev = torch.device("cuda:0")
    bench_chamfer.N = grid                                 # 512: the workload; a coarser grid gives the same sphere larger faces
    v, f = bench_chamfer.make_scan(dev, "surface")[:2]
    W, H = bench_meshclean.W, bench_meshclean.H
    mats = bench_meshclean.make_rig(dev)[0][:n_views]
    pos = v.double().contiguous()
    proj = torch.from_numpy(np.ascontiguousarray(mats[:, :3, :])).to(dev)
    normals = meshclean.vertex_normals(v, f, torch.float64)
    g = torch.Generator(device=dev).manual_seed(0)
    images = torch.randint(0, 256, (n_views, H, W, 3), dtype=torch.uint8, device=dev, generator=g)
    gap = 2.0 * meshrender.mean_edge_length(v, f)
    out = dict(grid=grid, verts=int(v.shape[0]), faces=int(f.shape[0]), views=n_views, H=H, W=W, chunk=CHUNK, reps=reps,
               large_threshold=meshrender.LARGE_THRESHOLD, min_gap=round(gap, 4))

    def whole(name, fn, ev):
        ev[name] = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[name][0].record()
        r = fn()
        ev[name][1].record()
        return r

    runs, counts = [], {}
    for rep in range(reps + 1):
        ms, counts, ev = {}, dict(small=0, large=0, covered=0), {}
        staged(pos, f, proj, H, W, meshrender.LARGE_THRESHOLD, ms, counts)
        r = whole("rasterize", lambda: meshrender.rasterize(v, f, mats, H, W, CHUNK), ev)
        del r
        vis = whole("visibility", lambda: meshrender.vertex_visibility(v, f, mats, H, W, gap, CHUNK), ev)
        colors, seen = whole("colour", lambda: meshrender.color_vertices(v, f, mats, images, normals, 1.0, gap), ev)
        torch.cuda.synchronize()
        ms.update({k: a.elapsed_time(b) for k, (a, b) in ev.items()})
        if rep:
            runs.append(ms)
    out.update(ms=median_ms(runs), entries_small=counts["small"], entries_large=counts["large"],
               covered_pixels=counts["covered"], visible_pairs=int(vis.sum()), vertices_seen=int((seen > 0).sum()))
    del vis, colors, seen, images
    if thresholds:
        sweep = {}
        for thr in thresholds:
            tr = []
            for rep in range(reps + 1):
                ms, cn = {}, dict(small=0, large=0, covered=0)
                staged(pos, f, proj, H, W, thr, ms, cn)
                if rep:
                    tr.append(ms)
            m = median_ms(tr)
            sweep[str(thr)] = dict(split=m.get("split", 0.0), draw_small=m.get("draw_small", 0.0),
                                   draw_large=m.get("draw_large", 0.0), entries_large=cn["large"],
                                   draws=round(m.get("split", 0.0) + m.get("draw_small", 0.0) + m.get("draw_large", 0.0), 3))
        out["threshold_sweep_ms"] = sweep
    if cpu_views:
        import meshraster_ref as R
        got = meshrender.rasterize(v, f, mats[:cpu_views], H, W, CHUNK)
        import threading
        vn, fn, done = pos.cpu().numpy(), f.cpu().numpy(), threading.Event()

        def alive():                                       # minutes of plain loops: say so once a minute
            while not done.wait(60.0):
                print("bench_meshraster: the numpy restatement is still drawing", file=sys.stderr, flush=True)
        threading.Thread(target=alive, daemon=True).start()
        t = time.perf_counter()
        want = R.rasterize(vn, fn, mats[:cpu_views], H, W)
        done.set()
        out["cpu_reference"] = dict(views=cpu_views, rasterize_s=round(time.perf_counter() - t, 1),
                                    **{name + "_equal": bool(g_.cpu().numpy().tobytes() == w.tobytes())
                                       for name, g_, w in zip(("depth", "face", "bary"), got, want)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--thresholds", default="", help="comma-separated large_threshold values to time the draws with")
    ap.add_argument("--cpu-reference", type=int, default=0, metavar="N", help="restate the first N views in numpy (slow)")
    ap.add_argument("--grid", type=int, default=512, help="resolution of the sphere's grid (coarser: larger faces)")
    a = ap.parse_args()
    thresholds = [int(t) for t in a.thresholds.split(",") if t.strip()]
    out = dict(bench="meshraster", device="cuda:0")
    out["sphere%d" % a.grid] = bench(a.reps, a.views, thresholds, a.cpu_reference, a.grid)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
