"""Time the GPU Chamfer evaluation (neuraludf_amd/evaluation.py, DTU protocol) on a synthetic DTU-scale scan in mm, with
HIP events per stage:

    mesh       udf_marching_cubes of |r - 280| on a 512^3 grid of a 600 mm box (not part of the evaluation)
    sample     sample_mesh at density 0.2 (tri_count, scan, tri_emit)
    thin       radius_downsample: the seeded shuffle and the thinning rounds
    masks      the ObsMask / box / plane selection
    d2gt       nearest: the down-sampled points inside the ObsMask against the GT cloud
    gt2d       nearest: the GT points above the plane against the down-sampled points in the box
    metrics    means, precision / recall

GT: about 3 M points on the sphere, radially perturbed (sigma 0.3 mm).  ObsMask: Res 2 mm with box-shaped holes; the plane
z > -150 cuts part of the GT.  Variant `outliers`: the sampled cloud (mode pcd) with 5 % of its points moved 5-20 mm off
the surface, the load of the ring search.  Per variant also the nearest-neighbour time at several cell sizes (--targets,
points per occupied cell), and with --cpu-reference the sklearn KD-tree path on the same arrays (radius_neighbors plus the
reference's mask loop, two kneighbors sweeps; n_jobs=16).

    python scripts/bench_chamfer.py [--variants surface outliers] [--reps 3] [--targets 4 8 16 32] [--cpu-reference]
                                    [--timeout 600]

Each variant runs in a child process of its own under a time limit (the parent never opens the GPU); a child that fails
ends the run.  Prints one JSON line: per variant the median milliseconds of each stage over --reps timed runs (after one
warm-up run), the point counts, the thinning rounds and the chosen cell."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

RADIUS, BOX, N = 280.0, 300.0, 512


def make_scan(dev, variant):
    import numpy as np
    import torch
    from neuraludf_amd import meshing
    from neuraludf_amd.models import udf_renderer_blending as rb
    bmin, bmax = (-BOX,) * 3, (BOX,) * 3
    ax = rb._grid_axes(bmin, bmax, N, dev)
    U = torch.empty((N, N, N), dtype=torch.float32, device=dev)
    G = torch.empty((N, N, N, 3), dtype=torch.float32, device=dev)
    for i in range(N):                                     # slab by slab: the full 512^3 x 3 float64 grid is not needed
        X = torch.stack(torch.meshgrid(ax[0][i:i + 1], ax[1], ax[2], indexing="ij"), -1)[0]
        r = X.norm(dim=-1, keepdim=True)
        U[i] = (r - RADIUS).abs()[..., 0]
        G[i] = X / r * torch.sign(r - RADIUS)
    ev = {}
    ev["mesh"] = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    ev["mesh"][0].record()
    v, f = meshing.udf_marching_cubes(U, G, bmin, bmax)
    ev["mesh"][1].record()
    del U, G
    g = torch.Generator(device=dev).manual_seed(1)
    d = torch.randn((3_000_000, 3), generator=g, device=dev, dtype=torch.float64)
    gt = d / d.norm(dim=1, keepdim=True) * (RADIUS + 0.3 * torch.randn((3_000_000, 1), generator=g, device=dev,
                                                                       dtype=torch.float64))
    res = 2.0
    bb = np.array([[-BOX, -BOX, -BOX], [BOX, BOX, BOX]])
    shape = (int(2 * BOX / res) + 1,) * 3
    rng = np.random.default_rng(2)
    obs = np.ones(shape, dtype=bool)
    for _ in range(40):                                     # holes
        c = rng.integers(0, shape[0] - 30, 3)
        obs[c[0]:c[0] + 30, c[1]:c[1] + 30, c[2]:c[2] + 30] = False
    plane = np.array([0.0, 0.0, 1.0, 150.0])
    return v.double(), f, gt, torch.as_tensor(obs, device=dev), bb, res, plane, ev


def child(variant, reps, targets, cpu_reference):
    import numpy as np
    import torch
    from neuraludf_amd import evaluation as E
    dev = torch.device("cuda:0")
    v, f, gt, obs, bb, res, plane, ev0 = make_scan(dev, variant)
    density, patch, max_dist, thr = 0.2, 60.0, 20.0, (1.0, 2.0)
    bound = max(max_dist, *thr)
    runs, sizes = [], {}

    def timed(ev, name, fn):
        ev[name] = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[name][0].record()
        out = fn()
        ev[name][1].record()
        return out

    outliers = None
    for rep in range(reps + 1):
        ev = dict(ev0) if rep == 0 else {}
        pcd = timed(ev, "sample", lambda: E.sample_mesh(v, f, density))
        if variant == "outliers":
            if outliers is None:                    # fixed set: 5 % of the points, 5-20 mm along the radius
                g = torch.Generator(device=dev).manual_seed(3)
                k = pcd.shape[0] // 20
                sel = torch.randperm(pcd.shape[0], generator=g, device=dev)[:k]
                off = 5.0 + 15.0 * torch.rand(k, generator=g, device=dev, dtype=torch.float64)
                sgn = torch.where(torch.rand(k, generator=g, device=dev) < 0.5, -1.0, 1.0).double()
                outliers = (sel, off * sgn)
            sel, off = outliers
            pcd = pcd.clone()
            pcd[sel] += pcd[sel] / pcd[sel].norm(dim=1, keepdim=True) * off[:, None]
        down, info = timed(ev, "thin", lambda: E.radius_downsample(pcd, density, seed=0))
        inbound, rows = timed(ev, "masks", lambda: E.dtu_masks(down, bb, res, obs, patch))
        data_in, data_in_obs = down[inbound], down[rows]
        above = E.above_plane(gt, plane)
        stl_above = gt[above]
        cells = {}
        d2s, _ = timed(ev, "d2gt", lambda: E.nearest(data_in_obs, gt, bound, _events=cells))
        s2d, _ = timed(ev, "gt2d", lambda: E.nearest(stl_above, data_in, bound))
        out = timed(ev, "metrics", lambda: E._metrics(d2s, s2d, max_dist, thr))
        torch.cuda.synchronize()
        if rep:
            runs.append({k: a.elapsed_time(b) for k, (a, b) in ev.items()})
        else:
            mesh_ms = ev["mesh"][0].elapsed_time(ev["mesh"][1])
        sizes = dict(verts=int(v.shape[0]), faces=int(f.shape[0]), n_data=int(pcd.shape[0]), n_down=int(down.shape[0]),
                     n_in=int(data_in.shape[0]), n_in_obs=int(data_in_obs.shape[0]), n_gt=int(gt.shape[0]),
                     n_gt_above=int(stl_above.shape[0]), thinning_rounds=info["rounds"], d2gt_cell_mm=cells["cell"],
                     d2gt_cells=cells["cells"], metrics={k: round(x, 6) for k, x in out.items()})
    ms = {k: round(statistics.median(r[k] for r in runs), 3) for k in runs[0]}
    total = round(sum(ms.values()), 3)
    by_target = {}
    for t in targets:                                         # the cell-size choice: d2gt + gt2d at `t` points per cell
        c1, c2 = E.nearest_cell_size(gt, t), E.nearest_cell_size(data_in, t)
        best = None
        for _ in range(2):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            x, _ = E.nearest(data_in_obs, gt, bound, cell=c1)
            y, _ = E.nearest(stl_above, data_in, bound, cell=c2)
            b.record()
            torch.cuda.synchronize()
            assert torch.equal(x, d2s) and torch.equal(y, s2d)
            best = a.elapsed_time(b) if best is None else min(best, a.elapsed_time(b))
        by_target[str(t)] = dict(ms=round(best, 3), cell_gt_mm=round(c1, 4), cell_data_mm=round(c2, 4))
    result = dict(variant=variant, ms=ms, total_ms=total, mesh_ms=round(mesh_ms, 3), reps=reps, nearest_by_target=by_target,
                  **sizes)
    if cpu_reference:
        result["cpu_reference"] = cpu_reference_times(pcd, info["perm"], down, data_in_obs, gt, stl_above, data_in, d2s,
                                                      s2d, density)
    return result


def cpu_reference_times(pcd, perm, down, data_in_obs, gt, stl_above, data_in, d2s, s2d, density):
    """the reference's sklearn path on the same arrays (seconds), checked against the GPU results"""
    import numpy as np
    try:
        import sklearn.neighbors as skln
    except ImportError:
        return dict(error="sklearn not importable")
    shuffled = pcd[perm].cpu().numpy()
    out = {}
    t = time.perf_counter()
    eng = skln.NearestNeighbors(n_neighbors=1, radius=density, algorithm="kd_tree", n_jobs=16)
    eng.fit(shuffled)
    nbrs = eng.radius_neighbors(shuffled, radius=density, return_distance=False)
    out["radius_neighbors_s"] = round(time.perf_counter() - t, 3)
    t = time.perf_counter()
    mask = np.ones(shuffled.shape[0], dtype=np.bool_)
    for cur, idxs in enumerate(nbrs):
        if mask[cur]:
            mask[idxs] = 0
            mask[cur] = 1
    out["mask_loop_s"] = round(time.perf_counter() - t, 3)
    del nbrs
    out["thin_equal"] = bool(np.array_equal(shuffled[mask], down.cpu().numpy()))
    t = time.perf_counter()
    eng.fit(gt.cpu().numpy())
    dist, _ = eng.kneighbors(data_in_obs.cpu().numpy(), n_neighbors=1, return_distance=True)
    out["d2gt_s"] = round(time.perf_counter() - t, 3)
    t = time.perf_counter()
    eng.fit(data_in.cpu().numpy())
    dist2, _ = eng.kneighbors(stl_above.cpu().numpy(), n_neighbors=1, return_distance=True)
    out["gt2d_s"] = round(time.perf_counter() - t, 3)
    a, b = d2s.cpu().numpy(), s2d.cpu().numpy()
    fa, fb = np.isfinite(a), np.isfinite(b)
    out["d2gt_equal_within_bound"] = bool(np.array_equal(a[fa], dist[fa, 0]) and (dist[~fa, 0] > 20.0).all())
    out["gt2d_equal_within_bound"] = bool(np.array_equal(b[fb], dist2[fb, 0]) and (dist2[~fb, 0] > 20.0).all())
    out["total_s"] = round(out["radius_neighbors_s"] + out["mask_loop_s"] + out["d2gt_s"] + out["gt2d_s"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variants", nargs="+", default=["surface", "outliers"], choices=["surface", "outliers"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--targets", type=int, nargs="*", default=[4, 8, 16, 32])
    ap.add_argument("--cpu-reference", action="store_true")
    ap.add_argument("--timeout", type=float, default=600.0, help="seconds per variant")
    ap.add_argument("--child", type=str, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child is not None:
        print("RESULT " + json.dumps(child(a.child, a.reps, a.targets, a.cpu_reference)))
        return 0
    out = dict(bench="chamfer_dtu", device="cuda:0", variants=[])
    for v in a.variants:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", v, "--reps", str(a.reps), "--targets",
               *map(str, a.targets)] + (["--cpu-reference"] if a.cpu_reference else [])
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
        except subprocess.TimeoutExpired:
            out["error"] = f"{v}: timed out after {a.timeout} s"
            break
        res = [ln[7:] for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not res:
            out["error"] = f"{v}: exit {p.returncode}: {p.stderr[-800:]}"
            break
        out["variants"].append(json.loads(res[-1]))
    print(json.dumps(out))
    return 1 if "error" in out else 0


if __name__ == "__main__":
    sys.exit(main())
