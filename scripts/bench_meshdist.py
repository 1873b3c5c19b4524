"""Time the exact point-to-mesh distance (neuraludf_amd/evaluation.py MeshIndex / closest_on_mesh / mesh_deviation,
csrc/meshdist.hip) with HIP events per stage, on the mesh of scripts/bench_chamfer.py: the radius-280 sphere at 512^3 in
a 600 mm box (1.07 M vertices, 2.14 M faces; h = the grid spacing).

    count, scan, emit, sort, cells      the index: the two binning kernels, torch's scan and stable sort between and
                                        after them, the cell table with its hash (nudf_pc_cells)
    query_sort, closest                 the queries' cell keys and their sort; the search kernel

    (a) queries     1 M of the mesh's own vertices, each displaced by up to 2 h along every axis; beside it the existing
                    way to the same information: sample_mesh at density h / 2, then nearest() to the samples (its error
                    against the exact distance is reported)
    (b) deviation   mesh_deviation of the sphere against its simplify_mesh at cells of 2 h and 8 h (vertices only)
    (c) factor      MESH_CELL_FACTOR swept: index and search time, references and cells, on (a)'s queries, and the
                    whole mesh_deviation call of (b) at 2 h, whose queries lie on or next to the surface

    python scripts/bench_meshdist.py [--reps 5] [--out profiles/meshdist_bench.json]

Run it under a time limit of its own.  Writes one JSON document (and prints it): median milliseconds per stage over
--reps timed runs after one warm-up run."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench_meshclean import median_ms      # noqa: E402

FACTORS = (0.5, 1.0, 2.0, 3.0, 4.0, 6.0, 8.0)
N_QUERY = 1_000_000


def _ms(events):
    return {k: a.elapsed_time(b) for k, (a, b) in events.items()}


def time_closest(v, f, q, reps, cell=None, factor=None):
    """-> (median ms per stage, index, Closest of the last run)"""
    import torch
    from neuraludf_amd import evaluation as E
    runs = []
    if factor is not None:
        saved, E.MESH_CELL_FACTOR = E.MESH_CELL_FACTOR, factor
    try:
        for rep in range(reps + 1):
            ev = {}
            index = E.MeshIndex(v, f, cell=cell, _events=ev)
            out = index.closest(q, _events=ev)
            torch.cuda.synchronize()
            if rep:
                ms = _ms(ev)
                ms["index"] = sum(ms[k] for k in ("count", "scan", "emit", "sort", "cells"))
                ms["total"] = ms["index"] + ms["query_sort"] + ms["closest"]
                runs.append(ms)
    finally:
        if factor is not None:
            E.MESH_CELL_FACTOR = saved
    return median_ms(runs), index, out


def time_samples(v, f, q, density, reps):
    """the existing way: sample the mesh, then nearest sample -> (median ms, distances, sample count)"""
    import torch
    from neuraludf_amd import evaluation as E
    runs = []
    for rep in range(reps + 1):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        pts = E.sample_mesh(v, f, density)
        ev[1].record()
        dist, _ = E.nearest(q, pts)
        ev[2].record()
        torch.cuda.synchronize()
        if rep:
            runs.append(dict(sample=ev[0].elapsed_time(ev[1]), nearest=ev[1].elapsed_time(ev[2]),
                             total=ev[0].elapsed_time(ev[2])))
    return median_ms(runs), dist, int(pts.shape[0])


def time_deviation(v, f, cell, reps, factor=None):
    """mesh_deviation(input, its simplification at `cell`), vertices only: both indices built, both directions searched"""
    import torch
    from neuraludf_amd import evaluation as E, meshclean as C
    s = C.simplify_mesh(v, f, cell)
    sv = s.verts.double()
    runs = []
    if factor is not None:
        saved, E.MESH_CELL_FACTOR = E.MESH_CELL_FACTOR, factor
    try:
        for rep in range(reps + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            dev = E.mesh_deviation((v, f), (sv, s.faces))
            b.record()
            torch.cuda.synchronize()
            if rep:
                runs.append(dict(total=a.elapsed_time(b)))
    finally:
        if factor is not None:
            E.MESH_CELL_FACTOR = saved
    return dict(cell=round(cell, 4), faces_out=int(s.faces.shape[0]), ms=median_ms(runs), deviation=dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "meshdist_bench.json"))
    a = ap.parse_args()
    import torch
    import bench_chamfer
    from neuraludf_amd import build, evaluation as E
    dev = torch.device("cuda:0")
    v, f = bench_chamfer.make_scan(dev, "surface")[:2]
    v = v.double().contiguous()
    h = 2.0 * bench_chamfer.BOX / (bench_chamfer.N - 1)
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    rows = torch.randperm(v.shape[0], generator=g, device=dev)[:N_QUERY]
    q = v[rows] + (torch.rand((rows.numel(), 3), generator=g, device=dev, dtype=torch.float64) * 2 - 1) * (2 * h)
    out = dict(bench="meshdist", device=torch.cuda.get_device_name(0), source_digest=build.source_digest("meshdist"),
               verts=int(v.shape[0]), faces=int(f.shape[0]), h=h, queries=int(q.shape[0]), reps=a.reps)
    # (a)
    ms, index, c = time_closest(v, f, q, a.reps)
    out["queries_2h"] = dict(ms=ms, cell=index.cell, cell_over_h=index.cell / h, grid=index.grid, refs=index.n_refs,
                             cells=index.n_cells, refs_per_face=index.n_refs / f.shape[0],
                             refs_per_cell=index.n_refs / index.n_cells, mean_dist_over_h=float(c.dist.mean()) / h,
                             max_dist_over_h=float(c.dist.max()) / h,
                             queries_per_s=q.shape[0] / (ms["closest"] * 1e-3))
    ms_s, d_s, n_s = time_samples(v, f, q, h / 2, a.reps)
    err = d_s - c.dist
    out["samples_h_over_2"] = dict(ms=ms_s, samples=n_s, bytes=24 * n_s, mean_excess_over_h=float(err.mean()) / h,
                                   max_excess_over_h=float(err.max()) / h, min_excess_over_h=float(err.min()) / h)
    del d_s, err, c, index
    # (b)
    out["deviation"] = [dict(spacings=k, **time_deviation(v, f, k * h, a.reps)) for k in (2, 8)]
    # (c)
    sweep = []
    for factor in FACTORS:
        ms, index, _ = time_closest(v, f, q, a.reps, factor=factor)
        sweep.append(dict(factor=factor, cell_over_h=index.cell / h, refs=index.n_refs, cells=index.n_cells,
                          refs_per_cell=index.n_refs / index.n_cells, ms=ms,
                          deviation_2h_ms=time_deviation(v, f, 2 * h, a.reps, factor=factor)["ms"]["total"]))
        del index
    out["factor_sweep"] = sweep
    out["default_factor"] = E.MESH_CELL_FACTOR
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text + "\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
