"""Time the GPU mesh simplification (neuraludf_amd/meshclean.py simplify_mesh, csrc/meshsimplify.hip) with HIP events per
stage, on the mesh of scripts/bench_chamfer.py: the radius-280 sphere at 512^3 in a 600 mm box (1.07 M vertices, 2.14 M
faces), with cells of 2, 4 and 8 grid spacings and both placements.

    keys      the key kernel, one thread per vertex
    sorts     the stable sort of the keys, the vertex and corner lists of the clusters (a stable sort of the 3 F corners'
              clusters, a count and a scan) and, with boundary quadrics, the edge table (meshclean._mesh_edges)
    place     the placement kernel, one thread per cluster: 72 B of vertex positions gathered per corner
    faces     the face kernel, one thread per face
    dedupe    the two stable sorts of the surviving faces' id triples and the first-of-run selection
    compact   compact_mesh over the cluster ids and the gathers of the outputs

With --cpu-reference the numpy restatement (tests/meshsimplify_ref.py) on the marching-cubes sphere at resolution 24, wall
time in seconds, next to the GPU's time on the same input, and whether the two agree.

    python scripts/bench_meshsimplify.py [--reps 5] [--cpu-reference]

Run it under a time limit of its own.  Prints one JSON line: median milliseconds per stage over --reps timed runs after
one warm-up run."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench_meshclean import median_ms      # noqa: E402

SPACINGS = (2, 4, 8)


def time_mesh(v, f, cell, placement, reps):
    """-> (median ms per stage and in total, facts about the result)"""
    import torch
    from neuraludf_amd import meshclean as C
    runs, info = [], {}
    for rep in range(reps + 1):
        info = dict(events={})
        whole = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        whole[0].record()
        out = C.simplify_mesh(v, f, cell, placement=placement, _info=info)
        whole[1].record()
        torch.cuda.synchronize()
        if rep:
            runs.append(dict({k: a.elapsed_time(b) for k, (a, b) in info["events"].items()},
                             total=whole[0].elapsed_time(whole[1])))
    corners = 3 * int(f.shape[0])
    facts = dict(cell=round(cell, 4), placement=placement, clusters=info["clusters"], grid=info["grid"],
                 verts_out=int(out.verts.shape[0]), faces_out=int(out.faces.shape[0]), fallbacks=info["fallbacks"],
                 corners_per_cluster=round(corners / max(info["clusters"], 1), 1))
    ms = median_ms(runs)
    if placement == "quadric" and ms["place"] > 0:
        # what the corner walk asks for: three positions (72 B), the face (24 B), the corner id (8 B) and two edge-table
        # look-ups (2 x 16 B) per corner; most of it is served on die, so this is demand, not HBM traffic
        facts["place_demand_gb_s"] = round(corners * (72 + 24 + 8 + 32) / (ms["place"] * 1e-3) / 1e9, 1)
    return ms, facts


def sphere(reps):
    import torch
    import bench_chamfer
    dev = torch.device("cuda:0")
    v, f = bench_chamfer.make_scan(dev, "surface")[:2]
    h = 2.0 * bench_chamfer.BOX / (bench_chamfer.N - 1)
    rows = []
    for k in SPACINGS:
        for placement in ("quadric", "mean"):
            ms, facts = time_mesh(v, f, k * h, placement, reps)
            rows.append(dict(spacings=k, ms=ms, **facts))
    return dict(verts=int(v.shape[0]), faces=int(f.shape[0]), reps=reps, runs=rows)


def cpu_reference(reps):
    """the restatement and the GPU on the resolution-24 sphere"""
    import numpy as np
    import torch
    import meshsimplify_ref as S
    from neuraludf_amd import meshclean as C
    case = S.cases()["sphere"]
    t = time.perf_counter()
    want = S.simplify(case["v"], case["f"], case["cell"])
    wall = time.perf_counter() - t
    dev = torch.device("cuda:0")
    v, f = torch.from_numpy(np.array(case["v"])).to(dev), torch.from_numpy(np.array(case["f"])).to(dev)
    ms, facts = time_mesh(v, f, case["cell"], "quadric", reps)
    got = C.simplify_mesh(v, f, case["cell"])
    return dict(verts=len(case["v"]), faces=len(case["f"]), numpy_s=round(wall, 4), gpu_ms=ms["total"], faces_out=facts["faces_out"],
                equal=bool(np.array_equal(got.faces.cpu().numpy(), want.faces) and
                           np.array_equal(got.accepted.cpu().numpy(), want.accepted)),
                max_position_error=float(np.abs(got.verts.cpu().numpy() - want.verts).max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu-reference", action="store_true")
    ap.add_argument("--skip-sphere", action="store_true")
    a = ap.parse_args()
    out = dict(bench="meshsimplify", device="cuda:0")
    if not a.skip_sphere:
        out["sphere512"] = sphere(a.reps)
    if a.cpu_reference:
        out["sphere24"] = cpu_reference(a.reps)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
