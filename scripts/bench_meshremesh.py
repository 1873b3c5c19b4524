"""Time the GPU isotropic remeshing (neuraludf_amd/meshclean.py remesh_isotropic, csrc/meshremesh.hip) with HIP events, on
the mesh of scripts/bench_chamfer.py: the radius-280 sphere at 512^3 in a 600 mm box (1.07 M vertices, 2.14 M faces), with
target_edge at twice its mean edge.

    remesh              the whole call, --iterations iterations with the projection
    stages              per iteration, from the events the driver records: split, collapse and flip (their sub-rounds with
                        the tables, sorts and compaction between the launches), relax, project
    rounds              per iteration the sub-rounds' candidates and winners
    quality             share of the edges within [0.8 L, 4/3 L], smallest and mean triangle quality, before and after

With --cpu-reference the numpy restatement (tests/meshremesh_ref.py) on the 1280-face sphere of the tests, wall time in
seconds, next to the GPU's time on the same input.

    python scripts/bench_meshremesh.py [--reps 3] [--iterations 3] [--cpu-reference]

Run it under a time limit of its own.  Prints one JSON line: median milliseconds over --reps timed runs after one warm-up
run."""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench_meshsmooth import EXTRACTION_MS_512, timed  # noqa: E402


def quality(v, f, target):
    """(share of the edges within [0.8 L, 4/3 L], smallest and mean of 4 sqrt(3) area / sum of squared edges, mean edge)"""
    import torch
    from neuraludf_amd import meshclean as C
    e = C.mesh_edges(f, v.shape[0]).edges
    e = e[e[:, 0] != e[:, 1]]
    p = v.double()
    length = (p[e[:, 0]] - p[e[:, 1]]).norm(dim=1)
    share = float(((length >= 0.8 * target) & (length <= target * 4 / 3)).double().mean())
    p0, p1, p2 = p[f[:, 0]], p[f[:, 1]], p[f[:, 2]]
    area = 0.5 * torch.linalg.cross(p1 - p0, p2 - p0).norm(dim=1)
    q = 4.0 * math.sqrt(3.0) * area / ((p0 - p1).pow(2).sum(1) + (p1 - p2).pow(2).sum(1) + (p2 - p0).pow(2).sum(1))
    return dict(share=round(share, 4), min_quality=round(float(q.min()), 4), mean_quality=round(float(q.mean()), 4),
                mean_edge=float(length.mean()))


def sphere(reps, iterations):
    import torch
    import bench_chamfer
    from neuraludf_amd import meshclean as C
    dev = torch.device("cuda:0")
    v, f = bench_chamfer.make_scan(dev, "surface")[:2]
    target = 2.0 * quality(v, f, 1.0)["mean_edge"]
    ms = dict(remesh=timed(lambda: C.remesh_isotropic(v, f, target, iterations), reps),
              no_projection=timed(lambda: C.remesh_isotropic(v, f, target, iterations, project=False), reps))
    info = dict(events={})
    out = C.remesh_isotropic(v, f, target, iterations, _info=info)
    torch.cuda.synchronize()
    stages = {r: {k: round(a.elapsed_time(b), 3) for k, (a, b) in ev.items()} for r, ev in info["events"].items()}
    rounds = [dict(collapse=[(r["candidates"], r["winners"]) for r in log["collapse"]],
                   flip=[(r["candidates"], r["winners"]) for r in log["flip"]]) for log in info["rounds"]]
    return dict(verts=int(v.shape[0]), faces=int(f.shape[0]), target_edge=target, iterations=iterations, reps=reps, ms=ms,
                stages_ms=stages, rounds=rounds, split=out.split, collapsed=out.collapsed, flipped=out.flipped,
                out_verts=int(out.verts.shape[0]), out_faces=int(out.faces.shape[0]),
                quality=dict(before=quality(v, f, target), after=quality(out.verts, out.faces, target)),
                share_of_extraction={k: round(x / EXTRACTION_MS_512, 3) for k, x in ms.items()})


def cpu_reference(reps):
    """the restatement and the GPU on the noisy 1280-face sphere of the tests"""
    import numpy as np
    import torch
    import meshremesh_ref as R
    from neuraludf_amd import meshclean as C
    v, f = R.meshes()["sphere"]
    target = 1.5 * R.mean_edge(v, f)
    dev = torch.device("cuda:0")
    vt, ft = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    t = time.perf_counter()
    want = R.remesh_isotropic(v, f, target, iterations=3)
    wall = round(time.perf_counter() - t, 4)
    ms = timed(lambda: C.remesh_isotropic(vt, ft, target, iterations=3), reps)
    got = C.remesh_isotropic(vt, ft, target, iterations=3)
    equal = bool(np.array_equal(got.verts.cpu().numpy(), want.verts) and np.array_equal(got.faces.cpu().numpy(), want.faces))
    before, after = R.quality(v, f, target), R.quality(want.verts, want.faces, target)
    return dict(verts=len(v), faces=len(f), target_edge=target, numpy_s=wall, gpu_ms=ms, equal=equal,
                quality=dict(before=before, after=after))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--iterations", type=int, default=3)
    ap.add_argument("--cpu-reference", action="store_true")
    ap.add_argument("--skip-sphere", action="store_true")
    a = ap.parse_args()
    out = dict(bench="meshremesh", device="cuda:0")
    if not a.skip_sphere:
        out["sphere512"] = sphere(a.reps, a.iterations)
    if a.cpu_reference:
        out["sphere1280"] = cpu_reference(a.reps)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
