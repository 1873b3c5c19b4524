"""Time the GPU hole closing (neuraludf_amd/meshclean.py border_loops / close_holes, csrc/meshhole.hip) with HIP events, on
the mesh of scripts/bench_chamfer.py: the radius-280 sphere at 512^3 in a 600 mm box (1.07 M vertices, 2.14 M faces), with
--holes holes of mixed length punched into it: the faces whose centroid lies within r of a point of a Fibonacci lattice on
the sphere are left out, r cycling through 0.6 ... 6 grid spacings, which gives rims from 3 edges to more than 64, some of
them pinched (a loop through a vertex twice).

    close_holes, border_loops     the whole calls
    stages                        from the events the driver records: edges (the edge table), link, rank (all rounds),
                                  count, triangulate, and glue: the sorts and scans in torch between them, summed

    python scripts/bench_meshhole.py [--reps 3] [--holes 3000]

Run it under a time limit of its own.  Prints one JSON line: median milliseconds over --reps timed runs after one warm-up
run."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench_meshsmooth import EXTRACTION_MS_512, timed  # noqa: E402

RADII = (0.6, 0.9, 1.3, 1.8, 2.4, 3.0, 4.0, 5.0, 6.0)        # in grid spacings; the lattice points lie about 15 apart


def punch(v, f, n_holes, h):
    """the faces that survive: centroid further than r_i from every lattice point i"""
    import torch
    dev = v.device
    i = torch.arange(n_holes, dtype=torch.float64, device=dev) + 0.5
    z = 1.0 - 2.0 * i / n_holes
    phi = i * (math.pi * (3.0 - math.sqrt(5.0)))
    s = torch.sqrt(1.0 - z * z)
    radius = float(v.double().norm(dim=1).mean())
    seeds = (torch.stack([s * torch.cos(phi), s * torch.sin(phi), z], 1) * radius).float()
    r = torch.tensor(RADII, dtype=torch.float32, device=dev)[torch.arange(n_holes, device=dev) % len(RADII)] * h
    centroid = v[f].float().mean(1)
    keep = torch.ones(f.shape[0], dtype=torch.bool, device=dev)
    for b in range(0, f.shape[0], 1 << 15):
        keep[b:b + (1 << 15)] = (torch.cdist(centroid[b:b + (1 << 15)], seeds) > r[None, :]).all(1)
    return f[keep].contiguous()


def sphere(reps, n_holes):
    import torch
    import bench_chamfer
    from neuraludf_amd import meshclean as C
    dev = torch.device("cuda:0")
    v, f = bench_chamfer.make_scan(dev, "surface")[:2]
    h = 2.0 * bench_chamfer.BOX / (bench_chamfer.N - 1)
    g = punch(v, f, n_holes, h)
    ms = dict(close_holes=timed(lambda: C.close_holes(v, g, 64), reps), border_loops=timed(lambda: C.border_loops(v, g), reps))
    runs = []
    for _ in range(reps + 1):
        info = dict(events={})
        out = C.close_holes(v, g, 64, _info=info)
        torch.cuda.synchronize()
        ev = {k: a.elapsed_time(b) for k, (a, b) in info["events"].items()}
        runs.append(dict(edges=ev["edges"], link=ev["link"], rank=ev["rank"], count=ev["count"], triangulate=ev["triangulate"],
                         glue=sum(x for k, x in ev.items() if k.startswith("glue"))))
    stages = {k: round(sorted(r[k] for r in runs[1:])[len(runs[1:]) // 2], 3) for k in runs[0]}
    loops = info["loops"]
    n = (loops.loop_off[1:] - loops.loop_off[:-1])
    tally = torch.bincount(out.status.long(), minlength=len(C.HOLE_STATUS_NAMES)).tolist()
    again = C.close_holes(v, g, 64)
    facts = dict(faces_removed=int(f.shape[0] - g.shape[0]), border_edges=int(n.sum()), loops=int(n.numel()),
                 rank_rounds=(2 * int(n.sum()) - 1).bit_length() + 1, longest_loop=int(n.max()),
                 loops_by_status={C.HOLE_STATUS_NAMES[k]: c for k, c in enumerate(tally) if c},
                 new_faces=int(out.faces.shape[0] - g.shape[0]), identical_rerun=bool(torch.equal(again.faces, out.faces)))
    return dict(verts=int(v.shape[0]), faces=int(g.shape[0]), reps=reps, holes=n_holes, ms=ms, stages_ms=stages,
                share_of_extraction={k: round(x / EXTRACTION_MS_512, 3) for k, x in ms.items()}, **facts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--holes", type=int, default=3000)
    a = ap.parse_args()
    print(json.dumps(dict(bench="meshhole", device="cuda:0", sphere512=sphere(a.reps, a.holes))))
    return 0


if __name__ == "__main__":
    sys.exit(main())
