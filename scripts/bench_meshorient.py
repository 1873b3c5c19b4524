"""Time the face orientation and the vertex normals (neuraludf_amd/meshclean.py orient_faces / vertex_normals,
csrc/meshorient.hip) with HIP events, on the meshes of scripts/bench_meshclean.py: the radius-280 sphere at 512^3 with 1 %
of its faces removed (2.1 M faces), and with --network N the mesh of the geometric-init network at resolution N next to
the time of its extraction.

    medges       the key sort of the 3 F half-edges and the list of manifold edges (orient_faces pays it once)
    orient       orient_faces, whole, fewest-flips rule; the number of rounds is reported
    outward      orient_faces, whole, with outward_from (adds the grouping of the faces by component and the sum kernel)
    normals      vertex_normals, whole (corner sort included), float32 output

    python scripts/bench_meshorient.py [--reps 3] [--network 512] [--skip-sphere]

Run it under a time limit of its own.  Prints one JSON line: median milliseconds over --reps timed runs after one warm-up
run."""
import argparse
import contextlib
import io
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench_meshclean import median_ms, separate_faces      # noqa: E402


def time_mesh(v, f, origin, reps):
    """-> (median ms per stage, facts about the result) of the four stages on one mesh"""
    import torch
    from neuraludf_amd import meshclean as C
    info, info_out, runs = {}, {}, []
    for rep in range(reps + 1):
        ev = {}

        def timed(name, fn):
            ev[name] = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            ev[name][0].record()
            r = fn()
            ev[name][1].record()
            return r
        me_a, _ = timed("medges", lambda: C._manifold_edges(f, v.shape[0]))
        got = timed("orient", lambda: C.orient_faces(v, f, _info=info))
        out = timed("outward", lambda: C.orient_faces(v, f, origin, _info=info_out))
        normals = timed("normals", lambda: C.vertex_normals(v, out.faces))
        torch.cuda.synchronize()
        if rep:
            runs.append({k: a.elapsed_time(b) for k, (a, b) in ev.items()})
    pos = v.double()
    tri = pos[out.faces]
    volume = float((tri[:, 0] * torch.linalg.cross(tri[:, 1], tri[:, 2])).sum() / 6.0)
    facts = dict(verts=int(v.shape[0]), faces=int(f.shape[0]), manifold_edges=int(me_a.numel()), rounds=info["rounds"],
                 components=info["components"], non_orientable=info["non_orientable"], flipped=info["flipped"],
                 flipped_outward=info_out["flipped"], signed_volume_outward=round(volume, 4),
                 normals_unit=int((normals.norm(dim=1) > 0.5).sum()))
    return median_ms(runs), facts


def sphere(reps):
    import torch
    import bench_chamfer
    dev = torch.device("cuda:0")
    v, f = bench_chamfer.make_scan(dev, "surface")[:2]
    gone = separate_faces(f, v.shape[0], 0.01)
    keep = torch.ones(f.shape[0], dtype=torch.bool, device=dev)
    keep[gone] = False
    ms, facts = time_mesh(v, f[keep].contiguous(), (0.0, 0.0, 0.0), reps)
    return dict(ms=ms, reps=reps, **facts)


def network(n, reps):
    """orientation and normals of the network's mesh at resolution n beside the extraction that produced it"""
    import torch
    from neuraludf_amd import meshing
    from neuraludf_amd.models import fields
    from neuraludf_amd.train import DTU_MODEL_CONF
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        udf = fields.UDFNetwork(**DTU_MODEL_CONF["udf_network"]).to(dev)
    box = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
    runs = []
    for rep in range(reps + 1):
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record()
        U, G = meshing.udf_grid(udf, n, *box)
        v, f = meshing.udf_marching_cubes(U, G, *box)
        del U, G
        v, f = meshing.filter_mesh(v, f, meshing._query_udf(udf, v), meshing.grid_spacing(*box, n))
        ev[1].record()
        torch.cuda.synchronize()
        if rep:
            runs.append(dict(extract=ev[0].elapsed_time(ev[1])))
    ms, facts = time_mesh(v, f, (0.0, 0.0, 0.0), reps)
    ms.update(median_ms(runs))
    both = round(ms["orient"] + ms["normals"], 3)
    return dict(N=n, ms=ms, orient_plus_normals_ms=both, share_of_extract=round(both / ms["extract"], 4), **facts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--network", type=int, default=0, help="also time the network mesh at this resolution")
    ap.add_argument("--skip-sphere", action="store_true")
    a = ap.parse_args()
    out = dict(bench="meshorient", device="cuda:0")
    if not a.skip_sphere:
        out["sphere512"] = sphere(a.reps)
    if a.network:
        out["network"] = network(a.network, a.reps)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
