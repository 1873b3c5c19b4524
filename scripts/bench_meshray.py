"""Time rays against a mesh (neuraludf_amd/evaluation.py MeshIndex.cast, csrc/meshray.hip) with HIP events per stage, on
the mesh of scripts/bench_chamfer.py: the radius-280 sphere at 512^3 in a 600 mm box (1.07 M vertices, 2.14 M faces;
h = the grid spacing).

    ray_sort, cast      the rays' cells of entry and their sort; the walk kernel

    (a) camera      the 1000 x 1000 pixel-centre rays of a pinhole camera 900 mm from the centre (the sphere fills most of
                    the image), in the three modes; beside it meshrender.rasterize of the same view: the same nearest
                    face per pixel by projection, as context
    (b) random      1 M rays from uniform origins in the box along uniform directions, in the three modes
    (c) factor      the cell factor swept on (a) and (b), mode "first": index time, ray_sort and cast

    python scripts/bench_meshray.py [--reps 5] [--out profiles/meshray_bench.json]

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
SIDE = 1000                                 # the camera's image: SIDE x SIDE rays
CAMERA_Z, FOCAL = -900.0, 1400.0
MODES = ("first", "any", "count")


def _ms(events):
    return {k: a.elapsed_time(b) for k, (a, b) in events.items()}


def time_index(v, f, reps, factor):
    import torch
    from neuraludf_amd import evaluation as E
    runs = []
    saved, E.MESH_CELL_FACTOR = E.MESH_CELL_FACTOR, factor
    try:
        for rep in range(reps + 1):
            ev = {}
            index = E.MeshIndex(v, f, _events=ev)
            torch.cuda.synchronize()
            if rep:
                runs.append(dict(index=sum(_ms(ev).values())))
    finally:
        E.MESH_CELL_FACTOR = saved
    return median_ms(runs)["index"], index


def time_cast(index, o, d, mode, reps):
    """-> (median ms per stage, the result of the last run)"""
    import torch
    runs = []
    for rep in range(reps + 1):
        ev = {}
        out = index.cast(o, d, mode=mode, _events=ev)
        torch.cuda.synchronize()
        if rep:
            ms = _ms(ev)
            ms["total"] = ms["ray_sort"] + ms["cast"]
            runs.append(ms)
    return median_ms(runs), out


def time_raster(v, f, world, reps):
    import torch
    from neuraludf_amd import meshrender
    runs = []
    for rep in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = meshrender.rasterize(v, f, world, SIDE, SIDE)
        b.record()
        torch.cuda.synchronize()
        if rep:
            runs.append(dict(total=a.elapsed_time(b)))
    return median_ms(runs), r


def summary(mode, out):
    if mode == "first":
        return dict(hit_share=float((out.face >= 0).double().mean()))
    if mode == "any":
        return dict(hit_share=float(out.double().mean()))
    return dict(mean_count=float(out.double().mean()), max_count=int(out.max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "meshray_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import bench_chamfer
    from neuraludf_amd import build, evaluation as E
    dev = torch.device("cuda:0")
    v, f = bench_chamfer.make_scan(dev, "surface")[:2]
    v = v.double().contiguous()
    h = 2.0 * bench_chamfer.BOX / (bench_chamfer.N - 1)
    centre = 0.5 * (v.amax(0) + v.amin(0))
    # (a) the camera looks along +z at the sphere's centre; pixel (px, py) is the screen point (px, py)
    c = (SIDE - 1) / 2.0
    K = np.array([[FOCAL, 0.0, c], [0.0, FOCAL, c], [0.0, 0.0, 1.0]])
    C = centre.cpu().numpy() + np.array([0.0, 0.0, CAMERA_Z])
    world = np.eye(4)
    world[:3, :3], world[:3, 3] = K, -K @ C
    py, px = torch.meshgrid(torch.arange(SIDE, dtype=torch.float64, device=dev),
                            torch.arange(SIDE, dtype=torch.float64, device=dev), indexing="ij")
    cam_d = torch.stack([(px.reshape(-1) - c) / FOCAL, (py.reshape(-1) - c) / FOCAL, torch.ones(SIDE * SIDE, device=dev,
                                                                                               dtype=torch.float64)], -1)
    cam_o = torch.from_numpy(C).to(dev).expand(SIDE * SIDE, 3).contiguous()
    # (b)
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    n = SIDE * SIDE
    rnd_o = centre + (torch.rand((n, 3), generator=g, device=dev, dtype=torch.float64) * 2 - 1) * bench_chamfer.BOX
    rnd_d = torch.randn((n, 3), generator=g, device=dev, dtype=torch.float64)
    out = dict(bench="meshray", device=torch.cuda.get_device_name(0), source_digest=build.source_digest("meshray"),
               verts=int(v.shape[0]), faces=int(f.shape[0]), h=h, rays=n, reps=a.reps, default_factor=E.MESH_CELL_FACTOR)
    index_ms, index = time_index(v, f, a.reps, E.MESH_CELL_FACTOR)
    out["index"] = dict(ms=index_ms, cell_over_h=index.cell / h, grid=index.grid, refs=index.n_refs, cells=index.n_cells,
                        refs_per_cell=index.n_refs / index.n_cells)
    for name, (o, d) in (("camera", (cam_o, cam_d)), ("random", (rnd_o, rnd_d))):
        out[name] = {}
        for mode in MODES:
            ms, res = time_cast(index, o, d, mode, a.reps)
            out[name][mode] = dict(ms=ms, rays_per_s=n / (ms["cast"] * 1e-3), **summary(mode, res))
            if name == "camera" and mode == "first":
                first = res
    ms, raster = time_raster(v, f, world[None], a.reps)
    same = (raster.face[0].reshape(-1).long() == first.face)
    out["camera"]["rasterize"] = dict(ms=ms, covered_share=float((raster.face[0] >= 0).double().mean()),
                                      same_face_share=float(same.double().mean()))
    del raster, first, res, index
    # (c)
    sweep = []
    for factor in FACTORS:
        index_ms, index = time_index(v, f, a.reps, factor)
        row = dict(factor=factor, cell_over_h=index.cell / h, refs=index.n_refs, cells=index.n_cells,
                   refs_per_cell=index.n_refs / index.n_cells, index_ms=index_ms)
        for name, (o, d) in (("camera", (cam_o, cam_d)), ("random", (rnd_o, rnd_d))):
            row[name] = time_cast(index, o, d, "first", a.reps)[0]
        sweep.append(row)
        del index
    out["factor_sweep"] = sweep
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text + "\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
