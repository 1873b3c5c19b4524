"""Time the GPU mesh smoothing and denoising (neuraludf_amd/meshclean.py smooth_mesh / denoise_mesh,
csrc/meshsmooth.hip) with HIP events, on the mesh of scripts/bench_chamfer.py: the radius-280 sphere at 512^3 in a 600 mm
box (1.07 M vertices, 2.14 M faces).

    adjacency   vertex_adjacency from a ready edge table: both directions, one stable sort, a count and a scan
    edges       the edge table itself (meshclean._mesh_edges), which the border mask and the adjacency share
    corners     the corner lists: a stable sort of the 3 F corners' vertices, a count and a scan
    uniform     one Laplacian step, uniform weights, one thread per vertex
    cotangent   one Laplacian step, cotangent weights
    frames      normals, areas and centres of the faces, one thread per face
    normals     one bilateral step on the face normals, one thread per face
    update      one vertex step towards the filtered normals, one thread per vertex
    smooth_mesh, smooth_mesh_cotangent, denoise_mesh   the whole calls with their default arguments

With --cpu-reference the numpy restatement (tests/meshsmooth_ref.py) on the 1280-face sphere of the tests, wall time in
seconds, next to the GPU's time on the same input.

    python scripts/bench_meshsmooth.py [--reps 3] [--cpu-reference]

Run it under a time limit of its own.  Prints one JSON line: median milliseconds over --reps timed runs after one warm-up
run."""
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

EXTRACTION_MS_512 = 675.0        # the dense extraction at N = 512, the yardstick of the mesh half


def timed(fn, reps):
    """median milliseconds of fn() over `reps` runs after one warm-up run, by HIP events"""
    import torch
    ms = []
    for rep in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if rep:
            ms.append(a.elapsed_time(b))
    return round(statistics.median(ms), 3)


def stages(v, f, reps):
    import torch
    from neuraludf_amd import _lib, meshclean as C
    from neuraludf_amd._lib import call, ptr
    n_verts, n_faces, dev = v.shape[0], f.shape[0], v.device
    out = {}
    out["edges"] = timed(lambda: C._mesh_edges(f, n_verts), reps)
    table = C._mesh_edges(f, n_verts)
    out["adjacency"] = timed(lambda: C._vertex_adjacency(f, n_verts, table), reps)
    out["corners"] = timed(lambda: C._corner_lists(f, n_verts), reps)
    nbr_off, nbr = C._vertex_adjacency(f, n_verts, table)
    corner_off, corner = C._corner_lists(f, n_verts)
    pos = v.double().contiguous()
    other = torch.empty_like(pos)
    d = _lib.MeshOrient(faces=ptr(f), pos=ptr(pos), corner_off=ptr(corner_off), corner=ptr(corner), n_faces=n_faces,
                        n_verts=n_verts, sm_nbr_off=ptr(nbr_off), sm_nbr=ptr(nbr), sm_n_nbr=nbr.numel(), sm_step=0.5,
                        sm_pos_out=ptr(other))
    for name, w in (("uniform", 0), ("cotangent", 1)):
        d.sm_weights = w
        out[name] = timed(lambda: call("nudf_meshsmooth_laplace", d), reps)
    out["frames"] = timed(lambda: C._face_frames(d, n_faces, dev), reps)
    fnormal, area, centre = C._face_frames(d, n_faces, dev)
    filtered = torch.empty_like(fnormal)
    sigma_c = C._mean_edge_length(pos, table)
    d.sm_fnormal, d.sm_fnormal_out = ptr(fnormal), ptr(filtered)
    d.sm_inv2sc, d.sm_inv2ss = 1.0 / (2.0 * sigma_c * sigma_c), 1.0 / (2.0 * 0.35 * 0.35)
    out["normals"] = timed(lambda: call("nudf_meshsmooth_normals", d), reps)
    d.sm_fnormal = ptr(filtered)
    out["update"] = timed(lambda: call("nudf_meshsmooth_update", d), reps)
    out["smooth_mesh"] = timed(lambda: C.smooth_mesh(v, f), reps)
    out["smooth_mesh_cotangent"] = timed(lambda: C.smooth_mesh(v, f, weights="cotangent"), reps)
    out["denoise_mesh"] = timed(lambda: C.denoise_mesh(v, f), reps)
    facts = dict(sigma_c=round(sigma_c, 4), neighbours=int(nbr.numel()),
                 share_of_extraction={k: round(out[k] / EXTRACTION_MS_512, 3) for k in ("smooth_mesh", "smooth_mesh_cotangent",
                                                                                      "denoise_mesh")})
    return out, facts


def sphere(reps):
    import torch
    import bench_chamfer
    dev = torch.device("cuda:0")
    v, f = bench_chamfer.make_scan(dev, "surface")[:2]
    ms, facts = stages(v, f, reps)
    return dict(verts=int(v.shape[0]), faces=int(f.shape[0]), reps=reps, ms=ms, **facts)


def cpu_reference(reps):
    """the restatement and the GPU on the noisy 1280-face sphere of the tests"""
    import numpy as np
    import torch
    import meshsmooth_ref as S
    from neuraludf_amd import meshclean as C
    v, f = S.noisy_sphere()
    wall = {}
    t = time.perf_counter()
    want_smooth = S.smooth_mesh(v, f)
    wall["smooth_mesh"] = round(time.perf_counter() - t, 4)
    t = time.perf_counter()
    want_pos, want_fn = S.denoise_mesh(v, f)
    wall["denoise_mesh"] = round(time.perf_counter() - t, 4)
    dev = torch.device("cuda:0")
    vt, ft = torch.from_numpy(v).to(dev), torch.from_numpy(np.ascontiguousarray(f)).to(dev)
    ms = dict(smooth_mesh=timed(lambda: C.smooth_mesh(vt, ft), reps), denoise_mesh=timed(lambda: C.denoise_mesh(vt, ft), reps))
    pos, fn = C.denoise_mesh(vt, ft)
    return dict(verts=len(v), faces=len(f), numpy_s=wall, gpu_ms=ms,
                smooth_equal=bool(np.array_equal(C.smooth_mesh(vt, ft).cpu().numpy(), want_smooth)),
                denoise_max_position_difference=float(np.abs(pos.cpu().numpy() - want_pos).max()),
                denoise_max_normal_difference=float(np.abs(fn.cpu().numpy() - want_fn).max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cpu-reference", action="store_true")
    ap.add_argument("--skip-sphere", action="store_true")
    a = ap.parse_args()
    out = dict(bench="meshsmooth", device="cuda:0")
    if not a.skip_sphere:
        out["sphere512"] = sphere(a.reps)
    if a.cpu_reference:
        out["sphere1280"] = cpu_reference(a.reps)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
