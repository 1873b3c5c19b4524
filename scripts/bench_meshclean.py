"""Time the GPU mesh clean-up (neuraludf_amd/meshclean.py, csrc/meshtopo.hip) with HIP events per stage, on the mesh of
scripts/bench_chamfer.py: the radius-280 sphere at 512^3 in a 600 mm box (1.07 M vertices, 2.14 M faces) with 1 % of its
faces removed as separate one-triangle holes, and a rig of 64 views with 1600 x 1200 disc masks.

    edges        mesh_edges: the key sort of the 3 F half-edges and the edge kernel
    boundary     the CSR of the boundary graph (sort of the 2 B directed pairs, count, scan)
    fill         fill_holes, whole (its own edge table and CSR included)
    smooth       smooth_borders, whole
    components   face_components, whole; the number of rounds is reported
    views        view_counts over the 64 views
    compact      compact_mesh with the vertex mask of the views
    dilate11/31  dilate_masks of the 64 masks (host-side plumbing of clean_dtu_mesh)

With --network N also the clean-up (fill_holes + smooth_borders + filter_components) of the mesh extract_udf_mesh gets from
the geometric-init network at resolution N, next to the time of the extraction itself.  With --cpu-reference the numpy /
scipy restatement (tests/meshclean_ref.py; components by scipy.sparse.csgraph) on the same arrays, wall time in seconds,
each result compared with the GPU's.

    python scripts/bench_meshclean.py [--reps 3] [--network 512] [--cpu-reference]

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

N_VIEWS, W, H = 64, 1600, 1200


def separate_faces(faces, n_verts, share, seed=0):
    """indices of about `share` of the faces such that no two of them have vertices that are equal or joined by an edge:
    random candidates, each kept when it has the smallest candidate id within one edge of all its vertices"""
    import torch
    dev = faces.device
    g = torch.Generator(device=dev).manual_seed(seed)
    F = faces.shape[0]
    cand = torch.randperm(F, generator=g, device=dev)[:int(2 * share * F)]
    big = torch.iinfo(torch.int64).max
    owner = torch.full((n_verts,), big, dtype=torch.int64, device=dev)
    ids = torch.arange(cand.numel(), device=dev)
    owner.scatter_reduce_(0, faces[cand].reshape(-1), ids.repeat_interleave(3), "amin")
    near = owner.clone()
    near.scatter_reduce_(0, faces.reshape(-1), owner[faces].amin(1).repeat_interleave(3), "amin")
    ok = (near[faces[cand]] == ids[:, None]).all(1)
    return torch.sort(cand[ok][:int(share * F)]).values


def make_rig(dev):
    """64 cameras on a wavy ring of radius 1500 mm looking at the origin; disc masks of radius 400 px"""
    import numpy as np
    import torch
    mats = []
    for i in range(N_VIEWS):
        th = 2 * np.pi * i / N_VIEWS
        c = 1500.0 * np.array([np.cos(th), np.sin(th), 0.4 * np.sin(3 * th)])
        z = -c / np.linalg.norm(c)
        x = np.cross(z, [0.0, 0.0, 1.0])
        x /= np.linalg.norm(x)
        R = np.stack([x, np.cross(z, x), z])
        K = np.array([[2400.0, 0, W / 2], [0, 2400.0, H / 2], [0, 0, 1]])
        P = np.eye(4)
        P[:3, :3], P[:3, 3] = K @ R, K @ (-R @ c)
        mats.append(P)
    yy, xx = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    disc = (((xx - W / 2) ** 2 + (yy - H / 2) ** 2) <= 400 ** 2).to(torch.uint8)
    return np.stack(mats), disc[None].repeat(N_VIEWS, 1, 1).contiguous()


def median_ms(runs):
    return {k: round(statistics.median(r[k] for r in runs), 3) for k in runs[0]}


def bench(reps, cpu_reference):
    import torch
    from neuraludf_amd import meshclean as C
    import bench_chamfer
    dev = torch.device("cuda:0")
    v, f = bench_chamfer.make_scan(dev, "surface")[:2]
    gone = separate_faces(f, v.shape[0], 0.01)
    keep = torch.ones(f.shape[0], dtype=torch.bool, device=dev)
    keep[gone] = False
    fh = f[keep].contiguous()
    mats, masks = make_rig(dev)
    n_verts = v.shape[0]
    info, out, runs = {}, {}, []

    def timed(ev, name, fn):
        ev[name] = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[name][0].record()
        r = fn()
        ev[name][1].record()
        return r

    for rep in range(reps + 1):
        ev = {}
        table = timed(ev, "edges", lambda: C._mesh_edges(fh, n_verts))
        bd = timed(ev, "boundary", lambda: C._boundary(table, n_verts))
        filled, n_filled = timed(ev, "fill", lambda: C.fill_holes(v, fh))
        smooth = timed(ev, "smooth", lambda: C.smooth_borders(v, fh))
        labels = timed(ev, "components", lambda: C.face_components(fh, n_verts, _info=info))
        count = timed(ev, "views", lambda: C.view_counts(v, mats, masks))
        cv, cf = timed(ev, "compact", lambda: C.compact_mesh(v, fh, vertex_mask=count > 40, drop_unreferenced=False))
        d11 = timed(ev, "dilate11", lambda: C.dilate_masks(masks, 11))
        timed(ev, "dilate31", lambda: C.dilate_masks(masks, 31))
        torch.cuda.synchronize()
        if rep:
            runs.append({k: a.elapsed_time(b) for k, (a, b) in ev.items()})
    out.update(ms=median_ms(runs), reps=reps, verts=n_verts, faces=int(fh.shape[0]), edges=int(table.edges.shape[0]),
               boundary_edges=bd.n_edges, holes_removed=int(gone.numel()), holes_filled=n_filled,
               closed_after_fill=bool((C._mesh_edges(filled, n_verts).edges[:, 2] == 2).all()),
               component_rounds=info["rounds"], components=int(torch.unique(labels).numel()),
               verts_after_views=int(cv.shape[0]), faces_after_views=int(cf.shape[0]))
    if cpu_reference:
        out["cpu_reference"] = cpu_times(v, fh, mats, masks, table, filled, smooth, labels, count, d11)
    return out


def cpu_times(v, fh, mats, masks, table, filled, smooth, labels, count, d11):
    import numpy as np
    import meshclean_ref as M
    from neuraludf_amd import meshclean as C
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    vn, fn, mk = v.cpu().numpy(), fh.cpu().numpy(), masks.cpu().numpy()
    res = {}

    def wall(name, fn_):
        t = time.perf_counter()
        r = fn_()
        res[name + "_s"] = round(time.perf_counter() - t, 3)
        return r
    edges, he_edge = wall("edges", lambda: M.edge_table(fn, len(vn)))
    res["edges_equal"] = bool(np.array_equal(edges, table.edges.cpu().numpy()) and
                              np.array_equal(he_edge, table.he_edge.cpu().numpy()))
    res["fill_equal"] = bool(np.array_equal(wall("fill", lambda: M.fill_holes(vn, fn))[0], filled.cpu().numpy()))
    res["smooth_equal"] = bool(np.array_equal(wall("smooth", lambda: M.smooth_borders(vn, fn)), smooth.cpu().numpy()))

    def scipy_labels():
        face = np.arange(len(he_edge)) // 3
        order = np.argsort(he_edge, kind="stable")
        same = he_edge[order][1:] == he_edge[order][:-1]
        a, b = face[order][:-1][same], face[order][1:][same]
        _, lab = connected_components(coo_matrix((np.ones(len(a)), (a, b)), shape=(len(fn), len(fn))), directed=False)
        first = np.full(lab.max() + 1, len(fn))
        np.minimum.at(first, lab, np.arange(len(fn)))
        return first[lab]
    res["components_equal"] = bool(np.array_equal(wall("components_scipy", scipy_labels), labels.cpu().numpy()))
    res["views_equal"] = bool(np.array_equal(wall("views", lambda: M.view_counts(vn, mats, mk)), count.cpu().numpy()))
    fp = C.ellipse_footprint(11)
    res["dilate11_equal"] = bool(np.array_equal(wall("dilate11", lambda: M.dilate(mk, fp)), d11.cpu().numpy()))
    return res


def network(n, reps):
    """the clean-up of the network's mesh at resolution n beside the extraction that produced it"""
    import contextlib
    import io
    import torch
    from neuraludf_amd import meshclean as C, meshing
    from neuraludf_amd.models import fields
    from neuraludf_amd.train import DTU_MODEL_CONF
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        udf = fields.UDFNetwork(**DTU_MODEL_CONF["udf_network"]).to(dev)
    box = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
    runs, sizes = [], {}
    for rep in range(reps + 1):
        ev = {k: (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
              for k in ("extract", "fill", "smooth", "components")}
        ev["extract"][0].record()
        U, G = meshing.udf_grid(udf, n, *box)
        v, f = meshing.udf_marching_cubes(U, G, *box)
        del U, G
        v, f = meshing.filter_mesh(v, f, meshing._query_udf(udf, v), meshing.grid_spacing(*box, n))
        ev["extract"][1].record()
        ev["fill"][0].record()
        f2, holes = C.fill_holes(v, f)
        ev["fill"][1].record()
        ev["smooth"][0].record()
        v2 = C.smooth_borders(v, f2)
        ev["smooth"][1].record()
        ev["components"][0].record()
        v3, f3 = C.filter_components(v2, f2, 500)
        ev["components"][1].record()
        torch.cuda.synchronize()
        if rep:
            runs.append({k: a.elapsed_time(b) for k, (a, b) in ev.items()})
        sizes = dict(verts=int(v.shape[0]), faces=int(f.shape[0]), holes_filled=holes, faces_after=int(f3.shape[0]))
    ms = median_ms(runs)
    clean = round(ms["fill"] + ms["smooth"] + ms["components"], 3)
    return dict(N=n, ms=ms, cleanup_ms=clean, cleanup_share_of_extract=round(clean / ms["extract"], 4), **sizes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--network", type=int, default=0, help="also time the clean-up of the network mesh at this resolution")
    ap.add_argument("--cpu-reference", action="store_true")
    ap.add_argument("--skip-sphere", action="store_true")
    a = ap.parse_args()
    out = dict(bench="meshclean", device="cuda:0")
    if not a.skip_sphere:
        out["sphere512"] = bench(a.reps, a.cpu_reference)
    if a.network:
        out["network"] = network(a.network, a.reps)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
