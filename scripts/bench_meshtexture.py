"""Time the texture atlas (neuraludf_amd/meshrender.py texture_atlas, bake_texture, shade_textured; csrc/meshtexture.hip)
with HIP events, on the sphere of the other mesh benchmarks (scripts/bench_chamfer.py: radius 280 at 512^3, 2.14 M faces)
simplified to about --faces faces (meshclean.simplify_to_faces), from the 64 cameras of scripts/bench_meshclean.py at
1600 x 1200 with random uint8 images:

    atlas        texture_atlas(size=--size): the bisection over the density and the layout
    layout       texture_atlas(density = the one found): the layout alone
    depth        the depth maps of all views (project, bounds, split, the draws and resolve, meshrender's own path)
    bake         nudf_meshtexture_bake alone, one launch over all views (depth maps resident)
    bake_texture the whole call: depth + bake + the argument plumbing
    shade        rasterize of one view aside, nudf_meshtexture_shade of that view
    colour       color_vertices on the same mesh and views, for scale

and the atlas's occupancy, owned texels / (W H).

    python scripts/bench_meshtexture.py [--reps 5] [--faces 100000] [--size 4096] [--out profiles/meshtexture_bench.json]

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

CHUNK = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--faces", type=int, default=100000)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "meshtexture_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import bench_chamfer
    import bench_meshclean
    from neuraludf_amd import _lib, build, meshclean, meshrender
    from neuraludf_amd._lib import call, ptr
    dev = torch.device("cuda:0")
    v, f = bench_chamfer.make_scan(dev, "surface")[:2]
    full = int(f.shape[0])
    s = meshclean.simplify_to_faces(v, f, a.faces)
    v, f = s.verts, s.faces
    del s
    W, H = bench_meshclean.W, bench_meshclean.H
    mats = bench_meshclean.make_rig(dev)[0][:a.views]
    normals = meshclean.vertex_normals(v, f, torch.float64)
    g = torch.Generator(device=dev).manual_seed(0)
    images = torch.randint(0, 256, (a.views, H, W, 3), dtype=torch.uint8, device=dev, generator=g)
    gap = 2.0 * meshrender.mean_edge_length(v, f)
    pos = v.double().contiguous()
    proj_np = np.ascontiguousarray(mats[:, :3, :])
    proj = torch.from_numpy(proj_np).to(dev)
    cam = torch.from_numpy(np.ascontiguousarray(meshrender.camera_positions(mats))).to(dev)

    def timed(ms, name, fn):
        x, y = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        x.record()
        r = fn()
        y.record()
        ms[name] = (x, y)
        return r

    def depth_maps():
        depth = torch.empty((a.views, H, W), dtype=torch.float32, device=dev)
        for s0 in range(0, a.views, CHUNK):
            ch = meshrender._draw_chunk(pos, f, proj[s0:s0 + CHUNK].contiguous(), H, W, meshrender.LARGE_THRESHOLD, None)
            ch.desc.depth = ptr(depth[s0:s0 + CHUNK])
            call("nudf_meshraster_resolve", ch.desc)
        return depth

    runs = []
    for rep in range(a.reps + 1):
        ms = {}
        atlas = timed(ms, "atlas", lambda: meshrender.texture_atlas(v, f, size=a.size))
        timed(ms, "layout", lambda: meshrender.texture_atlas(v, f, density=atlas.density))
        depth = timed(ms, "depth", depth_maps)
        colors = torch.empty((atlas.H, atlas.W, 3), dtype=torch.float32, device=dev)
        n_seen = torch.empty((atlas.H, atlas.W), dtype=torch.int32, device=dev)
        d = _lib.MeshRaster(pos=ptr(pos), faces=ptr(f), proj=ptr(proj), depth=ptr(depth), images=ptr(images),
                            normals=ptr(normals), cam_pos=ptr(cam), n_faces=f.shape[0], n_verts=v.shape[0],
                            n_views=a.views, H=H, W=W, image_f32=0, power=1.0, min_gap=gap, tx_colors=ptr(colors),
                            tx_n_seen=ptr(n_seen))
        d.fill[0] = d.fill[1] = d.fill[2] = 0.5
        meshrender._atlas_fields(d, atlas)
        timed(ms, "bake", lambda: call("nudf_meshtexture_bake", d))
        del depth
        tex = timed(ms, "bake_texture", lambda: meshrender.bake_texture(v, f, atlas, mats, images, normals, 1.0, gap,
                                                                        view_chunk=CHUNK))
        assert torch.equal(tex.n_seen, n_seen) and torch.equal(tex.colors, colors)
        raster = meshrender.rasterize(v, f, mats[:1], H, W)
        shaded = timed(ms, "shade", lambda: meshrender.shade_textured(raster, atlas, tex))
        cv = timed(ms, "colour", lambda: meshrender.color_vertices(v, f, mats, images, normals, 1.0, gap, view_chunk=CHUNK))
        torch.cuda.synchronize()
        if rep:
            runs.append({k: x.elapsed_time(y) for k, (x, y) in ms.items()})
    owned = int((tex.n_seen >= 0).sum())
    out = dict(bench="meshtexture", device=torch.cuda.get_device_name(0), source_digest=build.source_digest("meshtexture"),
               faces_full=full, verts=int(v.shape[0]), faces=int(f.shape[0]), views=a.views, H=H, W=W, chunk=CHUNK,
               reps=a.reps, size=a.size, atlas=dict(W=atlas.W, H=atlas.H, density=atlas.density, classes=list(atlas.class_k),
                                                   cells=int(atlas.cell_face.shape[0]), owned=owned,
                                                   occupancy=owned / (atlas.W * atlas.H)),
               texels_seen=int((tex.n_seen > 0).sum()), mean_views_per_seen_texel=float(tex.n_seen[tex.n_seen > 0].double().mean()),
               pixels_shaded=int((raster.face >= 0).sum()), vertices_seen=int((cv[1] > 0).sum()), min_gap=round(gap, 4),
               ms=median_ms(runs))
    out["bake_texel_views_per_s"] = owned * a.views / (out["ms"]["bake"] * 1e-3)
    del shaded
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text + "\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
