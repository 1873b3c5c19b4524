"""Time the generalised winding number (neuraludf_amd/evaluation.py MeshIndex.winding, csrc/meshwinding.hip) with HIP
events, on the mesh of scripts/bench_chamfer.py: the radius-280 sphere at 512^3 in a 600 mm box (1.07 M vertices, 2.14 M
faces), its faces wound outward by meshclean.orient_faces first, at 1 M uniform points of its box.

    tree        the build by stage, from the events the driver records: keys, sort, levels, moments
    winding     the query at beta = 2 and 3 (query_sort and the walk apart), with the mean number of faces evaluated
                exactly and of nodes replaced by their expansion per query, and the largest |w_2 - w_3|
    parity      contains_points(method="parity") on the same points: three crossing-count rays per point, the only
                comparable number the project owns
    factors     the walk at beta = 2 for several WINDING_LEAF_FACTOR values (--factors): what the default was picked from

    python scripts/bench_meshwinding.py [--reps 3] [--points 1000000] [--factors 1,2,4] [--out profiles/meshwinding_bench.json]

Run it under a time limit of its own.  Prints one JSON line and writes it to --out: median milliseconds over --reps timed
runs after one warm-up run; `kernels` holds what the compiler reports for the three kernels."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench_meshsmooth import timed  # noqa: E402


def kernel_resources():
    """{kernel: dict(vgprs, scratch_bytes, waves_per_simd)} from hipcc's resource remarks"""
    from neuraludf_amd import build
    try:
        hipcc = build._hipcc()
    except RuntimeError:
        return dict(note="hipcc not found")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-c",
               os.path.join(build.CSRC, "meshwinding.hip"), "-o", os.path.join(tmp, "mw.o"), "-I", build.CSRC, "-I",
               build.INCLUDE, "-Rpass-analysis=kernel-resource-usage"]
        text = subprocess.run(cmd, capture_output=True, text=True, timeout=600).stderr
    out = {}
    for m in re.finditer(r"Function Name: _Z\d+(\w+?)14NudfPointCloud(.*?)LDS Size", text, re.S):
        body = m.group(2)
        out[m.group(1)] = dict(vgprs=int(re.search(r" VGPRs: (\d+)", body).group(1)),
                               scratch_bytes=int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", body).group(1)),
                               waves_per_simd=int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", body).group(1)))
    return out


def _median(runs, keys):
    return {k: round(sorted(r[k] for r in runs)[len(runs) // 2], 3) for k in keys}


def measure(v, f, q, reps, factor=None, betas=(2.0, 3.0)):
    import torch
    from neuraludf_amd import evaluation as E
    old = E.WINDING_LEAF_FACTOR
    if factor is not None:
        E.WINDING_LEAF_FACTOR = factor
    try:
        index = E.MeshIndex(v, f)
        builds = []
        for _ in range(reps + 1):
            index._winding_tree = None
            ev = {}
            index.winding(q[:64], _events=ev)
            torch.cuda.synchronize()
            builds.append({k: a.elapsed_time(b) for k, (a, b) in ev.items()})
        tree = index._winding_tree
        out = dict(leaf_factor=E.WINDING_LEAF_FACTOR, leaf=tree.leaf, grid=list(tree.grid), nodes=int(tree.n_nodes),
                   levels=int(tree.level.max()) + 1, faces_in_tree=int(tree.faces.numel()),
                   largest_leaf=int(tree.count[tree.skip == torch.arange(1, tree.n_nodes + 1, device=v.device)].max()),
                   tree_ms=_median(builds[1:], ("keys", "sort", "levels", "moments")))
        out["tree_ms"]["total"] = round(sum(out["tree_ms"].values()), 3)
        ws = {}
        for beta in betas:
            runs = []
            for _ in range(reps + 1):
                ev = {}
                w, exact, far = index.winding(q, beta, _events=ev, _counts=True)
                torch.cuda.synchronize()
                runs.append({k: a.elapsed_time(b) for k, (a, b) in ev.items()})
            ws[beta] = w
            again = index.winding(q, beta)
            out["beta_%g" % beta] = dict(ms=_median(runs[1:], ("query_sort", "winding")),
                                         exact_faces_per_query=round(float(exact.double().mean()), 2),
                                         far_nodes_per_query=round(float(far.double().mean()), 2),
                                         exact_faces_max=int(exact.max()), inside=int((w.abs() > 0.5).sum()),
                                         identical_rerun=bool(torch.equal(again, w)))
        if len(betas) > 1:
            out["max_abs_w2_minus_w3"] = float((ws[betas[0]] - ws[betas[1]]).abs().max())
    finally:
        E.WINDING_LEAF_FACTOR = old
    return out, index, ws[betas[0]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--factors", type=str, default="1,2,4")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "meshwinding_bench.json"))
    a = ap.parse_args()
    import torch
    import bench_chamfer
    from neuraludf_amd import build, evaluation as E
    dev = torch.device("cuda:0")
    v, f = bench_chamfer.make_scan(dev, "surface")[:2]
    v = v.double()
    lo, hi = v.amin(0), v.amax(0)
    # the UDF mesher winds its faces as they come: the winding number needs them consistent (and outward, for the sign)
    from neuraludf_amd import meshclean
    info = {}
    f = meshclean.orient_faces(v, f, outward_from=(0.5 * (lo + hi)).tolist(), _info=info).faces.contiguous()
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    q = lo + (hi - lo) * torch.rand((a.points, 3), dtype=torch.float64, device=dev, generator=g)
    res, index, w = measure(v, f, q, a.reps)
    parity_ms = timed(lambda: E.contains_points(q, index), a.reps)
    parity = E.contains_points(q, index)
    res["parity"] = dict(ms=parity_ms, inside=int(parity.sum()), disagree_with_winding=int((parity != (w.abs() > 0.5)).sum()))
    factors = {}
    for fac in [float(x) for x in a.factors.split(",") if x]:
        r = measure(v, f, q, a.reps, factor=fac, betas=(2.0,))[0]
        factors["%g" % fac] = dict(nodes=r["nodes"], levels=r["levels"], largest_leaf=r["largest_leaf"],
                                   tree_ms=r["tree_ms"]["total"], winding_ms=r["beta_2"]["ms"]["winding"],
                                   exact_faces_per_query=r["beta_2"]["exact_faces_per_query"],
                                   far_nodes_per_query=r["beta_2"]["far_nodes_per_query"])
    out = dict(bench="meshwinding", device=torch.cuda.get_device_name(0), source_digest=build.source_digest("meshwinding"),
               reps=a.reps, verts=int(v.shape[0]), faces=int(f.shape[0]), points=a.points, kernels=kernel_resources(),
               oriented=dict(flipped=int(info.get("flipped", -1)), components=int(info.get("components", -1))),
               **res, factors=factors)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
