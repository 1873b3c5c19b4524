"""Time the GPU mesh subdivision (neuraludf_amd/meshclean.py subdivide_mesh / subdivide_to_edge, csrc/meshsubdiv.hip) with
HIP events, on the mesh of scripts/bench_chamfer.py: the radius-280 sphere at 512^3 in a 600 mm box (1.07 M vertices,
2.14 M faces).

    loop, midpoint      one level of subdivide_mesh: the whole call, and its stages from the events the driver records
                        (edges: the edge table; mark; adjacency: one-rings, border lists and classes, Loop only;
                        vertices: odd and even; faces: count, scan, emit)
    to_edge             subdivide_to_edge at half the longest edge: one round of splits and the round that finds none

With --cpu-reference the numpy restatement (tests/meshsubdiv_ref.py) on the 1280-face sphere of the tests, wall time in
seconds, next to the GPU's time on the same input.

    python scripts/bench_meshsubdiv.py [--reps 3] [--cpu-reference]

Run it under a time limit of its own.  Prints one JSON line: median milliseconds over --reps timed runs after one warm-up
run."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench_meshsmooth import EXTRACTION_MS_512, timed  # noqa: E402


def staged(fn):
    """one run of fn(_info) -> {round: {stage: milliseconds}} from the events the driver recorded"""
    import torch
    info = dict(events={})
    fn(info)
    torch.cuda.synchronize()
    return {r: {k: round(a.elapsed_time(b), 3) for k, (a, b) in ev.items()} for r, ev in info["events"].items()}


def sphere(reps):
    import torch
    import bench_chamfer
    from neuraludf_amd import meshclean as C
    dev = torch.device("cuda:0")
    v, f = bench_chamfer.make_scan(dev, "surface")[:2]
    longest = C.subdivide_mesh(v, f, 0).longest_edge
    ms, stages, facts = {}, {}, {}
    for scheme in ("loop", "midpoint"):
        ms[scheme] = timed(lambda: C.subdivide_mesh(v, f, 1, scheme), reps)
        stages[scheme] = staged(lambda info: C.subdivide_mesh(v, f, 1, scheme, _info=info))["round0"]
    out = C.subdivide_mesh(v, f, 1, "loop")
    facts["one_level"] = dict(verts=int(out.verts.shape[0]), faces=int(out.faces.shape[0]))
    del out
    bound = 0.5 * longest
    ms["to_edge"] = timed(lambda: C.subdivide_to_edge(v, f, bound), reps)
    stages["to_edge"] = staged(lambda info: C.subdivide_to_edge(v, f, bound, _info=info))
    out = C.subdivide_to_edge(v, f, bound)
    facts["to_edge"] = dict(max_edge=bound, input_longest=longest, rounds=out.rounds, longest_edge=out.longest_edge,
                            converged=out.converged, verts=int(out.verts.shape[0]), faces=int(out.faces.shape[0]))
    return dict(verts=int(v.shape[0]), faces=int(f.shape[0]), reps=reps, ms=ms, stages_ms=stages,
                share_of_extraction={k: round(x / EXTRACTION_MS_512, 3) for k, x in ms.items()}, **facts)


def cpu_reference(reps):
    """the restatement and the GPU on the noisy 1280-face sphere of the tests"""
    import numpy as np
    import torch
    import meshsubdiv_ref as R
    from neuraludf_amd import meshclean as C
    v, f = R.meshes()["sphere"]
    bound = 0.3 * R.longest_edge(v, R.edge_table(f, len(v)))
    dev = torch.device("cuda:0")
    vt, ft = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    runs = dict(loop=(lambda: R.subdivide_mesh(v, f, 1, "loop"), lambda: C.subdivide_mesh(vt, ft, 1, "loop")),
                midpoint=(lambda: R.subdivide_mesh(v, f, 1, "midpoint"), lambda: C.subdivide_mesh(vt, ft, 1, "midpoint")),
                to_edge=(lambda: R.subdivide_to_edge(v, f, bound), lambda: C.subdivide_to_edge(vt, ft, bound)))
    wall, ms, equal = {}, {}, {}
    for name, (ref, gpu) in runs.items():
        t = time.perf_counter()
        want = ref()
        wall[name] = round(time.perf_counter() - t, 4)
        ms[name] = timed(gpu, reps)
        got = gpu()
        equal[name] = bool(np.array_equal(got.verts.cpu().numpy(), want.verts)
                           and np.array_equal(got.faces.cpu().numpy(), want.faces))
    return dict(verts=len(v), faces=len(f), numpy_s=wall, gpu_ms=ms, equal=equal)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cpu-reference", action="store_true")
    ap.add_argument("--skip-sphere", action="store_true")
    a = ap.parse_args()
    out = dict(bench="meshsubdiv", device="cuda:0")
    if not a.skip_sphere:
        out["sphere512"] = sphere(a.reps)
    if a.cpu_reference:
        out["sphere1280"] = cpu_reference(a.reps)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
