"""Time the search for intersecting faces (neuraludf_amd/evaluation.py MeshIndex.intersections / self_intersections,
csrc/meshintersect.hip) with HIP events, on the mesh of scripts/bench_chamfer.py: the radius-280 sphere at 512^3 in a
600 mm box (1.07 M vertices, 2.14 M faces),

    clean       as it is: the mesher's surface does not cross itself, so the call is all broad phase and shared-vertex rules;
    doubled     with a copy shifted by half a grid spacing along a generic direction appended: two surfaces half a cell
                apart that cross along a circle.

    self_intersections      the whole call, index included
    stages                  from the events the drivers record: index (MeshIndex, all its stages), count, scan, emit, sort

    python scripts/bench_meshintersect.py [--reps 3] [--out profiles/meshintersect_bench.json]

Run it under a time limit of its own.  Prints one JSON line and writes it to --out: median milliseconds over --reps timed
runs after one warm-up run; `kernels` holds what the compiler reports for the two kernels."""
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

from bench_meshsmooth import EXTRACTION_MS_512, timed  # noqa: E402

SHIFT_DIRECTION = (0.5370861555295747, 0.2915274230636872, 0.7915368220043530)


def kernel_resources():
    """{kernel: dict(vgprs, scratch_bytes, waves_per_simd)} from hipcc's resource remarks, or a note when hipcc is absent"""
    from neuraludf_amd import build
    try:
        hipcc = build._hipcc()
    except RuntimeError:
        return dict(note="hipcc not found")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-c",
               os.path.join(build.CSRC, "meshintersect.hip"), "-o", os.path.join(tmp, "mi.o"), "-I", build.CSRC, "-I",
               build.INCLUDE, "-Rpass-analysis=kernel-resource-usage"]
        text = subprocess.run(cmd, capture_output=True, text=True, timeout=600).stderr
    out = {}
    for m in re.finditer(r"Function Name: _Z\d+(\w+?)14NudfPointCloud(.*?)LDS Size", text, re.S):
        body = m.group(2)
        out[m.group(1)] = dict(vgprs=int(re.search(r" VGPRs: (\d+)", body).group(1)),
                               scratch_bytes=int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", body).group(1)),
                               waves_per_simd=int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", body).group(1)))
    return out


def measure(v, f, reps):
    import torch
    from neuraludf_amd import evaluation as E
    ms = dict(self_intersections=timed(lambda: E.self_intersections(v, f), reps))
    runs = []
    for _ in range(reps + 1):
        build_ev, ev = {}, {}
        index = E.MeshIndex(v, f, _events=build_ev)
        res = index.intersections(_events=ev)
        torch.cuda.synchronize()
        run = {k: a.elapsed_time(b) for k, (a, b) in ev.items()}
        run["index"] = sum(a.elapsed_time(b) for a, b in build_ev.values())
        runs.append(run)
    stages = {k: round(sorted(r[k] for r in runs[1:])[len(runs[1:]) // 2], 3) for k in ("index", "count", "scan", "emit", "sort")}
    again = index.intersections()
    kinds = {name: int((res.kind == k).sum()) for name, k in E.ISECT_KINDS.items()}
    return dict(verts=int(v.shape[0]), faces=int(f.shape[0]), cell=index.cell, refs=int(index.n_refs), ms=ms, stages_ms=stages,
                share_of_extraction={k: round(x / EXTRACTION_MS_512, 3) for k, x in ms.items()},
                pairs=int(res.pairs.shape[0]), pairs_by_kind=kinds, flagged_faces=int(res.face_mask.sum()),
                identical_rerun=bool(torch.equal(again.pairs, res.pairs) and torch.equal(again.kind, res.kind)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "meshintersect_bench.json"))
    a = ap.parse_args()
    import torch
    import bench_chamfer
    from neuraludf_amd import build
    dev = torch.device("cuda:0")
    v, f = bench_chamfer.make_scan(dev, "surface")[:2]
    h = 2.0 * bench_chamfer.BOX / (bench_chamfer.N - 1)
    shift = torch.tensor(SHIFT_DIRECTION, dtype=v.dtype, device=dev) * (0.5 * h)
    out = dict(bench="meshintersect", device=torch.cuda.get_device_name(0), source_digest=build.source_digest("meshintersect"),
               reps=a.reps, kernels=kernel_resources(), clean=measure(v, f, a.reps),
               doubled=measure(torch.cat([v, v + shift]), torch.cat([f, f + v.shape[0]]), a.reps))
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
