"""Time the GPU open-surface mesher end to end (neuraludf_amd/meshing.py) on a UDFNetwork built from the shipped DTU
conf (its geometric init: a closed surface of radius about 0.24 .. 0.39), with HIP events:

    values     the dense-grid UDF query (udf_values)
    gradients  the gradient query in the band U < 2 h (udf_gradients_in_band)
    classify / scan / emit / vertices   the mesher's three kernels and the torch integer scans between them
    vertex_udf the network's UDF at the vertices
    filter     filter_mesh

    python scripts/bench_meshudf.py [--sizes 256 512] [--reps 3] [--timeout 600]

Each size runs in a child process of its own under a time limit (the parent never opens the GPU); a child that fails
ends the run.  Prints one JSON line: per size the median milliseconds of each stage over --reps timed runs (after one
warm-up run), the mesh size and the mesher's share of the total."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MESHER = ("classify", "scan", "emit", "vertices")


def child(n, reps):
    import contextlib
    import io
    import torch
    from neuraludf_amd import meshing
    from neuraludf_amd.models import fields
    from neuraludf_amd.train import DTU_MODEL_CONF

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        udf = fields.UDFNetwork(**DTU_MODEL_CONF["udf_network"]).to(dev)
    box = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
    h = meshing.grid_spacing(*box, n)

    def timed(ev, name, fn):
        ev[name] = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[name][0].record()
        out = fn()
        ev[name][1].record()
        return out

    runs = []
    for rep in range(reps + 1):
        ev = {}
        U = timed(ev, "values", lambda: meshing.udf_values(udf, n, *box))
        G = timed(ev, "gradients", lambda: meshing.udf_gradients_in_band(udf, U, *box))
        v, f = meshing.udf_marching_cubes(U, G, *box, _events=ev)
        vu = timed(ev, "vertex_udf", lambda: meshing._query_udf(udf, v))
        vf, ff = timed(ev, "filter", lambda: meshing.filter_mesh(v, f, vu, h))
        torch.cuda.synchronize()
        if rep:
            runs.append({k: a.elapsed_time(b) for k, (a, b) in ev.items()})
        sizes = dict(band_points=int((U < 2 * h).sum()), verts=int(v.shape[0]), faces=int(f.shape[0]),
                     verts_filtered=int(vf.shape[0]), faces_filtered=int(ff.shape[0]))
        del U, G, v, f, vu, vf, ff
    ms = {k: round(statistics.median(r[k] for r in runs), 3) for k in runs[0]}
    total = sum(ms.values())
    mesher = sum(ms[k] for k in MESHER)
    return dict(N=n, ms=ms, total_ms=round(total, 3), mesher_ms=round(mesher, 3),
                mesher_share=round(mesher / total, 4), reps=reps, **sizes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--timeout", type=float, default=600.0, help="seconds per size")
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child is not None:
        print("RESULT " + json.dumps(child(a.child, a.reps)))
        return 0
    out = dict(bench="meshudf", device="cuda:0", sizes=[])
    for n in a.sizes:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", str(n), "--reps", str(a.reps)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
        except subprocess.TimeoutExpired:
            out["error"] = f"N={n}: timed out after {a.timeout} s"
            break
        res = [ln[7:] for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not res:
            out["error"] = f"N={n}: exit {p.returncode}: {p.stderr[-800:]}"
            break
        out["sizes"].append(json.loads(res[-1]))
    print(json.dumps(out))
    return 1 if "error" in out else 0


if __name__ == "__main__":
    sys.exit(main())
