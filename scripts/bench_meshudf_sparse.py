"""Time sparse against dense open-surface extraction (neuraludf_amd/meshing.py) on a UDFNetwork built from the shipped
DTU conf (its geometric init: a closed surface of radius about 0.24 .. 0.39), with HIP events.  Per size the dense path
and the sparse path (lipschitz 2.0, B = 8 and B = 4) alternate inside one process, run after run; sizes above the dense
limit (1024) run the sparse path alone.

    dense   values / gradients / classify / scan / emit / vertices / vertex_udf / filter     (scripts/bench_meshudf.py)
    sparse  coarse    the UDF at the (nb+1)^3 coarse nodes
            select    block selection and the sorted unique node list
            fine      the UDF at the unique nodes of the selected blocks
            gradient  the gradient at the nodes with U < 2 h
            bricks    scatter of values and gradients into the bricks
            classify / sort / emit / vertices   the sparse mesher's kernels and the torch sorts between them
            vertex_udf / filter

    python scripts/bench_meshudf_sparse.py [--sizes 256 512 1024 2048] [--reps 3] [--timeout 900] [--out FILE]

Each size runs in a child process of its own under a time limit (the parent never opens the GPU); a child that fails
ends the run.  Prints one JSON line (and writes it to --out): per size and path the median milliseconds of each stage
over --reps timed runs (after one warm-up run each), the smallest and largest total, the counters, the peak memory and
the face count; per sparse path the measured speed-up over dense beside the query ratio N^3 / (n_coarse + n_queried)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MESHER = {"dense": ("classify", "scan", "emit", "vertices"), "sparse": ("classify", "sort", "emit", "vertices")}
LIPSCHITZ = 2.0


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

    def finish(ev, v, f, info):
        vu = timed(ev, "vertex_udf", lambda: meshing._query_udf(udf, v))
        vf, ff = timed(ev, "filter", lambda: meshing.filter_mesh(v, f, vu, h))
        torch.cuda.synchronize()
        info.update(faces=int(f.shape[0]), verts=int(v.shape[0]), faces_filtered=int(ff.shape[0]),
                    peak_mib=round(torch.cuda.max_memory_allocated() / 2 ** 20, 1))
        return {k: a.elapsed_time(b) for k, (a, b) in ev.items()}, info

    def dense():
        ev, info = {}, {}
        U = timed(ev, "values", lambda: meshing.udf_values(udf, n, *box))
        G = timed(ev, "gradients", lambda: meshing.udf_gradients_in_band(udf, U, *box))
        info["n_queried"], info["n_grad"] = n ** 3, int((U < 2 * h).sum())
        v, f = meshing.udf_marching_cubes(U, G, *box, _events=ev)
        del U, G
        return finish(ev, v, f, info)

    def sparse(block):
        ev = {}
        g = meshing.udf_sparse_grid(udf, n, *box, block=block, lipschitz=LIPSCHITZ, _events=ev)
        info = dict(n_coarse=g.n_coarse, n_blocks=g.n_blocks, n_total_blocks=g.nb ** 3, n_queried=g.n_queried,
                    n_grad=g.n_grad, query_ratio=round(n ** 3 / (g.n_coarse + g.n_queried), 2))
        v, f = meshing.udf_marching_cubes_sparse(g, _events=ev)
        del g
        return finish(ev, v, f, info)

    paths = ([("dense", dense)] if n <= meshing.MAX_N else []) + [("sparse_b8", lambda: sparse(8)),
                                                                 ("sparse_b4", lambda: sparse(4))]
    runs, infos = {k: [] for k, _ in paths}, {}
    for rep in range(reps + 1):
        for name, fn in paths:                                 # the paths alternate: drift hits them alike
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            ms, infos[name] = fn()
            if rep:
                runs[name].append(ms)
    out = dict(N=n, reps=reps, lipschitz=LIPSCHITZ, paths={})
    for name, _ in paths:
        ms = {k: round(statistics.median(r[k] for r in runs[name]), 3) for k in runs[name][0]}
        totals = [sum(r.values()) for r in runs[name]]
        mesher = sum(ms[k] for k in MESHER["dense" if name == "dense" else "sparse"])
        out["paths"][name] = dict(ms=ms, total_ms=round(sum(ms.values()), 3), total_min_ms=round(min(totals), 3),
                                  total_max_ms=round(max(totals), 3), mesher_ms=round(mesher, 3),
                                  mesher_share=round(mesher / sum(ms.values()), 4), **infos[name])
    if "dense" in out["paths"]:
        for name in ("sparse_b8", "sparse_b4"):
            p = out["paths"][name]
            p["speedup_vs_dense"] = round(out["paths"]["dense"]["total_ms"] / p["total_ms"], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512, 1024, 2048])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--timeout", type=float, default=900.0, help="seconds per size")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child is not None:
        print("RESULT " + json.dumps(child(a.child, a.reps)))
        return 0
    out = dict(bench="meshudf_sparse", device="cuda:0", sizes=[])
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
        print(f"N={n} done", file=sys.stderr, flush=True)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    return 1 if "error" in out else 0


if __name__ == "__main__":
    sys.exit(main())
