"""Time the level-set mesher (neuraludf_amd/meshing.py iso_*, csrc/isosurface.hip) on the sphere SDF |x| - 0.6 at level 0
and, beside it in the same process, the MeshUDF mesher on the unsigned field | |x| - 0.6 | with its exact gradient, with
HIP events.  Both fields are analytic (elementwise torch), so the query stages are small and the mesher stages stand out.

    dense   values / classify / scan / emit / vertices                      iso_marching_cubes, udf_marching_cubes
    sparse  coarse / select / fine / [gradient] / bricks / classify / sort / emit / vertices    B = 8, lipschitz 1.05

    python scripts/bench_isosurface.py [--dense 512] [--sparse 2049] [--reps 3] [--timeout 900] [--out FILE]

Each size runs in a child process of its own under a time limit (the parent never opens the GPU); a child that fails
ends the run.  Prints one JSON line (and writes it to --out): per size and path the median milliseconds of each stage
over --reps timed runs (after one warm-up run each), the total, the counters, the peak memory and the face count."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

RADIUS, LIPSCHITZ, BLOCK = 0.6, 1.05, 8


def child(mode, n, reps):
    import torch
    from neuraludf_amd import meshing
    from neuraludf_amd.models import udf_renderer_blending as rb

    dev = torch.device("cuda:0")
    box = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))

    def sdf(p):
        return torch.sqrt(p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1] + p[:, 2] * p[:, 2]) - RADIUS

    class Shell(torch.nn.Module):
        """| |x| - R | with .udf / .gradient, the interface udf_sparse_grid queries"""

        def __init__(self):
            super().__init__()
            self.dummy = torch.nn.Parameter(torch.zeros(1))

        def udf(self, p):
            return sdf(p).abs()[:, None]

        def gradient(self, p):
            return torch.nan_to_num(p / p.norm(dim=-1, keepdim=True) * torch.sign(sdf(p))[:, None])[:, None, :]

    shell = Shell().to(dev)

    def timed(ev, name, fn):
        ev[name] = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[name][0].record()
        out = fn()
        ev[name][1].record()
        return out

    def finish(ev, v, f, info):
        torch.cuda.synchronize()
        info.update(faces=int(f.shape[0]), verts=int(v.shape[0]),
                    peak_mib=round(torch.cuda.max_memory_allocated() / 2 ** 20, 1))
        return {k: a.elapsed_time(b) for k, (a, b) in ev.items()}, info

    def iso_dense():
        ev = {}
        F = timed(ev, "values", lambda: rb._grid_query_device(*box, n, sdf, dev, 1))
        return finish(ev, *meshing.iso_marching_cubes(F, 0.0, *box, _events=ev), {})

    def udf_dense():
        ev = {}
        U = timed(ev, "values", lambda: meshing.udf_values(shell, n, *box))
        G = timed(ev, "gradients", lambda: meshing.udf_gradients_in_band(shell, U, *box))
        return finish(ev, *meshing.udf_marching_cubes(U, G, *box, _events=ev), {})

    def iso_sparse():
        ev = {}
        g = meshing.iso_sparse_grid(sdf, n, 0.0, *box, block=BLOCK, lipschitz=LIPSCHITZ, device=dev, _events=ev)
        info = dict(n_blocks=g.n_blocks, n_total_blocks=g.nb ** 3, n_queried=g.n_queried)
        return finish(ev, *meshing.iso_marching_cubes_sparse(g, 0.0, _events=ev), info)

    def udf_sparse():
        ev = {}
        g = meshing.udf_sparse_grid(shell, n, *box, block=BLOCK, lipschitz=LIPSCHITZ, _events=ev)
        info = dict(n_blocks=g.n_blocks, n_total_blocks=g.nb ** 3, n_queried=g.n_queried, n_grad=g.n_grad)
        return finish(ev, *meshing.udf_marching_cubes_sparse(g, _events=ev), info)

    paths = [("isosurface", iso_dense), ("meshudf", udf_dense)] if mode == "dense" else \
        [("isosurface", iso_sparse), ("meshudf", udf_sparse)]
    runs, infos = {k: [] for k, _ in paths}, {}
    for rep in range(reps + 1):
        for name, fn in paths:                                 # the paths alternate: drift hits them alike
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            ms, infos[name] = fn()
            if rep:
                runs[name].append(ms)
    out = dict(mode=mode, N=n, reps=reps, block=BLOCK if mode == "sparse" else None, lipschitz=LIPSCHITZ, paths={})
    for name, _ in paths:
        ms = {k: round(statistics.median(r[k] for r in runs[name]), 3) for k in runs[name][0]}
        out["paths"][name] = dict(ms=ms, total_ms=round(sum(ms.values()), 3), **infos[name])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dense", type=int, nargs="*", default=[512])
    ap.add_argument("--sparse", type=int, nargs="*", default=[2049])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--timeout", type=float, default=900.0, help="seconds per size")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    ap.add_argument("--child", nargs=2, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child is not None:
        print("RESULT " + json.dumps(child(a.child[0], int(a.child[1]), a.reps)))
        return 0
    out = dict(bench="isosurface", device="cuda:0", sizes=[])
    for mode, n in [("dense", n) for n in a.dense] + [("sparse", n) for n in a.sparse]:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, str(n), "--reps", str(a.reps)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
        except subprocess.TimeoutExpired:
            out["error"] = f"{mode} N={n}: timed out after {a.timeout} s"
            break
        res = [ln[7:] for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not res:
            out["error"] = f"{mode} N={n}: exit {p.returncode}: {p.stderr[-800:]}"
            break
        out["sizes"].append(json.loads(res[-1]))
        print(f"{mode} N={n} done", file=sys.stderr, flush=True)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    return 1 if "error" in out else 0


if __name__ == "__main__":
    sys.exit(main())
