#!/usr/bin/env python
"""Starting points and rejection from prior draws: the device route (host/draws.py: PriorDraws — draws, link, log-posterior, selection and
accept / compaction on the GPU) against the route that existed before it (host/callers.py: guess_starting_position / octofit_rejection —
NumPy draws and link, a [D][N] host-to-device copy per batch, argmax / accept on the host).

    python tools/draws_latency.py                  # 20 timed repetitions of each route, alternating, after a warm-up -> text on stdout
    python tools/draws_latency.py --once           # one call of each device driver after a warm-up: the target of a kernel trace
                                                   #   rocprofv3 --kernel-trace --stats -d DIR -o k -- python tools/draws_latency.py --once
    python tools/draws_latency.py --kernel-db DB   # append the kernel split and the draw kernel's share of HBM bandwidth from that trace

Shape: one planet, a 50-row RA/Dec table, the D = 11 standard parameterisation; N = 5e5 draws for the starting point, 1e5 for rejection.
The clock is the host's around the blocking call (both routes end with their results on the host).
"""
import argparse
import sqlite3
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

HBM_PEAK = 8.0e12          # bytes/s, MI355X data sheet
SAMPLE_N = 1 << 20         # draws per call of the public sampler in --once


def build_model(pkg):
    import synth
    rng = np.random.default_rng(5)
    t = 50000.0 + 30.0 * np.arange(50)
    ra, dec = synth.truth_radec(t)
    table = dict(epoch=t, ra=ra + rng.normal(0, 10.0, 50), dec=dec + rng.normal(0, 10.0, 50), σ_ra=np.full(50, 10.0), σ_dec=np.full(50, 10.0))
    astrom = pkg.PlanetRelAstromObs(table, name="sim")
    b = pkg.Planet(name="b", basis="Visual{KepOrbit}", observations=[astrom],
                   variables=pkg.variables(a=pkg.LogUniform(5, 20), e=pkg.Uniform(0.0, 0.6), i=pkg.Sine(), ω=pkg.UniformCircular(),
                                           Ω=pkg.UniformCircular(), θ=pkg.UniformCircular(), tp=pkg.θ_at_epoch_to_tperi("θ", 50000)))
    sys_ = pkg.System(name="sim", companions=[b], observations=[],
                      variables=pkg.variables(M=pkg.truncated(pkg.Normal(1.2, 0.05), lower=0.1), plx=pkg.truncated(pkg.Normal(50.0, 0.1), lower=0.1)))
    return pkg.LogDensityModel(sys_)


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def summary(ms):
    ms = np.asarray(ms)
    return f"median {np.median(ms):9.3f} ms   min {ms.min():9.3f}   max {ms.max():9.3f}   (n = {ms.size})"


def kernel_split(db, D, n_best, n_rej):
    """Per-kernel totals of a `rocprofv3 --kernel-trace` database of `--once`, grouped into draw / log-posterior / selection / compaction."""
    con = sqlite3.connect(db)
    rows = con.execute("select name, count(*), sum(duration) / 1e3, avg(duration) / 1e3 from kernels group by name order by sum(duration) desc").fetchall()
    groups = {"draw": 0.0, "log-posterior": 0.0, "selection": 0.0, "compaction": 0.0, "copies and fills": 0.0}
    lines = [f"{'kernel':60s} {'calls':>6s} {'total_us':>12s} {'avg_us':>10s}"]
    for name, calls, tot, avg in rows:
        name = name.replace("(anonymous namespace)::", "")
        short = name.split("(")[0]
        if "k_draw" in short: g = "draw"
        elif "k_topk" in short: g = "selection"
        elif any(k in short for k in ("k_loglike", "k_max", "k_count", "k_scan", "k_scatter")): g = "compaction"
        elif "rocclr" in short or "k_kepler" in short: g = "copies and fills"      # (k_kepler: the one-element call of octo_draws_destroy)
        else: g = "log-posterior"
        groups[g] += tot
        lines.append(f"{name[:60]:60s} {calls:6d} {tot:12.3f} {avg:10.3f}")
    total = sum(groups.values())
    lines.append("split (warm-up calls and the five sampler calls included): " + "   ".join(f"{k} {v:.1f} us ({100 * v / total:.1f} %)" for k, v in groups.items()))
    # the public sampler (θ, θ_t and logprior_t of SAMPLE_N draws, the largest grid of the trace): one launch per Philox block of four coordinates
    big = con.execute("select grid_x, count(*), sum(duration), avg(duration) from kernels where name like '%k_draw%' group by grid_x order by grid_x desc").fetchall()
    if big:
        grid, calls, tot_ns, avg_ns = big[0]
        nblk = (D + 3) // 4
        n_calls = calls / nblk
        per_draw = 16 * D + 8
        rate = per_draw * SAMPLE_N * n_calls / (tot_ns * 1e-9)
        lines.append(f"k_draw, sampler calls of {SAMPLE_N} draws (grid_x {grid}): {calls} launches = {n_calls:.0f} calls x {nblk} coordinate blocks, {avg_ns / 1e3:.2f} us per launch, "
                     f"{tot_ns / 1e3 / n_calls:.2f} us per call")
        lines.append(f"  {per_draw} bytes stored per draw (16 D + 8) over the kernel time of a call: {rate / 1e12:.3f} TB/s = {rate / HBM_PEAK:.3f} of the {HBM_PEAK / 1e12:.1f} TB/s HBM peak")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--kernel-db")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--n-best", type=int, default=500_000)
    ap.add_argument("--n-rejection", type=int, default=100_000)
    a = ap.parse_args()
    if a.kernel_db:
        print(kernel_split(a.kernel_db, 11, a.n_best, a.n_rejection))
        return
    from __graft_entry__ import load_package
    pkg = load_package()
    from octofitter_jl_amd.host.draws import DRAWS_LIB_PATH, PriorDraws
    model = build_model(pkg)
    assert model.D == 11
    pd = PriorDraws(model)
    rng = np.random.default_rng(0)
    dev_best = lambda seed: pd.best(seed, a.n_best, keep=1)                                   # noqa: E731
    host_best = lambda seed: pkg.guess_starting_position(rng, model, a.n_best)                # noqa: E731
    dev_rej = lambda seed: pd.rejection(seed, a.n_rejection)                                  # noqa: E731
    host_rej = lambda seed: pkg.octofit_rejection(rng, model, draws=a.n_rejection)            # noqa: E731
    for f in (dev_best, dev_rej):
        f(1000)
    if a.once:
        import torch
        dev_best(1)
        dev_rej(1)
        for k in range(5):
            pd.sample(1, k * SAMPLE_N, SAMPLE_N)
        torch.cuda.synchronize()
        pd.close(); model.close()
        return
    for f in (host_best, host_rej):
        f(1000)
    t = {k: [] for k in ("dev_best", "host_best", "dev_rej", "host_rej")}
    acc = []
    for r in range(a.reps):
        t["dev_best"].append(timed(lambda: dev_best(r))[0])
        t["host_best"].append(timed(lambda: host_best(r))[0])
        ms, out = timed(lambda: dev_rej(r))
        t["dev_rej"].append(ms); acc.append(out["n_accepted"])
        t["host_rej"].append(timed(lambda: host_rej(r))[0])
    print(f"shape: 1 planet, 50 RA/Dec rows, D = {model.D}; host clock around the blocking call, routes alternating in one process")
    print(f"starting point, N = {a.n_best} draws")
    print(f"  device route  PriorDraws.best                 {summary(t['dev_best'])}")
    print(f"  host route    guess_starting_position         {summary(t['host_best'])}")
    print(f"  ratio of medians host / device: {np.median(t['host_best']) / np.median(t['dev_best']):.1f}")
    print(f"rejection, N = {a.n_rejection} draws (accepted per run: min {min(acc)}, median {int(np.median(acc))}, max {max(acc)})")
    print(f"  device route  PriorDraws.rejection            {summary(t['dev_rej'])}")
    print(f"  host route    octofit_rejection               {summary(t['host_rej'])}")
    print(f"  ratio of medians host / device: {np.median(t['host_rej']) / np.median(t['dev_rej']):.1f}")
    print(f"liboctofitter_hip_draws.so: {DRAWS_LIB_PATH.stat().st_size} bytes")
    pd.close(); model.close()


if __name__ == "__main__":
    main()
