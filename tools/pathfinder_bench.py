#!/usr/bin/env python
"""Cost of Pathfinder on the device (include/octofitter_hip_draws.h: octo_draws_pathfinder_device, octo_draws_pathfinder_draw_device); writes
profiles/pathfinder_throughput.txt.

    python tools/pathfinder_bench.py [--out profiles/pathfinder_throughput.txt] [--reps 30] [--rounds 20]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/pathfinder_bench.py --trace-only --shape 1      # k_pf_fit's own time, a run of its own

The three shapes of tools/lbfgs_bench.py (the D = 11 model of tools/hmc_bench.py: 64 and 1 024 chains on a 50-row table, 1e4 chains on the
1e4-row table). Per shape, from HIP events around one device call, median of `reps` after warm-up: one octo_draws_pathfinder_device of `rounds`
rounds (n_elbo = 5) against one octo_draws_lbfgs_device of as many rounds from the same starts — the ratio beside 1 + n_elbo, the ratio of
log-posterior columns a round — and one octo_draws_pathfinder_draw_device of 256 draws a chain. Then pathfinder_device end to end on the
tight model of the tests against optimize_starting_points_device (wall clock around a call that ends in a read). --trace-only runs the
warmed-up pathfinder calls alone. No figure is a pass condition.
"""
import argparse
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests")); sys.path.insert(0, str(ROOT / "tools"))
import numpy as np      # noqa: E402
import torch            # noqa: E402
from __graft_entry__ import load_package      # noqa: E402
from hmc_bench import event_times, make_model      # noqa: E402
from lbfgs_bench import SEED, SHAPES      # noqa: E402

N_ELBO, N_FINAL = 5, 256


def bench_shape(pkg, name, n_epochs, W, m, rounds, reps, lines, trace_only):
    model = make_model(pkg, n_epochs)
    pd = pkg.PriorDraws(model)
    try:
        start = pd.sample(SEED, 0, W, theta=False, logprior_t=False)[1]
        v = pd.sample(SEED, 0, 4096, theta=False, logprior_t=False)[1].var(dim=1).contiguous()
        tt = start.clone()
        last = [None]

        def run_pf():
            tt.copy_(start)      # every timed call starts from the same states (the copy is inside the bracket: D·W doubles)
            last[0] = pd.pathfinder(tt, inv_mass=v, m=m, n_rounds=rounds, gtol=0.0, seed=SEED, n_elbo=N_ELBO)

        def run_lb():
            tt.copy_(start)
            pd.lbfgs(tt, inv_mass=v, m=m, n_rounds=rounds, gtol=0.0)
        if trace_only:
            for _ in range(5 + reps):
                run_pf()
            torch.cuda.synchronize()
            return
        t_lb, lo_lb, hi_lb = event_times(run_lb, reps)
        t_pf, lo, hi = event_times(run_pf, reps)      # leaves the handle with the fits of `rounds` rounds
        t_dr, lo_dr, hi_dr = event_times(lambda: pd.pathfinder_draw(tt, N_FINAL, seed=SEED), reps)
        t_cp, _, _ = event_times(lambda: tt.copy_(start), reps)
        t_lp, _, _ = event_times(lambda: model.logpost_device(start, grad=True), reps)
        r = {k: x.cpu().numpy() for k, x in last[0].items() if x is not None}
        extra = (t_pf - t_lb) / rounds
        lines.append(f"\n{name}: D = {model.D}, m = {m}, {rounds} rounds a call, n_elbo = {N_ELBO}; fits a chain {r['n_fits'].min()} … {r['n_fits'].max()}, "
                     f"{np.sum(r['elbo_iter'] >= 0)} of {W} chains with a kept fit")
        lines.append(f"  one octo_draws_lbfgs_device (+ the reset copy)       : {t_lb * 1e3:9.3f} ms (min {lo_lb * 1e3:.3f}, max {hi_lb * 1e3:.3f}); the reset copy alone {t_cp * 1e3:.3f} ms")
        lines.append(f"  one octo_draws_pathfinder_device (+ the reset copy)  : {t_pf * 1e3:9.3f} ms (min {lo * 1e3:.3f}, max {hi * 1e3:.3f})")
        lines.append(f"  pathfinder / L-BFGS                                  : {(t_pf - t_cp) / (t_lb - t_cp):9.3f}   beside 1 + n_elbo = {1 + N_ELBO}, the ratio of log-posterior columns")
        lines.append(f"  what a round adds (fit, normals, map, ELBO batch)    : {extra * 1e3:9.3f} ms; one log-posterior call of W columns with its gradient {t_lp * 1e3:.3f} ms")
        lines.append(f"  one octo_draws_pathfinder_draw_device, {N_FINAL} a chain  : {t_dr * 1e3:9.3f} ms (min {lo_dr * 1e3:.3f}, max {hi_dr * 1e3:.3f}) = {N_FINAL * W / t_dr:.3e} draws/s, ℓπ included")
    finally:
        pd.close()
        model.close()


def end_to_end(pkg, lines):
    """pathfinder_device against optimize_starting_points_device, the model of the tests (D = 14, 12 RA/Dec epochs, 8 RV rows)"""
    import test_lbfgs
    model = test_lbfgs.tight_model(pkg)
    try:
        kw = dict(N=65536, seed=77)
        ts = {}
        for label, fn in (("opt", lambda: pkg.optimize_starting_points_device(model, n_starts=64, **kw)), ("pf", lambda: pkg.pathfinder_device(model, n_paths=64, **kw))):
            fn()      # warm-up: code objects, the work arrays
            t = []
            for _ in range(5):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = fn()
                t.append(time.perf_counter() - t0)
            ts[label] = (sorted(t)[2], out)
        (t_opt, opt), (t_pf, pf) = ts["opt"], ts["pf"]
        lines.append(f"\nend to end, 64 starts of 65 536 prior draws, D = {model.D}, gtol 1e-6 (wall clock, median of 5):")
        lines.append(f"  optimize_starting_points_device (draws, ranking, optimiser)            : {t_opt:8.3f} s; evaluations a chain {opt['evals'].min()} … {opt['evals'].max()}, "
                     f"best ℓπ {opt['logpost'].max():.8f}")
        lines.append(f"  pathfinder_device (the same, fits and ELBOs, 256 draws a path, PSIS, 1000 resampled) : {t_pf:8.3f} s = {t_pf / t_opt:.2f}x; k̂ {pf['pareto_k']:.3f}, "
                     f"best ELBO {pf['elbo'].max():.4f}, kept iterates {pf['elbo_iter'].min()} … {pf['elbo_iter'].max()} of {pf['iters'].min()} … {pf['iters'].max()}, "
                     f"{np.unique(pf['path']).size} paths among the draws, their ℓπ {pf['logpost'].min():.3f} … {pf['logpost'].max():.3f}")
    finally:
        model.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "pathfinder_throughput.txt"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--m", type=int, default=6)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--shape", type=int, default=None, help="one of the three shapes (0, 1, 2) instead of all")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pathfinder_bench: no GPU: the figures of this file are measured, never estimated")
    pkg = load_package()
    lines = [f"tools/pathfinder_bench.py on {torch.cuda.get_device_name(0)}: HIP events around one device call, median of {args.reps} after warm-up"]
    for name, n_epochs, W in (SHAPES if args.shape is None else SHAPES[args.shape:args.shape + 1]):
        bench_shape(pkg, name, n_epochs, W, args.m, args.rounds, args.reps, lines, args.trace_only)
    if args.trace_only:
        return
    end_to_end(pkg, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
