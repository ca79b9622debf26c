#!/usr/bin/env python
"""Cost of the batched L-BFGS on the device (include/octofitter_hip_draws.h: octo_draws_lbfgs_device); writes profiles/lbfgs_throughput.txt.

    python tools/lbfgs_bench.py [--out profiles/lbfgs_throughput.txt] [--reps 30] [--rounds 20]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/lbfgs_bench.py --trace-only --shape 1      # the advance kernel's own time, a run of its own

Three shapes of the D = 11 model of tools/hmc_bench.py (one planet, RA/Dec rows): 64 and 1 024 chains on a 50-row table, 1e4 chains on the
1e4-row table. Per shape, from HIP events around one device call, median of `reps` after warm-up: one octo_draws_lbfgs_device of `rounds`
rounds from prior draws (rounds + 1 log-posterior calls and as many advance launches) and one octo_model_logpost_device with its gradient on
the same batch; a round's own cost is the difference per round. Then optimize_starting_points_device end to end (wall clock around a call
that ends in a read) against scipy's L-BFGS-B over the host callback from the same 64 starts. --trace-only runs the warmed-up calls alone.
No figure is a pass condition.
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

SHAPES = (("64 chains, 50 rows", 50, 64), ("1 024 chains, 50 rows", 50, 1024), ("10 000 chains, 10 000 rows", 10_000, 10_000))
SEED = 20260929


def bench_shape(pkg, name, n_epochs, W, m, rounds, reps, lines, trace_only):
    model = make_model(pkg, n_epochs)
    pd = pkg.PriorDraws(model)
    try:
        start = pd.sample(SEED, 0, W, theta=False, logprior_t=False)[1]
        v = pd.sample(SEED, 0, 4096, theta=False, logprior_t=False)[1].var(dim=1).contiguous()
        tt = start.clone()
        last = [None]

        def run():
            tt.copy_(start)      # every timed call starts from the same states (the copy is inside the bracket: D·W doubles)
            last[0] = pd.lbfgs(tt, inv_mass=v, m=m, n_rounds=rounds, gtol=0.0)
        if trace_only:
            for _ in range(5 + reps):
                run()
            torch.cuda.synchronize()
            return
        t_run, lo, hi = event_times(run, reps)
        t_lp, lo_lp, hi_lp = event_times(lambda: model.logpost_device(start, grad=True), reps)
        t_cp, _, _ = event_times(lambda: tt.copy_(start), reps)
        calls = rounds + 1
        own = (t_run - t_cp - calls * t_lp) / calls
        acc = float(last[0]["iters"].double().mean()) / rounds
        lines.append(f"\n{name}: D = {model.D}, m = {m}, {rounds} rounds a call, {acc:.2f} of the decisions accept")
        lines.append(f"  one octo_draws_lbfgs_device (+ the reset copy)      : {t_run * 1e3:9.3f} ms (min {lo * 1e3:.3f}, max {hi * 1e3:.3f}); the reset copy alone {t_cp * 1e3:.3f} ms")
        lines.append(f"  one octo_model_logpost_device with its gradient    : {t_lp * 1e3:9.3f} ms (min {lo_lp * 1e3:.3f}, max {hi_lp * 1e3:.3f})  = {n_epochs * W / t_lp:.3e} row evaluations/s")
        lines.append(f"  one round (log-posterior call + advance launch)    : {(t_run - t_cp) / calls * 1e3:9.3f} ms = {(t_run - t_cp) / (calls * t_lp):.3f}x the log-posterior call")
        lines.append(f"  left for the advance launch                        : {own * 1e3:9.3f} ms = {own * calls / (t_run - t_cp):6.1%} of the round; {W * calls / (t_run - t_cp):.3e} chain rounds/s")
    finally:
        pd.close()
        model.close()


def end_to_end(pkg, lines):
    """optimize_starting_points_device against scipy over the host callback, the model of the tests (D = 14, 12 RA/Dec epochs, 8 RV rows)"""
    from scipy.optimize import minimize
    import test_lbfgs
    model = test_lbfgs.tight_model(pkg)
    try:
        kw = dict(N=65536, n_starts=64, seed=77)
        pkg.optimize_starting_points_device(model, **kw)      # warm-up: code objects, the work arrays
        ts = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = pkg.optimize_starting_points_device(model, **kw)
            ts.append(time.perf_counter() - t0)
        pd = pkg.PriorDraws(model)
        θ0, _, _ = pd.best(77, 65536, keep=64)
        v = pd.sample(77, 0, 4096, theta=False, logprior_t=False)[1].var(dim=1).cpu().numpy()
        pd.close()
        sc, starts = np.sqrt(v), model.link(θ0)

        def fun(z):
            lp, g = model.ᐁℓπcallback(z * sc)
            return -float(lp), -g * sc
        t0 = time.perf_counter()
        res = [minimize(fun, starts[:, w] / sc, jac=True, method="L-BFGS-B", options=dict(maxiter=5000, maxfun=20000, ftol=1e-15, gtol=1e-7, maxcor=10)) for w in range(64)]
        t_scipy = time.perf_counter() - t0
        lines.append(f"\nend to end, 64 starts of 65 536 prior draws, D = {model.D}, gtol 1e-6 (wall clock, median of 5 for the device):")
        lines.append(f"  optimize_starting_points_device (draws, ranking, optimiser) : {sorted(ts)[2]:8.3f} s; status counts {np.bincount(out['status'], minlength=5)}, "
                     f"evaluations a chain {out['evals'].min()} … {out['evals'].max()}, best ℓπ {out['logpost'].max():.8f}")
        lines.append(f"  scipy L-BFGS-B over the host callback, one θ a call, from the same starts : {t_scipy:8.3f} s; {sum(r.nfev for r in res)} evaluations, "
                     f"best ℓπ {max(-r.fun for r in res):.8f}")
    finally:
        model.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "lbfgs_throughput.txt"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--m", type=int, default=6)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--shape", type=int, default=None, help="one of the three shapes (0, 1, 2) instead of all")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lbfgs_bench: no GPU: the figures of this file are measured, never estimated")
    pkg = load_package()
    lines = [f"tools/lbfgs_bench.py on {torch.cuda.get_device_name(0)}: HIP events around one device call, median of {args.reps} after warm-up"]
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
