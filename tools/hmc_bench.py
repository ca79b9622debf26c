#!/usr/bin/env python
"""Cost of one tempered HMC step on the device (include/octofitter_hip_draws.h: octo_draws_hmc_step_device); writes
profiles/hmc_throughput.txt.

    python tools/hmc_bench.py [--out profiles/hmc_throughput.txt] [--reps 30] [--leapfrog 4]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/hmc_bench.py --trace-only --shape 1      # the kernels' own shares, a run of its own

Three shapes of the D = 11 model of bench.py's logpost workload (one planet, RA/Dec rows): config 5's 8 β x 1 024 chains and 1e4 chains on
the 1e4-row table, and 1 024 chains on a 50-row table. Per shape, from HIP events around one device call, median of `reps` after warm-up:
one octo_draws_hmc_step_device, and (n_leapfrog + 1) x one octo_model_logpost_device with its gradient on the same batch — the step's
log-posterior calls, unchanged code. The difference is what the explorer's own launches (momenta, the opening kernel, one kernel per
leapfrog step) add. --trace-only runs the warmed-up steps alone, for a kernel trace whose statistics give the explorer kernels' share.
No figure is a pass condition.
"""
import argparse
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import numpy as np      # noqa: E402
import torch            # noqa: E402
from __graft_entry__ import load_package      # noqa: E402

SHAPES = (("config 5: 8 β x 1 024 chains, 10 000 rows", 10_000, 8 * 1024, 8),
          ("10 000 chains, 10 000 rows", 10_000, 10_000, 1),
          ("1 024 chains, 50 rows", 50, 1024, 1))


def event_times(fn, reps, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3)
    return statistics.median(ts), min(ts), max(ts)


def make_model(pkg, n_epochs):
    import synth
    cfg0 = synth.config_astrom(n_epochs=n_epochs, n_walkers=16, cfg=3)
    astrom = pkg.PlanetRelAstromObs(cfg0["table"], name="astrom")
    b = pkg.Planet(name="b", basis="Visual{KepOrbit}", observations=[astrom],
                   variables=pkg.variables(a=pkg.LogUniform(1, 100), e=pkg.Uniform(0.0, 0.99), i=pkg.Sine(), ω=pkg.UniformCircular(),
                                           Ω=pkg.UniformCircular(), θ=pkg.UniformCircular(), tp=pkg.θ_at_epoch_to_tperi("θ", 50000)))
    sysm = pkg.System(name="bench", companions=[b], variables=pkg.variables(M=pkg.truncated(pkg.Normal(1.2, 0.1), lower=0.1),
                                                                          plx=pkg.truncated(pkg.Normal(50.0, 0.02), lower=0.1)))
    return pkg.LogDensityModel(sysm)


def bench_shape(pkg, name, n_epochs, W, n_temps, L, reps, lines, trace_only):
    model = make_model(pkg, n_epochs)
    pd = pkg.PriorDraws(model)
    try:
        start = pd.sample(20260929, 0, W, theta=False, logprior_t=False)[1]
        im = pd.sample(20260929, 0, 4096, theta=False, logprior_t=False)[1].var(dim=1).contiguous()
        beta = (torch.linspace(1.0, 0.0, n_temps, dtype=torch.float64, device=start.device) ** 3).repeat_interleave(W // n_temps) if n_temps > 1 else None
        tt = start.clone()
        step = [0]

        def hmc():
            tt.copy_(start)      # every timed step starts from the same states (the copy is inside the bracket: D·W doubles)
            pd.hmc_step(tt, beta=beta, eps=0.01, n_leapfrog=L, inv_mass=im, seed=1, step=step[0])
            step[0] += 1
        if trace_only:
            for _ in range(5 + reps):
                hmc()
            torch.cuda.synchronize()
            return
        t_hmc, lo, hi = event_times(hmc, reps)
        t_lp, lo_lp, hi_lp = event_times(lambda: model.logpost_device(start, grad=True), reps)
        t_cp, _, _ = event_times(lambda: tt.copy_(start), reps)
        own = t_hmc - t_cp - (L + 1) * t_lp
        lines.append(f"\n{name}: D = {model.D}, n_leapfrog = {L}")
        lines.append(f"  one octo_draws_hmc_step_device (+ the reset copy)   : {t_hmc * 1e3:9.3f} ms (min {lo * 1e3:.3f}, max {hi * 1e3:.3f}); the reset copy alone {t_cp * 1e3:.3f} ms")
        lines.append(f"  one octo_model_logpost_device with its gradient    : {t_lp * 1e3:9.3f} ms (min {lo_lp * 1e3:.3f}, max {hi_lp * 1e3:.3f})  = {n_epochs * W / t_lp:.3e} row evaluations/s")
        lines.append(f"  (n_leapfrog + 1) x the log-posterior call           : {(L + 1) * t_lp * 1e3:9.3f} ms; the step takes {(t_hmc - t_cp) / ((L + 1) * t_lp):.3f}x that")
        lines.append(f"  left for the explorer's {(model.D + 3) // 4 + 1 + L} launches                  : {own * 1e3:9.3f} ms = {own / (t_hmc - t_cp):6.1%} of the step; "
                     f"{W / (t_hmc - t_cp):.3e} chain steps/s, {n_epochs * W * (L + 1) / (t_hmc - t_cp):.3e} row evaluations/s inside the step")
    finally:
        pd.close()
        model.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "hmc_throughput.txt"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--leapfrog", type=int, default=4)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--shape", type=int, default=None, help="one of the three shapes (0, 1, 2) instead of all")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("hmc_bench: no GPU: the figures of this file are measured, never estimated")
    pkg = load_package()
    lines = [f"tools/hmc_bench.py on {torch.cuda.get_device_name(0)}: HIP events around one device call, median of {args.reps} after warm-up"]
    for name, n_epochs, W, n_temps in (SHAPES if args.shape is None else SHAPES[args.shape:args.shape + 1]):
        bench_shape(pkg, name, n_epochs, W, n_temps, args.leapfrog, args.reps, lines, args.trace_only)
    if args.trace_only:
        return
    text = "\n".join(lines) + "\n"
    print(text)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
