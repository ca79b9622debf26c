#!/usr/bin/env python
"""Cost of along-scan absolute astrometry on the device (include/octofitter_hip_draws.h, "The seventeenth"; csrc/draws/octo_draws_scan.hip); writes
profiles/scan_throughput.txt.

    python tools/scan_bench.py [--out profiles/scan_throughput.txt] [--reps 50]

  the evaluation   octo_draws_scan_eval_device on tables of 100 and 300 rows (five columns), 1 and 2 planets, W = 64, 1 024 and 10 000 walkers, sampled
                   and marginal, forward and forward + gradient: HIP events around one call on one stream, median of `reps` after warm-up. The rate is
                   Kepler solves a second, W·n·P a sampled call and 2·W·n·P a marginal one (its two passes). A shape whose time does not grow with W
                   is launch-bound: the launches and one wave's chain, not the device's arithmetic; the text says which.
  the yardstick    in the same run, the main library's config 3 (1 planet, 1e4 RA/Dec epochs × 1e4 walkers, forward + gradient) with
                   OCTO_OPT_BATCH_INVARIANT = 1: the cold loop, the same solve per (walker, row).
  the program      octo_draws_program_logpost_device of one model (one planet, a 100-row Hipparcos table, D = 8) with the table bound and unbound:
                   the added cost of the term in a sampler's callback.
The header records the hashes of the sources the figures belong to. No figure is a pass condition.
"""
import argparse
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests")); sys.path.insert(0, str(ROOT / "tools"))
import numpy as np      # noqa: E402
import torch            # noqa: E402
from __graft_entry__ import kernel_source_hash, load_package      # noqa: E402
from hmc_bench import event_times      # noqa: E402
from slice_bench import draws_source_hash      # noqa: E402

SEED = 20261021
SIZES = (64, 1024, 10_000)


def bench_tables(pkg, reps, lines):
    import scan_cases as sc
    import scan_reference as sref
    rng = np.random.default_rng(SEED)
    with pkg.PriorDraws(priors=[pkg.Uniform(0.0, 1.0)]) as pd:
        for n in (100, 300):
            tab = sc.draw_table(rng, n, 5)
            for P in (1, 2):
                planets = [(sref.VISUAL_KEP, 1)] * P
                pd.scan_set(planets, tab["t"], tab["u"], tab["v"], tab["y"], tab["sigma"], tab["c"])
                lines.append(f"\n{n} rows, {P} planet{'s' if P > 1 else ''} ({-(-n // 8)} tasks of 8 rows)")
                for mode in ("sampled", "marginal"):
                    times = {}
                    for W in SIZES:
                        elems = torch.as_tensor(sc.draw_elements(rng, planets, W), device=pd.device)
                        beta = torch.as_tensor(rng.normal(size=(5, W)), device=pd.device)
                        jit = torch.as_tensor(rng.uniform(0.1, 1.0, W), device=pd.device)
                        for grad in (False, True):
                            out = pd.scan_eval(elems, beta, jit, mode=mode, grad=grad)
                            med, lo, hi = event_times(lambda: pd.scan_eval(elems, beta, jit, mode=mode, grad=grad, out=out), reps)
                            solves = W * n * P * (2 if mode == "marginal" else 1)
                            times[(W, grad)] = med
                            lines.append(f"  {mode:8s} W = {W:>6,d} {'fwd+grad' if grad else 'fwd     '}: {med * 1e6:9.1f} µs (min {lo * 1e6:.1f}, max {hi * 1e6:.1f}) · "
                                         f"{solves / med:.3e} Kepler solves/s")
                    for grad in (False, True):
                        bound = [W for W in SIZES[:-1] if times[(SIZES[SIZES.index(W) + 1], grad)] < 2.0 * times[(W, grad)]]
                        lines.append(f"  {mode:8s} {'fwd+grad' if grad else 'fwd'}: launch-bound (the next size up costs less than twice as much) at W = {bound or 'none'}")


def bench_config3(pkg, reps, lines):
    import synth
    cfg = synth.config_astrom(cfg=3)
    astrom = pkg.PlanetRelAstromObs(cfg["table"], name="astrom")
    b = pkg.Planet(name="b", basis="Visual{KepOrbit}", observations=[astrom])
    fn = pkg.make_ln_like(pkg.System(name="bench", companions=[b], observations=[]), cfg["theta_example"])
    try:
        fn.set_option(pkg.capi.OPT_BATCH_INVARIANT, 1)
        elems = torch.as_tensor(cfg["elems"], device="cuda")
        out = fn.ln_like_device(elems, grad=True)
        med, lo, hi = event_times(lambda: fn.ln_like_device(elems, grad=True, out=out), max(reps // 5, 5))
        solves = cfg["n_epochs"] * cfg["n_walkers"]
        lines.append(f"\nthe yardstick: config 3 (1 planet, {cfg['n_epochs']} epochs × {cfg['n_walkers']} walkers, fwd+grad) with OCTO_OPT_BATCH_INVARIANT = 1 (the cold loop): "
                     f"{med * 1e3:.3f} ms (min {lo * 1e3:.3f}, max {hi * 1e3:.3f}) · {solves / med:.3e} Kepler solves/s")
    finally:
        fn.close()


def bench_program(pkg, reps, lines):
    rng = np.random.default_rng(SEED + 1)
    n = 100
    yr = np.sort(rng.uniform(1990.0, 1993.0, n))
    psi = rng.uniform(0, 2 * np.pi, n)
    V = pkg.variables
    obs = pkg.hipparcos_iad_obs(yr, rng.uniform(-0.7, 0.7, n), np.cos(psi), np.sin(psi), rng.normal(size=n) * 1.5, rng.uniform(0.8, 2.0, n), 50.0, 3.0, -2.0,
                                variables=V(dra=pkg.Normal(0, 5), ddec=pkg.Normal(0, 5), plx=pkg.Derived(lambda obs, system: system.plx), pmra=pkg.Normal(0, 5),
                                            pmdec=pkg.Normal(0, 5), jitter=0.3))
    b = pkg.Planet(name="b", basis="Visual{KepOrbit}", observations=[],
                   variables=V(a=pkg.LogUniform(2, 10), e=pkg.Uniform(0.0, 0.6), i=0.9, ω=1.1, Ω=2.3, tp=48000.0, mass=pkg.LogUniform(5.0, 60.0)))
    model = pkg.LogDensityModel(pkg.System(name="scan", companions=[b], observations=[obs], variables=V(M=1.1, plx=pkg.truncated(pkg.Normal(50.0, 0.5), lower=1.0))))
    try:
        with pkg.PriorDraws(model) as pd:
            lines.append("\nprogram_logpost of one model (1 planet, 100 rows, D = 8), the table bound and unbound")
            nodes = model._scan[1]
            for W in SIZES:
                _, tt, _ = pd.sample(SEED, 0, W)
                for grad in (False, True):
                    out = pd.program_logpost(tt, grad=grad)
                    t = {}
                    for name in ("bound", "unbound"):
                        pd.scan_bind(nodes, "sampled") if name == "bound" else pd.scan_unbind()
                        t[name] = event_times(lambda: pd.program_logpost(tt, grad=grad, out=out), reps)[0]
                    pd.scan_bind(nodes, "sampled")
                    lines.append(f"  W = {W:>6,d} {'fwd+grad' if grad else 'fwd     '}: bound {t['bound'] * 1e6:8.1f} µs · unbound {t['unbound'] * 1e6:8.1f} µs · "
                                 f"the term adds {(t['bound'] - t['unbound']) * 1e6:8.1f} µs")
    finally:
        model.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "scan_throughput.txt"))
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("scan_bench: no GPU: a timing is a run on the device")
    pkg = load_package()
    lines = [f"along-scan absolute astrometry on {torch.cuda.get_device_name(0)}: HIP events around one call, median of {args.reps}",
             f"main library source hash {kernel_source_hash()[:16]} · draws library source hash {draws_source_hash()[:16]}"]
    bench_tables(pkg, args.reps, lines)
    bench_config3(pkg, args.reps, lines)
    bench_program(pkg, args.reps, lines)
    text = "\n".join(lines) + "\n"
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)
    print(text)


if __name__ == "__main__":
    main()
