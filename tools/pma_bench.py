#!/usr/bin/env python
"""Cost of the catalogue proper-motion anomaly on the device (include/octofitter_hip_draws.h, "The eighteenth"; csrc/draws/octo_draws_pma.hip); writes
profiles/pma_throughput.txt.

    python tools/pma_bench.py [--out profiles/pma_throughput.txt] [--reps 50]

  the evaluation   octo_draws_pma_eval_device on tables of 100 and 300 rows (Q = 6, K = 2: the HGCA's shape), 1 and 2 planets, W = 64, 1 024 and 10 000
                   walkers, sampled and marginal, forward and forward + gradient: HIP events around one call on one stream, median of `reps` after
                   warm-up. The rate is Kepler solves a second, W·n·P a forward call and 2·W·n·P one with a gradient (k_pma_adj solves again). Beside
                   each sampled line, the scan term's sampled time (octo_draws_scan_eval_device, five columns) at the same (n, P, W) in the same run.
                   A shape whose time does not grow with W is launch-bound; the text says which, and names every shape where forward + gradient
                   costs more than twice the forward call.
  the yardstick    in the same run, the main library's config 3 (1 planet, 1e4 RA/Dec epochs × 1e4 walkers, forward + gradient) with
                   OCTO_OPT_BATCH_INVARIANT = 1: the cold loop, the same solve per (walker, row).
  the program      octo_draws_program_logpost_device of one model (one planet, hgca_obs on 50 + 50 scans, D = 7) with the table bound and unbound:
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
from scan_bench import bench_config3      # noqa: E402
from slice_bench import draws_source_hash      # noqa: E402

SEED = 20261021
SIZES = (64, 1024, 10_000)
HGCA_ROW = dict(epoch_ra_hip=1991.31, epoch_dec_hip=1991.18, epoch_ra_gaia=2016.02, epoch_dec_gaia=2016.11,
                pmra_hip=4.7, pmdec_hip=-6.8, pmra_hip_error=0.6, pmdec_hip_error=0.5, pmra_pmdec_hip=0.2,
                pmra_hg=5.05, pmdec_hg=-7.02, pmra_hg_error=0.02, pmdec_hg_error=0.018, pmra_pmdec_hg=0.1,
                pmra_gaia=5.3, pmdec_gaia=-7.4, pmra_gaia_error=0.05, pmdec_gaia_error=0.04, pmra_pmdec_gaia=-0.15)


def bench_tables(pkg, reps, lines):
    import pma_cases as pc
    import scan_cases as sc
    import scan_reference as sref
    rng = np.random.default_rng(SEED)
    over = []
    with pkg.PriorDraws(priors=[pkg.Uniform(0.0, 1.0)]) as pd:
        for n in (100, 300):
            tab, stab = pc.draw_table(rng, n, 6, 2), sc.draw_table(rng, n, 5)
            for P in (1, 2):
                planets = [(sref.VISUAL_KEP, 1)] * P
                pd.pma_set(planets, tab["t"], tab["u"], tab["v"], tab["L"], tab["d"], tab["cov"], tab["H"])
                pd.scan_set(planets, stab["t"], stab["u"], stab["v"], stab["y"], stab["sigma"], stab["c"])
                lines.append(f"\n{n} rows, {P} planet{'s' if P > 1 else ''} ({-(-n // 8)} tasks of 8 rows), Q = 6, K = 2")
                for mode in ("sampled", "marginal"):
                    times = {}
                    for W in SIZES:
                        elems = torch.as_tensor(sc.draw_elements(rng, planets, W), device=pd.device)
                        gamma = torch.as_tensor(rng.normal(size=(2, W)), device=pd.device)
                        beta = torch.as_tensor(rng.normal(size=(5, W)), device=pd.device)
                        jit = torch.as_tensor(rng.uniform(0.1, 1.0, W), device=pd.device)
                        for grad in (False, True):
                            out = pd.pma_eval(elems, gamma, mode=mode, grad=grad)
                            med, lo, hi = event_times(lambda: pd.pma_eval(elems, gamma, mode=mode, grad=grad, out=out), reps)
                            solves = W * n * P * (2 if grad else 1)
                            times[(W, grad)] = med
                            beside = ""
                            if mode == "sampled":
                                sout = pd.scan_eval(elems, beta, jit, grad=grad)
                                beside = f" · the scan term, sampled: {event_times(lambda: pd.scan_eval(elems, beta, jit, grad=grad, out=sout), reps)[0] * 1e6:9.1f} µs"
                            lines.append(f"  {mode:8s} W = {W:>6,d} {'fwd+grad' if grad else 'fwd     '}: {med * 1e6:9.1f} µs (min {lo * 1e6:.1f}, max {hi * 1e6:.1f}) · "
                                         f"{solves / med:.3e} Kepler solves/s{beside}")
                    for grad in (False, True):
                        bound = [W for W in SIZES[:-1] if times[(SIZES[SIZES.index(W) + 1], grad)] < 2.0 * times[(W, grad)]]
                        lines.append(f"  {mode:8s} {'fwd+grad' if grad else 'fwd'}: launch-bound (the next size up costs less than twice as much) at W = {bound or 'none'}")
                    for W in SIZES:
                        ratio = times[(W, True)] / times[(W, False)]
                        lines.append(f"  {mode:8s} W = {W:>6,d}: fwd+grad / fwd = {ratio:.2f}")
                        if ratio > 2.0:
                            over.append(f"n = {n}, P = {P}, {mode}, W = {W:,d}: {ratio:.2f}")
    lines.append("\nshapes where forward + gradient costs more than twice the forward call: " + ("; ".join(over) if over else "none"))


def bench_program(pkg, reps, lines):
    rng = np.random.default_rng(SEED + 1)
    nh = ng = 50
    yr, psi = np.sort(rng.uniform(1990.0, 1993.0, nh)), rng.uniform(0, 2 * np.pi, nh)
    hip = (yr, np.cos(psi), np.sin(psi), rng.uniform(0.8, 2.5, nh), rng.uniform(-0.7, 0.7, nh))
    gaia = (np.sort(rng.uniform(56900.0, 57900.0, ng)), rng.uniform(0, 2 * np.pi, ng), rng.uniform(-0.7, 0.7, ng))
    V = pkg.variables
    obs = pkg.hgca_obs(HGCA_ROW, hip, gaia, variables=V(pmra=pkg.Normal(5.0, 2.0), pmdec=pkg.Normal(-7.0, 2.0)))
    b = pkg.Planet(name="b", basis="Visual{KepOrbit}", observations=[],
                   variables=V(a=pkg.LogUniform(2, 10), e=pkg.Uniform(0.0, 0.6), i=pkg.Uniform(0.3, 1.2), ω=1.1, Ω=2.3, tp=48000.0, mass=pkg.LogUniform(5.0, 60.0)))
    model = pkg.LogDensityModel(pkg.System(name="pma", companions=[b], observations=[obs], variables=V(M=1.1, plx=pkg.truncated(pkg.Normal(50.0, 0.5), lower=1.0))))
    try:
        with pkg.PriorDraws(model) as pd:
            lines.append("\nprogram_logpost of one model (1 planet, 50 + 50 scans, D = 7), the table bound and unbound")
            nodes = model._pma[1]
            for W in SIZES:
                _, tt, _ = pd.sample(SEED, 0, W)
                for grad in (False, True):
                    out = pd.program_logpost(tt, grad=grad)
                    t = {}
                    for name in ("bound", "unbound"):
                        pd.pma_bind(nodes, "sampled") if name == "bound" else pd.pma_unbind()
                        t[name] = event_times(lambda: pd.program_logpost(tt, grad=grad, out=out), reps)[0]
                    pd.pma_bind(nodes, "sampled")
                    lines.append(f"  W = {W:>6,d} {'fwd+grad' if grad else 'fwd     '}: bound {t['bound'] * 1e6:8.1f} µs · unbound {t['unbound'] * 1e6:8.1f} µs · "
                                 f"the term adds {(t['bound'] - t['unbound']) * 1e6:8.1f} µs")
    finally:
        model.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "pma_throughput.txt"))
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pma_bench: no GPU: a timing is a run on the device")
    pkg = load_package()
    lines = [f"the catalogue proper-motion anomaly on {torch.cuda.get_device_name(0)}: HIP events around one call, median of {args.reps}",
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
