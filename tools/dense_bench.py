#!/usr/bin/env python
"""What the dense metric costs per round and what it buys per gradient (include/octofitter_hip_draws.h, the fourteenth part);
writes profiles/dense_throughput.txt.

    python tools/dense_bench.py [--out profiles/dense_throughput.txt] [--reps 30] [--max-depth 10] [--warmup 200] [--transitions 20] [--part a|b]

HIP events around the calls, median of `reps` after warm-up, the method of tools/nuts_bench.py.
  (a) the cost of a round. A k_nuts_leaf round is the difference of two opening calls of 8 and 24 rounds over 16 (ε tiny: no chain turns), a
      k_hmc_leap<STEP> round the difference of two steps of 9 and 25 leapfrogs over 16 — each with the diagonal metric and under use_metric with
      the factor of the same diagonal, so that both make the same trajectory. On the 50-row and the 10 000-row table of tools/adapt_bench.py at
      8 192 chains (the model's D = 11), and on a prior-only handle at D = 64. Reported: the extra µs per round and its share of the diagonal round.
  (b) what the metric is for. On both tables at their chains of tools/adapt_bench.py: Pathfinder's draws, hmc_warmup(max_depth=…) for `warmup`
      rounds with metric="diag" and metric="dense" (the same seed, the same budget), then `transitions` transitions with ε and the metric fixed:
      mean depth, mean n_leapfrog, divergences per transition, and min over the coordinates of ess_bulk (PriorDraws.diagnose of the recorded θ_t)
      per gradient evaluation.
No figure is a pass condition.
"""
import argparse
import importlib
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tools")); sys.path.insert(0, str(ROOT / "tests"))
import torch            # noqa: E402
from __graft_entry__ import load_package      # noqa: E402
from adapt_bench import SHAPES      # noqa: E402
from hmc_bench import event_times, make_model      # noqa: E402

SEED = 20261019
CHECK_FROM = 3
COST_W = 8192


def round_costs(pkg, pd, start, im, reps, lines):
    """(a) on one handle: the four rounds, diagonal and dense"""
    chol = importlib.import_module(pkg.__name__ + ".host.draws").pack_lower(torch.diag(torch.sqrt(im)))
    tt = start.clone()
    n = [0]

    def hmc(L, mass):
        def run():
            tt.copy_(start)
            pd.hmc_step(tt, eps=1e-4, n_leapfrog=L, inv_mass=mass, seed=1, step=n[0])
            n[0] += 1
        return run

    def nuts(rounds, mass):
        def run():
            tt.copy_(start)
            pd.nuts(tt, eps=1e-4, inv_mass=mass, max_depth=10, n_rounds=rounds, seed=1, step=n[0])
            n[0] += 1
        return run

    out = {}
    for name, factor, mass in (("diagonal", None, im), ("dense", chol, None)):
        pd.use_metric(factor)
        t_h9, t_h25 = event_times(hmc(9, mass), reps)[0], event_times(hmc(25, mass), reps)[0]
        t_n8, t_n24 = event_times(nuts(8, mass), reps)[0], event_times(nuts(24, mass), reps)[0]
        out[name] = ((t_h25 - t_h9) / 16, (t_n24 - t_n8) / 16)
    pd.use_metric(None)
    for k, kernel in enumerate(("k_hmc_leap<STEP>", "k_nuts_leaf")):
        d, e = out["diagonal"][k], out["dense"][k]
        lines.append(f"  one {kernel:<17} round: diagonal {d * 1e6:9.1f} µs, k_dense twin {e * 1e6:9.1f} µs: {(e - d) * 1e6:+9.1f} µs = {(e - d) / d:+7.2%} of the diagonal round")


def part_a(pkg, reps, lines):
    lines.append("\n(a) the cost of a round: the log-posterior call and one kernel, (call of 25 − call of 9 leapfrogs)/16 and (24 − 8 rounds)/16")
    for name, n_epochs, _W, _T in SHAPES:
        model = make_model(pkg, n_epochs)
        pd = pkg.PriorDraws(model)
        try:
            start = pd.sample(SEED, 0, COST_W, theta=False, logprior_t=False)[1]
            im = pd.sample(SEED, 0, 4096, theta=False, logprior_t=False)[1].var(dim=1).contiguous()
            lines.append(f"\n{n_epochs} rows ({name.split(':')[0]}): D = {model.D}, {COST_W} chains")
            round_costs(pkg, pd, start, im, reps, lines)
        finally:
            pd.close()
            model.close()
    D = 64
    kinds = [pkg.Uniform(-3, 7), pkg.LogUniform(0.1, 1000), pkg.Normal(1.2, 0.05), pkg.Sine(), pkg.truncated(pkg.Normal(0, 1), lower=3)]
    pd = pkg.PriorDraws(priors=[kinds[d % 5] for d in range(D)])
    try:
        start = pd.sample(SEED, 0, COST_W, theta=False, logprior_t=False)[1]
        im = start.var(dim=1).contiguous()
        lines.append(f"\npriors alone: D = {D}, {COST_W} chains (no log-posterior call: the round is the kernel)")
        round_costs(pkg, pd, start, im, reps, lines)
    finally:
        pd.close()


def sample_after_warmup(pkg, pd, model, W, metric, im, max_depth, n_warmup, n_trans, dev):
    theta_t = torch.as_tensor(pkg.pathfinder_device(model, n_draws=W, seed=SEED)["theta_t"], dtype=torch.float64, device=dev).contiguous()
    wu = pkg.hmc_warmup(pd, theta_t, n_warmup, eps=0.05, inv_mass=im, seed=SEED, max_depth=max_depth, metric=metric)
    eps_w = wu["eps"].expand(W).contiguous()
    tree = wu["tree"].cpu().numpy()
    dense = metric == "dense"
    pd.use_metric(importlib.import_module(pkg.__name__ + ".host.draws").pack_lower(wu["metric_chol"]) if dense else None)
    mass = None if dense else wu["inv_mass"]
    rec = torch.empty((n_trans, model.D, W), dtype=torch.float64, device=dev)
    depth_s = leaves = div = 0.0
    for k in range(n_trans):
        _lp, _ll, _la, _acc, depth, nleaf, dv = pd.nuts_step(theta_t, eps=eps_w, inv_mass=mass, max_depth=max_depth, seed=SEED, step=n_warmup + k, check_from=CHECK_FROM)
        rec[k] = theta_t
        depth_s += float(depth.double().mean()); leaves += float(nleaf.double().mean()); div += float(dv.sum())
    t_tr = event_times(lambda: pd.nuts_step(theta_t, eps=eps_w, inv_mass=mass, max_depth=max_depth, seed=SEED, step=n_warmup + n_trans, check_from=CHECK_FROM), 3, warmup=1)
    ess = pd.diagnose(rec)["ess_bulk"]
    pd.use_metric(None)
    grads = leaves * W                                   # Σ over the transitions and the chains of n_leapfrog
    corr = None
    if dense:
        L = wu["metric_chol"]
        S = L @ L.T
        sd = torch.sqrt(torch.diag(S))
        corr = float(((S / torch.outer(sd, sd)) - torch.eye(model.D, dtype=torch.float64, device=dev)).abs().max())
    return dict(eps=float(wu["eps"][0]), wu_depth=tree[-10:, 0].mean(), wu_leaves=tree[-10:, 1].mean(), wu_div=int(tree[-10:, 2].sum()), depth=depth_s / n_trans,
                leaves=leaves / n_trans, div=div / n_trans, ess_min=float(ess.min()), ess_per_grad=float(ess.min()) / grads, ms=t_tr[0] * 1e3, corr=corr)


def part_b(pkg, max_depth, n_warmup, n_trans, lines):
    lines.append(f"\n(b) after {n_warmup} warm-up rounds at depth <= {max_depth} from Pathfinder's draws, {n_trans} transitions with ε and the metric fixed (nuts_step, check_from = {CHECK_FROM})")
    for name, n_epochs, W, _T in SHAPES:
        model = make_model(pkg, n_epochs)
        pd = pkg.PriorDraws(model)
        try:
            dev = torch.device("cuda", model.ln_like.device_index)
            im = pd.sample(SEED, 0, 4096, theta=False, logprior_t=False)[1].var(dim=1).contiguous()
            lines.append(f"\n{name}: D = {model.D}, {W} chains")
            res = {}
            for metric in ("diag", "dense"):
                r = res[metric] = sample_after_warmup(pkg, pd, model, W, metric, im, max_depth, n_warmup, n_trans, dev)
                lines.append(f"  metric={metric:<5}: ε {r['eps']:.5f}; warm-up's last ten rounds mean depth {r['wu_depth']:.2f}, leaves {r['wu_leaves']:.1f}, divergences {r['wu_div']}")
                lines.append(f"                per transition: mean depth {r['depth']:.2f}, mean n_leapfrog {r['leaves']:.1f}, divergences {r['div']:.1f}, {r['ms']:.2f} ms; "
                             f"min ess_bulk {r['ess_min']:.1f} of {n_trans * W} draws = {r['ess_per_grad']:.3e} per gradient evaluation"
                             + (f"; largest |correlation| of the factor {r['corr']:.3f}" if r["corr"] is not None else ""))
            a, b = res["diag"], res["dense"]
            lines.append(f"  dense against diagonal: n_leapfrog x{b['leaves'] / a['leaves']:.3f}, transition time x{b['ms'] / a['ms']:.3f}, min ess_bulk per gradient x{b['ess_per_grad'] / a['ess_per_grad']:.3f}")
        finally:
            pd.close()
            model.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "dense_throughput.txt"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--max-depth", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--transitions", type=int, default=20)
    ap.add_argument("--part", choices=("a", "b"), default=None, help="one of the two parts instead of both")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dense_bench: no GPU: the figures of this file are measured, never estimated")
    pkg = load_package()
    lines = [f"tools/dense_bench.py on {torch.cuda.get_device_name(0)}: HIP events around the calls, median of {args.reps} after warm-up"]
    if args.part in (None, "a"):
        part_a(pkg, args.reps, lines)
    if args.part in (None, "b"):
        part_b(pkg, args.max_depth, args.warmup, args.transitions, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
