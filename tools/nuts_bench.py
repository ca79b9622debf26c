#!/usr/bin/env python
"""What the tree of the no-U-turn sampler costs per gradient, and how much of a lockstep transition's work is useful
(include/octofitter_hip_draws.h: octo_draws_nuts_device); writes profiles/nuts_throughput.txt.

    python tools/nuts_bench.py [--out profiles/nuts_throughput.txt] [--reps 30] [--max-depth 10] [--warmup 300] [--transitions 20]

The two shapes of tools/adapt_bench.py (the D = 11 model of tools/hmc_bench.py). Per shape, HIP events around the calls, median of `reps` after
warm-up:
  1. the cost of a round. Both samplers' rounds are one octo_model_logpost_device call and one kernel. A k_nuts_leaf round is the difference of
     two opening calls of 8 and 24 rounds over 16 (ε tiny: no chain turns, every chain builds in every round); a k_hmc_leap<STEP> round the
     difference of two steps of 9 and 25 leapfrogs over 16; the log-posterior call alone beside them. The difference of the two rounds is what
     the tree costs per gradient.
  2. lockstep utilisation. Chains at β = 1 from Pathfinder's draws, hmc_warmup(max_depth=…) for `warmup` rounds, then `transitions` transitions
     with ε and the metric fixed (nuts_step, check_from = 3): Σ n_leapfrog / (W · rounds made) of each, the rounds made being the first
     2^j − 1 >= the longest tree (j >= 3), with the mean and the longest tree, the mean depth and the divergences.
No figure is a pass condition.
"""
import argparse
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


def rounds_made(longest, max_depth):
    """the rounds nuts_step(check_from=3) makes when the longest tree has `longest` leaves"""
    j = min(CHECK_FROM, max_depth)
    while j < max_depth and (1 << j) - 1 < longest:
        j += 1
    return (1 << j) - 1


def bench_shape(pkg, name, n_epochs, W, reps, max_depth, n_warmup, n_trans, lines):
    model = make_model(pkg, n_epochs)
    pd = pkg.PriorDraws(model)
    try:
        dev = torch.device("cuda", model.ln_like.device_index)
        start = pd.sample(SEED, 0, W, theta=False, logprior_t=False)[1]
        im = pd.sample(SEED, 0, 4096, theta=False, logprior_t=False)[1].var(dim=1).contiguous()
        tt = start.clone()
        n = [0]

        def hmc(L):
            def run():
                tt.copy_(start)
                pd.hmc_step(tt, eps=1e-4, n_leapfrog=L, inv_mass=im, seed=1, step=n[0])
                n[0] += 1
            return run

        def nuts(rounds):
            def run():
                tt.copy_(start)
                pd.nuts(tt, eps=1e-4, inv_mass=im, max_depth=10, n_rounds=rounds, seed=1, step=n[0])
                n[0] += 1
            return run

        t_lp, lo_lp, hi_lp = event_times(lambda: model.logpost_device(start, grad=True), reps)
        t_h9, t_h25 = event_times(hmc(9), reps)[0], event_times(hmc(25), reps)[0]
        t_n8, t_n24 = event_times(nuts(8), reps)[0], event_times(nuts(24), reps)[0]
        r_hmc, r_nuts = (t_h25 - t_h9) / 16, (t_n24 - t_n8) / 16
        lines.append(f"\n{name}: D = {model.D}, {W} chains")
        lines.append(f"  one log-posterior call                                         : {t_lp * 1e3:9.3f} ms (min {lo_lp * 1e3:.3f}, max {hi_lp * 1e3:.3f})")
        lines.append(f"  one k_hmc_leap<STEP> round  (steps of 25 and 9 leapfrogs)/16   : {r_hmc * 1e3:9.3f} ms  ({t_h25 * 1e3:.3f} and {t_h9 * 1e3:.3f} ms)")
        lines.append(f"  one k_nuts_leaf round       (calls of 24 and 8 rounds)/16      : {r_nuts * 1e3:9.3f} ms  ({t_n24 * 1e3:.3f} and {t_n8 * 1e3:.3f} ms)")
        lines.append(f"  the tree per gradient: NUTS round − HMC round                  : {(r_nuts - r_hmc) * 1e3:9.3f} ms = {(r_nuts - r_hmc) / r_hmc:6.2%} of the HMC round")

        theta_t = torch.as_tensor(pkg.pathfinder_device(model, n_draws=W, seed=SEED)["theta_t"], dtype=torch.float64, device=dev).contiguous()
        wu = pkg.hmc_warmup(pd, theta_t, n_warmup, eps=0.05, inv_mass=im, seed=SEED, max_depth=max_depth)
        eps_w = wu["eps"].expand(W).contiguous()
        tree = wu["tree"].cpu().numpy()
        lines.append(f"  warm-up, {n_warmup} rounds at depth <= {max_depth}: ε {float(wu['eps'][0]):.5f}; last ten rounds mean depth {tree[-10:, 0].mean():.2f}, "
                     f"mean leaves {tree[-10:, 1].mean():.2f}, divergences {int(tree[-10:, 2].sum())}; acceptance statistic {float(wu['accept_stat'][-10:].mean()):.3f}")
        used, means, longest, depths, div = [], [], [], [], 0
        for k in range(n_trans):
            _lp, _ll, _la, _acc, depth, nleaf, dv = pd.nuts_step(theta_t, eps=eps_w, inv_mass=wu["inv_mass"], max_depth=max_depth, seed=SEED, step=n_warmup + k,
                                                                 check_from=CHECK_FROM)
            top = int(nleaf.max())
            used.append(float(nleaf.sum()) / (W * rounds_made(top, max_depth)))
            means.append(float(nleaf.double().mean())); longest.append(top); depths.append(float(depth.double().mean())); div += int(dv.sum())
        t_tr = event_times(lambda: pd.nuts_step(theta_t, eps=eps_w, inv_mass=wu["inv_mass"], max_depth=max_depth, seed=SEED, step=n_warmup + n_trans + n[0],
                                                check_from=CHECK_FROM), max(reps // 3, 3), warmup=1)
        lines.append(f"  {n_trans} transitions after it: lockstep utilisation Σ n_leapfrog / (W · rounds made) {sum(used) / len(used):.3f} (min {min(used):.3f}, max {max(used):.3f}); "
                     f"mean tree {sum(means) / len(means):.2f} leaves, mean depth {sum(depths) / len(depths):.2f}, longest tree {min(longest)} … {max(longest)}, divergences {div}")
        lines.append(f"  one transition (nuts_step, check_from = {CHECK_FROM})                      : {t_tr[0] * 1e3:9.3f} ms (min {t_tr[1] * 1e3:.3f}, max {t_tr[2] * 1e3:.3f})")
    finally:
        pd.close()
        model.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "nuts_throughput.txt"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--max-depth", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=300)
    ap.add_argument("--transitions", type=int, default=20)
    ap.add_argument("--shape", type=int, default=None, help="one of the two shapes (0, 1) instead of both")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("nuts_bench: no GPU: the figures of this file are measured, never estimated")
    pkg = load_package()
    lines = [f"tools/nuts_bench.py on {torch.cuda.get_device_name(0)}: HIP events around the calls, median of {args.reps} after warm-up"]
    for name, n_epochs, W, _T in (SHAPES if args.shape is None else SHAPES[args.shape:args.shape + 1]):
        bench_shape(pkg, name, n_epochs, W, args.reps, args.max_depth, args.warmup, args.transitions, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
