#!/usr/bin/env python
"""Cost of the variational tempering leg's three calls on the device (include/octofitter_hip_draws.h: octo_draws_reference_fit_device,
octo_draws_reference_exchange_device, and the masked octo_draws_moments_device call that feeds the fit) beside the calls of the scan they
join; writes profiles/vref_throughput.txt.

    python tools/vref_bench.py [--out profiles/vref_throughput.txt] [--reps 30] [--leapfrog 4]
    python tools/vref_bench.py --scatter [--seeds 8]      # both legs' log evidence, barrier and restarts on the suites' test model

Two shapes of tools/hmc_bench.py's D = 11 model on the 1e4-row table: 8 β × 1 024 chains and 32 β × 1 024 chains in each of two legs. Per
shape, from HIP events around the calls, median of `reps` after warm-up: reference_fit (one wave), reference_exchange (lane = chain), the
masked moments call over one leg (group 0 at ladder slot 0, −1 elsewhere, accumulate), next to one hmc_step (+ the reset copy, as hmc_bench
has it) and one TemperedSwap.swap_step over the same replicas; and the share a scan of two legs gains: two moments calls and one exchange
over two hmc_steps and two swap_steps (the fit runs once a round).
--scatter runs octofit_pigeons_device(explorer="hmc", n_temps_variational=T) at the GPU suite's shape (tests/pt_cases.py: DRIVER_*,
tests/vref_cases.py: DRIVER_FIRST_TUNING_ROUND) for `seeds` seeds and reports both legs' estimates against the independent value quoted there.
No time is a pass condition.
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tools")); sys.path.insert(0, str(ROOT / "tests"))
import torch            # noqa: E402
from __graft_entry__ import load_package      # noqa: E402
from hmc_bench import event_times, make_model      # noqa: E402

SHAPES = (("8 β x 1 024 chains a leg, 10 000 rows", 10_000, 8, 1024),
          ("32 β x 1 024 chains a leg, 10 000 rows", 10_000, 32, 1024))


def bench_shape(pkg, name, n_epochs, T, Cn, L, reps, lines):
    model = make_model(pkg, n_epochs)
    pd = pkg.PriorDraws(model)
    try:
        dev = torch.device("cuda", model.ln_like.device_index)
        W = T * Cn
        start = pd.sample(20260929, 0, W, theta=False, logprior_t=False)[1]
        im = start[:, :4096].var(dim=1).contiguous()
        legs = []
        for k in range(2):
            swap = pkg.TemperedSwap(model.ln_like, T, Cn, device=dev, seed=1 + k)
            tt = pd.sample(20260929, k * W, W, theta=False, logprior_t=False)[1]
            lp, ll, _, _ = pd.hmc_step(tt, beta=swap.beta.repeat_interleave(Cn), eps=0.01, n_leapfrog=L, inv_mass=im, seed=1, step=0, chain0=k * W)
            ll = torch.where(torch.isfinite(ll), ll, torch.full_like(ll, -1e4)).contiguous()
            for step in range(20):                                                           # permutations that are no longer the identity
                swap.swap_step(ll, step)
            legs.append((swap, tt, lp, ll))
        (sa, ta, pa, la), (sb, tb, pb, lb) = legs
        mom = (torch.zeros(1, dtype=torch.float64, device=dev), torch.zeros((1, model.D), dtype=torch.float64, device=dev),
               torch.zeros((1, model.D), dtype=torch.float64, device=dev))
        group = torch.full((W,), -1, dtype=torch.int32, device=dev)
        group[sa.slot2rep[:, 0].long() * Cn + torch.arange(Cn, device=dev)] = 0
        pd.moments(ta, group=group, G=1, out=mom, accumulate=True)
        ref = pd.reference_table()
        bad = pd.reference_fit(ref, mom[0], mom[1][0], mom[2][0])
        assert int(bad.item()) == 0
        beta_w = sa.beta.repeat_interleave(Cn)
        n = [20]

        def fit():
            pd.reference_fit(ref, mom[0], mom[1][0], mom[2][0], bad=bad)

        def exchange():
            pd.reference_exchange(sa.slot2rep, ta, pa, la, None, sb.slot2rep, tb, pb, lb, ref)

        def moments():
            pd.moments(ta, group=group, G=1, out=mom, accumulate=True)

        def swap_step():
            sa.swap_step(la, n[0])
            n[0] += 1

        def hmc():
            ta.copy_(start)
            pd.hmc_step(ta, beta=beta_w, eps=0.01, n_leapfrog=L, inv_mass=im, seed=1, step=n[0])

        t_f, lo_f, hi_f = event_times(fit, reps)
        t_x, lo_x, hi_x = event_times(exchange, reps)
        t_m, lo_m, hi_m = event_times(moments, reps)
        t_sw, lo_sw, hi_sw = event_times(swap_step, reps)
        t_h, lo_h, hi_h = event_times(hmc, reps)
        added, scan = 2 * t_m + t_x, 2 * t_h + 2 * t_sw
        lines.append(f"\n{name}: D = {model.D}, 2 x {W} replicas")
        lines.append(f"  reference_fit (k_vref_table, one wave)                        : {t_f * 1e3:9.4f} ms (min {lo_f * 1e3:.4f}, max {hi_f * 1e3:.4f}), once a round")
        lines.append(f"  reference_exchange (k_vref_exchange, {-(-Cn // 256)} blocks)                : {t_x * 1e3:9.4f} ms (min {lo_x * 1e3:.4f}, max {hi_x * 1e3:.4f})")
        lines.append(f"  moments of one leg, masked to the target replicas, accumulate : {t_m * 1e3:9.4f} ms (min {lo_m * 1e3:.4f}, max {hi_m * 1e3:.4f})")
        lines.append(f"  one TemperedSwap.swap_step                                    : {t_sw * 1e3:9.4f} ms (min {lo_sw * 1e3:.4f}, max {hi_sw * 1e3:.4f})")
        lines.append(f"  one hmc_step of one leg, n_leapfrog = {L} (+ the reset copy)    : {t_h * 1e3:9.4f} ms (min {lo_h * 1e3:.4f}, max {hi_h * 1e3:.4f})")
        lines.append(f"  a scan of two legs gains 2 moments + 1 exchange = {added * 1e3:.4f} ms on 2 hmc_step + 2 swap_step = {scan * 1e3:.4f} ms: {added / scan:6.2%}")
    finally:
        pd.close()
        model.close()


def scatter(pkg, seeds, lines):
    import numpy as np
    import pt_cases as pc
    import vref_cases as vc
    from draws_device import hmc_model
    model = hmc_model(pkg)
    try:
        rows, secs = [], []
        for seed in range(1, seeds + 1):
            t0 = time.perf_counter()
            out = pkg.octofit_pigeons_device(model, pc.DRIVER_T, pc.DRIVER_CN, pc.DRIVER_ROUNDS, explorer="hmc", seed=seed, n_temps_variational=pc.DRIVER_T,
                                             first_tuning_round=vc.DRIVER_FIRST_TUNING_ROUND)
            secs.append(time.perf_counter() - t0)
            var = out["variational"]
            ev, ev_v = out["log_evidence"], var["log_evidence"]
            rows.append((ev["fwd"], ev["rev"], ev["mean"], ev_v["fwd"], ev_v["rev"], ev_v["mean"], out["barrier_by_round"][-1], var["barrier_by_round"][-1],
                         out["restarts"]["total"], var["restarts"]["total"]))
            lines.append(f"  seed {seed}: prior leg fwd {ev['fwd']:.4f}, rev {ev['rev']:.4f}, mean {ev['mean']:.4f}, Λ {rows[-1][6]:.3f}, restarts {rows[-1][8]}; variational leg "
                         f"fwd {ev_v['fwd']:.4f}, rev {ev_v['rev']:.4f}, mean {ev_v['mean']:.4f}, Λ {rows[-1][7]:.3f}, restarts {rows[-1][9]}; bad "
                         f"{int(var['bad_by_round'].sum())}; Λ_var by round {np.round(var['barrier_by_round'], 3).tolist()}; {secs[-1]:.2f} s")
        a = np.array(rows)
        lines.append(f"octofit_pigeons_device(explorer=\"hmc\", n_temps_variational={pc.DRIVER_T}, first_tuning_round={vc.DRIVER_FIRST_TUNING_ROUND}), T = {pc.DRIVER_T}, "
                     f"Cn = {pc.DRIVER_CN}, n_rounds = {pc.DRIVER_ROUNDS} ({2 ** (pc.DRIVER_ROUNDS + 1) - 2} scans), seeds 1 … {seeds}, against log Z = {pc.MODEL_LOGZ} ± "
                     f"{pc.MODEL_LOGZ_SE} (prior importance sampling):")
        for k, name in enumerate(("prior leg fwd", "prior leg rev", "prior leg mean", "variational leg fwd", "variational leg rev", "variational leg mean")):
            lines.append(f"  {name:20s}: mean {a[:, k].mean():.4f} (error {a[:, k].mean() - pc.MODEL_LOGZ:+.4f}), sd {a[:, k].std(ddof=1):.4f}, "
                         f"rms error {np.sqrt(np.mean((a[:, k] - pc.MODEL_LOGZ) ** 2)):.4f}")
        ratio = a[:, 7] / a[:, 6]
        lines.append(f"  Λ of the last round: prior leg {a[:, 6].mean():.3f} ({a[:, 6].min():.3f} … {a[:, 6].max():.3f}), variational leg {a[:, 7].mean():.3f} "
                     f"({a[:, 7].min():.3f} … {a[:, 7].max():.3f}); Λ_var/Λ_fixed worst {ratio.max():.3f}, best {ratio.min():.3f}; Λ_var < Λ_fixed at "
                     f"{int(np.sum(ratio < 1.0))} of {seeds} seeds")
        lines.append(f"  restarts: prior leg {a[:, 8].mean():.0f}, variational leg {a[:, 9].mean():.0f} (mean over the seeds)")
        lines.append(f"  a run takes {statistics.median(secs):.2f} s (median)")
    finally:
        model.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "vref_throughput.txt"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--leapfrog", type=int, default=4)
    ap.add_argument("--scatter", action="store_true")
    ap.add_argument("--seeds", type=int, default=8)
    ap.add_argument("--shape", type=int, default=None, help="one of the two shapes (0, 1) instead of both")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("vref_bench: no GPU: the figures of this file are measured, never estimated")
    pkg = load_package()
    if args.scatter:
        lines = [f"tools/vref_bench.py --scatter on {torch.cuda.get_device_name(0)}"]
        scatter(pkg, args.seeds, lines)
        text = "\n".join(lines) + "\n"
        print(text)
        if args.out != str(ROOT / "profiles" / "vref_throughput.txt"):
            Path(args.out).write_text(text)
        return
    lines = [f"tools/vref_bench.py on {torch.cuda.get_device_name(0)}: HIP events around the calls, median of {args.reps} after warm-up"]
    for name, n_epochs, T, Cn in (SHAPES if args.shape is None else SHAPES[args.shape:args.shape + 1]):
        bench_shape(pkg, name, n_epochs, T, Cn, args.leapfrog, args.reps, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
