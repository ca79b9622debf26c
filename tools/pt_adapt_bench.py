#!/usr/bin/env python
"""Cost of the parallel-tempering statistics on the device (include/octofitter_hip_draws.h: octo_draws_pt_stats_device,
octo_draws_pt_schedule_device) beside the calls of the scan they join; writes profiles/pt_adapt_throughput.txt.

    python tools/pt_adapt_bench.py [--out profiles/pt_adapt_throughput.txt] [--reps 30] [--leapfrog 4]
    python tools/pt_adapt_bench.py --scatter [--seeds 8]      # the sampler's own scatter of the log evidence, on the suites' test model

Two shapes of tools/hmc_bench.py's D = 11 model on the 1e4-row table: 8 β × 1 024 chains (config 5) and 32 β × 1 024 chains. Per shape, from
HIP events around the calls, median of `reps` after warm-up:
  pt_stats (2 launches), next to one TemperedSwap.swap_step, one hmc_step (+ the reset copy, as hmc_bench has it) and one forward
  log-posterior call over the same replicas;
  pt_schedule (one launch behind a copy of β to the host, which waits for the stream);
  the same statistics from torch calls: a gather of ℓ by slot, exp / clamp / sum for Σα, two logsumexp over the chains and two logaddexp into
  the running pair, and indexing for the restarts — on finite ℓ only: the exclusions of the device call would add masks and launches.
--scatter runs octofit_pigeons_device(explorer="hmc") at the GPU suite's shape (tests/pt_cases.py: DRIVER_*) for `seeds` seeds and reports
the mean and the deviation of the three log-evidence estimates against the independent value quoted there. No figure is a pass condition.
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

SHAPES = (("config 5: 8 β x 1 024 chains, 10 000 rows", 10_000, 8, 1024),
          ("32 β x 1 024 chains, 10 000 rows", 10_000, 32, 1024))


def bench_shape(pkg, name, n_epochs, T, Cn, L, reps, lines):
    model = make_model(pkg, n_epochs)
    pd = pkg.PriorDraws(model)
    try:
        dev = torch.device("cuda", model.ln_like.device_index)
        W = T * Cn
        start = pd.sample(20260929, 0, W, theta=False, logprior_t=False)[1]
        im = pd.sample(20260929, 0, 4096, theta=False, logprior_t=False)[1].var(dim=1).contiguous()
        swap = pkg.TemperedSwap(model.ln_like, T, Cn, device=dev, seed=1)
        beta_w = swap.beta.repeat_interleave(Cn)
        tt = start.clone()
        ll = pd.hmc_step(tt, beta=beta_w, eps=0.01, n_leapfrog=L, inv_mass=im, seed=1, step=0)[1]
        ll = torch.where(torch.isfinite(ll), ll, torch.full_like(ll, -1e4)).contiguous()      # finite ℓ: the torch formulation has no exclusions
        for step in range(20):                                                               # permutations that are no longer the identity
            swap.swap_step(ll, step)
        state = pd.pt_state(T, Cn)
        n = [20]
        chains = torch.arange(Cn, device=dev)
        acc_t, lse_t = torch.zeros((T - 1, 2), dtype=torch.float64, device=dev), torch.full((T - 1, 2), -float("inf"), dtype=torch.float64, device=dev)
        leg_t, rst_t = torch.zeros((Cn, T), dtype=torch.int32, device=dev), torch.zeros(Cn, dtype=torch.int32, device=dev)

        def stats():
            pd.pt_stats(ll, swap.slot2rep, swap.beta, state)

        def schedule():
            pd.pt_schedule(state, swap.beta, adapt=False, reset=False)

        def swap_step():
            swap.swap_step(ll, n[0])
            n[0] += 1

        def hmc():
            tt.copy_(start)
            pd.hmc_step(tt, beta=beta_w, eps=0.01, n_leapfrog=L, inv_mass=im, seed=1, step=n[0])

        def forward():
            model.logpost_device(start, grad=False)

        def stats_torch():
            s2r = swap.slot2rep.long()
            by_slot = ll.view(T, Cn).gather(0, s2r.t())
            li, lj = by_slot[:-1], by_slot[1:]
            db = (swap.beta[:-1] - swap.beta[1:])[:, None]
            acc_t[:, 0] += Cn
            acc_t[:, 1] += torch.exp(db * (lj - li)).clamp(max=1.0).sum(dim=1)
            lse_t[:, 0] = torch.logaddexp(lse_t[:, 0], torch.logsumexp(db * lj, dim=1))
            lse_t[:, 1] = torch.logaddexp(lse_t[:, 1], torch.logsumexp(-db * li, dim=1))
            leg_t[chains, s2r[:, T - 1]] = 1
            hot = s2r[:, 0]
            back = leg_t[chains, hot] == 1
            rst_t.add_(back.int())
            leg_t[chains, hot] = torch.where(back, torch.zeros_like(rst_t), leg_t[chains, hot])

        t_st, lo_st, hi_st = event_times(stats, reps)
        t_sw, lo_sw, hi_sw = event_times(swap_step, reps)
        t_h, lo_h, hi_h = event_times(hmc, reps)
        t_f, lo_f, hi_f = event_times(forward, reps)
        t_sc, lo_sc, hi_sc = event_times(schedule, reps)
        t_to, lo_to, hi_to = event_times(stats_torch, reps)
        lines.append(f"\n{name}: D = {model.D}, {T * Cn} replicas, {-(-Cn // 256)} chain blocks x {T - 1} pairs")
        lines.append(f"  pt_stats (k_ptadapt_partials + k_ptadapt_merge)               : {t_st * 1e3:9.4f} ms (min {lo_st * 1e3:.4f}, max {hi_st * 1e3:.4f})")
        lines.append(f"  one TemperedSwap.swap_step                                    : {t_sw * 1e3:9.4f} ms (min {lo_sw * 1e3:.4f}, max {hi_sw * 1e3:.4f})")
        lines.append(f"  one hmc_step, n_leapfrog = {L} (+ the reset copy)               : {t_h * 1e3:9.4f} ms (min {lo_h * 1e3:.4f}, max {hi_h * 1e3:.4f}); "
                     f"pt_stats adds {t_st / t_h:6.2%} of it to a scan")
        lines.append(f"  one forward log-posterior call                                : {t_f * 1e3:9.4f} ms (min {lo_f * 1e3:.4f}, max {hi_f * 1e3:.4f})")
        lines.append(f"  pt_schedule (β copied to the host and checked, one launch)    : {t_sc * 1e3:9.4f} ms (min {lo_sc * 1e3:.4f}, max {hi_sc * 1e3:.4f}), once a round")
        lines.append(f"  the same statistics from torch calls (finite ℓ only)          : {t_to * 1e3:9.4f} ms (min {lo_to * 1e3:.4f}, max {hi_to * 1e3:.4f}) = "
                     f"{t_to / t_st:.1f} x pt_stats")
    finally:
        pd.close()
        model.close()


def scatter(pkg, seeds, lines):
    import numpy as np
    import pt_cases as pc
    from draws_device import hmc_model
    model = hmc_model(pkg)
    try:
        rows, spreads, secs = [], [], []
        for seed in range(1, seeds + 1):
            t0 = time.perf_counter()
            out = pkg.octofit_pigeons_device(model, pc.DRIVER_T, pc.DRIVER_CN, pc.DRIVER_ROUNDS, explorer="hmc", seed=seed)
            secs.append(time.perf_counter() - t0)
            ev = out["log_evidence"]
            rows.append((ev["fwd"], ev["rev"], ev["mean"]))
            spreads.append((pc.spread(out["rejection_by_round"][0]), pc.spread(out["rejection_by_round"][-1]), out["barrier_by_round"][-1], out["restarts"]["total"]))
            lines.append(f"  seed {seed}: fwd {ev['fwd']:.4f}, rev {ev['rev']:.4f}, mean {ev['mean']:.4f}; Λ {spreads[-1][2]:.3f}; spread of r_t, round 1 "
                         f"{spreads[-1][0]:.3f}, last {spreads[-1][1]:.3f}; restarts {spreads[-1][3]}; {secs[-1]:.2f} s")
        a = np.array(rows)
        lines.append(f"octofit_pigeons_device(explorer=\"hmc\"), T = {pc.DRIVER_T}, Cn = {pc.DRIVER_CN}, n_rounds = {pc.DRIVER_ROUNDS} "
                     f"({2 ** (pc.DRIVER_ROUNDS + 1) - 2} scans), seeds 1 … {seeds}, against log Z = {pc.MODEL_LOGZ} ± {pc.MODEL_LOGZ_SE} (prior importance sampling):")
        for k, name in enumerate(("fwd", "rev", "mean")):
            lines.append(f"  {name:4s}: mean {a[:, k].mean():.4f} (error {a[:, k].mean() - pc.MODEL_LOGZ:+.4f}), sd {a[:, k].std(ddof=1):.4f}, "
                         f"rms error {np.sqrt(np.mean((a[:, k] - pc.MODEL_LOGZ) ** 2)):.4f}")
        lines.append(f"  a run takes {statistics.median(secs):.2f} s (median)")
    finally:
        model.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "pt_adapt_throughput.txt"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--leapfrog", type=int, default=4)
    ap.add_argument("--scatter", action="store_true")
    ap.add_argument("--seeds", type=int, default=8)
    ap.add_argument("--shape", type=int, default=None, help="one of the two shapes (0, 1) instead of both")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pt_adapt_bench: no GPU: the figures of this file are measured, never estimated")
    pkg = load_package()
    if args.scatter:
        lines = [f"tools/pt_adapt_bench.py --scatter on {torch.cuda.get_device_name(0)}"]
        scatter(pkg, args.seeds, lines)
        print("\n".join(lines))
        return
    lines = [f"tools/pt_adapt_bench.py on {torch.cuda.get_device_name(0)}: HIP events around the calls, median of {args.reps} after warm-up"]
    for name, n_epochs, T, Cn in (SHAPES if args.shape is None else SHAPES[args.shape:args.shape + 1]):
        bench_shape(pkg, name, n_epochs, T, Cn, args.leapfrog, args.reps, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
