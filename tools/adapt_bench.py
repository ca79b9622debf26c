#!/usr/bin/env python
"""Cost of a warm-up round's statistics on the device (include/octofitter_hip_draws.h: octo_draws_hmc_adapt_device,
octo_draws_moments_device) beside the step they follow; writes profiles/adapt_throughput.txt.

    python tools/adapt_bench.py [--out profiles/adapt_throughput.txt] [--reps 30] [--leapfrog 4]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/adapt_bench.py --trace-only --shape 1      # the launches of a round, a run of its own

Two shapes of tools/hmc_bench.py (its D = 11 model): config 5's 8 β x 1 024 chains on the 1e4-row table, with one group per temperature, and
1 024 chains on a 50-row table, one group. Per shape, from HIP events around the calls, median of `reps` after warm-up:
  one hmc_step (+ the reset copy, as hmc_bench has it);
  one warm-up round = that step + adapt_step (dual averaging, ε of every chain written for the next step) + moments (accumulated);
  the same round with the ε update as octofit_pt_device(adapt="host") spells it in torch — index_add_ of the acceptance flags per
  temperature, the log ε rule, exp and a gather — in place of adapt_step;
  and the extras alone (adapt_step + moments; the torch update + moments), without the step in the bracket.
--trace-only runs the warmed-up device rounds alone, for a kernel trace whose statistics give the launches a round adds. No figure is a
pass condition.
"""
import argparse
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tools")); sys.path.insert(0, str(ROOT / "tests"))
import torch            # noqa: E402
from __graft_entry__ import load_package      # noqa: E402
from hmc_bench import event_times, make_model      # noqa: E402

SHAPES = (("config 5: 8 β x 1 024 chains, 10 000 rows", 10_000, 8 * 1024, 8),
          ("1 024 chains, 50 rows", 50, 1024, 1))


def bench_shape(pkg, name, n_epochs, W, T, L, reps, lines, trace_only):
    model = make_model(pkg, n_epochs)
    pd = pkg.PriorDraws(model)
    try:
        dev = torch.device("cuda", model.ln_like.device_index)
        start = pd.sample(20260929, 0, W, theta=False, logprior_t=False)[1]
        im = pd.sample(20260929, 0, 4096, theta=False, logprior_t=False)[1].var(dim=1).contiguous()
        Cn = W // T
        slot = torch.arange(T, device=dev).repeat_interleave(Cn)
        slot32 = slot.int() if T > 1 else None
        beta = (torch.linspace(1.0, 0.0, T, dtype=torch.float64, device=dev) ** 3)[slot] if T > 1 else None
        tt = start.clone()
        state = pd.adapt_init(T, 0.01)
        eps_w = torch.full((W,), 0.01, dtype=torch.float64, device=dev)
        mom = pd.moments(tt, slot32, T)
        log_eps = torch.full((T,), -4.6, dtype=torch.float64, device=dev)
        n = [0]
        last = {}

        def step():
            tt.copy_(start)      # every timed step starts from the same states, at the same ε (the adapted ε is written elsewhere)
            last["dH"], last["acc"] = pd.hmc_step(tt, beta=beta, eps=0.01, n_leapfrog=L, inv_mass=im, seed=1, step=n[0])[2:4]
            n[0] += 1

        def extras_device():
            pd.adapt_step(state, last["dH"], last["acc"], 1 + n[0] % 50, group=slot32, eps_w=eps_w)
            pd.moments(tt, slot32, T, out=mom, accumulate=True)

        def extras_torch():
            acc_t = torch.zeros(T, dtype=torch.float64, device=dev).index_add_(0, slot, last["acc"].double()) / Cn
            log_eps.add_((acc_t - 0.8) / (1 + n[0] % 50) ** 0.5)
            last["eps"] = torch.exp(log_eps)[slot]
            pd.moments(tt, slot32, T, out=mom, accumulate=True)

        def round_device():
            step(); extras_device()

        def round_torch():
            step(); extras_torch()

        if trace_only:
            for _ in range(5 + reps):
                round_device()
            torch.cuda.synchronize()
            print(f"adapt_bench --trace-only: {5 + reps} device rounds of {name}")
            return
        t_step, lo, hi = event_times(step, reps)
        t_dev, lo_d, hi_d = event_times(round_device, reps)
        t_tor, lo_t, hi_t = event_times(round_torch, reps)
        x_dev, lo_xd, hi_xd = event_times(extras_device, reps)
        x_tor, lo_xt, hi_xt = event_times(extras_torch, reps)
        lines.append(f"\n{name}: D = {model.D}, n_leapfrog = {L}, {T} group(s)")
        lines.append(f"  one hmc_step (+ the reset copy)                               : {t_step * 1e3:9.3f} ms (min {lo * 1e3:.3f}, max {hi * 1e3:.3f})")
        lines.append(f"  one warm-up round: step + adapt_step + moments                : {t_dev * 1e3:9.3f} ms (min {lo_d * 1e3:.3f}, max {hi_d * 1e3:.3f}); "
                     f"round − step {(t_dev - t_step) * 1e3:.3f} ms = {(t_dev - t_step) / t_step:6.2%} of the step")
        lines.append(f"  the same round, ε updated by the torch formulation            : {t_tor * 1e3:9.3f} ms (min {lo_t * 1e3:.3f}, max {hi_t * 1e3:.3f}); "
                     f"round − step {(t_tor - t_step) * 1e3:.3f} ms")
        lines.append(f"  the extras alone: adapt_step + moments (5 launches)           : {x_dev * 1e3:9.3f} ms (min {lo_xd * 1e3:.3f}, max {hi_xd * 1e3:.3f})")
        lines.append(f"  the extras alone: the torch ε update + moments                : {x_tor * 1e3:9.3f} ms (min {lo_xt * 1e3:.3f}, max {hi_xt * 1e3:.3f})")
    finally:
        pd.close()
        model.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "adapt_throughput.txt"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--leapfrog", type=int, default=4)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--shape", type=int, default=None, help="one of the two shapes (0, 1) instead of both")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("adapt_bench: no GPU: the figures of this file are measured, never estimated")
    pkg = load_package()
    lines = [f"tools/adapt_bench.py on {torch.cuda.get_device_name(0)}: HIP events around the calls, median of {args.reps} after warm-up"]
    for name, n_epochs, W, T in (SHAPES if args.shape is None else SHAPES[args.shape:args.shape + 1]):
        bench_shape(pkg, name, n_epochs, W, T, args.leapfrog, args.reps, lines, args.trace_only)
    if args.trace_only:
        return
    text = "\n".join(lines) + "\n"
    print(text)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
