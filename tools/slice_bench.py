#!/usr/bin/env python
"""Cost of the slice sampler on the device (include/octofitter_hip_draws.h: octo_draws_slice_device); writes profiles/slice_throughput.txt.

    python tools/slice_bench.py [--out profiles/slice_throughput.txt] [--reps 30] [--rounds 16]

The three shapes of tools/hmc_bench.py (the D = 11 model of bench.py's logpost workload). Per shape, from HIP events around one device call,
median of `reps` after warm-up:
  a round          one resumed octo_draws_slice_device call of `rounds` rounds on chains that are all still active, divided by `rounds`: one
                   forward octo_model_logpost_device call and one k_slice_round launch;
  the callback     one forward octo_model_logpost_device call alone on the same batch; the difference is what the sampler's launch adds;
  a transition     the rounds a chain takes at the defaults (w = 10, p = 3, n_passes = 3), mean and maximum over the chains, and the time of
                   one PriorDraws.slice_step (its 4-byte reads of the active count included);
  one hmc_step     octo_draws_hmc_step_device with tools/hmc_bench.py's settings (n_leapfrog = 4), for comparison.
The header records the hashes of the sources the figures belong to. No figure is a pass condition.
"""
import argparse
import hashlib
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests")); sys.path.insert(0, str(ROOT / "tools"))
import torch            # noqa: E402
from __graft_entry__ import CSRC, kernel_source_hash, load_package      # noqa: E402
from hmc_bench import SHAPES, event_times, make_model      # noqa: E402

W_DEFAULT, P_DEFAULT, PASSES_DEFAULT = 10.0, 3, 3
LONG_PASSES = 256      # the timed rounds run on a transition long enough that no chain finishes under the clock


def draws_source_hash():
    h = hashlib.sha256()
    for f in sorted((CSRC / "draws").glob("*.h")) + sorted((CSRC / "draws").glob("*.hip")):
        h.update(f.name.encode()); h.update(f.read_bytes())
    return h.hexdigest()


def bench_shape(pkg, name, n_epochs, W, n_temps, reps, rounds, lines):
    model = make_model(pkg, n_epochs)
    pd = pkg.PriorDraws(model)
    try:
        start = pd.sample(20260929, 0, W, theta=False, logprior_t=False)[1]
        im = pd.sample(20260929, 0, 4096, theta=False, logprior_t=False)[1].var(dim=1).contiguous()
        beta = (torch.linspace(1.0, 0.0, n_temps, dtype=torch.float64, device=start.device) ** 3).repeat_interleave(W // n_temps) if n_temps > 1 else None
        tt = start.clone()
        # a round: a long transition is opened once, the timed calls resume it
        args = dict(beta=beta, w=W_DEFAULT, p=P_DEFAULT, n_passes=LONG_PASSES, seed=1, step=0)
        out = pd.slice(tt, n_rounds=0, **args)
        t_rounds, lo, hi = event_times(lambda: pd.slice(tt, n_rounds=rounds, resume=True, out=out, **args), reps)
        still = int(out["n_active"].item())
        t_lp, lo_lp, hi_lp = event_times(lambda: model.logpost_device(start, grad=False), reps)
        # a transition at the defaults
        tt.copy_(start)
        r = pd.slice_step(tt, beta=beta, w=W_DEFAULT, p=P_DEFAULT, n_passes=PASSES_DEFAULT, seed=1, step=1)
        n_eval = r["n_eval"].double()
        counts = [float(r[k].double().mean()) for k in ("n_expand", "n_shrink", "n_stuck")]
        step = [2]

        def transition():
            tt.copy_(start)
            pd.slice_step(tt, beta=beta, w=W_DEFAULT, p=P_DEFAULT, n_passes=PASSES_DEFAULT, seed=1, step=step[0])
            step[0] += 1
        t_tr, lo_tr, hi_tr = event_times(transition, max(3, reps // 6), warmup=1)

        def hmc():
            tt.copy_(start)
            pd.hmc_step(tt, beta=beta, eps=0.01, n_leapfrog=4, inv_mass=im, seed=1, step=step[0])
            step[0] += 1
        t_hmc, lo_h, hi_h = event_times(hmc, reps)
        t_round = t_rounds / rounds
        lines.append(f"\n{name}: D = {model.D}")
        lines.append(f"  a round (one call of {rounds} rounds / {rounds}; {still} of {W} chains still active after the timing) : {t_round * 1e3:9.4f} ms (min {lo / rounds * 1e3:.4f}, max {hi / rounds * 1e3:.4f})")
        lines.append(f"  one forward octo_model_logpost_device                 : {t_lp * 1e3:9.4f} ms (min {lo_lp * 1e3:.4f}, max {hi_lp * 1e3:.4f})  = {n_epochs * W / t_lp:.3e} row evaluations/s")
        lines.append(f"  left for k_slice_round and its launch                 : {(t_round - t_lp) * 1e3:9.4f} ms = {(t_round - t_lp) / t_round:6.1%} of a round; {n_epochs * W / t_round:.3e} row evaluations/s inside a round")
        lines.append(f"  rounds of a transition at w = {W_DEFAULT:g}, p = {P_DEFAULT}, n_passes = {PASSES_DEFAULT} : mean {float(n_eval.mean()):.1f}, max {int(n_eval.max())} over the chains "
                     f"({float(n_eval.mean()) / (PASSES_DEFAULT * model.D):.2f} evaluations a coordinate update; doublings {counts[0]:.1f}, shrink proposals {counts[1]:.1f}, stuck updates {counts[2]:.3f} a chain)")
        lines.append(f"  one slice_step at those settings (+ the reset copy)   : {t_tr * 1e3:9.3f} ms (min {lo_tr * 1e3:.3f}, max {hi_tr * 1e3:.3f}) = {t_tr / float(n_eval.max()) * 1e3:.4f} ms a round of its longest chain")
        lines.append(f"  one octo_draws_hmc_step_device, n_leapfrog = 4 (+ the reset copy) : {t_hmc * 1e3:9.3f} ms (min {lo_h * 1e3:.3f}, max {hi_h * 1e3:.3f}) = {t_hmc / t_round:.1f} rounds of the slice sampler")
    finally:
        pd.close()
        model.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "slice_throughput.txt"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=16)
    ap.add_argument("--shape", type=int, default=None, help="one of the three shapes (0, 1, 2) instead of all")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("slice_bench: no GPU: the figures of this file are measured, never estimated")
    pkg = load_package()
    lines = [f"tools/slice_bench.py on {torch.cuda.get_device_name(0)}: HIP events around one device call, median of {args.reps} after warm-up",
             f"sources: csrc/draws sha256 {draws_source_hash()}; kernel_source_hash() of the main library {kernel_source_hash()}"]
    for name, n_epochs, W, n_temps in (SHAPES if args.shape is None else SHAPES[args.shape:args.shape + 1]):
        bench_shape(pkg, name, n_epochs, W, n_temps, args.reps, args.rounds, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
