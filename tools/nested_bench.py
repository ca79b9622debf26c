#!/usr/bin/env python
"""Cost of nested sampling on the device (include/octofitter_hip_draws.h: octo_draws_nested_cull_device, octo_draws_nested_move_device;
host/callers.py: octofit_nested_device); writes profiles/nested_throughput.txt.

    python tools/nested_bench.py [--out profiles/nested_throughput.txt] [--reps 30] [--rounds 16]

On the tight test model (tests/draws_device.py: tight_model, D = 14). From HIP events around one device call, median of `reps` after warm-up:
  a cull           one octo_draws_nested_cull_device call with replace = 1 at (K, B) = (1024, 256) and (4096, 1024), and the flush of 4096;
  a move round     one resumed octo_draws_nested_move_device call of `rounds` rounds on B = 256 and 1024 chains that are all still active,
                   divided by `rounds`: one forward log-posterior call and one k_nested_round launch;
  a slice round    the same for octo_draws_slice_device on the same batch (θ_t of the same B points), measured in the same run: what the move's
                   round is to be read against — the same forward call plus a kernel of the same kind; and the forward call alone;
  a whole run      octofit_nested_device at its defaults, wall clock, with what it reports.
The header records the hashes of the sources the figures belong to. No figure is a pass condition.
"""
import argparse
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests")); sys.path.insert(0, str(ROOT / "tools"))
import torch            # noqa: E402
from __graft_entry__ import kernel_source_hash, load_package      # noqa: E402
from hmc_bench import event_times      # noqa: E402
from slice_bench import draws_source_hash      # noqa: E402

LONG_PASSES = 256      # the timed rounds run on a transition long enough that no chain finishes under the clock
SEED = 20261020


def live_set(pd, model, K):
    u = pd.cube(SEED, 0, K)
    _, tt, lpt = pd.from_cube(u, theta=False)
    ll = model.logpost_device(tt, grad=False)[0] - lpt
    return u, torch.where(torch.isfinite(ll), ll, torch.full_like(ll, -float("inf"))).contiguous()


def bench(pkg, model, pd, K, B, reps, rounds, lines):
    u, ll = live_set(pd, model, K)
    state = pd.nested_state()
    t_cull, lo, hi = event_times(lambda: pd.nested_cull(u, ll, state, B, replace=True, seed=SEED, iter=0), reps)
    lines.append(f"\nK = {K} live points, B = {B}: D = {model.D}")
    lines.append(f"  a cull with replacement (sort, {B} records, {B}·D seed copies, widths) : {t_cull * 1e3:9.4f} ms (min {lo * 1e3:.4f}, max {hi * 1e3:.4f})")
    if K == 4096:
        t_fl, lo, hi = event_times(lambda: pd.nested_cull(u, ll, pd.nested_state(), K, replace=False), reps)
        lines.append(f"  the flush of all {K} (one lane walks {K} running sums)                 : {t_fl * 1e3:9.4f} ms (min {lo * 1e3:.4f}, max {hi * 1e3:.4f})")
    # a move round: a fresh live set, one cull, a long transition opened once; the timed calls resume it
    u, ll = live_set(pd, model, K)
    state = pd.nested_state()
    slot, width = pd.nested_cull(u, ll, state, B, replace=True, seed=SEED, iter=1)
    args = dict(w=width, max_steps=8, n_passes=LONG_PASSES, seed=SEED, iter=1)
    out = pd.nested_move(u, ll, state, slot, n_rounds=0, **args)
    t_rounds, lo, hi = event_times(lambda: pd.nested_move(u, ll, state, slot, n_rounds=rounds, resume=True, out=out, **args), reps)
    still = int(out["n_active"].item())
    t_move = t_rounds / rounds
    # the slice sampler's round on the same batch
    tt = pd.from_cube(u[:, slot.long()].contiguous(), theta=False, logprior_t=False)[1]
    sargs = dict(w=10.0, p=3, n_passes=LONG_PASSES, seed=SEED, step=1)
    sout = pd.slice(tt, n_rounds=0, **sargs)
    t_srounds, slo, shi = event_times(lambda: pd.slice(tt, n_rounds=rounds, resume=True, out=sout, **sargs), reps)
    s_still = int(sout["n_active"].item())
    t_slice = t_srounds / rounds
    t_lp, lo_lp, hi_lp = event_times(lambda: model.logpost_device(tt, grad=False), reps)
    lines.append(f"  a move round (one call of {rounds} rounds / {rounds}; {still} of {B} chains still active)  : {t_move * 1e3:9.4f} ms (min {lo / rounds * 1e3:.4f}, max {hi / rounds * 1e3:.4f})")
    lines.append(f"  a slice round on the same batch ({s_still} of {B} still active)               : {t_slice * 1e3:9.4f} ms (min {slo / rounds * 1e3:.4f}, max {shi / rounds * 1e3:.4f})")
    lines.append(f"  one forward log-posterior call on the batch                           : {t_lp * 1e3:9.4f} ms (min {lo_lp * 1e3:.4f}, max {hi_lp * 1e3:.4f})")
    lines.append(f"  move round / slice round                                              : {t_move / t_slice:9.3f}; left for k_nested_round and its launch {(t_move - t_lp) * 1e3:.4f} ms, "
                 f"for k_slice_round {(t_slice - t_lp) * 1e3:.4f} ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "nested_throughput.txt"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=16)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("nested_bench: no GPU: the figures of this file are measured, never estimated")
    pkg = load_package()
    from draws_device import tight_model
    lines = [f"tools/nested_bench.py on {torch.cuda.get_device_name(0)}: HIP events around one device call, median of {args.reps} after warm-up",
             f"sources: csrc/draws sha256 {draws_source_hash()}; kernel_source_hash() of the main library {kernel_source_hash()}"]
    model = tight_model(pkg)
    pd = pkg.PriorDraws(model)
    try:
        for K, B in ((1024, 256), (4096, 1024)):
            bench(pkg, model, pd, K, B, args.reps, args.rounds, lines)
    finally:
        pd.close()
    try:
        pkg.octofit_nested_device(model, seed=1, max_iter=3)      # warm-up: allocations, the first launches
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = pkg.octofit_nested_device(model, seed=1)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        lines.append(f"\na whole octofit_nested_device run at its defaults (n_live 1024, batch 256, n_passes 4, max_steps 8, dlogz 0.01): {dt:.3f} s wall clock")
        lines.append(f"  logZ {r['logz']:+.4f} ± {r['logz_err']:.4f}, information {r['information']:.3f} nats, {r['n_iter']} iterations, {r['n_evals']} likelihood evaluations "
                     f"({r['n_evals'] / dt:.3e} a second), {r['n_stuck']} stuck updates, ESS {r['ess']:.0f} of {r['loglike'].size} dead points")
    finally:
        model.close()
    text = "\n".join(lines) + "\n"
    print(text)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
