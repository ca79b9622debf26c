#!/usr/bin/env python
"""Cost of differential evolution on the device (include/octofitter_hip_draws.h: octo_draws_de_device; host/callers.py: global_search_device);
writes profiles/de_throughput.txt.

    python tools/de_bench.py [--out profiles/de_throughput.txt] [--reps 30] [--gens 16] [--blocks 3]

On the tight test model (tests/draws_device.py: tight_model, D = 14), at W = 1024 and 4096. From HIP events around one device call, median of
`reps` after warm-up, in `blocks` alternating blocks (generation, slice round, forward call; again) so that the spread between blocks of the
same thing is on the page beside the difference between things:
  a generation     one resumed octo_draws_de_device call of `gens` generations, divided by `gens`: one forward log-posterior call and one
                   k_de_round launch (the call's k_de_report launch is inside the quotient: 1/gens of it a generation);
  a slice round    the same for octo_draws_slice_device on the same W points, in the same process: the existing unit of the same shape;
  the forward call alone; what is left of a generation and of a slice round beside it is k_de_round's and k_slice_round's share with their launches.
Then the search itself: global_search_device at its defaults on that model, the best ℓπ against generations, and beside it the best that
optimize_starting_points_device reaches from the 64 best prior draws (its default call, which this library leaves bit for bit as it was).
The header records the hashes of the sources the figures belong to. No figure is a pass condition.
"""
import argparse
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests")); sys.path.insert(0, str(ROOT / "tools"))
import numpy as np      # noqa: E402
import torch            # noqa: E402
from __graft_entry__ import kernel_source_hash, load_package      # noqa: E402
from hmc_bench import event_times      # noqa: E402
from slice_bench import draws_source_hash      # noqa: E402

LONG_PASSES = 256      # the timed slice rounds run on a transition long enough that no chain finishes under the clock
SEED = 20261021


def bench(model, pd, W, reps, gens, blocks, lines):
    tt = pd.sample(SEED, 0, W, theta=False, logprior_t=False)[1]
    cloud = pd.sample(SEED, 0, 4096, theta=False, logprior_t=False)[1]
    lo, hi = torch.minimum(cloud.min(dim=1).values, tt.min(dim=1).values), torch.maximum(cloud.max(dim=1).values, tt.max(dim=1).values)
    pop = tt.clone()
    dargs = dict(lo=lo, hi=hi, radius=8, seed=SEED)
    dout = pd.de(pop, n_gen=0, **dargs)
    done = [0]

    def generation_call():
        pd.de(pop, n_gen=gens, gen0=done[0], resume=True, out=dout, **dargs)
        done[0] += gens

    chains = tt.clone()
    sargs = dict(w=10.0, p=3, n_passes=LONG_PASSES, seed=SEED, step=1)
    sout = pd.slice(chains, n_rounds=0, **sargs)
    lines.append(f"\nW = {W}: D = {model.D}, radius 8, bounds given")
    rows = []
    for b in range(blocks):
        t_de = event_times(generation_call, reps)
        t_sl = event_times(lambda: pd.slice(chains, n_rounds=gens, resume=True, out=sout, **sargs), reps)
        t_lp = event_times(lambda: model.logpost_device(tt, grad=False), reps)
        rows.append((t_de[0] / gens, t_sl[0] / gens, t_lp[0]))
        lines.append(f"  block {b}: a generation {t_de[0] / gens * 1e3:8.4f} ms (min {t_de[1] / gens * 1e3:.4f}, max {t_de[2] / gens * 1e3:.4f}) · a slice round "
                     f"{t_sl[0] / gens * 1e3:8.4f} ms (min {t_sl[1] / gens * 1e3:.4f}, max {t_sl[2] / gens * 1e3:.4f}) · the forward call {t_lp[0] * 1e3:8.4f} ms "
                     f"(min {t_lp[1] * 1e3:.4f}, max {t_lp[2] * 1e3:.4f})")
    r = np.array(rows)
    med, spread = np.median(r, axis=0), r.max(axis=0) - r.min(axis=0)
    lines.append(f"  medians of the blocks: generation {med[0] * 1e3:.4f} ms, slice round {med[1] * 1e3:.4f} ms, forward call {med[2] * 1e3:.4f} ms; spread between "
                 f"blocks {spread[0] * 1e3:.4f}, {spread[1] * 1e3:.4f}, {spread[2] * 1e3:.4f} ms")
    lines.append(f"  generation / slice round {med[0] / med[1]:.3f}; left for k_de_round and its launch {(med[0] - med[2]) * 1e3:.4f} ms, for k_slice_round "
                 f"{(med[1] - med[2]) * 1e3:.4f} ms — a difference below the spread is none")
    lines.append(f"  ({done[0]} generations made; {int(sout['n_active'].item())} of {W} slice chains still active; acceptances of the last generation {int(dout['n_improved'].item())})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "de_throughput.txt"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--gens", type=int, default=16)
    ap.add_argument("--blocks", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("de_bench: no GPU: the figures of this file are measured, never estimated")
    pkg = load_package()
    from draws_device import tight_model
    lines = [f"tools/de_bench.py on {torch.cuda.get_device_name(0)}: HIP events around one device call, median of {args.reps} after warm-up, {args.blocks} alternating blocks",
             f"sources: csrc/draws sha256 {draws_source_hash()}; kernel_source_hash() of the main library {kernel_source_hash()}"]
    model = tight_model(pkg)
    try:
        pd = pkg.PriorDraws(model)
        try:
            for W in (1024, 4096):
                bench(model, pd, W, args.reps, args.gens, args.blocks, lines)
        finally:
            pd.close()
        pkg.global_search_device(model, max_gen=25, seed=1)      # warm-up: allocations, the first launches
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = pkg.global_search_device(model, seed=1)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        lines.append(f"\nglobal_search_device at its defaults (n_pop 1024, N 500000, radius 8, segments of 25, patience 100, ftol 1e-3): {r['n_gen']} generations, {dt:.3f} s wall clock")
        lines.append("  best ℓπ against generations: " + ", ".join(f"{g}: {h:.4f}" for g, h in zip(r["generations"], r["history"])))
        t0 = time.perf_counter()
        o = pkg.optimize_starting_points_device(model, seed=1)
        torch.cuda.synchronize()
        lines.append(f"optimize_starting_points_device at its defaults (the 64 best of 500000 prior draws, L-BFGS): best start {np.max(o['start_logpost']):.4f}, best ℓπ reached "
                     f"{o['logpost'][o['best']]:.4f}, {time.perf_counter() - t0:.3f} s wall clock")
        i = pkg.initialize_device(model, seed=1)
        lines.append(f"initialize_device at its defaults (the search, then L-BFGS from its 64 best individuals): best ℓπ reached {i['logpost'][i['best']]:.4f}")
    finally:
        model.close()
    text = "\n".join(lines) + "\n"
    print(text)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
