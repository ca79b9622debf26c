#!/usr/bin/env python
"""Cost of the OFTI rejection sampler on the device (include/octofitter_hip_draws.h: octo_draws_ofti_rejection; host/callers.py:
octofit_ofti_device); writes profiles/ofti_draws_throughput.txt.

    python tools/ofti_draws_bench.py [--out profiles/ofti_draws_throughput.txt] [--reps 30] [--sizes 1000000 10000000 100000000]

On the two tables of tests/golden/ofti.json (8 rows; 37 rows with correlations) with the priors of tests/ofti_draws_cases.py (τ at t_ref = 50000).
  the whole call   octo_draws_ofti_rejection is a blocking host call on the handle's own stream, so it is timed by the host clock around it
                   (perf_counter; the call ends with a stream synchronisation), median of `reps` after two warm-up calls, at every size;
  the stages       one chunk of 2^18 draws each, HIP events around one device call on one stream, median of `reps` after warm-up: the prior draws
                   (k_draw, θ alone), k_oftis_nl, octo_ofti_eval_device with a NULL abfg as the driver calls it (k_ofti_main + k_ofti_finish), each the raw
                   call into buffers made once, and k_oftis_post on 2^18 parameter sets (in a run it sees the survivors only); the shares are of the sum of
                   the first three. k_oftis_ll and pass 2 cannot be called by themselves and are not among the stages: the sum is a lower bound of a chunk;
                   HIP events cannot bracket the whole call (it runs on the handle's stream and synchronises it), hence the host clock there;
  the NumPy route  beside it at the smallest size, once: the same draws brought to the host, OftiLinearSolver on them, NumPy's rejection step with
                   the same uniforms — what a caller had before this driver.
The header records the hashes of the sources the figures belong to. No figure is a pass condition; DESIGN.md §3b states what was expected.
"""
import argparse
import statistics
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

SEED = 20261021
CHUNK = 1 << 18
CAP = 1 << 20


def wall_times(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts), max(ts)


def bench_table(pkg, name, sizes, reps, lines):
    import hmc_reference as ref
    import ofti_draws_cases as oc
    from draws_device import mirror_priors
    tab = oc.table(name)
    n_rows = len(tab["epochs"])
    lines.append(f"\n{name}: {n_rows} rows")
    with pkg.PriorDraws(priors=mirror_priors(pkg, oc.PRIORS_TAU)) as pd:
        pd.ofti_set(*oc.columns(tab), tp_mode=1, t_ref=oc.T_REF)
        for N in sizes:
            last = {}
            med, lo, hi = wall_times(lambda: last.update(pd.ofti_rejection(SEED, N, cap=CAP)), reps)
            lines.append(f"  N = {N:>11,d}: {med * 1e3:9.3f} ms a call (min {lo * 1e3:.3f}, max {hi * 1e3:.3f}) · {N / med:.3e} draws/s · {N * n_rows / med:.3e} row evaluations/s · "
                         f"accepted {last['n_accepted']}, max ℓ {last['max_logml']:.4f}")
        # the stages on one chunk
        solver = pkg.OftiLinearSolver(*oc.columns(tab))
        # the raw calls as the driver makes them, into buffers made once: θ alone, nl, ℓ with a NULL abfg
        theta = torch.empty((5, CHUNK), dtype=torch.float64, device="cuda")
        nl = torch.empty((5, CHUNK), dtype=torch.float64, device="cuda")
        lm = torch.empty(CHUNK, dtype=torch.float64, device="cuda")
        index = np.arange(CHUNK, dtype=np.uint64)
        st = pd._stream(None, pd.device)

        def draw():
            pd._check(pd.lib.octo_draws_sample_device(pd._h, SEED, 0, CHUNK, CHUNK, theta.data_ptr(), None, None, st))

        def to_nl():
            pd._check(pd.lib.octo_draws_ofti_nl_device(pd._h, CHUNK, CHUNK, theta.data_ptr(), nl.data_ptr(), st))

        def score():
            solver._check(solver.lib.octo_ofti_eval_device(solver._ctx, solver._h, nl.data_ptr(), CHUNK, CHUNK, None, lm.data_ptr(), st), "octo_ofti_eval_device")

        draw(); to_nl()
        t_draw, t_nl, t_ev = event_times(draw, reps), event_times(to_nl, reps), event_times(score, reps)
        ix = torch.as_tensor(index.view(np.int64), device="cuda")
        out = torch.empty((16, CHUNK), dtype=torch.float64, device="cuda")
        t_post = event_times(lambda: pd._check(pd.lib.octo_draws_ofti_posterior_device(pd._h, SEED, CHUNK, CHUNK, ix.data_ptr(), nl.data_ptr(), out.data_ptr(), st)), reps)
        tot = t_draw[0] + t_nl[0] + t_ev[0]
        lines.append(f"  stages on one chunk of {CHUNK} draws (the raw calls into buffers made once; k_oftis_ll and pass 2 are reachable only inside the driver and are not among "
                     f"them): prior draws {t_draw[0] * 1e3:.4f} ms ({t_draw[0] / tot:.0%}) · k_oftis_nl {t_nl[0] * 1e3:.4f} ms ({t_nl[0] / tot:.0%}) · octo_ofti_eval_device, "
                     f"no means {t_ev[0] * 1e3:.4f} ms ({t_ev[0] / tot:.0%}) · sum {tot * 1e3:.4f} ms = {CHUNK / tot:.3e} draws/s if pass 1 were these alone")
        lines.append(f"  k_oftis_post on {CHUNK} parameter sets: {t_post[0] * 1e3:.4f} ms = {CHUNK * n_rows / t_post[0]:.3e} row evaluations/s (a run gives it the survivors only)")
        # the NumPy route at the smallest size
        N = sizes[0]
        t0 = time.perf_counter()
        th = pd.sample(SEED, 0, N, theta_t=False, logprior_t=False)[0]
        nl_h = pd.ofti_nl(th).cpu().numpy()
        res = solver(*nl_h)
        ll = res["log_marginal_likelihood"]
        ll = np.where(np.isfinite(ll), ll, -np.inf)
        u = ref.rejection_uniforms(SEED, np.arange(N, dtype=np.uint64))
        acc = (ll != -np.inf) & (u < np.exp(ll - ll.max()))
        dt = time.perf_counter() - t0
        lines.append(f"  the NumPy route at N = {N:,d} (draws to the host, OftiLinearSolver, NumPy rejection with the restated uniforms; means only, no Thiele-Innes draw, no "
                     f"elements): {dt * 1e3:.1f} ms, accepted {int(acc.sum())}")
        solver.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "ofti_draws_throughput.txt"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1_000_000, 10_000_000, 100_000_000])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ofti_draws_bench: no GPU: the figures of this file are measured, never estimated")
    pkg = load_package()
    lines = [f"tools/ofti_draws_bench.py on {torch.cuda.get_device_name(0)}: the whole call by the host clock, the stages by HIP events; medians of {args.reps} after warm-up",
             f"sources: csrc/draws sha256 {draws_source_hash()}; kernel_source_hash() of the main library {kernel_source_hash()}"]
    for name in ("ofti_example", "ofti_cor_37"):
        bench_table(pkg, name, args.sizes, args.reps, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
