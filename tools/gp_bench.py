#!/usr/bin/env python
"""Cost of the Gaussian-process RV term on the device (include/octofitter_hip_draws.h, "The nineteenth"; csrc/draws/octo_draws_gp.hip); writes
profiles/gp_throughput.txt.

    python tools/gp_bench.py --resources            # no GPU: registers and LDS of every k_gp_* instantiation -> profiles/gp_kernel_resources.txt
    python tools/gp_bench.py [--out profiles/gp_throughput.txt] [--reps 20]

  the evaluation   octo_draws_gp_eval_device on tables of n = 200, 1 000 and 5 000 rows (one RadialVelocityOrbit planet, K = 1), W = 64, 1 024 and 10 048
                   walkers, R = 2 slots (one SHO) and R = 8 (four COMPLEX), forward and forward + gradient: HIP events around one call on one stream,
                   median of `reps` after warm-up (a fifth of them at n = 5 000). Beside each shape the work array the call needs
                   (octo_draws_gp_work_doubles).
  the floor        the same table as a plain sampled absolute-RV table (per-walker offset and jitter) through the main library: what the Kepler part
                   alone costs.
  what it replaces the float64 NumPy recursion and reverse pass of tests/gp_reference.py on the host, once, at W = 64 (and n <= 1 000: it is O(n·R²·W)
                   interpreted row by row).
    python tools/gp_bench.py --dense --resources    # no GPU: the k_gpd_* kernels -> profiles/gp_dense_kernel_resources.txt
    timeout -k 10 300 python tools/gp_bench.py --dense --rows 50,192,193 && timeout -k 10 300 python tools/gp_bench.py --dense --rows 500 --append \
        && timeout -k 10 600 python tools/gp_bench.py --dense --rows 1000 --append

  --dense          the dense kernels (csrc/draws/octo_draws_gpd.hip) -> profiles/gp_dense_throughput.txt: one quasi-periodic term on n = 50 / LDS_ROWS / LDS_ROWS + 1 /
                   500 / 1 000 rows, W = 64 and 1 024, forward and forward + gradient; beside each the same rows under a celerite SHO on the device, and
                   numpy.linalg.cholesky on the [W, n, n] stack on the host (what a caller does today; skipped where the stack exceeds 2 GB). Each step is a
                   process of its own under its own time limit, chained with &&, as above.
The header records the hashes of the sources the figures belong to, and the kernels' registers and LDS as --resources wrote them. No figure is a pass
condition.
"""
import argparse
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests")); sys.path.insert(0, str(ROOT / "tools"))
import numpy as np      # noqa: E402

SEED = 20261021
ROWS = (200, 1000, 5000)
SIZES = (64, 1024, 10_048)
RESOURCES = ROOT / "profiles" / "gp_kernel_resources.txt"


def write_resources():
    import draws_build
    built = draws_build.kernels()
    lines = ["k_gp_* of liboctofitter_hip_draws.so as built for gfx950: VGPRs (AGPRs) · LDS bytes a block (k_gp_back: + its dynamic LDS, (15·R' + R'(R' + 1)/2)·512) · code bytes"]
    for family in sorted(k for k in built if k.startswith("k_gp_")):
        for r in built[family]:
            lines.append(f"  {r['name'].replace('void ', ''):40s} {r['vgpr_count']:4d} ({r['agpr_count']}) · {r['group_segment_fixed_size']:6d} · {r['code_bytes']:6d}"
                         f" · spills {r['vgpr_spill_count']} · scratch instructions {r['scratch_instructions']}")
    RESOURCES.write_text("\n".join(lines) + "\n")
    print(RESOURCES.read_text())


def bench(pkg, reps, lines):
    import torch
    import gp_cases as gc
    import gp_reference as gref
    from hmc_bench import event_times
    rng = np.random.default_rng(SEED)
    planets = [(gref.RADVEL, 1)]
    with pkg.PriorDraws(priors=[pkg.Uniform(0.0, 1.0)]) as pd:
        for n in ROWS:
            t = np.sort(rng.uniform(55000.0, 55000.0 + 2.0 * n, n))
            tab = gref.table(t, rng.normal(size=n) * 8.0, rng.uniform(0.5, 3.0, n), np.ones((1, n)))
            # the floor: the same rows as a sampled absolute-RV table of the main library
            planet = pkg.Planet(name="b", basis="RadialVelocityOrbit", observations=[])
            system = pkg.System(name="floor", companions=[planet], observations=[pkg.StarAbsoluteRVObs(dict(epoch=tab["t"], rv=tab["rv"], σ_rv=tab["sigma"]), name="rv")])
            fn = pkg.make_ln_like(system, dict(M=1.0, planets=dict(b=dict(a=1.0, e=0.1, ω=0.5, tp=55000.0, mass=1.0)), observations=dict(rv=dict(offset=0.0, jitter=1.0))))
            try:
                for terms, R in (([gref.SHO], 2), ([gref.COMPLEX] * 4, 8)):
                    pd.gp_set(planets, tab["t"], tab["rv"], tab["sigma"], tab["c"], terms)
                    lines.append(f"\nn = {n:,d} rows, R = {R} slots ({'one SHO' if R == 2 else 'four COMPLEX'}), 1 planet, K = 1")
                    for W in SIZES:
                        el = gc.draw_elements(rng, planets, W)
                        elems = torch.as_tensor(el, device=pd.device)
                        hy = gc.draw_hyper(rng, terms, W, "both")
                        hyper = torch.as_tensor(hy, device=pd.device)
                        beta_h, jit_h = rng.normal(size=(1, W)), rng.uniform(0.1, 2.0, W)
                        beta, jit = torch.as_tensor(beta_h, device=pd.device), torch.as_tensor(jit_h, device=pd.device)
                        nuis = torch.as_tensor(np.stack([beta_h[0], jit_h, np.zeros(W)]), device=pd.device)
                        k = max(reps // 5, 3) if n >= 5000 else reps
                        for grad in (False, True):
                            out = pd.gp_eval(elems, hyper, beta, jit, grad=grad)
                            med, lo, hi = event_times(lambda: pd.gp_eval(elems, hyper, beta, jit, grad=grad, out=out), k)
                            fo = fn.ln_like_device(elems, nuis, grad=grad)
                            fo = fo if grad else (fo, None, None)
                            fmed = event_times(lambda: fn.ln_like_device(elems, nuis, grad=grad, out=fo), k)[0]
                            work = pd.gp_work_doubles(W, grad=grad) * 8 / 2 ** 20
                            lines.append(f"  W = {W:>6,d} {'fwd+grad' if grad else 'fwd     '}: {med * 1e3:9.3f} ms (min {lo * 1e3:.3f}, max {hi * 1e3:.3f}) · "
                                         f"{med / n * 1e6:7.3f} µs a row · the plain RV table {fmed * 1e3:8.3f} ms · work array {work:9.1f} MiB")
                        if W == 64 and n <= 1000:
                            res = tab["rv"][:, None] - beta_h[0][None, :]
                            for grad in (False, True):
                                t0 = time.perf_counter()
                                gref.recursion(tab["t"], res, tab["sigma"], jit_h, terms, hy, grad=grad)
                                lines.append(f"  W = {W:>6,d} {'fwd+grad' if grad else 'fwd     '}: the NumPy recursion on the host, once: {(time.perf_counter() - t0) * 1e3:9.1f} ms")
            finally:
                fn.close()


DENSE_RESOURCES = ROOT / "profiles" / "gp_dense_kernel_resources.txt"
DENSE_OUT = ROOT / "profiles" / "gp_dense_throughput.txt"
DENSE_SIZES = (64, 1024)
HOST_STACK_LIMIT = 2e9      # bytes of the [W, n, n] stack beyond which the host's Cholesky is skipped


def write_dense_resources():
    import draws_build
    built = draws_build.kernels()
    lines = ["k_gpd_* of liboctofitter_hip_draws.so as built for gfx950: VGPRs (AGPRs) · static LDS bytes (the triangle and the vectors are dynamic: "
             "8·(n(n + 1)/2 + 4n + 128) with the triangle in LDS, 8·(4n + 128) with it in the work array) · code bytes",
             "OCTO_DRAWS_GP_DENSE_LDS_ROWS = 192: 155 392 bytes of the 163 840 a workgroup may hold"]
    for family in sorted(k for k in built if k.startswith("k_gpd_")):
        for r in built[family]:
            lines.append(f"  {r['name'].replace('void ', ''):40s} {r['vgpr_count']:4d} ({r['agpr_count']}) · {r['group_segment_fixed_size']:6d} · {r['code_bytes']:6d}"
                         f" · spills {r['vgpr_spill_count']} · scratch instructions {r['scratch_instructions']}")
    DENSE_RESOURCES.write_text("\n".join(lines) + "\n")
    print(DENSE_RESOURCES.read_text())


def dense_rows():
    import gpd_reference as dref
    return (50, dref.LDS_ROWS, dref.LDS_ROWS + 1, 500, 1000)


def bench_dense(pkg, rows, reps, lines):
    """one quasi-periodic term on n rows, W = 64 and 1 024, forward and forward + gradient; beside it the same rows under a celerite SHO on the device and
    numpy.linalg.cholesky on the [W, n, n] stack on the host (what a caller does today)"""
    import torch
    import gp_cases as gc
    import gp_reference as gref
    import gpd_cases as dc
    import gpd_reference as dref
    from hmc_bench import event_times
    rng = np.random.default_rng(SEED)
    planets = [(gref.RADVEL, 1)]
    with pkg.PriorDraws(priors=[pkg.Uniform(0.0, 1.0)]) as pd:
        for n in rows:
            t = np.sort(rng.uniform(55000.0, 55000.0 + 4.0 * n, n))
            tab = gref.table(t, rng.normal(size=n) * 8.0, rng.uniform(0.5, 3.0, n), np.ones((1, n)))
            lines.append(f"\nn = {n:,d} rows ({'triangle in LDS' if n <= dref.LDS_ROWS else 'triangle in the work array'}), one quasi-periodic term, 1 planet, K = 1")
            for W in DENSE_SIZES:
                k = reps if n <= dref.LDS_ROWS + 1 else (3 if n * W <= 100_000 else 2)      # the long tables take seconds a call: the first call below warms them
                warm = 5 if n <= dref.LDS_ROWS + 1 else (1 if n * W <= 100_000 else 0)
                elems = torch.as_tensor(gc.draw_elements(rng, planets, W), device=pd.device)
                hy = dc.draw_hyper(rng, [dref.QUASIPERIODIC], W)
                beta = torch.as_tensor(rng.normal(size=(1, W)), device=pd.device)
                jit_h = rng.uniform(0.1, 2.0, W)
                jit = torch.as_tensor(jit_h, device=pd.device)
                sho = torch.as_tensor(gc.draw_hyper(rng, [gref.SHO], W, "over"), device=pd.device)
                for grad in (False, True):
                    pd.gp_set(planets, tab["t"], tab["rv"], tab["sigma"], tab["c"], [dref.QUASIPERIODIC])
                    hyper = torch.as_tensor(hy, device=pd.device)
                    out = pd.gp_eval(elems, hyper, beta, jit, grad=grad)
                    med, lo, hi = event_times(lambda: pd.gp_eval(elems, hyper, beta, jit, grad=grad, out=out), k, warmup=warm)
                    work = pd.gp_work_doubles(W, grad=grad) * 8 / 2 ** 20
                    pd.gp_set(planets, tab["t"], tab["rv"], tab["sigma"], tab["c"], [gref.SHO])
                    out = pd.gp_eval(elems, sho, beta, jit, grad=grad)
                    cmed = event_times(lambda: pd.gp_eval(elems, sho, beta, jit, grad=grad, out=out), max(k, 5))[0]
                    lines.append(f"  W = {W:>6,d} {'fwd+grad' if grad else 'fwd     '}: {med * 1e3:10.3f} ms (min {lo * 1e3:.3f}, max {hi * 1e3:.3f}, of {k}) · "
                                 f"a celerite SHO on the same rows {cmed * 1e3:8.3f} ms · work array {work:9.1f} MiB")
                    print(lines[-1], flush=True)
                if 8.0 * W * n * n <= HOST_STACK_LIMIT:
                    tau = np.abs(tab["t"][:, None] - tab["t"][None, :])
                    t0 = time.perf_counter()
                    stack = np.stack([dref.kernel_np(dref.QUASIPERIODIC, hy[:, w], tau)[0] + np.diag(tab["sigma"] ** 2 + jit_h[w] ** 2) for w in range(W)])
                    t1 = time.perf_counter()
                    np.linalg.cholesky(stack)
                    lines.append(f"  W = {W:>6,d} the host: building the [W, n, n] stack {(t1 - t0) * 1e3:9.1f} ms, numpy.linalg.cholesky on it {(time.perf_counter() - t1) * 1e3:9.1f} ms")
                else:
                    lines.append(f"  W = {W:>6,d} the host: skipped, the [W, n, n] stack is {8.0 * W * n * n / 1e9:.1f} GB")
                print(lines[-1], flush=True)


def main_dense(args):
    import torch
    from __graft_entry__ import kernel_source_hash, load_package
    from slice_bench import draws_source_hash
    if not torch.cuda.is_available():
        raise SystemExit("gp_bench: no GPU: a timing is a run on the device")
    out = Path(args.out) if args.out else DENSE_OUT
    rows = [int(x) for x in args.rows.split(",")] if args.rows else list(dense_rows())
    lines = []
    if not args.append:
        lines = [f"Gaussian-process RV term under dense kernels on {torch.cuda.get_device_name(0)}: HIP events around one call, median of {args.reps} (fewer on the long tables)",
                 f"main library source hash {kernel_source_hash()[:16]} · draws library source hash {draws_source_hash()[:16]}"]
        if DENSE_RESOURCES.exists():
            lines += ["", DENSE_RESOURCES.read_text().rstrip()]
    bench_dense(load_package(), rows, args.reps, lines)
    out.parent.mkdir(parents=True, exist_ok=True)
    with open(out, "a" if args.append else "w") as f:
        f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--dense", action="store_true", help="the dense kernels (octo_draws_gpd.hip): profiles/gp_dense_throughput.txt, with --resources profiles/gp_dense_kernel_resources.txt")
    ap.add_argument("--rows", default=None, help="--dense: the table lengths of this step, comma-separated (default: 50, LDS_ROWS, LDS_ROWS + 1, 500, 1000)")
    ap.add_argument("--append", action="store_true", help="--dense: append to the output of an earlier step")
    args = ap.parse_args()
    if args.dense:
        return write_dense_resources() if args.resources else main_dense(args)
    args.out = args.out or str(ROOT / "profiles" / "gp_throughput.txt")
    if args.resources:
        return write_resources()
    import torch
    from __graft_entry__ import kernel_source_hash, load_package
    from slice_bench import draws_source_hash
    if not torch.cuda.is_available():
        raise SystemExit("gp_bench: no GPU: a timing is a run on the device")
    pkg = load_package()
    lines = [f"Gaussian-process RV term on {torch.cuda.get_device_name(0)}: HIP events around one call, median of {args.reps}",
             f"main library source hash {kernel_source_hash()[:16]} · draws library source hash {draws_source_hash()[:16]}"]
    if RESOURCES.exists():
        lines += ["", RESOURCES.read_text().rstrip()]
    bench(pkg, args.reps, lines)
    text = "\n".join(lines) + "\n"
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)
    print(text)


if __name__ == "__main__":
    main()
