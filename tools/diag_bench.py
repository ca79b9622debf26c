#!/usr/bin/env python
"""Time and accuracy bars of the convergence diagnostics (include/octofitter_hip_draws.h: octo_draws_diagnose_device); writes profiles/diag_throughput.txt.

    python tools/diag_bench.py [--part timing|accuracy|all] [--out profiles/diag_throughput.txt] [--reps 20]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/diag_bench.py --calls-only 10      # a run of its own, then:
    python tools/diag_bench.py --trace-csv DIR/…_kernel_stats.csv                               # its k_diag_ rows become the third section

Three sections; a run that makes one keeps the others as the file holds them.

timing (needs the GPU): PriorDraws.diagnose on AR(1) draws at n = 1000 and n = 200, K = 11, W = 1024, by HIP events around the device calls, median of
`reps` after warm-up. One C call launches every kernel family, so the families are timed in the groups the ABI can launch by itself, and by
differences: ranks(fold=False) is k_diag_keys + one sort (k_diag_sort_local, k_diag_sort_global) + k_diag_quant + k_diag_rank; ranks(fold=True)
adds the second k_diag_keys and sort; diagnose adds one more k_diag_rank and k_diag_moments, k_diag_acov, k_diag_finish. Beside them the same
statistics made of torch calls on the same device (torch.sort, torch.searchsorted, torch.special.ndtri, torch.fft for the autocovariances of all
lags, Geyer's rule in its vectorised form: pair sums, the first non-positive pair, a running minimum) — the route a user has without the library.
No ratio is promised: the file records what was found.

kernel trace: HIP events bracket a call, not a kernel inside it, so the time of each k_diag_ family comes from a kernel trace of --calls-only (n = 1000,
K = 11, W = 1024; nothing but `calls` diagnoses after two warm-up calls), condensed by --trace-csv: calls, mean and total per family.

accuracy (CPU only): for every case of tests/diag_cases.py the largest gap, relative to max(1, |value|), between the float64 restatement
(tests/diag_reference.py) and the same restatement in np.longdouble with normal scores from mpmath, per statistic; and every case's decision
margins. The `gap <statistic> <value>` lines are what tests/diag_cases.py's LONG_DOUBLE_GAP repeats and the bars of tests/test_diag.py are written
from: max(1e-11, 100 × gap).
"""
import argparse
import re
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import numpy as np      # noqa: E402

MARKS = {"timing": "== timing", "trace": "== kernel trace", "accuracy": "== accuracy"}


def event_times(torch, fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts), max(ts)


def torch_diagnose(torch, x):
    """rhat, ess_bulk, ess_tail, rhat_basic, ess_basic, q05, q50, q95 [K] of x [n, K, W] from torch calls: the split and the statistics of the header,
    sums in torch's own order, autocovariances by FFT, Geyer's rule vectorised."""
    n, K, W = x.shape
    N = n // 2
    v = torch.cat([x[:N], x[n - N:]], dim=2).permute(1, 2, 0).contiguous()      # [K, M, N]
    M, S = 2 * W, 2 * W * N
    flat = v.reshape(K, S)
    s = torch.sort(flat, dim=1).values
    q = torch.quantile(flat, torch.tensor([0.05, 0.5, 0.95], dtype=torch.float64, device=x.device), dim=1)      # type 7 is torch's default

    def scores(a, srt):
        lo, hi = torch.searchsorted(srt, a, right=False), torch.searchsorted(srt, a, right=True)
        r = lo + (hi - lo + 1) / 2.0
        return torch.special.ndtri((r - 0.375) / (S + 0.25)).reshape(K, M, N)

    z = scores(flat, s)
    y = (flat - q[1][:, None]).abs()
    zf = scores(y, torch.sort(y, dim=1).values)

    def lag0(a):
        mu = a.mean(dim=2)
        var = a.var(dim=2, unbiased=True)
        wbar = var.mean(dim=1)
        return mu, wbar, wbar * (N - 1) / N + mu.var(dim=1, unbiased=True)

    def rhat(a):
        _, wbar, vp = lag0(a)
        return torch.sqrt(vp / wbar)

    def ess(a):
        mu, wbar, vp = lag0(a)
        c = a - mu[:, :, None]
        f = torch.fft.rfft(c, n=2 * N, dim=2)
        acov = torch.fft.irfft(f * f.conj(), n=2 * N, dim=2)[:, :, :N] / N
        rho = 1.0 - (wbar[:, None] - acov.mean(dim=1)) / vp[:, None]      # [K, N]
        rho[:, 0] = 1.0
        pairs = rho[:, :N - N % 2].reshape(K, -1, 2).sum(dim=2)
        alive = torch.cumprod((pairs > 0).to(torch.float64), dim=1)
        mono = torch.cummin(pairs, dim=1).values * alive
        tau = torch.clamp(-1.0 + 2.0 * mono.sum(dim=1), min=1.0 / np.log10(S))
        return S / tau

    i05, i95 = ((v <= q[j][:, None, None]).to(torch.float64) for j in (0, 2))
    return torch.stack([torch.maximum(rhat(z), rhat(zf)), ess(z), torch.minimum(ess(i05), ess(i95)), rhat(v), ess(v), q[0], q[1], q[2]])


def timing(reps):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("diag_bench: no GPU: the times of this file are measured, never estimated")
    from __graft_entry__ import load_package
    import diag_cases as cases
    pkg = load_package()
    from octofitter_jl_amd.host import draws
    lines = [f"tools/diag_bench.py on {torch.cuda.get_device_name(0)}: HIP events around the device calls, median of {reps} after warm-up, milliseconds (min … max)"]
    K, W = 11, 1024
    with draws.PriorDraws(priors=[pkg.Uniform(0.0, 1.0)]) as pd:
        for n in (1000, 200):
            x = torch.as_tensor(cases.ar1(np.random.default_rng(n), n, K, W, np.linspace(0.0, 0.9, K)), device="cuda")
            N, S = n // 2, n // 2 * 2 * W
            words = pd.lib.octo_draws_diagnose_work_doubles(n, W, K)
            lines.append(f"\nn = {n}, K = {K}, W = {W}: N = {N} draws of M = {2 * W} split chains, S = {S} used draws a row; work array {words * 8 / 1e6:.1f} MB")
            t_rank = event_times(torch, lambda: pd.ranks(x), reps)
            t_fold = event_times(torch, lambda: pd.ranks(x, fold=True), reps)
            t_all = event_times(torch, lambda: pd.diagnose(x), reps)
            t_torch = event_times(torch, lambda: torch_diagnose(torch, x), max(3, reps // 4), warmup=2)
            fmt = lambda t: f"{t[0]:9.3f} ({t[1]:.3f} … {t[2]:.3f})"      # noqa: E731
            lines.append(f"  ranks(fold=False): k_diag_keys, one sort, k_diag_quant, k_diag_rank (two output fills included) : {fmt(t_rank)}")
            lines.append(f"  ranks(fold=True): the same and the second k_diag_keys and sort                                  : {fmt(t_fold)}")
            lines.append(f"    by difference, one k_diag_keys + bitonic sort of K rows of P keys                            : {t_fold[0] - t_rank[0]:9.3f}")
            lines.append(f"  diagnose: everything                                                                           : {fmt(t_all)}")
            lines.append(f"    by difference, one more k_diag_rank + k_diag_moments + k_diag_acov + k_diag_finish            : {t_all[0] - t_fold[0]:9.3f}")
            lines.append(f"  the same statistics from torch calls (sort, searchsorted, ndtri, fft, cummin)                   : {fmt(t_torch)}")
            lines.append(f"    diagnose / torch = {t_all[0] / t_torch[0]:.2f}")
            got = torch.stack([pd.diagnose(x)[k] for k in draws.DIAG_NAMES]).cpu().numpy()
            alt = torch_diagnose(torch, x).cpu().numpy()
            gap = np.abs(got - alt) / np.maximum(1.0, np.abs(alt))
            lines.append("    largest relative difference of the two per statistic (another summation order, Geyer's rule vectorised): " +
                         ", ".join(f"{name} {gap[j].max():.1e}" for j, name in enumerate(draws.DIAG_NAMES)))
            lines.append("    ess_bulk of the rows (φ = 0 … 0.9): " + " ".join(f"{v:.0f}" for v in got[1]))
    return lines


def calls_only(calls):
    import torch
    from __graft_entry__ import load_package
    import diag_cases as cases
    pkg = load_package()
    from octofitter_jl_amd.host import draws
    n, K, W = 1000, 11, 1024
    x = torch.as_tensor(cases.ar1(np.random.default_rng(n), n, K, W, np.linspace(0.0, 0.9, K)), device="cuda")
    with draws.PriorDraws(priors=[pkg.Uniform(0.0, 1.0)]) as pd:
        for _ in range(calls + 2):
            pd.diagnose(x)
        torch.cuda.synchronize()


def trace_section(path):
    import csv
    rows = {}
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            hit = re.search(r"\bk_diag_\w+", r["Name"])
            if hit:
                name = hit.group(0)
                c, tot = rows.get(name, (0, 0.0))
                rows[name] = (c + int(r["Calls"]), tot + float(r["TotalDurationNs"]))
    total = sum(t for _, t in rows.values())
    lines = ["kernel trace of tools/diag_bench.py --calls-only (n = 1000, K = 11, W = 1024; warm-up calls included): launches, mean per launch, share of the k_diag_ time"]
    for name, (c, tot) in sorted(rows.items(), key=lambda kv: -kv[1][1]):
        lines.append(f"  {name:20s} {c:6d} launches  {tot / c / 1e3:10.2f} µs each  {100 * tot / total:5.1f} %")
    return lines


def accuracy():
    import diag_cases as cases
    lines = ["float64 restatement (tests/diag_reference.py) against the same in np.longdouble (normal scores from mpmath, 80 bits), the cases of tests/diag_cases.py;",
             "gaps relative to max(1, |value|); margins: the smallest |even + odd| of a Geyer test, the smallest gap of a monotone comparison"]
    worst = {s: 0.0 for s in cases.STATISTICS}
    for name in cases.CASES:
        g, m = cases.gaps(name), cases.reference(name)["margins"]
        worst = {s: max(worst[s], g[s]) for s in worst}
        lines.append(f"  {name:14s} (n, W, K) = {cases.CASES[name][2]}: " + ", ".join(f"{s} {g[s]:.3e}" for s in cases.STATISTICS) +
                     f"; margins {m.geyer:.3e}, {m.monotone:.3e}")
    lines.append("the largest gap of each statistic, and the bar max(1e-11, 100 × gap) of tests/test_diag.py:")
    for s in cases.STATISTICS:
        lines.append(f"gap {s} {worst[s]!r}   bar {max(1e-11, 100 * worst[s]):.3e}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("timing", "accuracy", "all"), default="all")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "diag_throughput.txt"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--calls-only", type=int, default=0, help="make this many diagnose calls at n = 1000 and write nothing: the workload of a kernel trace")
    ap.add_argument("--trace-csv", default=None, help="the kernel statistics of such a trace: its k_diag_ rows become the kernel trace section")
    args = ap.parse_args()
    if args.calls_only:
        return calls_only(args.calls_only)
    out = Path(args.out)
    sections = {k: [] for k in MARKS}
    if out.exists():
        cur = None
        for line in out.read_text().splitlines():
            hit = [k for k, m in MARKS.items() if line.startswith(m)]
            if hit:
                cur = hit[0]
            elif cur:
                sections[cur].append(line)
    if args.trace_csv:
        sections["trace"] = trace_section(args.trace_csv)
    else:
        if args.part in ("timing", "all"):
            sections["timing"] = timing(args.reps)
        if args.part in ("accuracy", "all"):
            sections["accuracy"] = accuracy()
    text = "".join(f"{MARKS[k]} ==\n" + "\n".join(sections[k]).strip("\n") + "\n\n" for k in MARKS if sections[k])
    print(text)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(text)


if __name__ == "__main__":
    main()
