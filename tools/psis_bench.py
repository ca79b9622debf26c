#!/usr/bin/env python
"""Throughput and accuracy of the PSIS-LOO library (include/octofitter_hip_psis.h) on the device; writes profiles/psis_throughput.txt.

    python tools/psis_bench.py [--out profiles/psis_throughput.txt] [--reps 30]

Two shapes, (R, S) = (1000, 10 000) — the pointwise library's user shape: one planet, 1 000 RA/Dec rows x 1e4 samples scattered about the truth as a posterior is, an
80 MB matrix — and (5000, 4096) — BASELINE config 4's tables at 4 096 samples, 164 MB. Per shape, in one run after warm-up: the k_psis time from HIP
events around one device call (median of `reps`) beside the time to read the matrix ONCE at the 6.29 TB/s copy rate (the floor it cannot
beat) and beside the pointwise matrix kernel that produced its input; the host-buffer octo_psis_loo call end to end; and loo() against the
route it replaces — pointwise_like_rows (the matrix over PCIe) plus psis_reference.psis_row per row on the host, timed on 64 rows and SCALED
to R. Then the observed error maxima of the cases of tests/test_psis.py and the size of the library. No figure is a pass condition.
"""
import argparse
import ctypes as C
import statistics
import sys
import time
import types
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import numpy as np      # noqa: E402
import torch            # noqa: E402
from __graft_entry__ import PSIS_LIB, load_package      # noqa: E402

COPY_RATE = 6.29e12      # bytes/s, float4 copy on this GPU (the microarchitecture notes' measured figure)


def event_times(fn, reps, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3)
    return statistics.median(ts), min(ts), max(ts)


def posterior_like(truths, W, seed, rel=0.002):
    """elems [9·P, W]: walkers scattered about the truth the data were drawn from, as a posterior is (prior draws leave fewer than five
    entries above the underflow cut-off in every row: no row would be fitted). Rows a, e, i, ω, Ω, tp, M, plx, mass per planet."""
    rng = np.random.default_rng(seed)
    cols = []
    for el, mass in truths:
        base = np.array([el["a"], el["e"], el["i"], el["w"], el["O"], el["tp"], el["M"], el["plx"], mass])
        scale = rel * np.array([el["a"], 1.0, 1.0, 1.0, 1.0, 1000.0, 0.0, el["plx"], mass])
        cols.append(base[:, None] + scale[:, None] * rng.standard_normal((9, W)))
    return np.concatenate(cols)


class TableModel:
    """What loo() / pointwise_like_rows() read of a LogDensityModel, over given tables: θ = the element rows, then the nuisance rows."""

    def __init__(self, tabs, planets, n_el, with_nuis):
        self.D = n_el + (3 * len(tabs) if with_nuis else 0)
        self.n_el, self.with_nuis = n_el, with_nuis
        self.ln_like = types.SimpleNamespace(obs_tables=tabs, planet_desc=planets, device_index=0,
                                             obs_entries=[(None, t["planet"], None, f"table{i}") for i, t in enumerate(tabs)])

    def kernel_inputs(self, θ):
        return np.ascontiguousarray(θ[:self.n_el]), (np.ascontiguousarray(θ[self.n_el:]) if self.with_nuis else None)


def bench_shape(pkg, name, tabs, planets, elems, nuis, reps, lines):
    import psis_reference as pr
    W = elems.shape[1]
    dev = torch.device("cuda", 0)
    pw, ps = pkg.Pointwise(tabs, planets), pkg.Psis()
    try:
        R = pw.n_rows
        d_el = torch.from_numpy(np.ascontiguousarray(elems)).to(dev)
        d_nu = None if nuis is None else torch.from_numpy(np.ascontiguousarray(nuis)).to(dev)
        d_ll = torch.empty((R, W), dtype=torch.float64, device=dev)
        d_out = torch.empty((pkg.psis.N_STATS, R), dtype=torch.float64, device=dev)
        d_lw = torch.empty((R, W), dtype=torch.float64, device=dev)
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        nu_ptr = None if d_nu is None else d_nu.data_ptr()
        lines.append(f"\n{name}: R = {R} rows, S = {W} samples: {R * W * 8 / 1e6:.1f} MB matrix, tail M(S) = {pr.tail_len(W)}")
        pmed, lo, hi = event_times(lambda: pw.lib.octo_pointwise_eval_device(pw._h, d_el.data_ptr(), W, W, nu_ptr, d_ll.data_ptr(), W, stream), reps)
        lines.append(f"  pointwise matrix kernel (produces the input)  : {pmed * 1e3:8.3f} ms (min {lo * 1e3:.3f}, max {hi * 1e3:.3f})")
        n_fin = int(torch.isfinite(d_ll).sum().item())
        med, lo, hi = event_times(lambda: ps.lib.octo_psis_loo_device(ps._h, d_ll.data_ptr(), W, R, W, d_out.data_ptr(), None, 0, stream), reps)
        floor = R * W * 8 / COPY_RATE
        lines.append(f"  k_psis, statistics only                       : {med * 1e3:8.3f} ms (min {lo * 1e3:.3f}, max {hi * 1e3:.3f})  = {med / floor:.1f}x the {floor * 1e3:.4f} ms "
                     f"that reading the matrix once at 6.29 TB/s takes, {med / pmed:.2f}x the pointwise matrix kernel's time  ({n_fin} of {R * W} entries finite)")
        wmed, lo, hi = event_times(lambda: ps.lib.octo_psis_loo_device(ps._h, d_ll.data_ptr(), W, R, W, d_out.data_ptr(), d_lw.data_ptr(), W, stream), reps)
        lines.append(f"  k_psis, with the log-weights stored           : {wmed * 1e3:8.3f} ms (min {lo * 1e3:.3f}, max {hi * 1e3:.3f})")
        k = d_out[2].cpu().numpy()
        fit = k[np.isfinite(k)]
        lines.append(f"    k̂ of this matrix: {fit.size} of {R} rows fitted" + (f", min {fit.min():.3f}, median {np.median(fit):.3f}, max {fit.max():.3f}; {int(np.sum(fit > 0.7))} rows above 0.7" if fit.size else ""))
        LL = d_ll.cpu().numpy()
        ts = []
        for _ in range(4):
            t0 = time.perf_counter(); ps.loo(LL); ts.append(time.perf_counter() - t0)
        lines.append(f"  host-buffer octo_psis_loo, copies included (wall): {min(ts[1:]) * 1e3:8.1f} ms = {R * W * 8 / min(ts[1:]) / 1e9:.2f} GB/s from the host")
    finally:
        ps.close(); pw.close()
    # loo() against the route it replaces, in the same run
    model = TableModel(tabs, planets, elems.shape[0], nuis is not None)
    θ = elems if nuis is None else np.vstack([elems, nuis])
    ts = []
    for _ in range(4):
        t0 = time.perf_counter(); pkg.loo(model, θ); ts.append(time.perf_counter() - t0)
    t_loo = min(ts[1:])
    ts = []
    for _ in range(3):
        t0 = time.perf_counter(); LLt, _ = pkg.pointwise_like_rows(model, θ); ts.append(time.perf_counter() - t0)
    t_rows = min(ts[1:])
    rows = np.ascontiguousarray(LLt.T[:64])
    t0 = time.perf_counter()
    for row in rows:
        pr.psis_row(row)
    per_row = (time.perf_counter() - t0) / len(rows)
    lines.append(f"  loo(model, θ), handles created and closed inside (wall): {t_loo * 1e3:8.1f} ms")
    lines.append(f"  the route it replaces: pointwise_like_rows {t_rows * 1e3:.1f} ms + psis_reference.psis_row (NumPy, one core) {per_row * 1e3:.3f} ms per row, timed on 64 rows; "
                 f"SCALED to R = {R}: {(t_rows + per_row * R) * 1e3:.1f} ms = {(t_rows + per_row * R) / t_loo:.1f}x loo()")


def accuracy(pkg, lines):
    import psis_reference as pr
    sys.path.insert(0, str(ROOT / "tests"))
    import test_psis as tp
    lines.append("\nobserved error maxima against the 40-digit reference (the cases of tests/test_psis.py; bars: elpd_loo, lppd, lw 1e-11 · max(1, |ref|); "
                 "k̂ and ess 100 x the float64 restatement's own largest gap):")
    rest = dict(pareto_k=0.0, ess=0.0, elpd_loo=0.0, lppd=0.0, lw=0.0)
    worst = dict(rest)
    ps = pkg.Psis()
    try:
        for name in pr.CASES:
            LL, ref = pr.case(name)
            g = pr.gaps(pr.psis_matrix(LL), ref)
            rest = {k: max(v, g[k]) for k, v in rest.items()}
            g = pr.gaps(tp.device_loo(pkg, ps, LL), ref)
            worst = {k: max(v, g[k]) for k, v in worst.items()}
        # the edge rows (psis_reference.EDGE_ROWS): every select route, tails up to 4096, tie blocks, sparse rows, offsets
        base = dict(pareto_k=100 * rest["pareto_k"], ess=100 * rest["ess"], elpd_loo=1e-11, lppd=1e-11, lw=1e-11)
        erest, eworst, per_row = dict.fromkeys(rest, 0.0), dict.fromkeys(rest, 0.0), []
        for name in pr.EDGE_ROWS:
            LL, ref, gather = pr.edge_case(name)
            row_bars, g = pr.edge_bars(name, base)
            erest = {k: max(v, g[k]) for k, v in erest.items()}
            d = pr.gaps(tp.device_loo(pkg, ps, LL), ref)
            eworst = {k: max(v, d[k]) for k, v in eworst.items()}
            if name in pr.ROUTE_ROWS:
                per_row.append(f"    {name:8s} gather at pass {gather}, tail {ref['tail_len'][0]:.0f}, k̂ {ref['pareto_k'][0]:.3f}: restatement k̂ {g['pareto_k']:.3e}, device k̂ {d['pareto_k']:.3e}; bars "
                               + ", ".join(f"{k} {v:.3e}" for k, v in row_bars.items()) + f"; one entry more or less in the tail moves k̂ by {pr.cut_sensitivity(name):.1e}")
    finally:
        ps.close()
    lines.append("  float64 restatement (NumPy): " + ", ".join(f"{k} {v:.3e}" for k, v in rest.items()))
    lines.append("  device                     : " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    lines.append(f"  bars of the device         : pareto_k {100 * rest['pareto_k']:.3e} (absolute), ess {100 * rest['ess']:.3e} (relative), elpd_loo, lppd, lw 1e-11")
    lines.append(f"the same over the {len(pr.EDGE_ROWS)} edge rows of tests/psis_reference.py (S up to {max(pr.edge_case(k)[0].shape[1] for k in pr.EDGE_ROWS)}; the hybrid reference above S = 120 001):")
    lines.append("  float64 restatement (NumPy): " + ", ".join(f"{k} {v:.3e}" for k, v in erest.items()))
    lines.append("  device                     : " + ", ".join(f"{k} {v:.3e}" for k, v in eworst.items()))
    lines.append("  bars: the ones above, except on the rows whose tail lies within 1e-2 … 1e-8 of the cut-off (max(the bar above, 100 x the restatement's gap on that row), k̂'s capped at 1e-5):")
    lines.extend(per_row)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "psis_throughput.txt"))
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("psis_bench: no GPU: the figures of this file are measured, never estimated")
    import synth
    pkg = load_package()
    capi = pkg.capi
    lines = [f"tools/psis_bench.py on {torch.cuda.get_device_name(0)}: kernel times from HIP events around one device call, median of {args.reps} after warm-up",
             f"liboctofitter_hip_psis.so: {PSIS_LIB.stat().st_size} bytes"]
    V = capi.ORBIT_VISUAL_KEP
    cfg = synth.config_astrom(n_epochs=1_000, n_walkers=10_000, cfg=3)
    t = cfg["table"]
    tabs = [dict(kind=capi.ASTROM_RADEC, planet=0, epoch=t["epoch"], y1=t["ra"], y2=t["dec"], s1=t["σ_ra"], s2=t["σ_dec"], cor=None, extra=None)]
    bench_shape(pkg, "user shape", tabs, [dict(orbit_kind=V, has_mass=0)], posterior_like([(synth.TRUTH, 0.0)], 10_000, seed=1), None, args.reps, lines)
    c4 = synth.config_two_planet()
    a, r = c4["astrom"], c4["rv"]
    tabs = [dict(kind=capi.ASTROM_RADEC, planet=1, epoch=a["epoch"], y1=a["ra"], y2=a["dec"], s1=a["σ_ra"], s2=a["σ_dec"], cor=None, extra=None),
            dict(kind=capi.RV_ABS, planet=-1, epoch=r["epoch"], y1=r["rv"], y2=None, s1=r["σ_rv"], s2=None, cor=None, extra=None)]
    inner, outer = dict(a=3.0, e=0.1, i=1.0, w=1.0, O=2.0, tp=50100.0, M=1.2, plx=50.0), dict(synth.TRUTH, a=15.0)      # synth.config_two_planet's truth
    rng = np.random.default_rng(2)
    nuis = np.zeros((6, 4096))
    nuis[0], nuis[1], nuis[2] = rng.uniform(0.0, 1.0, 4096), rng.normal(1.0, 1e-4, 4096), rng.normal(0.0, 1e-4, 4096)
    nuis[3], nuis[4] = rng.normal(12.0, 0.2, 4096), rng.uniform(0.1, 1.0, 4096)
    bench_shape(pkg, "config 4's tables", tabs, [dict(orbit_kind=V, has_mass=1), dict(orbit_kind=V, has_mass=1)],
                posterior_like([(inner, 5.0), (outer, 10.0)], 4096, seed=3), nuis, args.reps, lines)
    accuracy(pkg, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
