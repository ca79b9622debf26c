#!/usr/bin/env python
"""Throughput and accuracy of the pointwise log-likelihood library (include/octofitter_hip_pointwise.h) on the device; writes
profiles/pointwise_throughput.txt.

    python tools/pointwise_bench.py [--out profiles/pointwise_throughput.txt] [--reps 30]

Two shapes: the one a user would run — one planet, 1 000 RA/Dec rows x 1e4 walkers, an 80 MB matrix — and BASELINE config 4's tables (two
planets, 2 500 RA/Dec rows on the outer + 2 500 absolute RV rows, nuisances) at 4 096 walkers. Per shape, in one run after warm-up: the matrix
and the summary kernel times from HIP events around one device call (median of `reps`); the matrix kernel's values per second beside its two
candidate bounds — 8 bytes stored per value against the 6.29 TB/s copy rate, and k_main's forward cold row loop (OCTO_OPT_WARM_START = 0) on the
same tables; the host-buffer calls end to end; and the only route to the same matrix without this library — R one-row datasets through
octo_eval, timed on 32 rows and SCALED to R. Then the observed error maxima of the cases of tests/test_pointwise.py and the size of the
library. No figure is a pass condition.
"""
import argparse
import ctypes as C
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import numpy as np      # noqa: E402
import torch            # noqa: E402
from __graft_entry__ import POINTWISE_LIB, load_package      # noqa: E402

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


def k_main_cold(pkg, tabs, planets, d_el, d_nu, W, reps):
    """Median time of the dominant (row-loop) kernel of a forward-only octo_eval_device with the cold row loop, from the library's own event timer."""
    import gpu_binding
    capi = pkg.capi
    g = gpu_binding.GpuPath(tabs, planets, small_batch=0, options={capi.OPT_WARM_START: 0})
    try:
        d_ll = torch.empty(W, dtype=torch.float64, device=d_el.device)
        stream = C.c_void_p(torch.cuda.current_stream(d_el.device).cuda_stream)

        def call():
            g._chk(g.lib.octo_eval_device(g.ctx, g.ds, d_el.data_ptr(), None if d_nu is None else d_nu.data_ptr(), W, W, d_ll.data_ptr(), None, None, stream))
        for _ in range(5):
            call()
        torch.cuda.synchronize()
        g._chk(g.lib.octo_timing_enable(g.ctx, 1))
        for _ in range(reps):
            call()
        torch.cuda.synchronize()
        med, lo, hi, n = C.c_double(), C.c_double(), C.c_double(), C.c_int64()
        g._chk(g.lib.octo_timing_stats(g.ctx, C.byref(med), C.byref(lo), C.byref(hi), C.byref(n)))
        g._chk(g.lib.octo_timing_enable(g.ctx, 0))
        return med.value * 1e-3
    finally:
        g.close()


def one_row_route(pkg, tabs, planets, elems, nuis, n_rows=32):
    """Seconds per row of the route through the main ABI alone: a one-row dataset per datum and one octo_eval each (host buffers), on the first
    n_rows rows of the first table."""
    import gpu_binding
    import pointwise_reference as tp
    nu = None if nuis is None else np.ascontiguousarray(nuis[0:3])
    g0 = gpu_binding.GpuPath([tp.one_row(tabs[0], 0)], planets)      # context creation and the first launch are not the route's cost
    g0.eval(elems, nu, grad=False); g0.close()
    t0 = time.perf_counter()
    for j in range(n_rows):
        with gpu_binding.GpuPath([tp.one_row(tabs[0], j)], planets) as g:
            g.eval(elems, nu, grad=False)
    return (time.perf_counter() - t0) / n_rows


def bench_shape(pkg, name, tabs, planets, elems, nuis, reps, lines):
    W = elems.shape[1]
    pw = pkg.Pointwise(tabs, planets)
    dev = torch.device("cuda", 0)
    d_el = torch.from_numpy(np.ascontiguousarray(elems)).to(dev)
    d_nu = None if nuis is None else torch.from_numpy(np.ascontiguousarray(nuis)).to(dev)
    R = pw.n_rows
    d_out = torch.empty((R, W), dtype=torch.float64, device=dev)
    d_sum = torch.empty((7, R), dtype=torch.float64, device=dev)
    lib, h = pw.lib, pw._h
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    nu_ptr = None if d_nu is None else d_nu.data_ptr()
    # Kepler solves per value: the planets a table's rows read (its own and every planet with a mass)
    solves = sum(len(t["epoch"]) * sum(1 for p, pl in enumerate(planets) if pl["has_mass"] or p == t["planet"]) for t in tabs) * W
    lines.append(f"\n{name}: {len(planets)} planet(s), R = {R} rows, W = {W}: {R * W:.3e} values, {R * W * 8 / 1e6:.1f} MB matrix, {solves:.3e} solves")
    try:
        med, lo, hi = event_times(lambda: lib.octo_pointwise_eval_device(h, d_el.data_ptr(), W, W, nu_ptr, d_out.data_ptr(), W, stream), reps)
        vps = R * W / med
        lines.append(f"  matrix kernel                         : {med * 1e3:8.3f} ms (min {lo * 1e3:.3f}, max {hi * 1e3:.3f})  {vps:.3e} values/s, {solves / med:.3e} solves/s")
        lines.append(f"    bound 1, stores: 8 B per value at 6.29 TB/s allows {COPY_RATE / 8:.3e} values/s: the kernel runs at {vps * 8 / COPY_RATE:5.1%} of it ({vps * 8 / 1e12:.3f} TB/s stored)")
        kmed = k_main_cold(pkg, tabs, planets, d_el, d_nu, W, reps)
        lines.append(f"    bound 2, arithmetic: k_main, forward only, cold row loop (OCTO_OPT_WARM_START = 0), same tables: {kmed * 1e3:8.3f} ms = {R * W / kmed:.3e} rows/s, "
                     f"{solves / kmed:.3e} solves/s: the matrix kernel takes {med / kmed:.2f}x its time")
        lines.append(f"    -> {'the stores bind' if vps * 8 / COPY_RATE > 0.7 else 'the cold solve and the density bind, not the stores'}")
        smed, lo, hi = event_times(lambda: lib.octo_pointwise_summary_device(h, d_el.data_ptr(), W, W, nu_ptr, d_sum.data_ptr(), stream), reps)
        lines.append(f"  summary (block partials + merge)      : {smed * 1e3:8.3f} ms (min {lo * 1e3:.3f}, max {hi * 1e3:.3f})  {R * W / smed:.3e} values/s reduced = {smed / med:.2f}x the matrix kernel's time")
        ts = []
        for _ in range(4):
            t0 = time.perf_counter(); pw.values(elems, nuis); ts.append(time.perf_counter() - t0)
        lines.append(f"  host-buffer matrix call, copies included (wall): {min(ts[1:]) * 1e3:8.1f} ms = {R * W * 8 / min(ts[1:]) / 1e9:.2f} GB/s to the host")
        ts = []
        for _ in range(4):
            t0 = time.perf_counter(); pw.summary(elems, nuis); ts.append(time.perf_counter() - t0)
        lines.append(f"  host-buffer summary call, copies included (wall): {min(ts[1:]) * 1e3:8.2f} ms")
        per_row = one_row_route(pkg, tabs, planets, elems, nuis)
        lines.append(f"  without this library — a one-row dataset and one octo_eval per datum (octo_dataset_create + octo_eval + destroy, host buffers): "
                     f"{per_row * 1e3:.3f} ms per row, timed on 32 rows; SCALED to R = {R}: {per_row * R * 1e3:.1f} ms = {per_row * R / min(ts[1:]):.0f}x the host-buffer summary call")
    finally:
        pw.close()


def accuracy(pkg, lines):
    import oracle_binding as ob
    import predict_reference as ref
    import pointwise_reference as tp
    lines.append("\nobserved error maxima against oracle_eval on one-row sub-tables (the cases of tests/test_pointwise.py; bar for a value: 1e-11 · max(1, |ll|)):")
    tabs, planets, elems, nuis, _ = ref.two_planet_system(seed=11, W=600)
    tabs = [tp.head(t) for t in tabs]
    refm = tp.reference_matrix(ob, tabs, planets, elems, nuis)
    pw = pkg.Pointwise(tabs, planets)
    try:
        err = tp.check_values("two planets, four tables, W = 600", pw.values(elems, nuis), refm)
        worst = tp.check_summary("two planets, W = 600", pw.summary(elems, nuis), refm)
    finally:
        pw.close()
    lines.append(f"  values, two planets x (RA/Dec + cor, sep/PA, RV_ABS + basis, RV_REL), 7 rows each, W = 600: {err:.3e}   (|ll| up to {np.abs(refm).max():.3e})")
    lines.append("  summary of the same, error / bar (the bars of tests/test_pointwise.py): " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    tabs, planets, elems, nuis = tp.five_planets(pkg, 70)
    refm = tp.reference_matrix(ob, tabs, planets, elems, nuis)
    pw = pkg.Pointwise(tabs, planets)
    try:
        err = tp.check_values("five planets", pw.values(elems, nuis), refm)
    finally:
        pw.close()
    lines.append(f"  values, five planets (the run-time route), RA/Dec + cor on planet 3 and RV_ABS + basis, W = 70: {err:.3e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "pointwise_throughput.txt"))
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pointwise_bench: no GPU: the figures of this file are measured, never estimated")
    import synth
    pkg = load_package()
    capi = pkg.capi
    lines = [f"tools/pointwise_bench.py on {torch.cuda.get_device_name(0)}: kernel times from HIP events around one device call, median of {args.reps} after warm-up",
             f"liboctofitter_hip_pointwise.so: {POINTWISE_LIB.stat().st_size} bytes"]
    V = capi.ORBIT_VISUAL_KEP
    cfg = synth.config_astrom(n_epochs=1_000, n_walkers=10_000, cfg=3)
    t = cfg["table"]
    tabs = [dict(kind=capi.ASTROM_RADEC, planet=0, epoch=t["epoch"], y1=t["ra"], y2=t["dec"], s1=t["σ_ra"], s2=t["σ_dec"], cor=None, extra=None)]
    bench_shape(pkg, "user shape", tabs, [dict(orbit_kind=V, has_mass=0)], cfg["elems"], None, args.reps, lines)
    c4 = synth.config_two_planet()
    a, r = c4["astrom"], c4["rv"]
    tabs = [dict(kind=capi.ASTROM_RADEC, planet=1, epoch=a["epoch"], y1=a["ra"], y2=a["dec"], s1=a["σ_ra"], s2=a["σ_dec"], cor=None, extra=None),
            dict(kind=capi.RV_ABS, planet=-1, epoch=r["epoch"], y1=r["rv"], y2=None, s1=r["σ_rv"], s2=None, cor=None, extra=None)]
    bench_shape(pkg, "config 4's tables", tabs, [dict(orbit_kind=V, has_mass=1), dict(orbit_kind=V, has_mass=1)], c4["elems"], c4["nuis"], args.reps, lines)
    accuracy(pkg, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
