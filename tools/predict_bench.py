#!/usr/bin/env python
"""Throughput and accuracy of the model-value library (include/octofitter_hip_predict.h) on the device; writes profiles/predict_throughput.txt.

    python tools/predict_bench.py [--out profiles/predict_throughput.txt] [--walkers 10000] [--epochs 1000] [--reps 30]

For W walkers x T epochs (default 1e4 x 1e3): 1 planet x {RAOFF, DECOFF, RADVEL} and 2 planets x {ASTROM_RA, ASTROM_DEC, RV_STAR}, the cube
kernel in both store widths (8-byte and 16-byte stores) and the summary. Per case: kernel time from HIP events around one device call
(median of `reps` after warm-up), bytes stored per second against the 6.29 TB/s float4-copy rate measured for this GPU, Kepler solves per second
against the cold rate of k_main (OCTO_OPT_WARM_START = 0 on BASELINE config 3, timed in this same run), and the host-buffer call with its
copies. Then the observed error maxima per quantity against the oracle (the cases of tests/test_predict.py). No figure is a pass condition.
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import numpy as np      # noqa: E402
import torch            # noqa: E402
from __graft_entry__ import PREDICT_LIB, load_package      # noqa: E402

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


def k_main_cold_rate(pkg, lines, reps):
    """Kepler solves per second of k_main's cold row loop on config 3 (1 planet, 1e4 RA/Dec epochs x 1e4 walkers), from the library's own event timer."""
    import synth
    cfg = synth.config_astrom(n_epochs=10_000, n_walkers=10_000, cfg=3)
    obs, planet = synth.to_mirror(pkg, cfg)
    fn = pkg.make_ln_like(pkg.System(name="s", companions=[planet]), cfg["theta_example"])
    rates = {}
    try:
        fn.set_option(pkg.capi.OPT_WARM_START, 0)
        el = torch.tensor(np.ascontiguousarray(cfg["elems"]), device="cuda")
        W = el.shape[1]
        for grad in (False, True):
            out = (torch.empty(W, dtype=torch.float64, device="cuda"), torch.empty_like(el) if grad else None, None)
            for _ in range(10):
                fn.ln_like_device(el, None, grad=grad, out=out)
            torch.cuda.synchronize()
            fn.timing_enable(1)
            for _ in range(reps):
                fn.ln_like_device(el, None, grad=grad, out=out)
            torch.cuda.synchronize()
            kmed = fn.timing_stats()[0] * 1e-3
            fn.timing_read(reset=True)
            fn.timing_enable(0)
            rates[grad] = 1e8 / kmed
            lines.append(f"k_main, cold row loop (OCTO_OPT_WARM_START = 0), config 3, {'fwd+grad' if grad else 'forward only'}: {kmed * 1e3:8.3f} ms "
                         f"= {rates[grad]:.3e} solves/s")
    finally:
        fn.close()
    return rates


def bench_case(pkg, name, planets, channels, W, T, reps, lines, cold):
    import predict_reference as ref
    P, Cn = len(planets), len(channels)
    elems = ref.random_elements(planets, W, seed=1, e_max=0.95)
    epochs = np.linspace(55000.0, 62000.0, T)
    pr = pkg.Predictor(planets, epochs, channels)
    dev = torch.device("cuda", 0)
    d_el = torch.from_numpy(elems).to(dev)
    ldo = W + (W & 1)
    d_out = torch.empty((Cn * T, ldo), dtype=torch.float64, device=dev)
    d_sum = torch.empty((5, Cn, T), dtype=torch.float64, device=dev)
    lib, h = pr.lib, pr._h
    stream = torch.cuda.current_stream(dev).cuda_stream
    import ctypes as C
    lines.append(f"\n{name}: {P} planet(s), channels {[pkg.predict.QUANTITY_NAMES[q] for q, _ in channels]}, W = {W}, T = {T}: "
                 f"{Cn * T * W * 8 / 1e6:.1f} MB stored, {P * T * W:.2e} solves")
    try:
        for variant, label in ((1, "one walker per lane, 8-byte stores"), (2, "two walkers per lane, 16-byte stores")):
            pr.set_variant(variant)
            med, lo, hi = event_times(lambda: lib.octo_predict_eval_device(h, d_el.data_ptr(), W, W, None, None, d_out.data_ptr(), ldo, C.c_void_p(stream)), reps)
            bps, sps = Cn * T * W * 8 / med, P * T * W / med
            lines.append(f"  cube, {label:38s}: {med * 1e3:8.3f} ms (min {lo * 1e3:.3f}, max {hi * 1e3:.3f})  {bps / 1e12:6.3f} TB/s stored = {bps / COPY_RATE:5.1%} of 6.29 TB/s"
                         f"  {sps:.3e} solves/s = {sps / cold[False]:.2f}x k_main cold fwd, {sps / cold[True]:.2f}x fwd+grad")
        pr.set_variant(0)
        med, lo, hi = event_times(lambda: lib.octo_predict_summary_device(h, d_el.data_ptr(), W, W, None, None, d_sum.data_ptr(), C.c_void_p(stream)), reps)
        sps = P * T * W / med
        lines.append(f"  summary (block partials + merge kernel)           : {med * 1e3:8.3f} ms (min {lo * 1e3:.3f}, max {hi * 1e3:.3f})  {sps:.3e} solves/s = {sps / cold[False]:.2f}x k_main cold fwd")
        ts = []
        for _ in range(4):
            t0 = time.perf_counter(); pr.values(elems); ts.append(time.perf_counter() - t0)
        lines.append(f"  host-buffer cube call, copies included (wall)      : {min(ts[1:]) * 1e3:8.1f} ms = {Cn * T * W * 8 / min(ts[1:]) / 1e9:.2f} GB/s to the host")
        ts = []
        for _ in range(4):
            t0 = time.perf_counter(); pr.summary(elems); ts.append(time.perf_counter() - t0)
        lines.append(f"  host-buffer summary call, copies included (wall)   : {min(ts[1:]) * 1e3:8.2f} ms")
    finally:
        pr.close()


def accuracy(pkg, lines):
    import predict_reference as ref
    p_ = pkg.predict
    lines.append("\nobserved error maxima against the oracle, relative to the quantity's natural scale per walker (bar: 1e-8; e from 0 to 0.999,")
    lines.append("unsorted grids with repeats and epochs 1e5 days from tp):")
    worst = {}
    for kinds in ((0,), (1,), (2,), (3,), (0, 2), (0, 1, 3, 0), (0, 0, 2, 0, 3, 0)):
        planets = [dict(orbit_kind=k, has_mass=0) for k in kinds]
        ch = []
        for i, k in enumerate(kinds):
            if k in (0, 2):
                ch += [(p_.RAOFF, i), (p_.DECOFF, i), (p_.SEP, i), (p_.PA, i)]
            if k != 2:
                ch += [(p_.RADVEL, i)]
        rng = np.random.default_rng(3)
        epochs = rng.uniform(50000.0, 62000.0, 12)
        epochs[1] = epochs[0]; epochs[3] = 160000.0; epochs[5] = -45000.0
        elems = ref.random_elements(planets, 20, seed=100 + len(kinds))
        pr = pkg.Predictor(planets, epochs, ch)
        try:
            errs, _ = ref.channel_errors(planets, elems, epochs, ch, pr.values(elems))
        finally:
            pr.close()
        for k, v in errs.items():
            worst[k] = max(worst.get(k, 0.0), v)
    for P in (2, 4):
        planets = [dict(orbit_kind=0, has_mass=m) for m in (1, 1, 0, 1)[:P]]
        ch = [(p_.RV_STAR, -1)] + [(q, i) for i in range(P) for q in (p_.ASTROM_RA, p_.ASTROM_DEC, p_.ASTROM_SEP, p_.ASTROM_PA, p_.RV_REL)]
        epochs = np.random.default_rng(5).uniform(50000.0, 62000.0, 10)
        elems = ref.random_elements(planets, 18, seed=7 + P, e_max=0.95)
        pr = pkg.Predictor(planets, epochs, ch)
        try:
            errs, _ = ref.channel_errors(planets, elems, epochs, ch, pr.values(elems))
        finally:
            pr.close()
        for k, v in errs.items():
            worst[k] = max(worst.get(k, 0.0), v)
    for k in p_.QUANTITY_NAMES:
        lines.append(f"  {k:11s} {worst[k]:.2e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "predict_throughput.txt"))
    ap.add_argument("--walkers", type=int, default=10_000)
    ap.add_argument("--epochs", type=int, default=1_000)
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("predict_bench: no GPU: the figures of this file are measured, never estimated")
    pkg = load_package()
    p_ = pkg.predict
    lines = [f"tools/predict_bench.py on {torch.cuda.get_device_name(0)}: kernel times from HIP events around one device call, median of {args.reps} after warm-up",
             f"liboctofitter_hip_predict.so: {PREDICT_LIB.stat().st_size} bytes"]
    cold = k_main_cold_rate(pkg, lines, args.reps)
    V = pkg.capi.ORBIT_VISUAL_KEP
    bench_case(pkg, "one planet", [dict(orbit_kind=V, has_mass=0)], [(p_.RAOFF, 0), (p_.DECOFF, 0), (p_.RADVEL, 0)], args.walkers, args.epochs, args.reps, lines, cold)
    bench_case(pkg, "two planets", [dict(orbit_kind=V, has_mass=1), dict(orbit_kind=V, has_mass=1)],
               [(p_.ASTROM_RA, 1), (p_.ASTROM_DEC, 1), (p_.RV_STAR, -1)], args.walkers, args.epochs, args.reps, lines, cold)
    accuracy(pkg, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
