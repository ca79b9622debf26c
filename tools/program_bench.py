#!/usr/bin/env python
"""Cost of the expression-program callback (include/octofitter_hip_draws.h: octo_draws_program_logpost_device) against the device model's
octo_model_logpost_device, for the D = 11 reference test model (tools/hmc_bench.py: make_model) written as a program; writes
profiles/program_throughput.txt.

    python tools/program_bench.py [--out profiles/program_throughput.txt] [--reps 30] [--epochs 8 10000]

Per table size and W = 1, 1 024 and 10 000, from HIP events around the calls, median of `reps` after warm-up: the model callback with its
gradient, the program callback with its gradient, and the three steps of the latter as far as the public calls reach them — the likelihood
call alone (octo_eval_device on the program's own inputs, with gradients), the forward sweep alone (octo_draws_program_values_device of one
node: k_prog_fwd's arithmetic without the streamed values), and the rest (the streamed values and k_prog_bwd) as the difference. The
expectation the file confirms or refutes: at W >= 1 024 the two program kernels together (callback − likelihood) cost less than the
likelihood call between them; at W = 1 the program route, three launches, loses to the model's single fused launch, and the file says by
how much. No time is a pass condition.
"""
import argparse
import math
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tools")); sys.path.insert(0, str(ROOT / "tests"))
import torch            # noqa: E402
from __graft_entry__ import load_package      # noqa: E402
from hmc_bench import event_times, make_model      # noqa: E402

BATCHES = (1, 1024, 10_000)


def identity_program(pkg, model):
    """The standard model as a program (host/derived.py): THETA sources are bare nodes, a UniformCircular pair is ATAN2 + MULC + its
    UnitLength term, tp is a TPERI binding."""
    d, cap = pkg.derived, pkg.capi
    prog, binds, angle = d.Program(model.D), [], {}
    for kind, i0, i1, flags, value in list(model._esrc) + list(model._nsrc):
        if kind == cap.SRC_CONST:
            binds.append((d.BIND_NODE, prog.node(d.Sym.of(value)), 0.0))
        elif kind == cap.SRC_THETA:
            binds.append((d.BIND_NODE, i0, 0.0))
        else:
            x, y = d.theta(i0), d.theta(i1)
            if (i0, i1) not in angle:
                angle[(i0, i1)] = d.atan(y, x)
            if flags & cap.SRC_FLAG_UNITLEN:
                prog.term(d.unit_length(x, y))
            binds.append((d.BIND_NODE, prog.node(angle[(i0, i1)] * (value * (1.0 / (2 * math.pi)))), 0.0) if kind == cap.SRC_CIRCULAR
                         else (d.BIND_TPERI, prog.node(angle[(i0, i1)]), value))
    return prog, binds


def bench_table(pkg, n_epochs, reps, lines):
    model = make_model(pkg, n_epochs)
    prog, binds = identity_program(pkg, model)
    pd = pkg.PriorDraws(model, program=(prog, binds))
    try:
        lines.append(f"\n{n_epochs} RA/Dec rows, D = {model.D}, {len(prog.ops)} ops ({model.D + len(prog.ops)} nodes, {(model.D + len(prog.ops)) * 512} B of LDS a block), "
                     f"{len(prog.terms)} terms")
        for W in BATCHES:
            tt = pd.sample(20261020, 0, W, theta=False, logprior_t=False)[1]
            el, nu = model.kernel_inputs(model.invlink(tt.cpu().numpy()))
            el_t = torch.as_tensor(el, device=tt.device).contiguous()
            nu_t = None if nu is None else torch.as_tensor(nu, device=tt.device).contiguous()
            lp_m, g_m = model.logpost_device(tt)
            lp_p, g_p = pd.program_logpost(tt)
            torch.cuda.synchronize()
            fin = torch.isfinite(lp_m)
            err = float(((lp_p - lp_m).abs() / lp_m.abs().clamp(min=1.0))[fin].max()) if bool(fin.any()) else float("nan")
            t_m, lo_m, hi_m = event_times(lambda: model.logpost_device(tt), reps)
            t_p, lo_p, hi_p = event_times(lambda: pd.program_logpost(tt, out=(lp_p, g_p)), reps)
            t_l, lo_l, hi_l = event_times(lambda: model.ln_like.ln_like_device(el_t, nu_t, grad=True), reps)
            t_f, lo_f, hi_f = event_times(lambda: pd.program_values(tt, [model.D]), reps)
            kernels = t_p - t_l
            lines.append(f"  W = {W}: largest |Δℓπ|/max(1, |ℓπ|) against the model {err:.2e}")
            lines.append(f"    octo_model_logpost_device (with gradient)          : {t_m * 1e3:9.4f} ms (min {lo_m * 1e3:.4f}, max {hi_m * 1e3:.4f})")
            lines.append(f"    octo_draws_program_logpost_device (with gradient)  : {t_p * 1e3:9.4f} ms (min {lo_p * 1e3:.4f}, max {hi_p * 1e3:.4f}): {t_p / t_m:5.2f} x the model")
            lines.append(f"    … octo_eval_device on its inputs (with gradients)  : {t_l * 1e3:9.4f} ms (min {lo_l * 1e3:.4f}, max {hi_l * 1e3:.4f}): {t_l / t_p:6.1%} of the callback")
            lines.append(f"    … the forward sweep alone (program_values, 1 node) : {t_f * 1e3:9.4f} ms (min {lo_f * 1e3:.4f}, max {hi_f * 1e3:.4f}): {t_f / t_p:6.1%}")
            lines.append(f"    … the rest (streamed values, k_prog_bwd)           : {max(kernels - t_f, 0.0) * 1e3:9.4f} ms: {max(kernels - t_f, 0.0) / t_p:6.1%}")
            lines.append(f"    the two program kernels together {kernels * 1e3:.4f} ms {'<' if kernels < t_l else '>='} the likelihood call {t_l * 1e3:.4f} ms")
    finally:
        pd.close()
        model.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "program_throughput.txt"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--epochs", type=int, nargs="+", default=[8, 10_000])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("program_bench: no GPU: the figures of this file are measured, never estimated")
    pkg = load_package()
    lines = [f"tools/program_bench.py on {torch.cuda.get_device_name(0)}: HIP events around the calls, median of {args.reps} after warm-up"]
    for n_epochs in args.epochs:
        bench_table(pkg, n_epochs, args.reps, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
