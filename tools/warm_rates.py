#!/usr/bin/env python
"""Fallback rates of k_main's warm-started row loop, simulated on the CPU (NumPy) for a table and a batch of walkers — VERDICT r5 item 1:
"fallback-rate histogram by eccentricity bin", and what tiling the walkers by a severity key buys before it is built.

  python tools/warm_rates.py [config3|wide_prior] [--walkers N]

For every walker and every row: 1/D of the PREVIOUS row's solution against the lane's bound thr = warm_thr(e, ΔM) (octo_device.h; restated in
tests/warm_bound_model.py), and — for comparison — against the e-blind form (tol/ΔM³)^(1/5) it replaced (`--parent` prints that one alone);
a wave-row is cold when any of its 64 lanes fails, a wave whose fastest lane vetoes the step bound (ΔM > 0.0314) is cold altogether.
Orders compared: the batch as drawn; walkers sorted by the expected lane failure rate p (the share of the orbit, in mean anomaly, with
1/D >= thr — closed form) in segments of 4 096 (what k_tile_sort does) and over the whole batch.

  python tools/warm_rates.py [config3|wide_prior] [--walkers N] --theta [--rows R]

The θ-loop's pricing (octo_tile.h, octo_api.hip: tile_settle) against a row-by-row simulation (tests/warm_theta_model.py): the tiles that qualify as drawn and in
the order of the device's key (segments of 1 024), the closed-form price (qualifying-tile difference x the saving per wave-row of a slow tile) and, on the first R
rows (default 156), the share of wave-rows each arm takes with today's loop as drawn and with the per-tile rule on the sorted tiles."""
import sys
from pathlib import Path
import numpy as np
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
import synth
import warm_bound_model as wm

VETO = wm.WARM_DM_VETO
which = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith("-") else "config3"
W = int(sys.argv[sys.argv.index("--walkers") + 1]) if "--walkers" in sys.argv else 4096
cfg = synth.config_wide_prior(n_epochs=10_000, n_walkers=W) if which == "wide_prior" else synth.config_astrom(n_epochs=10_000, n_walkers=W, cfg=3)
t = cfg["table"]["epoch"]
el = cfg["elems"]
a, e, tp, M = el[0], el[1], el[5], el[6]
P = synth.K_YR * np.sqrt(a ** 3 / M)
dm = 2 * np.pi * np.median(np.diff(t))
dM = dm / P
veto = dM > VETO


def theta_report():
    import warm_newton_mid_model as wmm
    import warm_theta_model as wtm
    rows = int(sys.argv[sys.argv.index("--rows") + 1]) if "--rows" in sys.argv else 156
    h = float(np.median(np.diff(t)))
    Wt = W - W % 64
    els = el[:, :Wt]
    order = wtm.sorted_order(els, h, synth.K_YR)
    q_given, q_sorted = wtm.qualifying_tiles(els, h, synth.K_YR), wtm.qualifying_tiles(els, h, synth.K_YR, order)
    row_ns = 10.0      # octo_api.hip: TILE_THETA_ROW_US
    print(f"{which}: {Wt} walkers; tiles that qualify for the theta-loop (x < {wtm.WARM_THETA_X0}): {int(q_given.sum())} of {q_given.size} as drawn, {int(q_sorted.sum())} sorted")
    print(f"  closed-form price at {t.size} rows: ({int(q_sorted.sum())} - {int(q_given.sum())}) tiles x {t.size} rows x {row_ns} ns / 1024 SIMDs = "
          f"{(q_sorted.sum() - q_given.sum()) * t.size * row_ns * 1e-3 / 1024:.2f} us per evaluation")
    rng = np.random.default_rng(5)
    tt = t[:rows]
    drawn = wmm.simulate(els, tt, synth.K_YR, rng)["cls"]
    th = wtm.simulate(els[:, order], tt, synth.K_YR, rng)["cls"]
    nw = wmm.simulate(els[:, order], tt, synth.K_YR, rng)["cls"]
    rule = wtm.per_tile_rule(th, nw, q_sorted)
    names = {wtm.NEWTON: "Newton-only", wtm.MIDDLE: "middle", wtm.FOURTH: "fourth order", wtm.STARTUP: "start-up", wtm.COLD: "cold"}
    for label, c in (("as drawn, today's loop", drawn), ("sorted, today's loop", nw), ("sorted, per-tile rule", rule)):
        print(f"  {label:24s} " + "  ".join(f"{n} {float((c == k).mean()):.4f}" for k, n in names.items()))
    print(f"  row-by-row: wave-rows in the theta-loop {float(np.repeat(q_sorted[:, None], rows, axis=1).mean()):.4f} of all (the closed form prices every one of them)")


def lane_fail_share(e, thr):
    """share of the orbit (in mean anomaly) where 1/(1 - e cos E) >= thr, i.e. e cos E >= 1 - 1/thr"""
    g = 1.0 - 1.0 / thr
    c = np.clip(g / np.maximum(e, 1e-300), -1.0, 1.0)
    E0 = np.arccos(c)
    p = (E0 - e * np.sin(E0)) / np.pi
    return np.where(e <= g, 0.0, p)



def report(label, thr):
    print(f"--- bound: {label}")
    p = np.where(veto, 1.0 + dM, lane_fail_share(e, thr))      # vetoing lanes last, fastest at the very end

    # per-lane failure of every row (from the previous row's solution)
    fail = np.zeros((W, t.size), dtype=bool)
    for lo in range(0, W, 256):
        sl = slice(lo, min(lo + 256, W))
        Mm = 2 * np.pi * (t[None, :] - tp[sl, None]) / P[sl, None]
        E = synth._kepler(Mm, e[sl, None])
        invD = 1.0 / (1.0 - e[sl, None] * np.cos(E))
        fail[sl, 1:] = invD[:, :-1] >= thr[sl, None]
    fail[veto, :] = True


    def wave_rows_cold(order):
        n_tiles = W // 64
        f = fail[order[:n_tiles * 64]].reshape(n_tiles, 64, -1)
        return f.any(axis=1).mean()


    ident = np.arange(W)
    seg = np.concatenate([lo + np.argsort(p[lo:lo + 4096], kind="stable") for lo in range(0, W, 4096)])
    for sz in (512, 1024, 2048):
        o = np.concatenate([lo + np.argsort(p[lo:lo + sz], kind="stable") for lo in range(0, W, sz)])
        print(f"  (segments of {sz}: {wave_rows_cold(o):.3%})")
    glob = np.argsort(p, kind="stable")
    print(f"{which}: {W} walkers x {t.size} rows, step {dm / (2 * np.pi):.3f} d; lanes vetoing the step bound: {veto.mean():.3%}; lane-rows failing: {fail[~veto].mean():.3%}")
    print(f"  wave-rows cold   as drawn: {wave_rows_cold(ident):.3%}   sorted by p in segments of 4096: {wave_rows_cold(seg):.3%}   sorted over the batch: {wave_rows_cold(glob):.3%}")
    print("  by eccentricity bin (lanes that do not veto): share of lane-rows failing | mean closed-form p")
    bins = np.linspace(0, 1.0, 11)
    for lo, hi in zip(bins[:-1], bins[1:]):
        m = (e >= lo) & (e < hi) & ~veto
        if m.any():
            print(f"    e in [{lo:.1f}, {hi:.1f}): {fail[m].mean():8.4%} | {p[m].mean():8.4%}   ({m.sum()} walkers)")


if "--theta" in sys.argv:
    theta_report()
    raise SystemExit(0)
if "--parent" not in sys.argv:
    report("warm_thr(e, ΔM) = max((tol/ΔM³)^(1/5), min(c(e), 0.06)/ΔM)", wm.warm_thr(e, dM))
report("the e-blind form (tol/ΔM³)^(1/5)", wm.warm_thr_parent(dM))
