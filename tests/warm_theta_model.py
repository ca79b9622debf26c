"""NumPy restatement (float64) of k_main's θ-loop (octo_device.h: kepler_warm_theta), of the rule that routes a tile to it (octo_kernels.h) and of the walker-tile
sort's key (octo_tile.h: k_tile_sort with TileArgs::theta), on top of warm_newton_model.py / warm_newton_mid_model.py, which stay as they are — shared by
tests/test_warm_theta_model.py and tools/warm_rates.py. No GPU, no package import.

Once four steps θ_j = E_j − E_{j−1} are recorded the row extrapolates the whole step, dE = 4(θ₁ + θ₃) − 6θ₂ − θ₄, in place of the second-order predictor plus the
extrapolated miss; the rotation, f0, the Newton head and the exits (a-priori reject -> cold; every |δ| <= τ -> Newton-only; <= τ₂ -> middle; <= WARM_TOL -> fourth
order; else cold) are warm_newton_mid_model's. While fewer than four steps are recorded the row is the parent's warm step (class STARTUP). A tile takes the loop when
every lane is valid and has x = ΔM/(1 − e) < WARM_THETA_X0; the other tiles keep warm_newton_mid_model's loop. As there, every row is modelled from the EXACT previous
state, and the recorded θ is the true step (the arms agree with it to rounding)."""
import numpy as np

import warm_bound_model as wbm
import warm_newton_mid_model as wmm
import warm_newton_model as wnm

WARM_THETA_X0 = 0.012      # octo_device.h: WARM_THETA_X0
TILE_SEG = 1024            # octo_tile.h
TILE_XK = 17
L = np.longdouble
COLD, FOURTH, NEWTON, MIDDLE, STARTUP = 0, 1, 2, 3, 4
TWO_PI = 2 * np.pi


def step_dm(elems, h, k_yr):
    """ΔM of one table step of h days"""
    return TWO_PI * h / (k_yr * np.sqrt(elems[0] ** 3 / elems[6]))


def slow(elems, h, k_yr, x0=WARM_THETA_X0):
    """the lane's half of the routing rule: a valid e and ΔM/(1 − e) below x0 (a NaN fails)"""
    e = elems[1]
    with np.errstate(invalid="ignore", divide="ignore"):
        return (e >= 0.0) & (e < 1.0) & (np.abs(step_dm(elems, h, k_yr)) / (1.0 - e) < x0)


def qualifying_tiles(elems, h, k_yr, order=None, x0=WARM_THETA_X0):
    """per tile of 64 (the last one may be partial) in the given order: every lane slow"""
    s = slow(elems, h, k_yr, x0)
    s = s if order is None else s[order]
    return np.array([bool(s[i:i + 64].all()) for i in range(0, s.size, 64)])


def sort_key(elems, h, k_yr, theta=True, x0=WARM_THETA_X0):
    """k_tile_sort's bucket per walker: TILE_XK classes of x for the lanes that never fail the a-priori test (one class with theta off), 24 log-spaced classes of the
    expected failing share p, 7 veto classes"""
    e = elems[1].astype(np.float64)
    dM = np.abs(step_dm(elems, h, k_yr))
    with np.errstate(invalid="ignore", divide="ignore"):
        veto = ~(dM <= wbm.WARM_DM_VETO) | ~(e >= 0.0) | ~(e < 1.0)
        xv = np.log2(dM / wbm.WARM_DM_VETO) * 2.0
        bv = TILE_XK + 24 + np.where(xv >= 0.0, np.minimum(np.nan_to_num(xv, nan=6.0, posinf=6.0), 6.0).astype(int), np.where(xv < 0.0, 0, 6))
        thr = wbm.warm_thr(e, dM)
        g = 1.0 - 1.0 / thr
        never = e <= g
        xs = dM / (1.0 - e)
        bx = np.clip(np.floor(2.0 * np.log2(xs / x0) + 8.0), 0, TILE_XK - 1)
        bx = np.where(theta, np.nan_to_num(bx, nan=0.0), 0.0).astype(int)
        c = np.clip(g / e, -1.0, 1.0)
        E0 = np.arccos(c)
        p = np.clip((E0 - e * np.sin(E0)) / np.pi, 0.0, 1.0)
        xp = (np.log2(np.maximum(p, 1e-30)) + 17.0) * (24.0 / 17.0)
        bp = TILE_XK + np.where(xp > 0.0, np.minimum(np.nan_to_num(xp, nan=0.0), 23.0).astype(int), 0)
    return np.where(veto, bv, np.where(never, bx, bp))


def sorted_order(elems, h, k_yr, theta=True, seg=TILE_SEG):
    """perm[sorted position] = walker: a stable sort by bucket inside every segment"""
    key = sort_key(elems, h, k_yr, theta)
    return np.concatenate([s0 + np.argsort(key[s0:s0 + seg], kind="stable") for s0 in range(0, key.size, seg)])


def simulate(elems, t, k_yr, rng):
    """The θ-loop on EVERY tile of elems [9, W] (W a multiple of 64, tiles in the order given) over the evenly spaced rows t: cls [tiles, rows] and lane_cls; per
    lane-row delta (|δ| of the Newton head on θ rows), err_theta (D-weighted error of (sin E, cos E) of the arm the row took), err_parent (the parent's warm step
    on the same row), invd_rel (relative error of 1/D on Newton-only rows). Which tiles would take the loop is qualifying_tiles()."""
    e = elems[1].astype(np.float64)
    W, n = e.size, t.size
    assert W % 64 == 0
    E, dM = wnm.exact_anomalies(elems, t, k_yr)
    el = e.astype(L)[:, None]
    sE = np.sin(E).astype(np.float64); cE = np.cos(E).astype(np.float64)
    Dl = 1 - el * np.cos(E)
    invD = (1 / Dl).astype(np.float64); D = Dl.astype(np.float64)
    thr = wbm.warm_thr(e, dM * (1 + 2.0 ** -18))
    veto = (np.abs(dM) > wbm.WARM_DM_VETO).reshape(-1, 64).any(axis=1)
    tl, tl2 = wnm.tau(e), wmm.tau2(e)
    T = W // 64
    cls = np.zeros((T, n), dtype=np.int8)
    nan = lambda: np.full((W, n), np.nan)
    err_th, err_par, invd_rel, delta = nan(), nan(), nan(), nan()
    hist = np.zeros((4, W))
    cnt = np.zeros(T, dtype=np.int64)
    lane = lambda x: np.repeat(x, 64)
    every = lambda m: ~(m.reshape(T, 64).any(axis=1))
    derr = lambda s, c, j: np.maximum(np.abs(s - sE[:, j]), np.abs(c - cE[:, j])) * D[:, j]
    for j in range(1, n):
        s0, c0, i0 = sE[:, j - 1], cE[:, j - 1], invD[:, j - 1]
        full = cnt >= 4
        dE = 4.0 * (hist[0] + hist[2]) + (-6.0 * hist[1] - hist[3])
        s1, c1, f0 = wnm.rotate_f0(s0, c0, dE, dM, e)
        r1, d = wnm.newton_head(c1, f0, e, rng)
        apriori = every(i0 >= thr) & ~veto
        with np.errstate(invalid="ignore"):
            cold = ~apriori | (full & ~every(np.abs(d) > wbm.WARM_TOL))
            newton = full & ~cold & every(np.abs(d) > tl)
            middle = full & ~cold & ~newton & every(np.abs(d) > tl2)
        startup = ~full & ~cold
        cls[:, j] = np.where(cold, COLD, np.where(startup, STARTUP, np.where(newton, NEWTON, np.where(middle, MIDDLE, FOURTH))))
        sn, cn, rn = wnm.newton_tail(s1, c1, r1, d, e)
        sm, cm, _, _ = wmm.middle_arm(s1, c1, r1, d, e)
        s4, c4, _ = wnm.fourth_order(s1, c1, f0, e, rng)
        sp, cpar = wbm.warm_arm(s0, c0, i0, dM, e, rng)
        k = lane(cls[:, j])
        s = np.where(k == NEWTON, sn, np.where(k == MIDDLE, sm, np.where(k == FOURTH, s4, sp)))
        c = np.where(k == NEWTON, cn, np.where(k == MIDDLE, cm, np.where(k == FOURTH, c4, cpar)))
        cl = k == COLD
        delta[:, j] = np.where(lane(full), np.abs(d), np.nan)
        err_th[:, j] = np.where(cl, np.nan, derr(s, c, j))
        err_par[:, j] = np.where(cl, np.nan, derr(sp, cpar, j))
        invd_rel[:, j] = np.where(k == NEWTON, np.abs(rn * D[:, j] - 1.0), np.nan)
        th = (E[:, j] - E[:, j - 1]).astype(np.float64)
        hist = np.where(cl[None, :], 0.0, np.concatenate([th[None, :], hist[:-1]], axis=0))
        cnt = np.where(cold, 0, np.minimum(cnt + 1, 4))
    return dict(cls=cls, lane_cls=np.repeat(cls, 64, axis=0), delta=delta, err_theta=err_th, err_parent=err_par, invd_rel=invd_rel, tau=tl, tau2=tl2)


def per_tile_rule(theta_cls, newton_cls, qual):
    """the routing the kernel makes: a qualifying tile's rows from the θ-loop, every other tile's from warm_newton_mid_model.simulate"""
    return np.where(qual[:, None], theta_cls, newton_cls)
