"""
The slice-sampling transition of include/octofitter_hip_draws.h (octo_draws_slice_device), restated in NumPy on top of tests/hmc_reference.py
(the counter generator, the priors, the tempered target) and the evaluation rule of tests/nuts_reference.py (a linked x that rounds onto a
bound of its support is dead): purpose 9 of the generator, Neal's doubling, shrinkage and acceptance test, and the lockstep walk of the chains
through their coordinates one evaluation per chain per round. Vectorised over the chains; a round evaluates the chains still active, the others
are frozen. It imports nothing of the library; `logpost` is the callable hmc_reference.hmc_step takes (its gradient is never looked at).

    r = slice_transition(priors, theta_t, beta, w, p, n_passes, max_shrink, seed, step, chain0=0, logpost=None)
    r["theta_t"], r["logpost"], r["loglike"], r["n_eval"], r["n_expand"], r["n_shrink"], r["n_stuck"], r["status"]
    r["margin"], r["rounds"], and what shows which paths a chain took: r["grow_early"], r["grow_full"] (updates whose doubling stopped by the
    level / ran out to k = p), r["test_rejects"] (candidates the acceptance test rejected), r["dead_trials"] (evaluations at a dead point)

margin: per chain the smallest margin of any comparison it made — |z − E| of every evaluated E, |x − M|/w and |x′ − M|/w of every midpoint of
the acceptance test, |u − ½| of every doubling, |(R̂ − L̂) − 1.1·w|/w of every test iteration. A chain whose margin exceeds MARGIN = 1e-6 is
DECIDED: a computation that differs in the last bits makes the same decisions.

slice_plain states the transition a second time, as plainly as it can be: chain by chain and update by update, Neal's three procedures as
loops with every evaluation made where the figure makes it. No rounds, no phases.

accept_test=False is a deliberately wrong sampler for a condition of tests/test_slice_reference.py: every candidate inside the slice is taken
without the acceptance test, which doubling needs to be reversible.
"""
import numpy as np

import hmc_reference as ref
import nuts_reference as nuts

PURPOSE_SLICE = 9
MAX_DOUBLINGS, MAX_SHRINK, MAX_PASSES = 8, 64, 1024
ACTIVE, DONE, DEAD = 0, 1, 2
MARGIN = 1e-6
PH_L, PH_R, PH_GROW_L, PH_GROW_R, PH_X, PH_TEST_L, PH_TEST_R = range(7)
DO_NOTHING, DO_GROW, DO_TEST, DO_REJECT, DO_SHRINK, DO_ACCEPT, DO_MOVE = range(7)


def slice_counter(c, j, i, step):
    """(c, j·128 + i, 9, step): i = 0 the level (word 0) and the interval's position (word 1), i = k the doubling k, i = 64 + s the shrink proposal s"""
    assert 0 <= i < 128
    return (int(c) & ref.M64, int(j) * 128 + int(i), PURPOSE_SLICE, int(step) & ref.M64)


def slice_uniforms(seed, step, chains, j, i):
    """(u, u′) of words 0 and 1 of the counter (c, j·128 + i, 9, step), one pair per chain index"""
    words = ref.philox_vec((seed, ref.KEY1), np.asarray(chains, dtype=np.uint64), np.asarray(j, dtype=np.uint64) * np.uint64(128) + np.asarray(i, dtype=np.uint64),
                           PURPOSE_SLICE, np.uint64(step))
    return ref.u01(words[0]), ref.u01(words[1])


def slice_transition(priors, theta_t, beta, w, p, n_passes, max_shrink, seed, step, chain0=0, logpost=None, accept_test=True):
    assert 0 <= p <= MAX_DOUBLINGS and 1 <= max_shrink <= MAX_SHRINK and 1 <= n_passes <= MAX_PASSES
    S = nuts._Setup(priors, theta_t, beta, 1.0, None, seed, step, chain0, logpost)
    D, W = S.D, S.W
    widths = np.array(np.broadcast_to(np.asarray(w, dtype=np.float64), (D,)))
    n_updates = n_passes * D
    with np.errstate(all="ignore"):
        theta = S.theta_t.copy()
        E0, _g, dead0, lp0, lpt0 = S.evaluate(theta, slice(None))
        E0 = E0.copy()
        status = np.where(dead0, DEAD, ACTIVE)
        out_lp, out_lpt = lp0.copy(), lpt0.copy()
        trial = theta.copy()
        z, L, R, EL, ER, Lb, Rb, Lh, Rh, ELh, ERh, xp, Ep, lpp, lptp = (np.zeros(W) for _ in range(15))
        j, phase, i, n_eval, n_expand, n_shrink, n_stuck, grow_early, grow_full, test_rejects, dead_trials = (np.zeros(W, dtype=np.int64) for _ in range(11))
        flag = np.zeros(W, dtype=bool)
        margin = np.full(W, np.inf)
        rounds = 0

        def note(idx, m):
            margin[idx] = np.minimum(margin[idx], m)

        def open_update(idx, jj):
            d = jj % D
            u, u1 = slice_uniforms(seed, step, S.chains[idx], jj, 0)
            left = theta[d, idx] - widths[d] * u1
            z[idx] = E0[idx] + np.log(u)
            L[idx] = left
            R[idx] = left + widths[d]
            trial[d, idx] = left
            j[idx] = jj
            phase[idx] = PH_L

        s = np.nonzero(status == ACTIVE)[0]
        open_update(s, np.zeros(s.size, dtype=np.int64))
        while s.size:
            rounds += 1
            E, _g, dead, lp, lpt = S.evaluate(trial[:, s], s)
            E = np.where(dead, -np.inf, E)
            dead_trials[s] += dead
            n_eval[s] += 1
            js, ph, ii = j[s], phase[s], i[s].copy()
            d = js % D
            wd, zs, x = widths[d], z[s], theta[d, s].copy()
            act = np.full(s.size, DO_NOTHING)
            note(s, np.where(np.isfinite(E), np.abs(zs - E), np.inf))
            # 1. the evaluation arrives
            m = ph == PH_L
            EL[s[m]] = E[m]
            trial[d[m], s[m]] = R[s[m]]
            phase[s[m]] = PH_R
            m = ph == PH_GROW_L
            EL[s[m]] = E[m]
            m = (ph == PH_R) | (ph == PH_GROW_R)
            ER[s[m]] = E[m]
            m = (ph == PH_R) | (ph == PH_GROW_L) | (ph == PH_GROW_R)
            ii[m] = np.where(ph[m] == PH_R, 1, ii[m] + 1)
            act[m] = DO_GROW
            m = ph == PH_X
            t = s[m]
            Ep[t], lpp[t], lptp[t] = E[m], lp[m], lpt[m]
            cand = m & (zs < E)
            t = s[cand]
            Lh[t], Rh[t], ELh[t], ERh[t], flag[t] = L[t], R[t], EL[t], ER[t], False
            act[cand] = DO_TEST if accept_test else DO_ACCEPT
            act[m & ~cand] = DO_REJECT
            m = ph == PH_TEST_L
            ELh[s[m]] = E[m]
            m = ph == PH_TEST_R
            ERh[s[m]] = E[m]
            m = (ph == PH_TEST_L) | (ph == PH_TEST_R)
            rej = m & flag[s] & (zs >= ELh[s]) & (zs >= ERh[s])
            test_rejects[s[rej]] += 1
            act[m] = DO_TEST
            act[rej] = DO_REJECT
            # 2. doubling number ii, or the interval stands
            g = act == DO_GROW
            more = g & (ii <= p) & ((zs < EL[s]) | (zs < ER[s]))
            t = s[more]
            u = slice_uniforms(seed, step, S.chains[t], js[more], ii[more])[0]
            note(t, np.abs(u - 0.5))
            left = u < 0.5
            e = np.where(left, L[t] - (R[t] - L[t]), R[t] + (R[t] - L[t]))
            L[t[left]], R[t[~left]] = e[left], e[~left]
            trial[d[more], t] = e
            phase[t] = np.where(left, PH_GROW_L, PH_GROW_R)
            i[t] = ii[more]
            n_expand[t] += 1
            stand = g & ~more
            t = s[stand]
            grow_early[t] += ii[stand] <= p
            grow_full[t] += (ii[stand] > p) & (p > 0)
            Lb[t], Rb[t] = L[t], R[t]
            ii[stand] = 0
            act[stand] = DO_SHRINK
            # 3. the next midpoint of the acceptance test, or the candidate has passed
            tm = act == DO_TEST
            t = s[tm]
            note(t, np.abs((Rh[t] - Lh[t]) - 1.1 * wd[tm]) / wd[tm])
            wide = tm.copy()
            wide[tm] = Rh[t] - Lh[t] > 1.1 * wd[tm]
            t = s[wide]
            M = (Lh[t] + Rh[t]) / 2
            note(t, np.abs(x[wide] - M) / wd[wide])
            note(t, np.abs(xp[t] - M) / wd[wide])
            flag[t] |= (x[wide] < M) != (xp[t] < M)
            low = xp[t] < M
            Rh[t[low]], Lh[t[~low]] = M[low], M[~low]
            trial[d[wide], t] = M
            phase[t] = np.where(low, PH_TEST_R, PH_TEST_L)
            act[tm & ~wide] = DO_ACCEPT
            # 4. a proposal that failed shrinks the interval towards x
            m = act == DO_REJECT
            t = s[m]
            low = xp[t] < x[m]
            Lb[t[low]], Rb[t[~low]] = xp[t[low]], xp[t[~low]]
            ii[m] += 1
            act[m] = DO_SHRINK
            # 5. shrink proposal number ii, or the update is stuck
            sh = act == DO_SHRINK
            stuck = sh & (ii == max_shrink)
            n_stuck[s[stuck]] += 1
            act[stuck] = DO_MOVE
            go = sh & ~stuck
            t = s[go]
            u = slice_uniforms(seed, step, S.chains[t], js[go], 64 + ii[go])[0]
            xp[t] = Lb[t] + u * (Rb[t] - Lb[t])
            trial[d[go], t] = xp[t]
            phase[t] = PH_X
            i[t] = ii[go]
            n_shrink[t] += 1
            # 6. the proposal becomes the coordinate, with what was evaluated there
            m = act == DO_ACCEPT
            t = s[m]
            x[m] = xp[t]
            theta[d[m], t] = xp[t]
            E0[t], out_lp[t], out_lpt[t] = Ep[t], lpp[t], lptp[t]
            act[m] = DO_MOVE
            # 7. the trial point takes the coordinate back; the next update opens, or the chain is done
            m = act == DO_MOVE
            t = s[m]
            trial[d[m], t] = x[m]
            last = js[m] + 1 == n_updates
            status[t[last]] = DONE
            open_update(t[~last], js[m][~last] + 1)
            s = s[status[s] == ACTIVE]
        ll = out_lp - out_lpt
        ll = np.where(np.isfinite(ll), ll, -np.inf)
    return dict(theta_t=theta, logpost=out_lp, loglike=ll, n_eval=n_eval, n_expand=n_expand, n_shrink=n_shrink, n_stuck=n_stuck, status=status, margin=margin,
                rounds=rounds, grow_early=grow_early, grow_full=grow_full, test_rejects=test_rejects, dead_trials=dead_trials)


def slice_plain(priors, theta_t, beta, w, p, n_passes, max_shrink, seed, step, chain0=0, logpost=None):
    """The same transition without the lockstep: one chain after the other, Neal's Fig. 4 (doubling), Fig. 5 (shrinkage) and Fig. 6 (the
    acceptance test) as nested loops. Returns theta_t, logpost and the four counts and the status."""
    S = nuts._Setup(priors, theta_t, beta, 1.0, None, seed, step, chain0, logpost)
    D, W = S.D, S.W
    widths = np.array(np.broadcast_to(np.asarray(w, dtype=np.float64), (D,)))
    theta = S.theta_t.copy()
    out_lp = np.zeros(W)
    counts = {k: np.zeros(W, dtype=np.int64) for k in ("n_eval", "n_expand", "n_shrink", "n_stuck", "status")}
    with np.errstate(all="ignore"):
        for c in range(W):
            idx = np.array([c])

            def energy(q):
                E, _g, dead, lp, lpt = S.evaluate(q[:, None], idx)
                return (-np.inf if dead[0] else E[0]), lp[0], dead[0]

            def uniforms(jj, ii):
                u, u1 = slice_uniforms(seed, step, S.chains[idx], jj, ii)
                return u[0], u1[0]

            q = theta[:, c].copy()
            E0, out_lp[c], dead = energy(q)
            if dead:
                counts["status"][c] = DEAD
                continue
            for jj in range(n_passes * D):
                d = jj % D
                x, wd = q[d], widths[d]

                def f(v):
                    qq = q.copy()
                    qq[d] = v
                    counts["n_eval"][c] += 1
                    return energy(qq)

                u, u1 = uniforms(jj, 0)
                z = E0 + np.log(u)
                L = x - wd * u1
                R = L + wd
                EL = f(L)[0]
                ER = f(R)[0]
                for k in range(1, p + 1):
                    if not (z < EL or z < ER):
                        break
                    if uniforms(jj, k)[0] < 0.5:
                        L = L - (R - L)
                        EL = f(L)[0]
                    else:
                        R = R + (R - L)
                        ER = f(R)[0]
                    counts["n_expand"][c] += 1
                Lb, Rb = L, R
                for s in range(max_shrink):
                    xp = Lb + uniforms(jj, 64 + s)[0] * (Rb - Lb)
                    Ep, lpp, _dead = f(xp)
                    counts["n_shrink"][c] += 1
                    ok = z < Ep
                    if ok:
                        Lh, Rh, ELh, ERh, differ = L, R, EL, ER, False
                        while Rh - Lh > 1.1 * wd:
                            M = (Lh + Rh) / 2
                            if (x < M) != (xp < M):
                                differ = True
                            if xp < M:
                                Rh = M
                                ERh = f(M)[0]
                            else:
                                Lh = M
                                ELh = f(M)[0]
                            if differ and z >= ELh and z >= ERh:
                                ok = False
                                break
                    if ok:
                        q[d], E0, out_lp[c] = xp, Ep, lpp
                        break
                    if xp < x:
                        Lb = xp
                    else:
                        Rb = xp
                else:
                    counts["n_stuck"][c] += 1
            theta[:, c] = q
            counts["status"][c] = DONE
    return dict(theta_t=theta, logpost=out_lp, **counts)
