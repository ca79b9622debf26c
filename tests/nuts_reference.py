"""
The NUTS transition of include/octofitter_hip_draws.h (octo_draws_nuts_device), restated in NumPy on top of tests/hmc_reference.py: the
three new purposes of the counter generator, the lockstep build of the tree one leaf per chain per round, the checkpointed no-U-turn
tests, multinomial sampling inside a subtree and the biased progressive merge. Vectorised over the chains; a round evaluates the
chains still building, the others are frozen. It imports nothing of the library; `logpost` is the callable hmc_reference.hmc_step takes.

    r = nuts_transition(priors, theta_t, beta, eps, inv_mass, max_depth, seed, step, chain0=0, logpost=None)
    r["theta_t"], r["logpost"], r["loglike"], r["log_accept"], r["accepted"], r["depth"], r["n_leapfrog"], r["diverged"]
    r["stop"] (STOP_*), r["selected"] (the leaf number of the returned point, 0 = the start), r["margin"], r["rounds"]

margin: per chain the smallest margin of any decision it made — both products of every U-turn test relative to ‖p‖·‖ρ‖ in the inv_mass
metric, |log u − threshold| of every leaf and merge draw, |Δ − 1000| of every leaf. A chain whose margin exceeds 1e-6 is DECIDED: a
computation that differs in the last bits makes the same decisions.

nuts_brute_force states the stopping rule a second time, as plainly as it can be: every doubling is built in full, its leaves laid out in
a list, and every aligned block of 2^k leaves inside it tested by direct sums.

Two deliberately wrong samplers serve conditions of tests/test_nuts_reference.py. variant="uniform_leaf" picks a subtree's proposal with
equal weights: the stationarity condition fails on it. variant="short_stack" stores its checkpoints in slot min(imax, SHORT_STACK − 1), a stack of
four planes, while the walk-back reads the slots imin … imax it always reads: identical while popc(n >> 1) <= 3, that is in subtrees of at
most 16 leaves (trees of depth <= 5), and wrong from leaf n = 30 of a longer subtree on — the store of n = 30 overwrites the checkpoint
of n = 28, and the test of n = 31 reads a plane that was never written.
"""
import math

import numpy as np

import hmc_reference as ref

PURPOSE_NUTS_DIRECTION, PURPOSE_NUTS_LEAF, PURPOSE_NUTS_MERGE = 6, 7, 8
MAX_DEPTH = 10
DELTA_MAX = 1000.0
STOP_NONE, STOP_MAX_DEPTH, STOP_TURN_SUBTREE, STOP_TURN_TREE, STOP_DIVERGED, STOP_DEAD = 0, 1, 2, 3, 4, 5
MARGIN = 1e-6
SHORT_STACK = 4      # the planes of variant="short_stack": popc(n >> 1) <= 3 for n <= 15


def nuts_counter(purpose, c, word1, step):
    """(c, j or the leaf number, purpose, step)"""
    assert purpose in (PURPOSE_NUTS_DIRECTION, PURPOSE_NUTS_LEAF, PURPOSE_NUTS_MERGE)
    return (int(c) & ref.M64, int(word1), purpose, int(step) & ref.M64)


def nuts_uniforms(seed, step, chains, word1, purpose):
    """u of word 0 of the counter (c, word1, purpose, step), one per chain index"""
    return ref.u01(ref.philox_vec((seed, ref.KEY1), np.asarray(chains, dtype=np.uint64), np.asarray(word1, dtype=np.uint64), purpose, np.uint64(step))[0])


class _Setup:
    """What the two statements share: the inputs broadcast, the generator of a chain subset, the sums in index order, the leapfrog halves."""

    def __init__(self, priors, theta_t, beta, eps, inv_mass, seed, step, chain0, logpost):
        self.priors, self.logpost, self.seed, self.step = priors, logpost, seed, step
        self.theta_t = np.array(theta_t, dtype=np.float64)
        self.D, self.W = D, W = self.theta_t.shape
        assert D == len(priors)
        self.beta = np.zeros(W) if logpost is None else (np.ones(W) if beta is None else np.array(np.broadcast_to(np.asarray(beta, dtype=np.float64), (W,))))
        self.eps = np.array(np.broadcast_to(np.asarray(eps, dtype=np.float64), (W,)))
        self.inv_mass = inv_mass
        self.im = np.ones(D) if inv_mass is None else np.asarray(inv_mass, dtype=np.float64)
        self.chains = ref.chain_indices(chain0, W)
        self.chain0 = chain0

    def uniforms(self, s, word1, purpose):
        return nuts_uniforms(self.seed, self.step, self.chains[s], word1, purpose)

    def dot(self, x, y):
        """xᵀ(inv_mass ⊙ y), index order"""
        a = np.zeros(x.shape[1])
        for d in range(self.D):
            a = a + x[d] * (self.im[d] * y[d])
        return a

    def kinetic(self, p):
        K = np.zeros(p.shape[1])
        for d in range(self.D):
            K = K + self.im[d] * p[d] * p[d]
        return 0.5 * K

    def evaluate(self, q, s):
        """hmc_reference.tempered, and the header's dead test where that module's analytic log|J| = θ_t of a one-sided link hides it: a
        linked x that rounds onto the bound of its support has log|J| = log 0, a non-finite term — the prior is healed, the point dead"""
        E, g, dead, lp, lpt = ref.tempered(self.priors, q, self.beta[s], self.logpost)
        for d, pr in enumerate(self.priors):
            a, b = ref.support(pr)
            if math.isfinite(a) != math.isfinite(b):
                dead = dead | (ref.invlink(pr, q[d])[0] == (a if math.isfinite(a) else b))
        return E, g, dead, lp, lpt

    def open(self):
        p0 = ref.momentum(self.seed, self.step, self.chain0, self.W, self.D, self.inv_mass)
        E0, g0, dead0, lp0, lpt0 = self.evaluate(self.theta_t, slice(None))
        return p0, g0, dead0, lp0, lpt0, -E0 + self.kinetic(p0)

    def half_kick_and_drift(self, q, p, g, v, e):
        ph = p + (v * (0.5 * e)) * g
        return q + (v * e) * (self.im[:, None] * ph), ph

    def closing_half_kick(self, ph, g, v, e):
        return ph + (v * (0.5 * e)) * g

    def direction(self, s, j):
        return np.where(self.uniforms(s, j, PURPOSE_NUTS_DIRECTION) < 0.5, 1.0, -1.0)


def _finish(S, theta_t, out_lp, out_lpt, sum_acc, nleaf, accepted, depth, diverged, stop, selected, margin, rounds):
    with np.errstate(all="ignore"):
        ll = out_lp - out_lpt
        ll = np.where(np.isfinite(ll), ll, -np.inf)
        log_accept = np.log(sum_acc / nleaf)
    return dict(theta_t=theta_t, logpost=out_lp, loglike=ll, log_accept=log_accept, accepted=accepted, depth=depth, n_leapfrog=nleaf, diverged=diverged,
                stop=stop, selected=selected, margin=margin, rounds=rounds)


def nuts_transition(priors, theta_t, beta, eps, inv_mass, max_depth, seed, step, chain0=0, logpost=None, variant=None):
    assert 1 <= max_depth <= MAX_DEPTH and variant in (None, "uniform_leaf", "short_stack")
    slot = (lambda i: np.minimum(i, SHORT_STACK - 1)) if variant == "short_stack" else (lambda i: i)      # where a checkpoint is stored
    S = _Setup(priors, theta_t, beta, eps, inv_mass, seed, step, chain0, logpost)
    D, W = S.D, S.W
    with np.errstate(all="ignore"):
        p0, g0, dead0, lp0, lpt0, H0 = S.open()
        theta = S.theta_t.copy()
        qL, pL, gL, qR, pR, gR = theta.copy(), p0.copy(), g0.copy(), theta.copy(), p0.copy(), g0.copy()
        prop, prop_lp, prop_lpt = theta.copy(), lp0.copy(), lpt0.copy()
        sprop, sprop_lp, sprop_lpt = theta.copy(), lp0.copy(), lpt0.copy()
        rho, rho_s = p0.copy(), np.zeros((D, W))
        ck_p, ck_r = np.zeros((max_depth, D, W)), np.zeros((max_depth, D, W))
        out_lp, out_lpt = lp0.copy(), lpt0.copy()
        logw, logw_s, sum_acc = np.zeros(W), np.zeros(W), np.zeros(W)
        j, n, nleaf, sel, ssel = (np.zeros(W, dtype=np.int64) for _ in range(5))
        stop = np.where(dead0, STOP_DEAD, STOP_NONE)
        diverged, accepted = np.zeros(W, dtype=bool), np.zeros(W, dtype=bool)
        margin = np.full(W, np.inf)
        v = np.ones(W)
        trial, pt = theta.copy(), p0.copy()
        s = np.nonzero(stop == STOP_NONE)[0]
        v[s] = S.direction(s, j[s])
        trial[:, s], pt[:, s] = S.half_kick_and_drift(theta[:, s], p0[:, s], g0[:, s], v[s], S.eps[s])
        rounds = 0

        def note(idx, m):
            margin[idx] = np.minimum(margin[idx], m)

        def turn_test(idx, pa, pb, r):
            """whether the block with end momenta pa, pb and sum r turns; the margins of both products"""
            a, b = S.dot(pa, r), S.dot(pb, r)
            nr = np.sqrt(S.dot(r, r))
            note(idx, np.abs(a) / (np.sqrt(S.dot(pa, pa)) * nr))
            note(idx, np.abs(b) / (np.sqrt(S.dot(pb, pb)) * nr))
            return (a <= 0.0) | (b <= 0.0)

        while s.size:
            rounds += 1
            vs, es = v[s], S.eps[s]
            q1 = trial[:, s]
            E1, g1, dead1, lp1, lpt1 = S.evaluate(q1, s)
            p1 = S.closing_half_kick(pt[:, s], g1, vs, es)
            delta = (-E1 + S.kinetic(p1)) - H0[s]
            div = dead1 | ~(delta <= DELTA_MAX)
            fin = ~dead1 & np.isfinite(delta)
            note(s[fin], np.abs(delta[fin] - DELTA_MAX))
            nleaf[s] += 1
            sum_acc[s] += np.where(div, 0.0, np.minimum(1.0, np.exp(-delta)))
            lw = np.where(div, -np.inf, -delta)
            first = n[s] == 0
            lws = np.where(first, lw, np.logaddexp(logw_s[s], lw))
            logw_s[s] = lws
            thr = -np.log(n[s] + 1.0) if variant == "uniform_leaf" else lw - lws
            lu = np.log(S.uniforms(s, nleaf[s], PURPOSE_NUTS_LEAF))
            take = ~div & (first | (lu < thr))
            drawn = ~div & ~first
            note(s[drawn], np.abs(lu - thr)[drawn])
            right = vs > 0
            for side, (qe, pe, ge) in ((right, (qR, pR, gR)), (~right, (qL, pL, gL))):
                qe[:, s[side]], pe[:, s[side]], ge[:, s[side]] = q1[:, side], p1[:, side], g1[:, side]
            rs = np.where(first[None, :], p1, rho_s[:, s] + p1)
            rho_s[:, s] = rs
            t = s[take]
            sprop[:, t], sprop_lp[t], sprop_lpt[t], ssel[t] = q1[:, take], lp1[take], lpt1[take], nleaf[t]
            # checkpoints: leaf n even stores, leaf n odd tests every aligned sub-subtree that ends at it
            ns = n[s]
            imax = np.array([bin(int(x) >> 1).count("1") for x in ns], dtype=np.int64)
            tz = np.array([(int(x) ^ (int(x) + 1)).bit_length() - 1 for x in ns], dtype=np.int64)      # trailing one-bits of n
            imin = imax - tz + 1
            even = ns % 2 == 0
            ck_p[slot(imax[even]), :, s[even]] = p1[:, even].T
            ck_r[slot(imax[even]), :, s[even]] = rs[:, even].T
            turned = np.zeros(s.size, dtype=bool)
            for k in range(max_depth):
                i = imax - k
                m = ~even & ~div & ~turned & (i >= imin)
                if not m.any():
                    continue
                cp, cr = ck_p[i[m], :, s[m]].T, ck_r[i[m], :, s[m]].T
                turned[m] = turn_test(s[m], cp, p1[:, m], rs[:, m] - cr + cp)
            ended = div | turned
            stop[s[div]] = STOP_DIVERGED
            diverged[s[div]] = True
            stop[s[turned]] = STOP_TURN_SUBTREE
            complete = ~ended & (ns + 1 == (1 << j[s]))
            c = s[complete]
            if c.size:
                thr = logw_s[c] - logw[c]
                lu = np.log(S.uniforms(c, j[c], PURPOSE_NUTS_MERGE))
                note(c, np.abs(lu - thr))
                t = c[lu < thr]
                prop[:, t], prop_lp[t], prop_lpt[t], sel[t] = sprop[:, t], sprop_lp[t], sprop_lpt[t], ssel[t]
                logw[c] = np.logaddexp(logw[c], logw_s[c])
                rho[:, c] = rho[:, c] + rho_s[:, c]
                j[c] += 1
                turn_tree = turn_test(c, pL[:, c], pR[:, c], rho[:, c])
                stop[c[j[c] == max_depth]] = STOP_MAX_DEPTH
                stop[c[turn_tree]] = STOP_TURN_TREE
                go = c[stop[c] == STOP_NONE]
                v[go] = S.direction(go, j[go])
                n[go] = 0
            more = s[~ended & ~complete]
            n[more] += 1
            done = s[stop[s] != STOP_NONE]
            moved = done[sel[done] != 0]
            theta[:, moved], out_lp[moved], out_lpt[moved] = prop[:, moved], prop_lp[moved], prop_lpt[moved]
            accepted[moved] = True
            trial[:, done] = theta[:, done]
            s = s[stop[s] == STOP_NONE]
            right = v[s] > 0
            qe, pe, ge = (np.where(right[None, :], a[:, s], b[:, s]) for a, b in ((qR, qL), (pR, pL), (gR, gL)))
            trial[:, s], pt[:, s] = S.half_kick_and_drift(qe, pe, ge, v[s], S.eps[s])
        return _finish(S, theta, out_lp, out_lpt, sum_acc, nleaf, accepted, j, diverged, stop, sel, margin, rounds)


def nuts_brute_force(priors, theta_t, beta, eps, inv_mass, max_depth, seed, step, chain0=0, logpost=None):
    """The same transition with the stopping rule in its plainest form. Every doubling is built in full for every chain that reached it;
    then, chain by chain, the list of its leaves is walked: the subtree is abandoned at the first leaf that diverges or at which an aligned
    block of 2^k leaves (k >= 1) ending there turns, the block's ρ being the direct sum of its momenta. Returns depth, stop, selected, theta_t."""
    S = _Setup(priors, theta_t, beta, eps, inv_mass, seed, step, chain0, logpost)
    D, W = S.D, S.W
    with np.errstate(all="ignore"):
        p0, g0, dead0, lp0, lpt0, H0 = S.open()
        theta = S.theta_t.copy()
        ends = {+1: [theta.copy(), p0.copy(), g0.copy()], -1: [theta.copy(), p0.copy(), g0.copy()]}
        stop = np.where(dead0, STOP_DEAD, STOP_NONE)
        depth, selected, nleaf = np.zeros(W, dtype=np.int64), np.zeros(W, dtype=np.int64), np.zeros(W, dtype=np.int64)
        tree_p = [[p0[:, c]] for c in range(W)]      # every momentum of the chain's tree
        logw = np.zeros(W)
        all_chains = np.arange(W)
        for j in range(max_depth):
            going = stop == STOP_NONE
            if not going.any():
                break
            v = S.direction(all_chains, np.full(W, j))
            right = v > 0
            q, p, g = (np.where(right[None, :], ends[+1][k], ends[-1][k]) for k in range(3))
            Q, P, LW, DIV = [], [], [], []
            for _n in range(1 << j):
                q, ph = S.half_kick_and_drift(q, p, g, v, S.eps)
                E1, g, dead1, _lp1, _lpt1 = S.evaluate(q, all_chains)
                p = S.closing_half_kick(ph, g, v, S.eps)
                delta = (-E1 + S.kinetic(p)) - H0
                div = dead1 | ~(delta <= DELTA_MAX)
                Q.append(q); P.append(p); LW.append(np.where(div, -np.inf, -delta)); DIV.append(div)
            for k in range(3):
                ends[+1][k] = np.where(right[None, :], (q, p, g)[k], ends[+1][k])
                ends[-1][k] = np.where(right[None, :], ends[-1][k], (q, p, g)[k])
            for c in np.nonzero(going)[0]:
                first_leaf = nleaf[c] + 1
                pick = None
                for n in range(1 << j):
                    nleaf[c] += 1
                    if DIV[n][c]:
                        stop[c] = STOP_DIVERGED
                        break
                    for k in range(1, j + 1):
                        size = 1 << k
                        if (n + 1) % size == 0:
                            block = [P[m][:, c] for m in range(n + 1 - size, n + 1)]
                            r = np.sum(np.array(block), axis=0)
                            if np.sum(block[0] * S.im * r) <= 0.0 or np.sum(block[-1] * S.im * r) <= 0.0:
                                stop[c] = STOP_TURN_SUBTREE
                    if stop[c] != STOP_NONE:
                        break
                    lws = np.logaddexp.reduce([LW[m][c] for m in range(n + 1)])
                    u = nuts_uniforms(seed, step, S.chains[c:c + 1], first_leaf + n, PURPOSE_NUTS_LEAF)[0]
                    if n == 0 or np.log(u) < LW[n][c] - lws:
                        pick = n
                if stop[c] != STOP_NONE:
                    continue
                u = nuts_uniforms(seed, step, S.chains[c:c + 1], j, PURPOSE_NUTS_MERGE)[0]
                if np.log(u) < lws - logw[c]:
                    selected[c] = first_leaf + pick
                    theta[:, c] = Q[pick][:, c]
                logw[c] = np.logaddexp(logw[c], lws)
                tree_p[c] += [P[m][:, c] for m in range(1 << j)]
                depth[c] = j + 1
                r = np.sum(np.array(tree_p[c]), axis=0)
                if np.sum(ends[-1][1][:, c] * S.im * r) <= 0.0 or np.sum(ends[+1][1][:, c] * S.im * r) <= 0.0:
                    stop[c] = STOP_TURN_TREE
                elif j + 1 == max_depth:
                    stop[c] = STOP_MAX_DEPTH
    return dict(theta_t=theta, depth=depth, stop=stop, selected=selected, n_leapfrog=nleaf)
