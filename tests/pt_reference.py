"""
The parallel-tempering statistics of include/octofitter_hip_draws.h ("Parallel tempering between the scans"), restated in NumPy in the
stated order: octo_draws_pt_stats_device (stats, restarts), octo_draws_pt_schedule_device (schedule), and the round loop of
host/callers.py: octofit_pigeons_device around any explorer callback (pigeons). plain_stats is the same statistic stated a second time,
as plainly as it goes: a loop over calls, chains and pairs with no blocks and one maximum. It imports nothing of the library.

The layout is k_pt_swap's: ℓ [T][Cn] by replica, slot2rep [Cn][T], β [T] with slot 0 the target. The state acc is [T − 1][8] =
(n, A, n_f, m_f, s_f, n_b, m_b, s_b) per pair (slots t, t + 1).
"""
import numpy as np

TPB, WAVE = 256, 64
MAX_GROUPS = 64                      # OCTO_DRAWS_MAX_GROUPS: the most temperatures
MAX_CHAINS = 1 << 24
N, A, NF, MF, SF, NB, MB, SB = range(8)      # the columns of acc
LAMBDA, FWD, REV, MEAN = range(4)            # the entries of the summary


def new_acc(T):
    """the state before its first call: every m = −Inf, the rest 0"""
    acc = np.zeros((T - 1, 8))
    acc[:, (MF, MB)] = -np.inf
    return acc


def block_sums(x):
    """Σ over the last axis [Cn] per block of 256 consecutive chains, [..., nblk], in the order of octo_draws_moments_device: a butterfly over
    the 64 lanes of each wave (a lane beyond Cn holds 0), the four waves added in wave order from 0."""
    x = np.asarray(x, dtype=np.float64)
    Cn = x.shape[-1]
    nblk = -(-Cn // TPB)
    pad = np.zeros(x.shape[:-1] + (nblk * TPB,))
    pad[..., :Cn] = x
    a = pad.reshape(x.shape[:-1] + (nblk, TPB // WAVE, WAVE))
    lanes = np.arange(WAVE)
    for o in (32, 16, 8, 4, 2, 1):
        a = a + a[..., lanes ^ o]
    total = np.zeros(x.shape[:-1] + (nblk,))
    for q in range(TPB // WAVE):
        total = total + a[..., q, 0]
    return total


def by_block(x, fill):
    """x [..., Cn] as [..., nblk, 256], the lanes beyond Cn holding `fill`"""
    Cn = x.shape[-1]
    nblk = -(-Cn // TPB)
    pad = np.full(x.shape[:-1] + (nblk * TPB,), fill, dtype=x.dtype)
    pad[..., :Cn] = x
    return pad.reshape(x.shape[:-1] + (nblk, TPB))


def pair_terms(ll, slot2rep, beta):
    """Per pair and chain, [T − 1][Cn] each: α, the forward term (−Inf: none) and whether the chain counts in n_f, the backward term and whether it
    counts in n_b."""
    ll, beta = np.asarray(ll, dtype=np.float64), np.asarray(beta, dtype=np.float64)
    s2r = np.asarray(slot2rep)
    T, Cn = ll.shape
    inside = (s2r >= 0) & (s2r < T)                                                          # a replica index outside 0 … T − 1 reads ℓ = NaN
    by_slot = np.where(inside.T, ll[np.where(inside, s2r, 0).T, np.arange(Cn)[None, :]], np.nan)      # [T][Cn]: ℓ of the replica at slot t of chain c
    li, lj = by_slot[:-1], by_slot[1:]
    db = (beta[:-1] - beta[1:])[:, None]
    fi, fj = np.isfinite(li), np.isfinite(lj)
    both = fi & fj
    with np.errstate(over="ignore", invalid="ignore"):
        alpha = np.where(both, np.minimum(1.0, np.exp(db * np.where(both, lj - li, 0.0))), np.where(fj & ~fi & (beta[:-1] > beta[1:])[:, None], 1.0, 0.0))
        n_f = fj | (lj == -np.inf)                # a dead prior draw counts and adds exp(−Inf) = 0: decided before the multiply, db = 0 gives no NaN
        v_f = np.where(fj, db * np.where(fj, lj, 0.0), -np.inf)
        v_b = np.where(fi, -(db * np.where(fi, li, 0.0)), -np.inf)
    return alpha, v_f, n_f, v_b, fi


def lse_merge(n, m, s, nb, mb, sb):
    """(n, m, s) held, merged with (nb, mb, sb): the counts add; m' = max(m, mb), s' = s·exp(m − m') + sb·exp(mb − m'); a side without a term
    (m = −Inf) leaves the other's (m, s) untouched"""
    if mb == -np.inf:
        return n + nb, m, s
    if m == -np.inf:
        return n + nb, mb, sb
    mm = max(m, mb)
    return n + nb, mm, s * np.exp(m - mm) + sb * np.exp(mb - mm)


def call_lse(v, counted):
    """(n, m, s) per pair of one call: per block the count, the maximum of the terms (exact) and Σ exp(v − max) in block_sums' order; the blocks
    merged in block order"""
    vm = by_block(v, -np.inf)                                         # [P][nblk][256]
    n_b = by_block(counted, False).sum(axis=-1)
    m_b = vm.max(axis=-1)
    with np.errstate(invalid="ignore"):
        e = np.where(vm > -np.inf, np.exp(vm - m_b[..., None]), 0.0)
    s_b = block_sums(e.reshape(e.shape[0], -1))
    out = []
    for p in range(v.shape[0]):
        n, m, s = 0, -np.inf, 0.0
        for b in range(n_b.shape[1]):
            n, m, s = lse_merge(n, m, s, int(n_b[p, b]), m_b[p, b], s_b[p, b])
        out.append((n, m, s))
    return out


def stats(ll, slot2rep, beta, acc):
    """octo_draws_pt_stats_device without the restarts: acc after the call (a new array)"""
    alpha, v_f, ok_f, v_b, ok_b = pair_terms(ll, slot2rep, beta)
    Cn = alpha.shape[1]
    out = np.array(acc, dtype=np.float64)
    A_b = block_sums(alpha)
    fwd, bwd = call_lse(v_f, ok_f), call_lse(v_b, ok_b)
    for p in range(alpha.shape[0]):
        a = 0.0
        for b in range(A_b.shape[1]):
            a = a + A_b[p, b]
        out[p, N] += Cn
        out[p, A] += a
        out[p, NF], out[p, MF], out[p, SF] = lse_merge(out[p, NF], out[p, MF], out[p, SF], *fwd[p])
        out[p, NB], out[p, MB], out[p, SB] = lse_merge(out[p, NB], out[p, MB], out[p, SB], *bwd[p])
    return out


def restarts(slot2rep, leg, count):
    """The tempered restarts of one scan, in place: the replica at slot T − 1 gets leg = 1; the replica at slot 0 with leg = 1 adds one to its
    chain's count and gets leg = 0. leg [Cn][T] by replica, count [Cn]."""
    s2r = np.asarray(slot2rep)
    c = np.arange(s2r.shape[0])
    leg[c, s2r[:, -1]] = 1
    back = leg[c, s2r[:, 0]] == 1
    count[back] += 1
    leg[c[back], s2r[back, 0]] = 0


def plain_stats(calls):
    """acc after the calls [(ℓ, slot2rep, β), …] from zero, stated without blocks: running sums over the calls, the chains and the pairs, one
    maximum over everything and Σ exp(v − that maximum)."""
    T = np.asarray(calls[0][0]).shape[0]
    acc = new_acc(T)
    terms = [[[], []] for _ in range(T - 1)]
    for ll, s2r, beta in calls:
        ll, beta = np.asarray(ll, dtype=np.float64), np.asarray(beta, dtype=np.float64)
        for c in range(ll.shape[1]):
            for t in range(T - 1):
                li, lj, db = ll[s2r[c][t], c], ll[s2r[c][t + 1], c], beta[t] - beta[t + 1]
                if np.isfinite(li) and np.isfinite(lj):
                    with np.errstate(over="ignore"):
                        alpha = min(1.0, np.exp(db * (lj - li)))
                else:
                    alpha = 1.0 if np.isfinite(lj) and not np.isfinite(li) and beta[t] > beta[t + 1] else 0.0
                acc[t, N] += 1
                acc[t, A] += alpha
                if lj == -np.inf:
                    acc[t, NF] += 1                       # a dead prior draw: exp(−Inf) = 0 to the sum, one to the count
                elif np.isfinite(lj):
                    acc[t, NF] += 1
                    terms[t][0].append(db * lj)
                if np.isfinite(li):
                    acc[t, NB] += 1
                    terms[t][1].append(-db * li)
    for t in range(T - 1):
        for (n, m, s), v in zip(((NF, MF, SF), (NB, MB, SB)), terms[t]):
            if v:
                v = np.array(v)
                acc[t, m] = v.max()
                acc[t, s] = np.exp(v - v.max()).sum()
    return acc


def barrier(acc):
    """(r [T − 1], Λ_t [T]): r_t = 1 − A/n clipped to [0, 1] (NaN with n = 0), Λ_0 = 0, Λ_{t+1} = Λ_t + r_t in t order"""
    acc = np.asarray(acc, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(acc[:, N] > 0, np.minimum(np.maximum(1.0 - acc[:, A] / acc[:, N], 0.0), 1.0), np.nan)
    lam = np.zeros(r.size + 1)
    for t in range(r.size):
        lam[t + 1] = lam[t] + r[t]
    return r, lam


def targets(lam):
    """g_k = k·Λ/(T − 1), k = 1 … T − 2"""
    T = lam.size
    return np.arange(1, T - 1) * lam[-1] / (T - 1)


def schedule(acc, beta, adapt=True, reset=True):
    """octo_draws_pt_schedule_device: dict(beta [T], rej [T − 1], summary [4] = (Λ, fwd, rev, ½(fwd + rev)), acc: the state after the call)"""
    acc, beta = np.asarray(acc, dtype=np.float64), np.asarray(beta, dtype=np.float64)
    T = beta.size
    r, lam = barrier(acc)
    new = beta.copy()
    if adapt and np.isfinite(lam[-1]) and lam[-1] > 0.0:
        for k, g in zip(range(1, T - 1), targets(lam)):
            t = 0
            while t < T - 2 and not lam[t + 1] >= g:      # the first t with Λ_{t+1} >= g
                t += 1
            new[k] = beta[t] + (beta[t + 1] - beta[t]) * (g - lam[t]) / (lam[t + 1] - lam[t])
    fwd = rev = 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        for t in range(T - 1):
            fwd = fwd + (acc[t, MF] + np.log(acc[t, SF] / acc[t, NF]))
            rev = rev + (acc[t, MB] + np.log(acc[t, SB] / acc[t, NB]))
    rev = -rev
    return dict(beta=new, rej=r, summary=np.array([lam[-1], fwd, rev, 0.5 * (fwd + rev)]), acc=new_acc(T) if reset else acc.copy())


def margins(acc):
    """The least distance of a target g_k from a node Λ_t, relative to Λ: which t "the first Λ_{t+1} >= g" names is decided by at least this.
    Inf when no slot is re-placed (T = 2; Λ is 0 or not finite)."""
    _, lam = barrier(acc)
    if lam.size < 3 or not (np.isfinite(lam[-1]) and lam[-1] > 0.0):
        return np.inf
    return float(np.min(np.abs(targets(lam)[:, None] - lam[None, :])) / lam[-1])


def swap(ll, beta, slot2rep, parity, u):
    """k_pt_swap's rule on the pairs of one parity with the uniforms u [Cn][T] in (0, 1]: (slot2rep after, accepted per slot [T])"""
    ll, beta = np.asarray(ll, dtype=np.float64), np.asarray(beta, dtype=np.float64)
    T, Cn = ll.shape
    out = np.array(slot2rep)
    c = np.arange(Cn)
    accepted = np.zeros(T, dtype=np.int64)
    for t in range(parity, T - 1, 2):
        ri, rj = out[:, t].copy(), out[:, t + 1].copy()
        li, lj = ll[ri, c], ll[rj, c]
        both = np.isfinite(li) & np.isfinite(lj)
        with np.errstate(invalid="ignore"):
            acc = np.where(both, np.log(u[:, t]) < (beta[t] - beta[t + 1]) * np.where(both, lj - li, 0.0), np.isfinite(lj) & ~np.isfinite(li) & (beta[t] > beta[t + 1]))
        out[acc, t], out[acc, t + 1] = rj[acc], ri[acc]
        accepted[t] = np.count_nonzero(acc)
    return out, accepted


def cubic_ladder(T):
    """TemperedSwap's default: linspace(1, 0, T)³"""
    return np.linspace(1.0, 0.0, T) ** 3


def pigeons(explore, T, Cn, n_rounds, rng, beta0=None, adapt=True, stats_fn=stats):
    """The round loop of octofit_pigeons_device. Round r = 1 … n_rounds makes 2^r scans; a scan is explore(β of every replica [T][Cn], scan
    number) -> ℓ [T][Cn] by replica (the exploration and the refresh of the β = 0 replicas), the statistics and the restarts on that ℓ and the
    slot2rep the swap is about to see, then the swap of parity scan % 2 (its uniforms are rng's, not the kernel's hash). Every round ends
    with one schedule(reset) that writes the new ladder; adaptation is off in the last round (adapt=False: in every round).
    Returns dict(betas_by_round [n_rounds + 1][T], rejection_by_round [n_rounds][T − 1], barrier_by_round, log_evidence (fwd, rev, mean of
    the last round), restarts [Cn], n_scans, slot2rep, accepted [T])."""
    beta = cubic_ladder(T) if beta0 is None else np.array(beta0, dtype=np.float64)
    s2r = np.tile(np.arange(T), (Cn, 1))
    leg, count = np.zeros((Cn, T), dtype=np.int64), np.zeros(Cn, dtype=np.int64)
    acc = new_acc(T)
    accepted = np.zeros(T, dtype=np.int64)
    betas, rej, lam, scan, s = [beta.copy()], [], [], 0, None
    c = np.arange(Cn)
    for r in range(1, n_rounds + 1):
        for _ in range(2 ** r):
            rep2slot = np.empty_like(s2r)
            rep2slot[c[:, None], s2r] = np.arange(T)[None, :]
            ll = explore(beta[rep2slot.T], scan)
            acc = stats_fn(ll, s2r, beta, acc)
            restarts(s2r, leg, count)
            s2r, a = swap(ll, beta, s2r, scan % 2, 1.0 - rng.random((Cn, T)))
            accepted += a
            scan += 1
        s = schedule(acc, beta, adapt=adapt and r < n_rounds, reset=True)
        beta, acc = s["beta"], s["acc"]
        betas.append(beta.copy())
        rej.append(s["rej"])
        lam.append(s["summary"][LAMBDA])
    return dict(betas_by_round=np.array(betas), rejection_by_round=np.array(rej), barrier_by_round=np.array(lam), log_evidence=tuple(s["summary"][1:]),
                restarts=count, n_scans=scan, slot2rep=s2r, accepted=accepted)
