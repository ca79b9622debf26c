"""
Batched callers of the hot path: the reference's drivers that already hold a walker batch on the
host, re-expressed on the LogDensityModel mirror so that every likelihood evaluation goes through ONE device call.

  guess_starting_position(rng, model, N)     src/initialization.jl:14-66    N prior draws -> link -> ℓπcallback -> argmax
  octofit_rejection(rng, model, draws)       src/sampling.jl:168-256        prior draws, accept with prob exp(ll − max ll)
  rejection_evaluate_likelihoods(model, θ)   src/sampling.jl:260-268        the inner batch: non-finite -> -Inf

  guess_starting_position_device / octofit_rejection_device: the same two drivers with the draws, the link, the argmax and the
  accept / compaction step on the device too (host/draws.py: PriorDraws) — only the winners / the accepted chain cross PCIe.

  octofit_ofti_device: the OFTI rejection sampler (examples/ofti_rejection_sampling.jl:78-108) — prior draws, the marginal likelihood, the rejection
  step, the Thiele-Innes draw of every survivor and its Campbell elements on the device (PriorDraws.ofti_set / ofti_rejection).

  octofit_pt_device: parallel tempering with a tempered HMC explorer, fresh prior draws at β = 0 and the swap step all on the device
  (PriorDraws.hmc_step, host/tempering.py: TemperedSwap) — the device-resident twin of julia/OctofitterHIP.jl: octofit_pigeons_hip.
  octofit_pigeons_device: that driver in Pigeons' rounds — the ladder re-placed from the communication barrier, the log evidence and the tempered
  restarts, from per-scan reductions on the device (PriorDraws.pt_stats / pt_schedule). With n_temps_variational it runs Pigeons' second leg beside the
  first: replicas annealed from a mean-field normal fitted to the target's own draws (PriorDraws.reference_fit / reference / reference_exchange).

  warmup_windows / hmc_warmup / octofit_hmc_device: the single-temperature sampler — Pathfinder starts, then HMC whose step size (dual
  averaging on the mean acceptance probability) and diagonal metric (the pooled variance of the chains, Stan's windowed schedule) are adapted
  from cross-chain reductions on the device (PriorDraws.moments / metric / adapt_init / adapt_step), with R̂ from per-chain running moments.

  optimize_starting_points_device: stage 2 of the reference's initialisation (src/initialization.jl:188-289) — a batched L-BFGS from the best
  prior draws, every chain on the device (PriorDraws.lbfgs); the host reads one status vector a segment.

  pathfinder_device: stage 3 — multi-path Pathfinder from the same starts (PriorDraws.pathfinder / pathfinder_draw): a normal fit at every
  L-BFGS iterate, the one with the best ELBO kept per path, draws from every path's fit, and PSIS importance resampling of their union
  (host/psis.py: Psis.loo on one row). Only the resampling is on the host.

  octofit_nested_device: nested sampling, the reference's fourth sampler (dynesty behind a hypercube prior transform) — the live set in the unit cube,
  the ordered cull with its evidence bookkeeping and the constrained-prior slice moves on the device (PriorDraws.cube / from_cube / nested_step);
  the host reads the 8-double state once per iteration, and computes the information and the resampling from the dead records.

  pointwise_like_rows / waic: the pointwise log-likelihood at the grain model comparison needs — one column per DATUM (table row), not per
  table — and its WAIC / importance-sampling LOO sums, computed (and for waic reduced over the samples) on the device
  (host/pointwise.py: Pointwise).

  simulate_tables / posterior_predictive: the back end of the workflow — the tables' model values (`simulate!`) and the orbit / RV curves
  of posterior draws over a time grid, computed or reduced to a band on the device (host/predict.py: Predictor).

The accept/reject and argmax logic is the reference's, line for line; random numbers come from NumPy's Generator
(the reference uses Julia's Xoshiro), so individual draws differ while the sampled distribution is the same.
"""
from __future__ import annotations

import numpy as np


def guess_starting_position(rng, model, N=500_000, batch=250_000, prior_samples=None):
    """Sample IID from the prior N times and return the highest-posterior sample: (bestparams, bestlogpost).
    prior_samples ([D, N], natural domain): use these draws instead of drawing (parity tests feed the same draws to the oracle)."""
    if prior_samples is not None:
        prior_samples = np.asarray(prior_samples, dtype=np.float64)
        N = prior_samples.shape[1]
    bestparams = model.sample_priors(rng) if prior_samples is None else prior_samples[:, 0].copy()
    bestlogpost = -np.inf
    done = 0
    while done < N:
        n = min(batch, N - done)
        params = model.sample_priors(rng, n) if prior_samples is None else prior_samples[:, done:done + n]
        logpost = model.ℓπcallback(model.link(params))
        k = int(np.argmax(logpost))
        if logpost[k] > bestlogpost:                      # initialization.jl:41-44
            bestlogpost, bestparams = float(logpost[k]), params[:, k].copy()
        done += n
    return bestparams, bestlogpost


def rejection_evaluate_likelihoods(model, prior_samples):
    """src/sampling.jl:260-268 for a [D, n] batch of natural-domain prior draws: ll per draw, non-finite -> -Inf."""
    elems, nuis = model.kernel_inputs(prior_samples)
    ll = model.ln_like.ln_like_arrays(elems, nuis)
    # epoch-free likelihood terms of the standard parameterisation (UnitLengthPrior, variables.jl:309-323)
    ll = ll + _unit_length_terms(model, prior_samples)
    return np.where(np.isfinite(ll), ll, -np.inf)


def _unit_length_terms(model, θ):
    tot = np.zeros(θ.shape[1])
    for (kind, i0, i1, flag, _v) in list(model._esrc) + list(model._nsrc):
        if kind in (2, 3) and (flag & 1):
            r = np.sqrt(θ[i0] ** 2 + θ[i1] ** 2)
            tot += -np.log(r) - np.log(0.1 * np.sqrt(2 * np.pi)) - np.log(r) ** 2 / (2 * 0.01)
    return tot


def octofit_rejection(rng, model, draws=100_000, verbosity=0, prior_samples=None, uniforms=None):
    """Rejection sampling with the prior as proposal. Returns dict(samples [D, n_accepted] (natural domain), loglike,
    logpost, draws, n_accepted, acceptance_rate, accept) — the chain the reference packs into MCMCChains.
    prior_samples / uniforms: use these draws (parity tests feed the same ones to the oracle)."""
    if prior_samples is None:
        prior_samples = model.sample_priors(rng, draws)                       # sampling.jl:178
    else:
        prior_samples = np.asarray(prior_samples, dtype=np.float64)
        draws = prior_samples.shape[1]
    log_likes = rejection_evaluate_likelihoods(model, prior_samples)          # :189-191
    max_ll = np.max(log_likes)                                                # :194
    if not np.isfinite(max_ll):
        raise RuntimeError(f"All {draws} prior samples produced non-finite log-likelihoods. Check your model and priors.")
    u = rng.uniform(0.0, 1.0, draws) if uniforms is None else np.asarray(uniforms, dtype=np.float64)
    with np.errstate(over="ignore"):
        accept = (log_likes != -np.inf) & (u < np.exp(log_likes - max_ll))    # :202-210
    idx = np.nonzero(accept)[0]
    if idx.size == 0:
        raise RuntimeError(f"No samples were accepted out of {draws} draws. The posterior may be extremely concentrated relative "
                           "to the prior. Consider increasing `draws` or using a different sampler.")
    samples = prior_samples[:, idx]
    logpost = model.ℓπcallback(model.link(samples))                           # _rejection_build_chain, :270-
    return dict(samples=samples, loglike=log_likes[idx], logpost=logpost, draws=draws, n_accepted=int(idx.size),
                acceptance_rate=idx.size / draws, names=list(model.names), accept=accept, all_loglike=log_likes)


def guess_starting_position_device(model, N=500_000, seed=0, keep=1):
    """guess_starting_position with the N prior draws made, linked, scored and ranked on the device (draws 0 … N − 1 of the counter-based
    stream `seed`): (bestparams, bestlogpost) like the host twin; with keep > 1 the `keep` best, best first: ([D, keep], [keep])."""
    from .draws import PriorDraws
    with PriorDraws(model) as draws:
        θ, lp, _ = draws.best(seed, N, keep=keep)
    if keep == 1:
        return θ[:, 0].copy(), float(lp[0])
    return θ, lp


def octofit_rejection_device(model, draws=100_000, seed=0):
    """octofit_rejection with the prior draws, their likelihoods, the uniforms and the accept / compaction step on the device (draws
    0 … draws − 1 of the counter-based stream `seed`). Returns the host twin's dict for the accepted chain: samples [D, n_accepted]
    (natural domain), loglike, logpost, draws, n_accepted, acceptance_rate, names, accept (the mask, rebuilt on the host from the accepted
    draw indices `index`) — and all_loglike = None: the per-draw likelihoods stay on the device."""
    from . import capi
    from .draws import PriorDraws
    with PriorDraws(model) as pd:
        try:
            r = pd.rejection(seed, draws)
        except capi.OctoError as e:
            if e.status == capi.OCTO_EINVAL and "non-finite log-likelihoods" in str(e):
                raise RuntimeError(str(e).split(": ", 1)[1]) from None
            raise
    if r["n_accepted"] == 0:
        raise RuntimeError(f"No samples were accepted out of {draws} draws. The posterior may be extremely concentrated relative "
                           "to the prior. Consider increasing `draws` or using a different sampler.")
    accept = np.zeros(int(draws), dtype=bool)
    accept[r["index"].astype(np.int64)] = True
    return dict(samples=r["samples"], loglike=r["loglike"], logpost=r["logpost"], draws=int(draws), n_accepted=r["n_accepted"],
                acceptance_rate=r["n_accepted"] / draws, names=list(model.names), accept=accept, all_loglike=None,
                index=r["index"], max_loglike=r["max_loglike"])


def octofit_ofti_device(epochs, ra, dec, σ_ra, σ_dec, cor, σ_ABFG, priors, draws=1_000_000, seed=0, t_ref=None, cap=None, device=0):
    """The reference's OFTI rejection sampler (examples/ofti_rejection_sampling.jl:78-108) in one call, on the device: `draws` prior draws of
    (e, a, tp | τ, M, plx), each scored by the marginal likelihood of ofti_linear_solve, accepted with probability exp(ℓ − max ℓ), and for every
    accepted draw the Thiele-Innes constants drawn from their conditional normal and turned into Campbell elements (PriorDraws.ofti_rejection).
    priors: a variables(e=…, a=…, tp=… or τ=…, M=…, plx=…) block of host/priors.py; τ (the orbit fraction at t_ref) needs t_ref [MJD].
    Returns a dict of NumPy columns over the accepted draws, in draw-index order: the five drawn parameters (e, a, tp or τ, M, plx), tp, the 16
    rows of draws.OFTI_OUTPUTS by name (A, B, F, G, their means, alpha [mas], a_ti [AU], i, ω, Ω, P_d, M_dyn, logml), index, and the scalars
    n_accepted, max_logml, draws, acceptance_rate. (a_ti, e, i, ω, Ω, tp, M_dyn, plx) are the elements posterior_predictive and Predictor take:
    `a` is the semi-major axis the period of the solve was made from, a_ti the one the drawn constants have — the linear model leaves the scale of
    the orbit free — and M_dyn is the total mass at which an orbit of semi-major axis a_ti has that period."""
    from . import capi
    from .draws import OFTI_OUTPUTS, PriorDraws
    names = list(priors)
    third = "τ" if "τ" in names else "tp"
    if names != ["e", "a", third, "M", "plx"]:
        raise ValueError("octofit_ofti_device: priors must be variables(e=…, a=…, tp=… or τ=…, M=…, plx=…), in that order")
    if third == "τ" and t_ref is None:
        raise ValueError("octofit_ofti_device: a τ prior needs t_ref")
    with PriorDraws(priors=[priors[n] for n in names], device=device) as pd:
        pd.ofti_set(epochs, ra, dec, σ_ra, σ_dec, cor, σ_ABFG, tp_mode=int(third == "τ"), t_ref=0.0 if t_ref is None else float(t_ref))
        try:
            r = pd.ofti_rejection(seed, draws, cap=cap)
        except capi.OctoError as e:
            if e.status == capi.OCTO_EINVAL and "non-finite log-likelihoods" in str(e):
                raise RuntimeError(str(e).split(": ", 1)[1]) from None
            raise
    if r["n_accepted"] == 0:
        raise RuntimeError(f"No samples were accepted out of {draws} draws. The posterior may be extremely concentrated relative "
                           "to the prior. Consider increasing `draws` or using a different sampler.")
    out = {n: r["theta"][k] for k, n in enumerate(names)}
    out["tp"] = r["nl"][2]
    out.update({n: r["post"][k] for k, n in enumerate(OFTI_OUTPUTS)})
    out.update(index=r["index"], n_accepted=r["n_accepted"], max_logml=r["max_logml"], draws=int(draws), acceptance_rate=r["n_accepted"] / int(draws))
    return out


def _default_metric(pd, seed, dev, inv_mass):
    """inv_mass — by default the per-coordinate variance of prior draws 0 … 4095 in θ_t — as a contiguous float64 [D] tensor on dev."""
    import torch
    if inv_mass is None:
        inv_mass = pd.sample(seed, 0, 4096, theta=False, logprior_t=False)[1].var(dim=1)
    return torch.as_tensor(inv_mass, dtype=torch.float64, device=dev).contiguous()


def _finite_or_neg_inf(x):
    """x with −Inf in place of every non-finite value."""
    import torch
    return torch.where(torch.isfinite(x), x, torch.full_like(x, -float("inf")))


def _recorded(model, rec_t, rec_lp, pd):
    """What a sampler returns of its recorded rounds rec_t [n, D, n_chains] (θ_t) and rec_lp [n, n_chains]: samples, samples_t, logpost; of a
    model with Derived variables also derived: {name: [n, n_chains]}, each variable's column from the handle's program (PriorDraws.program_values)."""
    samples_t = rec_t.cpu().numpy()
    out = dict(samples=np.stack([model.invlink(x) for x in samples_t]), samples_t=samples_t, logpost=rec_lp.cpu().numpy())
    if getattr(model, "derived_names", None):
        n, D, Cn = rec_t.shape
        cols = pd.derived_columns(rec_t.permute(1, 0, 2).reshape(D, n * Cn).contiguous())
        out["derived"] = {name: v.reshape(n, Cn).cpu().numpy() for name, v in cols.items()}
    return out


def octofit_pt_device(model, n_temps, n_chains, n_rounds, n_leapfrog=4, eps=None, betas=None, inv_mass=None, seed=0, n_adapt=None, adapt="host",
                      explorer="hmc", slice_w=10.0, slice_p=3, n_passes=3):
    """Parallel tempering with every piece on the device — the device-resident twin of julia/OctofitterHIP.jl: octofit_pigeons_hip, with a
    gradient-based explorer in place of its random walk: n_chains independent PT chains of n_temps replicas each (replica r of chain c is
    walker r·n_chains + c, the layout of TemperedSwap), θ_t never leaving the device during a round. Single rank.

    Initial states are prior draws 0 … n_temps·n_chains − 1 of the counter stream `seed`; inv_mass defaults to the per-coordinate variance of
    prior draws 0 … 4095 in θ_t. A round is, in order:
      1. β and ε of every replica from slot2rep (indexing only);
      2. one PriorDraws.hmc_step over all n_temps·n_chains replicas (chain index = walker index, step = round);
      3. the replicas at β = 0 replaced by fresh IID prior draws (Pigeons' sample_iid!, OctofitterPigeonsExt.jl:42-50) — the draw indices go on
         from where the initial states stopped, n_chains a round — with ℓ of the new states from one forward log-posterior call;
      4. TemperedSwap.swap_step on ℓ.
    During the first n_adapt rounds (default: half of them) ε of every temperature follows log ε_t += (acc_t − 0.8)/√(round + 1), acc_t that
    temperature's mean acceptance of the round. eps: the starting ε, a number or one per temperature (default 0.1).
    adapt="device" replaces that rule by dual averaging on the mean acceptance probability min(1, exp(dH)) of every temperature
    (PriorDraws.adapt_init / adapt_step, group = ladder slot, update number = round + 1, Stan's constants); after the n_adapt rounds every
    temperature runs at its averaged ε̄. The metric is the same in both.

    explorer="slice" explores with the reference's own explorer instead, Pigeons' SliceSampler (PriorDraws.slice_step: coordinate-wise, no
    gradient, nothing to tune): step 2 of a round becomes one slice-sampling transition of every replica — n_passes sweeps over the
    coordinates with width slice_w (a number, or one per coordinate of θ_t) and slice_p doublings. n_leapfrog, eps, inv_mass, n_adapt and
    adapt are ignored in that mode, and the result carries slice_evals [n_temps] — the mean log-posterior evaluations per replica per round
    of every temperature — in place of hmc_acceptance and eps.

    Returns dict(samples [n_rounds, D, n_chains] natural domain, samples_t the same as θ_t, logpost [n_rounds, n_chains] — the β = 1 replica of
    every chain after the exploration of each round —, hmc_acceptance [n_temps], swap_acceptance [n_temps − 1], eps [n_temps], betas, names,
    and state = dict(theta_t [D, n_temps·n_chains], slot2rep, refreshed (walker indices the last round redrew), refreshed_first (their first
    draw index)) for a driver that goes on, all NumPy)."""
    import torch
    from .draws import PriorDraws
    from .tempering import TemperedSwap
    T, Cn, R = int(n_temps), int(n_chains), int(n_rounds)
    if T < 2 or Cn < 1 or R < 1:
        raise ValueError("octofit_pt_device: n_temps >= 2, n_chains >= 1, n_rounds >= 1")
    n_adapt = R // 2 if n_adapt is None else int(n_adapt)
    if adapt not in ("host", "device"):
        raise ValueError('octofit_pt_device: adapt is "host" or "device"')
    if explorer not in ("hmc", "slice"):
        raise ValueError('octofit_pt_device: explorer is "hmc" or "slice"')
    use_slice = explorer == "slice"
    if use_slice:
        n_adapt = 0      # nothing to adapt
    fn = model.ln_like
    dev = torch.device("cuda", fn.device_index)
    W, D = T * Cn, int(model.D)
    with PriorDraws(model) as pd:
        swap = TemperedSwap(fn, T, Cn, device=dev, seed=seed, betas=betas)
        cold_last = float(swap.beta[-1]) == 0.0      # the ladder ends at the prior: its replicas are redrawn IID every round
        if not use_slice:
            inv_mass = _default_metric(pd, seed, dev, inv_mass)
        log_eps = torch.log(torch.as_tensor(0.1 if eps is None or use_slice else eps, dtype=torch.float64, device=dev).expand(T).clone())
        theta_t = pd.sample(seed, 0, W, theta=False, logprior_t=False)[1]
        da_state = None
        if adapt == "device" and not use_slice:
            da_state = pd.adapt_init(T, torch.as_tensor(0.1 if eps is None else eps, dtype=torch.float64, device=dev).expand(T).contiguous())
            log_eps = da_state[:, 0].clone()
        next_draw = W
        slots = torch.arange(T, dtype=torch.int32, device=dev).repeat(Cn, 1)
        chains = torch.arange(Cn, device=dev)
        acc_sum = torch.zeros(T, dtype=torch.float64, device=dev)      # with the slice sampler: the evaluations
        rec_t = torch.empty((R, D, Cn), dtype=torch.float64, device=dev)
        rec_lp = torch.empty((R, Cn), dtype=torch.float64, device=dev)
        refreshed = None
        for r in range(R):
            rep2slot = torch.empty_like(swap.slot2rep)
            rep2slot.scatter_(1, swap.slot2rep.long(), slots)
            slot_w = rep2slot.t().contiguous().reshape(-1).long()                     # the ladder slot of walker r·n_chains + c
            if use_slice:
                so = pd.slice_step(theta_t, beta=swap.beta[slot_w], w=slice_w, p=slice_p, n_passes=n_passes, seed=seed, step=r)
                lp, ll, acc = so["logpost"], so["loglike"], so["n_eval"]
            else:
                lp, ll, _dH, acc = pd.hmc_step(theta_t, beta=swap.beta[slot_w], eps=torch.exp(log_eps)[slot_w], n_leapfrog=n_leapfrog,
                                               inv_mass=inv_mass, seed=seed, step=r)
            if cold_last:
                refreshed = swap.slot2rep[:, T - 1].long() * Cn + chains
                _, fresh, lpt = pd.sample(seed, next_draw, Cn, theta=False)
                lp_f, _ = model.logpost_device(fresh, grad=False)
                ll_f = lp_f - lpt
                theta_t[:, refreshed] = fresh
                lp[refreshed] = lp_f
                ll[refreshed] = _finite_or_neg_inf(ll_f)
                next_draw += Cn
            acc_t = torch.zeros(T, dtype=torch.float64, device=dev).index_add_(0, slot_w, acc.double()) / Cn
            acc_sum += acc_t
            if r < n_adapt and da_state is not None:
                pd.adapt_step(da_state, _dH, acc, r + 1, group=slot_w.int(), want_eps=False)
                log_eps = da_state[:, 1 if r == n_adapt - 1 else 0].clone()      # the next round's slots differ: ε is gathered by slot there
            elif r < n_adapt:
                log_eps += (acc_t - 0.8) / (r + 1) ** 0.5
            target = swap.slot2rep[:, 0].long() * Cn + chains
            rec_t[r] = theta_t[:, target]
            rec_lp[r] = lp[target]
            swap.swap_step(ll, r)
        torch.cuda.synchronize(dev)
        pairs = np.arange(T - 1)
        attempts = np.array([(R + 1 - (t % 2)) // 2 for t in pairs]) * Cn            # pair (t, t + 1) is tried in the rounds of parity t % 2
        explored = dict(slice_evals=(acc_sum / R).cpu().numpy()) if use_slice else dict(hmc_acceptance=(acc_sum / R).cpu().numpy())
        return dict(**_recorded(model, rec_t, rec_lp, pd), **explored, swap_acceptance=swap.accepted.cpu().numpy()[:T - 1] / np.maximum(attempts, 1),
                    **({} if use_slice else dict(eps=torch.exp(log_eps).cpu().numpy())), betas=swap.beta.cpu().numpy(), names=list(model.names),
                    state=dict(theta_t=theta_t.cpu().numpy(), slot2rep=swap.slot2rep.cpu().numpy(),
                               refreshed=None if refreshed is None else refreshed.cpu().numpy(), refreshed_first=next_draw - Cn if cold_last else None))


def octofit_pigeons_device(model, n_temps, n_chains, n_rounds, explorer="slice", n_leapfrog=4, eps=None, betas=None, inv_mass=None, seed=0, slice_w=10.0,
                           slice_p=3, n_passes=3, n_temps_variational=0, first_tuning_round=5, inflate=1.0):
    """octofit_pt_device with what Pigeons does BETWEEN its scans (non-reversible parallel tempering, Syed et al. 2021) — the device-resident twin of
    the reference's octofit_pigeons in its round structure too. Round r = 1 … n_rounds makes 2^r scans, 2^(n_rounds + 1) − 2 in all. A scan is
    exactly a round of octofit_pt_device (β per replica from slot2rep; explore; the β = 0 replicas redrawn IID; record the target replica; swap), its
    step number the scan's number over the whole run, with PriorDraws.pt_stats on ℓ and slot2rep ahead of the swap: the swap acceptance
    probabilities of every pair, the stepping-stone sums and the tempered restarts, accumulated on the device. Every round ends with one
    PriorDraws.pt_schedule, which writes the ladder that equalises the rejection rates into TemperedSwap.beta in place and starts the next
    round's sums; adaptation is off in the last round, whose ladder is the one its draws and its log evidence belong to. Only the last
    round's 2^n_rounds draws are kept (Pigeons' rule).

    explorer="slice" (the default here: Pigeons' own) or "hmc" (octofit_pt_device's default). With "hmc", ε of every ladder slot follows the
    device dual averaging of octofit_pt_device(adapt="device") through every round but the last, which runs at the averaged ε̄. Inside a round the
    host waits for nothing with "hmc"; "slice" keeps slice_step's 4-byte read per segment. pt_schedule waits once, at the end of a round.
    betas: the starting ladder (default TemperedSwap's cubic one); its two ends stay.

    Returns what octofit_pt_device returns — samples, samples_t [2^n_rounds, D, n_chains], logpost of the last round; hmc_acceptance and eps or
    slice_evals, and swap_acceptance, over all scans; betas (the final ladder), names, state — plus log_evidence = dict(fwd, rev, mean: the
    stepping-stone estimates of log Z of the last round; n, n_fwd, n_rev [n_temps − 1]: the pairs' scans × chains and the terms behind the two); betas_by_round [n_rounds + 1, n_temps] (row 0 the start, row r the ladder after round
    r); rejection_by_round [n_rounds, n_temps − 1]; barrier_by_round [n_rounds] (Λ); restarts = dict(total, per_chain [n_chains]): the tempered
    restarts over the run; n_scans. All NumPy.

    n_temps_variational = Tv >= 2 runs Pigeons' second leg beside the first (its default run is two-legged): Tv·n_chains more replicas that anneal
    not from the prior but from a mean-field normal q on θ_t, fitted by moment matching to the target's own draws round after round
    (PriorDraws.reference_fit on the grouped moments of the target replicas of BOTH legs; σ times `inflate`), the two legs joined at the
    target. Recalled, not checked against Pigeons' source: the first tuning round, moment matching on the target's draws of the previous
    round, and the two legs joined at the target. The second leg has its own TemperedSwap, pt_state, ladder (TemperedSwap's cubic one; `betas`
    is the first leg's) and, with "hmc", dual-averaging state; the metric is shared. Its swap potential is ℓπ − log q. A scan is, in order:
    explore both legs — the second under PriorDraws.reference(its table) once it has one, under the prior until then —; refresh each leg's
    β = 0 replicas from its own reference; accumulate the target replicas of both legs into the round's moments; PriorDraws.reference_exchange
    (the two target replicas of a chain trade places: always accepted, both are at β = 1); record the targets; pt_stats and the swap step per
    leg. At the end of round r >= first_tuning_round − 1 (not of the last: its reference is the one its log evidence belongs to) the normal is
    re-fitted from that round's moments into a staging table; every round ends by resetting the moments. The count of bad coordinates is read
    right after the round's pt_schedule calls, which have waited for the stream anyway — no new synchronisation inside a round —, and with
    bad > 0 the leg keeps the reference it had.
    Counter ranges, so that no (seed, purpose, step, chain) tuple serves both legs: the first leg explores as chains 0 … n_temps·n_chains − 1,
    takes prior draws 0, 1, … (below 2^50) and swaps at steps 0 … n_scans − 1; the second explores as chains n_temps·n_chains …
    (n_temps + Tv)·n_chains − 1, takes draws 2^62, 2^62 + 1, … and swaps at steps 2^40 + scan (the same parity).
    The result then gains variational = dict(log_evidence, betas_by_round, rejection_by_round, barrier_by_round, restarts as above, of the second
    leg; samples, samples_t, logpost of ITS target replicas over the last round; mean_by_round, sd_by_round [n_rounds, D]: the reference the leg
    holds after each round, NaN while it has none; bad_by_round [n_rounds]: the bad coordinates of each round's fit, 0 where none was made)."""
    import torch
    from .draws import PriorDraws
    from .tempering import TemperedSwap
    T, Cn, R = int(n_temps), int(n_chains), int(n_rounds)
    if T < 2 or Cn < 1 or R < 1 or R > 24:
        raise ValueError("octofit_pigeons_device: n_temps >= 2, n_chains >= 1, 1 <= n_rounds <= 24")
    if explorer not in ("hmc", "slice"):
        raise ValueError('octofit_pigeons_device: explorer is "hmc" or "slice"')
    if int(n_temps_variational) != 0:
        return _pigeons_two_legs(model, T, int(n_temps_variational), Cn, R, explorer == "slice", n_leapfrog, eps, betas, inv_mass, seed, slice_w, slice_p,
                                 n_passes, int(first_tuning_round), float(inflate))
    use_slice = explorer == "slice"
    fn = model.ln_like
    dev = torch.device("cuda", fn.device_index)
    W, D = T * Cn, int(model.D)
    n_scans, n_keep = 2 ** (R + 1) - 2, 2 ** R
    n_adapt = 0 if use_slice else n_scans - n_keep
    with PriorDraws(model) as pd:
        swap = TemperedSwap(fn, T, Cn, device=dev, seed=seed, betas=betas)
        cold_last = float(swap.beta[-1]) == 0.0      # the ladder ends at the prior: its replicas are redrawn IID every scan
        theta_t = pd.sample(seed, 0, W, theta=False, logprior_t=False)[1]
        da_state = log_eps = None
        if not use_slice:
            inv_mass = _default_metric(pd, seed, dev, inv_mass)
            da_state = pd.adapt_init(T, torch.as_tensor(0.1 if eps is None else eps, dtype=torch.float64, device=dev).expand(T).contiguous())
            log_eps = da_state[:, 0].clone()
        next_draw = W
        slots = torch.arange(T, dtype=torch.int32, device=dev).repeat(Cn, 1)
        chains = torch.arange(Cn, device=dev)
        acc_sum = torch.zeros(T, dtype=torch.float64, device=dev)      # with the slice sampler: the evaluations
        rec_t = torch.empty((n_keep, D, Cn), dtype=torch.float64, device=dev)
        rec_lp = torch.empty((n_keep, Cn), dtype=torch.float64, device=dev)
        pt = pd.pt_state(T, Cn)
        betas_by_round = torch.empty((R + 1, T), dtype=torch.float64, device=dev)
        betas_by_round[0] = swap.beta
        rejection_by_round = torch.empty((R, T - 1), dtype=torch.float64, device=dev)
        summary_by_round = torch.empty((R, 4), dtype=torch.float64, device=dev)
        refreshed, scan = None, 0
        for r in range(1, R + 1):
            for _ in range(2 ** r):
                rep2slot = torch.empty_like(swap.slot2rep)
                rep2slot.scatter_(1, swap.slot2rep.long(), slots)
                slot_w = rep2slot.t().contiguous().reshape(-1).long()                 # the ladder slot of walker r·n_chains + c
                if use_slice:
                    so = pd.slice_step(theta_t, beta=swap.beta[slot_w], w=slice_w, p=slice_p, n_passes=n_passes, seed=seed, step=scan)
                    lp, ll, acc = so["logpost"], so["loglike"], so["n_eval"]
                else:
                    lp, ll, dH, acc = pd.hmc_step(theta_t, beta=swap.beta[slot_w], eps=torch.exp(log_eps)[slot_w], n_leapfrog=n_leapfrog,
                                                  inv_mass=inv_mass, seed=seed, step=scan)
                if cold_last:
                    refreshed = swap.slot2rep[:, T - 1].long() * Cn + chains
                    _, fresh, lpt = pd.sample(seed, next_draw, Cn, theta=False)
                    lp_f, _ = model.logpost_device(fresh, grad=False)
                    theta_t[:, refreshed] = fresh
                    lp[refreshed] = lp_f
                    ll[refreshed] = _finite_or_neg_inf(lp_f - lpt)
                    next_draw += Cn
                acc_sum += torch.zeros(T, dtype=torch.float64, device=dev).index_add_(0, slot_w, acc.double()) / Cn
                if scan < n_adapt:
                    pd.adapt_step(da_state, dH, acc, scan + 1, group=slot_w.int(), want_eps=False)
                    log_eps = da_state[:, 1 if scan == n_adapt - 1 else 0].clone()      # the next scan's slots differ: ε is gathered by slot there
                if r == R:
                    target = swap.slot2rep[:, 0].long() * Cn + chains
                    rec_t[scan - (n_scans - n_keep)] = theta_t[:, target]
                    rec_lp[scan - (n_scans - n_keep)] = lp[target]
                pd.pt_stats(ll, swap.slot2rep, swap.beta, pt)
                swap.swap_step(ll, scan)
                scan += 1
            if r == R:
                counts = pt["acc"][:, [0, 2, 5]].clone()
            s = pd.pt_schedule(pt, swap.beta, adapt=r < R, reset=True, beta_out=swap.beta)
            betas_by_round[r] = swap.beta
            rejection_by_round[r - 1] = s["rejection"]
            summary_by_round[r - 1] = s["summary"]
        torch.cuda.synchronize(dev)
        pairs = np.arange(T - 1)
        attempts = np.array([(n_scans + 1 - (t % 2)) // 2 for t in pairs]) * Cn      # pair (t, t + 1) is tried in the scans of parity t % 2
        explored = dict(slice_evals=(acc_sum / n_scans).cpu().numpy()) if use_slice else dict(hmc_acceptance=(acc_sum / n_scans).cpu().numpy(),
                                                                                             eps=torch.exp(log_eps).cpu().numpy())
        summary = summary_by_round.cpu().numpy()
        per_chain = pt["restarts"].cpu().numpy()
        counts = counts.cpu().numpy().astype(np.int64)
        return dict(**_recorded(model, rec_t, rec_lp, pd), **explored, swap_acceptance=swap.accepted.cpu().numpy()[:T - 1] / np.maximum(attempts, 1),
                    betas=swap.beta.cpu().numpy(), names=list(model.names),
                    state=dict(theta_t=theta_t.cpu().numpy(), slot2rep=swap.slot2rep.cpu().numpy(),
                               refreshed=None if refreshed is None else refreshed.cpu().numpy(), refreshed_first=next_draw - Cn if cold_last else None),
                    log_evidence=dict(fwd=float(summary[-1, 1]), rev=float(summary[-1, 2]), mean=float(summary[-1, 3]), n=counts[:, 0], n_fwd=counts[:, 1],
                                      n_rev=counts[:, 2]),
                    betas_by_round=betas_by_round.cpu().numpy(), rejection_by_round=rejection_by_round.cpu().numpy(), barrier_by_round=summary[:, 0].copy(),
                    restarts=dict(total=int(per_chain.sum()), per_chain=per_chain), n_scans=n_scans)


VARIATIONAL_FIRST_DRAW = 1 << 62      # the second leg's prior / reference draws start here; the first leg's stay below 2^50
VARIATIONAL_SWAP_STEP = 1 << 40       # … and its swap steps (even: the parity of a scan is kept)


def _pigeons_two_legs(model, T, Tv, Cn, R, use_slice, n_leapfrog, eps, betas, inv_mass, seed, slice_w, slice_p, n_passes, first_tuning_round, inflate):
    """octofit_pigeons_device with a variational leg of Tv temperatures (its docstring states the scan, the fit and the counter ranges)."""
    import math
    from types import SimpleNamespace
    import torch
    from .draws import PriorDraws
    from .tempering import TemperedSwap
    if Tv < 2 or first_tuning_round < 1 or not (math.isfinite(inflate) and inflate > 0.0):
        raise ValueError("octofit_pigeons_device: n_temps_variational is 0 or >= 2, first_tuning_round >= 1, inflate finite and > 0")
    fn = model.ln_like
    dev = torch.device("cuda", fn.device_index)
    D = int(model.D)
    n_scans, n_keep = 2 ** (R + 1) - 2, 2 ** R
    n_adapt = 0 if use_slice else n_scans - n_keep
    f64 = dict(dtype=torch.float64, device=dev)
    with PriorDraws(model) as pd:
        if not use_slice:
            inv_mass = _default_metric(pd, seed, dev, inv_mass)
        chains = torch.arange(Cn, device=dev)

        def new_leg(Tl, chain0, draw0, step0, ladder):
            swap = TemperedSwap(fn, Tl, Cn, device=dev, seed=seed, betas=ladder)
            g = SimpleNamespace(T=Tl, chain0=chain0, next_draw=draw0 + Tl * Cn, step0=step0, swap=swap, cold_last=float(swap.beta[-1]) == 0.0,
                                theta_t=pd.sample(seed, draw0, Tl * Cn, theta=False, logprior_t=False)[1], pt=pd.pt_state(Tl, Cn),
                                slots=torch.arange(Tl, dtype=torch.int32, device=dev).repeat(Cn, 1), acc_sum=torch.zeros(Tl, **f64), da=None, log_eps=None,
                                rec_t=torch.empty((n_keep, D, Cn), **f64), rec_lp=torch.empty((n_keep, Cn), **f64), betas_by_round=torch.empty((R + 1, Tl), **f64),
                                rejection_by_round=torch.empty((R, Tl - 1), **f64), summary_by_round=torch.empty((R, 4), **f64), refreshed=None, counts=None)
            g.betas_by_round[0] = swap.beta
            if not use_slice:
                g.da = pd.adapt_init(Tl, torch.as_tensor(0.1 if eps is None else eps, **f64).expand(Tl).contiguous())
                g.log_eps = g.da[:, 0].clone()
            return g

        def explore(g, scan, ref):
            """steps 1 and 2 of a scan for one leg: ℓπ and the swap potential of every replica under the leg's reference"""
            rep2slot = torch.empty_like(g.swap.slot2rep)
            rep2slot.scatter_(1, g.swap.slot2rep.long(), g.slots)
            g.slot_w = rep2slot.t().contiguous().reshape(-1).long()                   # the ladder slot of walker r·n_chains + c
            with pd.reference(ref):
                if use_slice:
                    so = pd.slice_step(g.theta_t, beta=g.swap.beta[g.slot_w], w=slice_w, p=slice_p, n_passes=n_passes, seed=seed, step=scan, chain0=g.chain0)
                    g.lp, g.ll, acc = so["logpost"], so["loglike"], so["n_eval"]
                else:
                    g.lp, g.ll, dH, acc = pd.hmc_step(g.theta_t, beta=g.swap.beta[g.slot_w], eps=torch.exp(g.log_eps)[g.slot_w], n_leapfrog=n_leapfrog,
                                                      inv_mass=inv_mass, seed=seed, step=scan, chain0=g.chain0)
                if g.cold_last:
                    g.refreshed = g.swap.slot2rep[:, g.T - 1].long() * Cn + chains
                    _, fresh, lpt = pd.sample(seed, g.next_draw, Cn, theta=False)
            if g.cold_last:
                lp_f, _ = model.logpost_device(fresh, grad=False)
                g.theta_t[:, g.refreshed] = fresh
                g.lp[g.refreshed] = lp_f
                g.ll[g.refreshed] = _finite_or_neg_inf(lp_f - lpt)
                g.next_draw += Cn
            g.acc_sum += torch.zeros(g.T, **f64).index_add_(0, g.slot_w, acc.double()) / Cn
            if scan < n_adapt:
                pd.adapt_step(g.da, dH, acc, scan + 1, group=g.slot_w.int(), want_eps=False)
                g.log_eps = g.da[:, 1 if scan == n_adapt - 1 else 0].clone()          # the next scan's slots differ: ε is gathered by slot there

        A = new_leg(T, 0, 0, 0, betas)
        B = new_leg(Tv, T * Cn, VARIATIONAL_FIRST_DRAW, VARIATIONAL_SWAP_STEP, None)
        ref, staging, active = pd.reference_table(), pd.reference_table(), None       # active: the table the second leg anneals from, None = the prior
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
        mom = (torch.zeros(1, **f64), torch.zeros((1, D), **f64), torch.zeros((1, D), **f64))
        mean_by_round = torch.full((R, D), float("nan"), **f64)
        sd_by_round = torch.full((R, D), float("nan"), **f64)
        bad_by_round = np.zeros(R, dtype=np.int64)
        scan = 0
        for r in range(1, R + 1):
            for _ in range(2 ** r):
                explore(A, scan, None)
                explore(B, scan, active)
                for g in (A, B):
                    pd.moments(g.theta_t, group=torch.where(g.slot_w == 0, 0, -1).int(), G=1, out=mom, accumulate=True)
                pd.reference_exchange(A.swap.slot2rep, A.theta_t, A.lp, A.ll, None, B.swap.slot2rep, B.theta_t, B.lp, B.ll, active)
                for g in (A, B):
                    if r == R:
                        target = g.swap.slot2rep[:, 0].long() * Cn + chains
                        g.rec_t[scan - (n_scans - n_keep)] = g.theta_t[:, target]
                        g.rec_lp[scan - (n_scans - n_keep)] = g.lp[target]
                    pd.pt_stats(g.ll, g.swap.slot2rep, g.swap.beta, g.pt)
                    g.swap.swap_step(g.ll, g.step0 + scan)
                scan += 1
            fit = first_tuning_round - 1 <= r < R
            if fit:
                pd.reference_fit(staging, mom[0], mom[1][0], mom[2][0], inflate=inflate, bad=bad)
            for t in mom:
                t.zero_()
            for g in (A, B):
                if r == R:
                    g.counts = g.pt["acc"][:, [0, 2, 5]].clone()
                s = pd.pt_schedule(g.pt, g.swap.beta, adapt=r < R, reset=True, beta_out=g.swap.beta)
                g.betas_by_round[r] = g.swap.beta
                g.rejection_by_round[r - 1] = s["rejection"]
                g.summary_by_round[r - 1] = s["summary"]
            if fit:
                bad_by_round[r - 1] = int(bad.item())      # pt_schedule has waited for the stream: the fit is done
                if bad_by_round[r - 1] == 0:
                    ref.copy_(staging)
                    active = ref
            if active is not None:
                mean_by_round[r - 1], sd_by_round[r - 1] = pd.reference_moments(ref)
        torch.cuda.synchronize(dev)

        def result(g):
            pairs = np.arange(g.T - 1)
            attempts = np.array([(n_scans + 1 - (t % 2)) // 2 for t in pairs]) * Cn  # pair (t, t + 1) is tried in the scans of parity t % 2
            explored = dict(slice_evals=(g.acc_sum / n_scans).cpu().numpy()) if use_slice else dict(hmc_acceptance=(g.acc_sum / n_scans).cpu().numpy(),
                                                                                                 eps=torch.exp(g.log_eps).cpu().numpy())
            summary = g.summary_by_round.cpu().numpy()
            per_chain = g.pt["restarts"].cpu().numpy()
            counts = g.counts.cpu().numpy().astype(np.int64)
            return dict(**_recorded(model, g.rec_t, g.rec_lp, pd), **explored, swap_acceptance=g.swap.accepted.cpu().numpy()[:g.T - 1] / np.maximum(attempts, 1),
                        betas=g.swap.beta.cpu().numpy(),
                        log_evidence=dict(fwd=float(summary[-1, 1]), rev=float(summary[-1, 2]), mean=float(summary[-1, 3]), n=counts[:, 0], n_fwd=counts[:, 1],
                                          n_rev=counts[:, 2]),
                        betas_by_round=g.betas_by_round.cpu().numpy(), rejection_by_round=g.rejection_by_round.cpu().numpy(),
                        barrier_by_round=summary[:, 0].copy(), restarts=dict(total=int(per_chain.sum()), per_chain=per_chain))

        out = result(A)
        out.update(names=list(model.names), n_scans=n_scans,
                   state=dict(theta_t=A.theta_t.cpu().numpy(), slot2rep=A.swap.slot2rep.cpu().numpy(),
                              refreshed=None if A.refreshed is None else A.refreshed.cpu().numpy(), refreshed_first=A.next_draw - Cn if A.cold_last else None),
                   variational=dict(**result(B), mean_by_round=mean_by_round.cpu().numpy(), sd_by_round=sd_by_round.cpu().numpy(), bad_by_round=bad_by_round))
        return out


def warmup_windows(n_warmup):
    """Stan's windowed warm-up schedule, scaled to n_warmup rounds: (initial buffer, [slow window lengths], terminal buffer), which tile
    rounds 0 … n_warmup − 1 in that order.
      n_warmup < 20: (n_warmup, [], 0) — the step size alone adapts.
      Otherwise the buffers are 75 and 50 rounds and the first window 25; if those 150 do not fit they are 15 % and 10 % of n_warmup (rounded
      down) and the first window takes the rest. Each window is twice as long as the one before; a window after which the next one would not
      fit in front of the terminal buffer is stretched to reach it. n_warmup = 1000: (75, [25, 50, 100, 200, 500], 50)."""
    n = int(n_warmup)
    if n < 0:
        raise ValueError("warmup_windows: n_warmup >= 0")
    if n < 20:
        return n, [], 0
    init, term, size = 75, 50, 25
    if init + size + term > n:
        init, term = 15 * n // 100, 10 * n // 100
        size = n - init - term
    windows, start, end = [], init, n - term
    while start < end:
        stop = start + size
        if stop + 2 * size > end:
            stop = end
        windows.append(stop - start)
        start, size = stop, 2 * size
    return init, windows, term


def _tree_means(depth, n_leapfrog, diverged):
    """[3] on the device: the mean depth, the mean n_leapfrog and the number of divergences of one NUTS round"""
    import torch
    return torch.stack([depth.double().mean(), n_leapfrog.double().mean(), diverged.double().sum()])


def hmc_warmup(pd, theta_t, n_warmup, n_leapfrog=8, eps=0.1, inv_mass=None, target_accept=0.8, seed=0, step=0, chain0=0, gamma=0.05, t0=10.0, kappa=0.75,
               record=None, max_depth=None, metric="diag"):
    """Warm-up of PriorDraws.hmc_step on the W chains of theta_t ([D, W] on the device, updated in place) at β = 1 — on a handle without a
    model: on the prior. n_warmup rounds on the schedule of warmup_windows; round r is one hmc_step with step number step + r and then
      * the dual-averaging update of ε from the round's mean acceptance probability (PriorDraws.adapt_step, one group, δ = target_accept);
      * inside a slow window: the chains' states merged into the pooled moments (PriorDraws.moments, accumulate from the window's second round on);
      * at a window's last round: inv_mass <- metric(regularize=True) of those moments, the moments restart with the next window, and the
        dual averaging restarts from ε̄ (x = x̄ = log ε̄, H̄ = 0, μ = log 10ε̄, update number 1 next).
    After the last round ε = ε̄. Nothing is read back: every statistic stays on the device.
    record: a list that receives one dict a round with copies of what each call of the round read and wrote (dH, accepted, theta_t, the
    dual-averaging state before and after, the moments before and after, inv_mass after), for a caller who follows the adaptation.
    max_depth: None, or the tree depth of PriorDraws.nuts_step, which then is the round's step (n_leapfrog is not used): its log_accept goes where
    dH went — min(1, exp(·)) of it is the transition's mean acceptance statistic — and the result gains tree [n_warmup, 3], per round the mean
    depth, the mean n_leapfrog and the number of divergences.
    metric: "diag", or "dense": the rounds run under the dense metric L·Lᵀ (PriorDraws.use_metric, D <= DENSE_MAX_D), L starting at diag(√inv_mass);
    inside a slow window the states enter the pooled co-moments (PriorDraws.cov) where the moments are, and at a window's last round
    L <- metric_dense(regularize=True) of them, written only where the factorisation holds: otherwise the previous factor stays, decided on the
    device. The dual averaging, the schedule and the restart of ε are the same. The result gains metric_chol [D, D] (lower), and inv_mass is
    diag(L·Lᵀ); record gains cov's triples under mom_in / mom, and chol (packed) and info after a window's factorisation. On return the handle
    is back on the metric it had.
    inv_mass: [D] (a copy is adapted) or None = 1. Returns dict(theta_t, eps (a [1] tensor), inv_mass [D], accept_stat [n_warmup], step (the
    next step number)), device tensors."""
    import torch
    from .draws import pack_lower, unpack_lower
    if metric not in ("diag", "dense"):
        raise ValueError('hmc_warmup: metric must be "diag" or "dense"')
    dense = metric == "dense"
    dev = theta_t.device
    D, W = int(theta_t.shape[0]), int(theta_t.shape[1])
    n = int(n_warmup)
    init, windows, _term = warmup_windows(n)
    first, last = set(), set()
    at = init
    for length in windows:
        first.add(at)
        at += length
        last.add(at - 1)
    inv_mass = torch.ones(D, dtype=torch.float64, device=dev) if inv_mass is None else torch.as_tensor(inv_mass, dtype=torch.float64, device=dev).clone().contiguous()
    state = pd.adapt_init(1, eps)
    eps_w = torch.exp(state[:, 0]).expand(W).contiguous()
    accept_stat = torch.empty(n, dtype=torch.float64, device=dev)
    tree = None if max_depth is None else torch.empty((n, 3), dtype=torch.float64, device=dev)
    mom, in_window, k = None, False, 0
    chol, before = None, getattr(pd, "_active_metric", None)
    if dense:
        chol = pack_lower(torch.diag(torch.sqrt(inv_mass)))
        pd.use_metric(chol)
    step_mass = None if dense else inv_mass
    for r in range(n):
        if max_depth is None:
            _lp, _ll, dH, acc = pd.hmc_step(theta_t, eps=eps_w, n_leapfrog=n_leapfrog, inv_mass=step_mass, seed=seed, step=step + r, chain0=chain0)
        else:
            _lp, _ll, dH, acc, *counts = pd.nuts_step(theta_t, eps=eps_w, inv_mass=step_mass, max_depth=max_depth, seed=seed, step=step + r, chain0=chain0)
            tree[r] = _tree_means(*counts)
        k += 1
        rec = None if record is None else dict(round=r, k=k, dH=dH, accepted=acc, theta_t=theta_t.clone(), state_in=state.clone(), use_average=r == n - 1,
                                               mom_in=None if mom is None else tuple(t.clone() for t in mom))
        a, _ = pd.adapt_step(state, dH, acc, k, delta=target_accept, gamma=gamma, t0=t0, kappa=kappa, use_average=r == n - 1, eps_w=eps_w)
        accept_stat[r:r + 1] = a
        in_window = in_window or r in first
        if in_window:
            mom = (pd.cov if dense else pd.moments)(theta_t, out=mom, accumulate=r not in first)
        if rec is not None:
            rec.update(state=state.clone(), accept_stat=a, eps_w=eps_w.clone(), in_window=in_window, first=r in first, last=r in last,
                       mom=tuple(t.clone() for t in mom) if in_window else None, inv_mass_in=inv_mass.clone())
            record.append(rec)
        if r in last:
            if dense:
                _, info = pd.metric_dense(mom[0], mom[2], chol, regularize=True)      # chol is written only where info = 0: nothing is read back
                if rec is not None:
                    rec.update(chol=chol.clone(), info=info)
            else:
                pd.metric(mom[0], mom[1][0], mom[2][0], inv_mass, regularize=True)
            pd.adapt_init(1, torch.exp(state[:, 1]), state=state)
            eps_w = torch.exp(state[:, 0]).expand(W).contiguous()
            in_window, k = False, 0
            if rec is not None:
                rec.update(inv_mass=inv_mass.clone(), state_restart=state.clone())
    if dense:
        pd.use_metric(before)
        L = unpack_lower(chol, D)
        inv_mass = (L * L).sum(dim=1)
    out = dict(theta_t=theta_t, eps=eps_w[:1].clone() if W else torch.exp(state[:, 1]), inv_mass=inv_mass, accept_stat=accept_stat, step=step + n)
    if dense:
        out["metric_chol"] = L
    if tree is not None:
        out["tree"] = tree
    return out


def rhat_from_chain_moments(pd, cmean, cm2, n):
    """R̂ [K] of n samples per chain from their running moments (PriorDraws.chain_moments) by two PriorDraws.moments calls, as
    include/octofitter_hip_draws.h states it. A device tensor."""
    import torch
    cnt, _, m2b = pd.moments(cmean)
    _, mw, _ = pd.moments(cm2)
    b_over_n = m2b[0] / (cnt[0] - 1.0)
    wv = mw[0] / (n - 1.0)
    return torch.sqrt(((n - 1.0) / n * wv + b_over_n) / wv)


DIAGNOSE_KEYS = dict(ess_bulk="ess_bulk", ess_tail="ess_tail", rhat_rank="rhat", ess_basic="ess_basic")      # a sampler's key -> PriorDraws.diagnose's


def _diagnosed(pd, rec_t):
    """What diagnose=True adds to a sampler's dict: DIAGNOSE_KEYS of its recorded rounds rec_t [n, D, n_chains], [D] device tensors made before the
    copy; NaN when there are fewer than 8 rounds."""
    import torch
    if rec_t.shape[0] < 8:
        return {k: torch.full((rec_t.shape[1],), float("nan"), dtype=torch.float64, device=rec_t.device) for k in DIAGNOSE_KEYS}
    d = pd.diagnose(rec_t)
    return {k: d[v] for k, v in DIAGNOSE_KEYS.items()}


def diagnose_draws_device(samples, device=0):
    """The table the reference's user reads after octofit, of stored draws samples [n, D, n_chains] (NumPy or a tensor), n >= 8, on the device:
    dict of NumPy [D] arrays — PriorDraws.diagnose's rhat (rank-normalised split-R̂), ess_bulk, ess_tail, rhat_basic, ess_basic, q05, q50, q95 — plus
    mcse_mean = sd/√ess_basic, sd the standard deviation of all draws of the row."""
    import torch
    from .draws import PriorDraws
    from .priors import Uniform
    dev = torch.device("cuda", int(device))
    x = samples if torch.is_tensor(samples) else torch.from_numpy(np.array(samples, dtype=np.float64))      # a copy: the array may be read-only
    x = x.to(device=dev, dtype=torch.float64).contiguous()
    if x.ndim != 3:
        raise ValueError("diagnose_draws_device: samples must be [n, D, n_chains]")
    with PriorDraws(priors=[Uniform(0.0, 1.0)], device=int(device)) as pd:      # the call needs no model: a handle that only samples serves
        d = pd.diagnose(x)
        d["mcse_mean"] = x.transpose(0, 1).reshape(x.shape[1], -1).std(dim=1) / torch.sqrt(d["ess_basic"])
        torch.cuda.synchronize(dev)
        return {k: v.cpu().numpy() for k, v in d.items()}


def _sampling_metric(pd, wu, pack_lower):
    """(the inv_mass of the sampling rounds, what the result gains) after hmc_warmup: a dense warm-up's factor is set on the handle (the rounds
    then pass no inv_mass) and returned as metric_chol; the handle is closed by its driver, which ends the setting"""
    if "metric_chol" not in wu:
        return wu["inv_mass"], {}
    pd.use_metric(pack_lower(wu["metric_chol"]))
    return None, dict(metric_chol=wu["metric_chol"])


def octofit_hmc_device(model, n_chains=1024, n_warmup=200, n_samples=200, n_leapfrog=8, target_accept=0.8, init=None, eps=0.1, seed=0, diagnose=False,
                       metric="diag"):
    """The reference's main entry (octofit: Pathfinder start, then HMC with step-size and metric adaptation) with every piece on the device:
    n_chains chains at β = 1, static trajectories of n_leapfrog steps, a diagonal metric.
      starts    init [D, n_chains] in θ_t, or pathfinder_device(model, n_draws=n_chains, seed=seed)["theta_t"];
      metric    starts at the per-coordinate variance of prior draws 0 … 4095 in θ_t (the default of the other drivers);
      warm-up   hmc_warmup: n_warmup rounds, step numbers 0 … n_warmup − 1;
      sampling  n_samples rounds with ε and the metric fixed, step numbers going on; every round is recorded and enters the per-chain
                running moments (PriorDraws.chain_moments); R̂ from two PriorDraws.moments calls at the end.
    Returns dict(samples [n_samples, D, n_chains] natural domain, samples_t the same as θ_t, logpost [n_samples, n_chains], accept_stat
    [n_warmup + n_samples] (the mean of min(1, exp(dH)) of each round), eps, inv_mass [D], rhat [D], names, state = dict(theta_t, step)), NumPy.
    diagnose=True adds ess_bulk, ess_tail, rhat_rank and ess_basic [D] of samples_t (PriorDraws.diagnose; NaN with n_samples < 8).
    metric="dense": hmc_warmup(metric="dense") and the sampling rounds under the factor it ends with; the dict gains metric_chol [D, D] (lower),
    and inv_mass is diag(L·Lᵀ)."""
    import torch
    from .draws import PriorDraws, pack_lower
    Cn, nw, ns = int(n_chains), int(n_warmup), int(n_samples)
    if Cn < 2 or nw < 0 or ns < 1:
        raise ValueError("octofit_hmc_device: n_chains >= 2, n_warmup >= 0, n_samples >= 1")
    dev = torch.device("cuda", model.ln_like.device_index)
    D = int(model.D)
    if init is None:
        init = pathfinder_device(model, n_draws=Cn, seed=seed)["theta_t"]
    theta_t = torch.as_tensor(init, dtype=torch.float64, device=dev).clone().contiguous()
    if tuple(theta_t.shape) != (D, Cn):
        raise ValueError(f"octofit_hmc_device: init must be [D = {D}, n_chains = {Cn}] in θ_t")
    with PriorDraws(model) as pd:
        inv_mass = _default_metric(pd, seed, dev, None)
        wu = hmc_warmup(pd, theta_t, nw, n_leapfrog=n_leapfrog, eps=eps, inv_mass=inv_mass, target_accept=target_accept, seed=seed, metric=metric)
        eps_w, inv_mass = wu["eps"].expand(Cn).contiguous(), wu["inv_mass"]
        step_mass, dense = _sampling_metric(pd, wu, pack_lower)
        rec_t = torch.empty((ns, D, Cn), dtype=torch.float64, device=dev)
        rec_lp = torch.empty((ns, Cn), dtype=torch.float64, device=dev)
        acc_s = torch.empty(ns, dtype=torch.float64, device=dev)
        cmean, cm2 = torch.empty_like(theta_t), torch.empty_like(theta_t)
        state = pd.adapt_init(1, eps)      # never fed back: adapt_step is the reduction that gives the round's acceptance statistic
        for r in range(ns):
            lp, _ll, dH, acc = pd.hmc_step(theta_t, eps=eps_w, n_leapfrog=n_leapfrog, inv_mass=step_mass, seed=seed, step=nw + r)
            acc_s[r:r + 1] = pd.adapt_step(state, dH, acc, r + 1, delta=target_accept, want_eps=False)[0]
            rec_t[r] = theta_t
            rec_lp[r] = lp
            pd.chain_moments(theta_t, r + 1, cmean, cm2)
        rhat = rhat_from_chain_moments(pd, cmean, cm2, ns)
        extra = _diagnosed(pd, rec_t) if diagnose else {}
        torch.cuda.synchronize(dev)
        return dict(**_recorded(model, rec_t, rec_lp, pd),
                    accept_stat=torch.cat([wu["accept_stat"], acc_s]).cpu().numpy(), eps=float(wu["eps"][0]), inv_mass=inv_mass.cpu().numpy(),
                    rhat=rhat.cpu().numpy(), names=list(model.names), state=dict(theta_t=theta_t.cpu().numpy(), step=nw + ns),
                    **{k: v.cpu().numpy() for k, v in {**extra, **dense}.items()})


def octofit_nuts_device(model, n_chains=1024, n_warmup=200, n_samples=200, max_depth=10, target_accept=0.8, init=None, eps=0.1, seed=0, diagnose=False,
                        metric="diag"):
    """octofit_hmc_device with the reference's own sampler: every round is one NUTS transition (PriorDraws.nuts_step: multinomial sampling, the
    generalised no-U-turn criterion, trees of depth <= max_depth) instead of a static trajectory. The starts, the metric, the warm-up
    (hmc_warmup(max_depth=max_depth)), the recording and R̂ are octofit_hmc_device's.
    Returns its dict — accept_stat is the mean over the chains of each transition's mean acceptance statistic — plus, per round of warm-up and
    sampling, depth and n_leapfrog [n_warmup + n_samples] (means over the chains) and diverged [n_warmup + n_samples] (counts); diagnose=True adds
    octofit_hmc_device's four keys; metric="dense" as there: the reference's dense Euclidean metric."""
    import torch
    from .draws import PriorDraws, pack_lower
    Cn, nw, ns = int(n_chains), int(n_warmup), int(n_samples)
    if Cn < 2 or nw < 0 or ns < 1:
        raise ValueError("octofit_nuts_device: n_chains >= 2, n_warmup >= 0, n_samples >= 1")
    dev = torch.device("cuda", model.ln_like.device_index)
    D = int(model.D)
    if init is None:
        init = pathfinder_device(model, n_draws=Cn, seed=seed)["theta_t"]
    theta_t = torch.as_tensor(init, dtype=torch.float64, device=dev).clone().contiguous()
    if tuple(theta_t.shape) != (D, Cn):
        raise ValueError(f"octofit_nuts_device: init must be [D = {D}, n_chains = {Cn}] in θ_t")
    with PriorDraws(model) as pd:
        inv_mass = _default_metric(pd, seed, dev, None)
        wu = hmc_warmup(pd, theta_t, nw, eps=eps, inv_mass=inv_mass, target_accept=target_accept, seed=seed, max_depth=max_depth, metric=metric)
        eps_w, inv_mass = wu["eps"].expand(Cn).contiguous(), wu["inv_mass"]
        step_mass, dense = _sampling_metric(pd, wu, pack_lower)
        rec_t = torch.empty((ns, D, Cn), dtype=torch.float64, device=dev)
        rec_lp = torch.empty((ns, Cn), dtype=torch.float64, device=dev)
        acc_s = torch.empty(ns, dtype=torch.float64, device=dev)
        tree = torch.empty((ns, 3), dtype=torch.float64, device=dev)
        cmean, cm2 = torch.empty_like(theta_t), torch.empty_like(theta_t)
        state = pd.adapt_init(1, eps)      # never fed back: adapt_step is the reduction that gives the round's acceptance statistic
        for r in range(ns):
            lp, _ll, la, acc, *counts = pd.nuts_step(theta_t, eps=eps_w, inv_mass=step_mass, max_depth=max_depth, seed=seed, step=nw + r)
            acc_s[r:r + 1] = pd.adapt_step(state, la, acc, r + 1, delta=target_accept, want_eps=False)[0]
            tree[r] = _tree_means(*counts)
            rec_t[r] = theta_t
            rec_lp[r] = lp
            pd.chain_moments(theta_t, r + 1, cmean, cm2)
        rhat = rhat_from_chain_moments(pd, cmean, cm2, ns)
        extra = _diagnosed(pd, rec_t) if diagnose else {}
        torch.cuda.synchronize(dev)
        tree = torch.cat([wu["tree"], tree]).cpu().numpy()
        return dict(**_recorded(model, rec_t, rec_lp, pd),
                    accept_stat=torch.cat([wu["accept_stat"], acc_s]).cpu().numpy(), eps=float(wu["eps"][0]), inv_mass=inv_mass.cpu().numpy(),
                    rhat=rhat.cpu().numpy(), depth=tree[:, 0], n_leapfrog=tree[:, 1], diverged=tree[:, 2].astype(np.int64), names=list(model.names),
                    state=dict(theta_t=theta_t.cpu().numpy(), step=nw + ns), **{k: v.cpu().numpy() for k, v in {**extra, **dense}.items()})


def _optimizer_starts(pd, model, N, n_starts, seed, dev, inv_mass, starts=None):
    """Where the two optimiser drivers start: (θ0 [D, n_starts] the best of prior draws 0 … N − 1, their ℓπ, inv_mass [D] on dev — by default
    _default_metric —, theta_t = link(θ0) on dev). starts: θ_t [D, n] (an array or a tensor) used in place of the best prior draws — θ0 is then
    its inverse link and the ℓπ is the callback's there; N and n_starts are not looked at."""
    import torch
    if starts is None:
        θ0, lp0, _ = pd.best(seed, N, keep=n_starts)
        theta_t = torch.as_tensor(model.link(θ0), dtype=torch.float64, device=dev).contiguous()
    else:
        theta_t = torch.as_tensor(starts, dtype=torch.float64, device=dev).clone().contiguous()
        if theta_t.ndim != 2 or theta_t.shape[0] != pd.D or theta_t.shape[1] < 1:
            raise ValueError(f"starts must be a [D = {pd.D}, n >= 1] array in θ_t")
        θ0 = model.invlink(theta_t.cpu().numpy())
        lp0 = model.logpost_device(theta_t, grad=True)[0].cpu().numpy()      # the call the optimisers open with
    inv_mass = _default_metric(pd, seed, dev, inv_mass)
    return θ0, lp0, inv_mass, theta_t


def _run_segments(segment, max_rounds, rounds_per_call):
    """segment(n_rounds, resume) -> result dict, in segments of rounds_per_call rounds until no chain is active or after max_rounds: the last result."""
    from .draws import LBFGS_ACTIVE
    done, r = 0, None
    while done < max_rounds:
        n = min(int(rounds_per_call), int(max_rounds) - done)
        r = segment(n, done > 0)
        done += n
        if not bool((r["status"] == LBFGS_ACTIVE).any()):      # the one read of a segment
            break
    return r


def _to_numpy_with_best(r):
    """(an optimiser's result dict as NumPy, the index of its highest finite logpost)."""
    out = {k: v.cpu().numpy() for k, v in r.items()}
    return out, int(np.argmax(np.where(np.isfinite(out["logpost"]), out["logpost"], -np.inf)))


def optimize_starting_points_device(model, N=500_000, n_starts=64, seed=0, m=6, gtol=1e-6, ftol=0.0, max_rounds=1000, rounds_per_call=50, inv_mass=None,
                                    starts=None):
    """MAP candidates from the best prior draws: the n_starts (<= 64) best of draws 0 … N − 1 of the counter stream `seed` (PriorDraws.best),
    each optimised by the batched L-BFGS of include/octofitter_hip_draws.h in θ_t, all chains in lockstep on the device. inv_mass, the
    scaling of the optimiser, defaults to the per-coordinate variance of prior draws 0 … 4095 in θ_t (the default of octofit_pt_device). The
    optimiser runs in segments of rounds_per_call rounds; the host reads the status between them and stops when no chain is active or after
    max_rounds rounds. starts: θ_t [D, n] to start from in place of the best prior draws (global_search_device's individuals, say).

    Returns a dict in start order (best start first), NumPy: theta [D, n] natural domain, theta_t, logpost, start_logpost, status (LBFGS_* of
    host/draws.py), gnorm, iters, evals, inv_hess_diag [D, n] (the Pathfinder diagonal in θ_t: a natural inv_mass for hmc_step), best (the index of
    the highest ℓπ), names."""
    import torch
    from .draws import PriorDraws
    if max_rounds < 1 or rounds_per_call < 1:
        raise ValueError("optimize_starting_points_device: max_rounds >= 1, rounds_per_call >= 1")
    dev = torch.device("cuda", model.ln_like.device_index)
    with PriorDraws(model) as pd:
        θ0, lp0, inv_mass, theta_t = _optimizer_starts(pd, model, N, n_starts, seed, dev, inv_mass, starts)
        r = _run_segments(lambda n, resume: pd.lbfgs(theta_t, inv_mass=inv_mass, m=m, n_rounds=n, gtol=gtol, ftol=ftol, resume=resume, want_inv_hess_diag=True),
                          max_rounds, rounds_per_call)
        tt = theta_t.cpu().numpy()
        out, best = _to_numpy_with_best(r)
        return dict(theta=model.invlink(tt), theta_t=tt, start_logpost=lp0, best=best, names=list(model.names), **out)


def global_search_device(model, n_pop=1024, N=500_000, radius=8, max_gen=2000, gens_per_call=25, patience=100, ftol=1e-3, seed=0):
    """The global stage of the reference's initialisation (src/initialization.jl:188-289, between its prior search and Pathfinder) on the device:
    differential evolution (PriorDraws.de) on a population of n_pop points in θ_t. The population is prior draws 0 … n_pop − 1 of the counter
    stream `seed`, with slots 0 … 63 overwritten by the 64 best of draws 0 … N − 1 (PriorDraws.best; fewer with n_pop or N below 64). The bounds
    are the per-coordinate minimum and maximum of θ_t over prior draws 0 … 4095 and over the population. The search runs in segments of
    gens_per_call generations; the host reads the best ℓπ between them (8 bytes, the only synchronisation) and stops when it has not risen by
    ftol over the last `patience` generations, or after max_gen generations.

    Returns a dict, NumPy: theta [D, n_pop] natural domain, theta_t, logpost [n_pop], best (the index of the highest ℓπ), best_logpost, history
    (the best ℓπ at the opening and after every segment), generations (after each of them), n_gen, n_accept [n_pop], lo, hi, names."""
    import torch
    from .draws import MAX_KEEP, PriorDraws
    if n_pop < 4 or max_gen < 0 or gens_per_call < 1 or patience < 1:
        raise ValueError("global_search_device: n_pop >= 4, max_gen >= 0, gens_per_call >= 1, patience >= 1")
    dev = torch.device("cuda", model.ln_like.device_index)
    with PriorDraws(model) as pd:
        theta_t = pd.sample(seed, 0, n_pop, theta=False, logprior_t=False)[1]
        keep = min(MAX_KEEP, int(n_pop), int(N))
        if keep > 0:
            θ0, _lp0, _ = pd.best(seed, N, keep=keep)
            theta_t[:, :keep] = torch.as_tensor(model.link(θ0), dtype=torch.float64, device=dev)
        cloud = pd.sample(seed, 0, 4096, theta=False, logprior_t=False)[1]
        lo = torch.minimum(cloud.min(dim=1).values, theta_t.min(dim=1).values)
        hi = torch.maximum(cloud.max(dim=1).values, theta_t.max(dim=1).values)
        args = dict(lo=lo, hi=hi, radius=radius, seed=seed)
        out = pd.de(theta_t, n_gen=0, **args)
        history, generations, done = [float(out["best_logpost"].item())], [0], 0
        while done < max_gen:
            n = min(int(gens_per_call), int(max_gen) - done)
            out = pd.de(theta_t, n_gen=n, gen0=done, resume=True, out=out, **args)
            done += n
            history.append(float(out["best_logpost"].item()))      # the one read of a segment
            generations.append(done)
            back = next((h for h, g in zip(reversed(history), reversed(generations)) if g <= done - patience), None)
            if back is not None and not history[-1] - back >= ftol:
                break
        tt = theta_t.cpu().numpy()
        return dict(theta=model.invlink(tt), theta_t=tt, logpost=out["logpost"].cpu().numpy(), best=int(out["best"].item()), best_logpost=history[-1],
                    history=np.array(history), generations=np.array(generations), n_gen=done, n_accept=out["n_accept"].cpu().numpy(),
                    lo=lo.cpu().numpy(), hi=hi.cpu().numpy(), names=list(model.names))


def initialize_device(model, n_starts=64, n_pop=1024, N=500_000, radius=8, max_gen=2000, gens_per_call=25, patience=100, search_ftol=1e-3, seed=0, m=6,
                      gtol=1e-6, ftol=0.0, max_rounds=1000, rounds_per_call=50, inv_mass=None):
    """The reference's initialisation up to its local stage, on the device throughout: global_search_device, then the n_starts individuals of the
    highest ℓπ (best first, ties to the lower index) as the starts of optimize_starting_points_device. Returns that function's dict — its
    start_logpost is the individuals' ℓπ — with the search's outputs under `search`, and search_index [n_starts]: the individual each start was."""
    search = global_search_device(model, n_pop=n_pop, N=N, radius=radius, max_gen=max_gen, gens_per_call=gens_per_call, patience=patience, ftol=search_ftol,
                                  seed=seed)
    lp = np.where(np.isfinite(search["logpost"]), search["logpost"], -np.inf)
    order = np.argsort(-lp, kind="stable")[:max(1, min(int(n_starts), lp.size))]
    r = optimize_starting_points_device(model, seed=seed, m=m, gtol=gtol, ftol=ftol, max_rounds=max_rounds, rounds_per_call=rounds_per_call, inv_mass=inv_mass,
                                        starts=np.ascontiguousarray(search["theta_t"][:, order]))
    return dict(r, search=search, search_index=order)


def pathfinder_device(model, N=500_000, n_paths=64, n_draws=1000, n_draws_per_path=256, n_elbo=5, seed=0, m=6, gtol=1e-6, ftol=0.0, max_rounds=1000,
                      rounds_per_call=50, inv_mass=None, starts=None):
    """Multi-path Pathfinder (Zhang et al. 2022; stage 3 of the reference's initialisation, src/initialization.jl:188-289) on the device:
    the starts and the default inv_mass of optimize_starting_points_device (path p starts from the p-th best of draws 0 … N − 1 and owns
    chain p of the counter stream `seed`), PriorDraws.pathfinder in segments of rounds_per_call rounds until no chain is active or after
    max_rounds, then n_draws_per_path draws from every path's kept fit (PriorDraws.pathfinder_draw). The log ratios r = ℓπ − log q over the
    union of the draws of paths with a fit (non-finite: −Inf) are Pareto-smoothed by Psis.loo on the one row ll = −r, and n_draws are
    resampled with replacement from the smoothed weights on the host: NumPy Generator(Philox(key=seed)), inverse CDF. starts: θ_t [D, n] to
    start the paths from in place of the best prior draws.

    Returns a dict, NumPy: theta [D, n_draws] natural domain, theta_t, logpost [n_draws], path [n_draws] (the start index of each draw),
    pareto_k, log_ratios and log_weights (over the n_paths·n_draws_per_path draws, draw j of path p at j·n_paths + p), per path elbo,
    elbo_iter, n_fits and the outputs of optimize_starting_points_device (path_theta, path_theta_t, path_logpost, start_logpost, status, gnorm,
    iters, evals, inv_hess_diag, best), names. Raises RuntimeError if no path has a fit."""
    import torch
    from .draws import PriorDraws
    from .psis import Psis
    if max_rounds < 1 or rounds_per_call < 1 or n_draws < 1 or n_draws_per_path < 1:
        raise ValueError("pathfinder_device: max_rounds, rounds_per_call, n_draws, n_draws_per_path >= 1")
    dev = torch.device("cuda", model.ln_like.device_index)
    with PriorDraws(model) as pd:
        θ0, lp0, inv_mass, theta_t = _optimizer_starts(pd, model, N, n_paths, seed, dev, inv_mass, starts)
        r = _run_segments(lambda n, resume: pd.pathfinder(theta_t, inv_mass=inv_mass, m=m, n_rounds=n, gtol=gtol, ftol=ftol, resume=resume,
                                                          want_inv_hess_diag=True, seed=seed, n_elbo=n_elbo), max_rounds, rounds_per_call)
        if not bool((r["elbo_iter"] >= 0).any()):
            raise RuntimeError("pathfinder_device: no path has a fit (every start is dead, never accepted a step, or has only non-finite ELBOs)")
        phi, logq, lp = pd.pathfinder_draw(theta_t, n_draws_per_path, seed=seed)
        ratio = _finite_or_neg_inf(lp - logq)
        with Psis(device=model.ln_like.device_index) as ps:
            s = ps.loo((-ratio).reshape(1, -1), weights=True)      # its step 1 smooths r − max r
            lw = s["log_weights"][0].cpu().numpy()
            cdf = np.cumsum(np.exp(lw - lw.max()))
            u = np.random.Generator(np.random.Philox(key=int(seed))).random(int(n_draws))
            pick = np.minimum(np.searchsorted(cdf, u * cdf[-1], side="right"), cdf.size - 1)
            W = theta_t.shape[1]
            tt = phi[:, torch.as_tensor(pick, device=dev)].cpu().numpy()
            path_tt = theta_t.cpu().numpy()
            out, best = _to_numpy_with_best(r)
            path_lp = out.pop("logpost")
            return dict(theta=model.invlink(tt), theta_t=tt, logpost=lp.cpu().numpy()[pick], path=(pick % W).astype(np.int64), pareto_k=float(s["pareto_k"][0]),
                        log_ratios=ratio.cpu().numpy(), log_weights=lw, path_theta=model.invlink(path_tt), path_theta_t=path_tt, path_logpost=path_lp,
                        start_logpost=lp0, best=best, names=list(model.names), **out)


def pointwise_like(model, θ_samples):
    """`Octofitter.pointwise_like` (src/cross-validation.jl:17-46) on the batch path: the log-likelihood of every posterior sample under
    EACH observation table separately — LL_out[n_samples, n_observations], one device call per observation over all samples (the
    reference builds one single-observation system per table and loops over samples on the CPU). θ_samples: [D, n] natural domain.
    Returns (LL_out, names)."""
    from .system import BatchedLnLike, Planet, System
    θ_samples = np.asarray(θ_samples, dtype=np.float64).reshape(model.D, -1)
    elems, nuis = model.kernel_inputs(θ_samples)
    fn = model.ln_like
    n = θ_samples.shape[1]
    out = np.zeros((n, len(fn.obs_entries)))
    names = []
    θex = dict(planets={pl.name: {k: 0.0 for k in (pl.variables or {})} for pl in model.system.planets})
    for io, (obs, ip, plname, key) in enumerate(fn.obs_entries):
        planets = [Planet(name=pl.name, basis=pl.basis, observations=[obs] if (ip >= 0 and pl.name == plname) else [], variables=pl.variables)
                   for pl in model.system.planets]
        sub = System(name=f"{model.system.name}_{key}", companions=planets, observations=[obs] if ip < 0 else [], variables=model.system.variables)
        one = BatchedLnLike(sub, θex, device=fn.device_index, consts=None)
        try:
            nu = None if nuis is None else np.ascontiguousarray(nuis[io * 3:(io + 1) * 3])
            out[:, io] = one.ln_like_arrays(elems, nu)
        finally:
            one.close()
        names.append(key)
    return out, names


def _pointwise_handle(model):
    """The Pointwise handle of a model's tables and their labels [(table name, row index)] in the matrix's row order. A model that holds a
    table whose value is no sum over its rows (marginalised RV, HGCA, the O'Neil prior) raises OctoError(OCTO_ENOTSUP)."""
    from .pointwise import Pointwise
    fn = model.ln_like
    pw = Pointwise(fn.obs_tables, fn.planet_desc, device=fn.device_index)
    labels = [(key, j) for (_obs, _ip, _pl, key), t in zip(fn.obs_entries, fn.obs_tables) for j in range(len(t["epoch"]))]
    return pw, labels


def pointwise_like_rows(model, θ_samples):
    """`Octofitter.pointwise_like` (src/cross-validation.jl:17-46) per DATUM: LL[n_samples, R], the log-likelihood of every posterior sample
    under each table ROW alone (what a one-row table scores, constant terms included), in ONE device call — the matrix WAIC, IS-LOO and
    PSIS-LOO consume (PSIS smoothing on the device: include/octofitter_hip_psis.h, `loo`). θ_samples: [D, n] natural domain.
    Returns (LL, labels) with labels[r] = (table name, row index). The rows of a table sum to its column of pointwise_like."""
    θ_samples = np.asarray(θ_samples, dtype=np.float64).reshape(model.D, -1)
    elems, nuis = model.kernel_inputs(θ_samples)
    pw, labels = _pointwise_handle(model)
    with pw:
        LL = pw.values(elems, nuis)
    return np.ascontiguousarray(LL.T), labels


def _add_totals(out, keys, R):
    """For each of the per-row arrays out[k], k in keys: out[k_total], the sum over the R rows, and out[k_se] = √(R · var over the rows)."""
    for k in keys:
        out[k + "_total"] = float(np.sum(out[k]))
        out[k + "_se"] = float(np.sqrt(R * np.var(out[k], ddof=1))) if R > 1 else float("nan")


def waic(model, θ_samples):
    """WAIC and importance-sampling LOO of a model from posterior samples θ_samples [D, n] (natural domain), reduced over the samples on the
    device: the matrix of pointwise_like_rows is never stored. Per row r, over the samples with a finite value:
        lppd[r] = log mean exp(ll),  p_waic[r] = sample variance of ll,  elpd_waic[r] = lppd[r] − p_waic[r],  elpd_is_loo[r] = −log mean exp(−ll).
    Returns dict(lppd, p_waic, elpd_waic, elpd_is_loo: [R] arrays; <name>_total: their sums over the rows; <name>_se = √(R · var over the
    rows): the totals' standard errors; n_valid [R]; n_samples; labels [(table name, row index)])."""
    θ_samples = np.asarray(θ_samples, dtype=np.float64).reshape(model.D, -1)
    elems, nuis = model.kernel_inputs(θ_samples)
    pw, labels = _pointwise_handle(model)
    with pw:
        s = pw.summary(elems, nuis)
    out = dict(lppd=s["lppd"], p_waic=s["var"], elpd_waic=s["lppd"] - s["var"], elpd_is_loo=s["elpd_is_loo"])
    _add_totals(out, ("lppd", "p_waic", "elpd_waic", "elpd_is_loo"), len(labels))
    out.update(n_valid=s["n"], n_samples=int(θ_samples.shape[1]), labels=labels)
    return out


def loo(model, θ_samples, weights=False):
    """PSIS-LOO (Pareto-smoothed importance-sampling leave-one-out; Vehtari, Gelman & Gabry 2017) of a model from posterior samples θ_samples
    [D, n] (natural domain), on the device: the matrix of pointwise_like_rows is formed there by the Pointwise handle and smoothed there by
    Psis (include/octofitter_hip_psis.h states the algorithm), so it never crosses PCIe. It is STORED on the device: R·n·8 bytes of HBM (plus as
    much again for the log-weights when asked). Per row r, over the samples with a finite value:
        pareto_k[r] = the fitted Pareto shape k̂ (> 0.7: do not trust this row; +Inf: no fit was made),  elpd_loo[r] = logsumexp(ll + lw),
        lppd[r] = log mean exp(ll),  p_loo[r] = lppd[r] − elpd_loo[r],  ess[r] = 1/Σ exp(2·lw).
    Returns dict(elpd_loo, pareto_k, lppd, p_loo, ess, n_valid, tail_len: [R] arrays; <name>_total and <name>_se = √(R · var over the rows) for
    elpd_loo and p_loo, as waic() forms them; n_bad_k = count(pareto_k > 0.7); n_samples; labels [(table name, row index)]; and, with
    weights=True, log_weights [R, n]: the smoothed normalised log-weights). A model with a marginalised-RV, HGCA or O'Neil table raises
    OctoError(OCTO_ENOTSUP), as waic() does."""
    import torch
    from .psis import Psis
    θ_samples = np.asarray(θ_samples, dtype=np.float64).reshape(model.D, -1)
    elems, nuis = model.kernel_inputs(θ_samples)
    pw, labels = _pointwise_handle(model)
    with pw, Psis(device=pw.device_index) as ps:
        dev = torch.device("cuda", pw.device_index)
        d_el = torch.from_numpy(np.ascontiguousarray(elems, dtype=np.float64)).to(dev)
        d_nu = None if nuis is None else torch.from_numpy(np.ascontiguousarray(nuis, dtype=np.float64)).to(dev)
        s = ps.loo(pw.values(d_el, d_nu), weights=weights)
        s = {k: v.cpu().numpy() for k, v in s.items()}      # the copy waits for the stream both calls ran on
    out = dict(elpd_loo=s["elpd_loo"], pareto_k=s["pareto_k"], lppd=s["lppd"], p_loo=s["lppd"] - s["elpd_loo"], ess=s["ess"],
               n_valid=s["n"], tail_len=s["tail_len"])
    _add_totals(out, ("elpd_loo", "p_loo"), len(labels))
    out.update(n_bad_k=int(np.count_nonzero(out["pareto_k"] > 0.7)), n_samples=int(θ_samples.shape[1]), labels=labels)
    if weights:
        out["log_weights"] = s["log_weights"]
    return out


def simulate_tables(obs_tables, planets, elems, nuis=None, device=0, consts=None):
    """`simulate!` of every observation table for a batch of parameter sets (relative-astrometry.jl:104-142, rv-absolute.jl:135-158,
    rv-absolute-margin.jl:106-126, rv-relative.jl:121-164), on the device: one Predictor per table at the table's own epochs, with the
    channels its kind needs and the RV offset / trend coefficient wired from `nuis`.
    obs_tables / planets: as given to capi.pack_obs / pack_planets; elems [P*9, W]; nuis [n_obs*3, W] or None (the defaults).
    Returns one dict per table of [n_epochs, W] arrays: RADEC / ONEIL_RADEC -> ra, dec; SEPPA / ONEIL_SEPPA -> pa, sep (the wrapped
    table's model); RV_ABS, RV_ABS_MARG (no offset), RV_REL -> rv. The platescale and northangle nuisances act on the data, not on these.
    An HGCA table raises OctoError(OCTO_ENOTSUP): its model values are not on the device path."""
    from . import capi, predict
    elems = np.ascontiguousarray(elems, dtype=np.float64)
    nu = None if nuis is None else np.ascontiguousarray(nuis, dtype=np.float64)
    out = []
    for io, t in enumerate(obs_tables):
        kind, ip = int(t["kind"]), int(t["planet"])
        if kind == capi.HGCA:
            raise capi.OctoError(capi.OCTO_ENOTSUP, f"simulate_tables: table {io} is an HGCA table: its model values are not on the device path")
        basis = add0 = add1 = None
        if kind in (capi.ASTROM_RADEC, capi.ONEIL_RADEC):
            names, channels = ("ra", "dec"), [(predict.ASTROM_RA, ip), (predict.ASTROM_DEC, ip)]
        elif kind in (capi.ASTROM_SEPPA, capi.ONEIL_SEPPA):
            names, channels = ("pa", "sep"), [(predict.ASTROM_PA, ip), (predict.ASTROM_SEP, ip)]
        elif kind in (capi.RV_ABS, capi.RV_ABS_MARG, capi.RV_REL):
            names, channels = ("rv",), [(predict.RV_REL, ip) if kind == capi.RV_REL else (predict.RV_STAR, -1)]
            extra = t.get("extra")
            if nu is not None:
                rows = nu[io * capi.N_NUIS:(io + 1) * capi.N_NUIS]
                if kind != capi.RV_ABS_MARG:
                    add0 = rows[capi.NU_RV_OFFSET:capi.NU_RV_OFFSET + 1]
                if extra is not None and len(extra) == len(t["epoch"]):      # the trend applies only to a table uploaded with a basis column
                    basis, add1 = extra, rows[capi.NU_RV_TREND:capi.NU_RV_TREND + 1]
        else:
            raise capi.OctoError(capi.OCTO_EINVAL, f"simulate_tables: table {io} has an unknown kind {kind}")
        if len(t["epoch"]) == 0:
            out.append({n: np.empty((0, elems.shape[1])) for n in names})
            continue
        with predict.Predictor(planets, t["epoch"], channels, basis=basis, device=device, consts=consts) as pr:
            cube = pr.values(elems, add0=add0, add1=add1)
        out.append({n: cube[k] for k, n in enumerate(names)})
    return out


def posterior_predictive(planets, elems, epochs, channels, summary=True, basis=None, add0=None, add1=None, device=0, consts=None):
    """The model curves of posterior draws over a time grid: `channels` [(quantity, planet)] (host/predict.py) of every draw in `elems`
    [P*9, W] at `epochs` [T]. summary=True: dict(n_valid, mean, sd, min, max), each [C, T], reduced over the draws on the device (the
    cube is never stored); summary=False: the cube [C, T, W]. NumPy or device (torch) elements, as Predictor takes them."""
    from . import predict
    with predict.Predictor(planets, epochs, channels, basis=basis, device=device, consts=consts) as pr:
        res = pr.summary(elems, add0=add0, add1=add1) if summary else pr.values(elems, add0=add0, add1=add1)
        pr.sync()
        if not isinstance(res, (dict, np.ndarray)) or (isinstance(res, dict) and not isinstance(res["mean"], np.ndarray)):
            import torch
            torch.cuda.synchronize()      # device inputs ran on torch's current stream: the handle is destroyed below
        return res


def octofit_nested_device(model, n_live=1024, batch=256, n_passes=4, max_steps=8, max_shrink=64, dlogz=0.01, max_iter=2000, n_samples=4096, seed=0):
    """Nested sampling (the reference's fourth sampler: dynesty behind a hypercube prior transform) with the live set, the cull, the
    constrained-prior moves and the evidence bookkeeping on the device (PriorDraws.cube / from_cube / nested_step / nested_cull). n_live prior
    points of the unit cube are scored; every iteration removes the `batch` lowest and replaces them by slice moves in the cube from copies of
    survivors (n_passes sweeps, stepping out up to max_steps widths of the live set's extent per coordinate), until the remaining-evidence bound
    of the state falls below dlogz or after max_iter iterations; then the live set is flushed. The host reads the 8-double state once per
    iteration and the count of active chains once per segment of rounds. The defaults are the project's own.
    Returns dict(logz, logz_err = √(information/n_live), information, theta [D, n] (natural domain), theta_t [D, n], loglike [n], logwt [n] of
    the n dead points in the order they died, weights [n] = exp(logwt − logz), samples [D, n_samples] (natural domain) and samples_t, equally
    weighted by systematic resampling from one uniform of the counter generator (coordinate 0 of prior draw n_live of `seed`), ess, n_iter,
    n_evals, n_stuck, names)."""
    import torch
    from .draws import PriorDraws
    K, B, most = int(n_live), int(batch), int(max_iter)
    if not 1 <= B <= K - 1 or most < 1 or int(n_samples) < 1:
        raise ValueError("octofit_nested_device: 1 <= batch <= n_live - 1, max_iter >= 1, n_samples >= 1")
    dev = torch.device("cuda", model.ln_like.device_index)
    D = int(model.D)
    with PriorDraws(model) as pd:
        u = pd.cube(seed, 0, K)
        _, tt, lpt = pd.from_cube(u, theta=False)
        ll = _finite_or_neg_inf(model.logpost_device(tt, grad=False)[0] - lpt).contiguous()
        state = pd.nested_state()
        room = most * B + K
        dead = dict(u=torch.empty((D, room), dtype=torch.float64, device=dev), loglike=torch.empty(room, dtype=torch.float64, device=dev),
                    logvol=torch.empty(room, dtype=torch.float64, device=dev), logwt=torch.empty(room, dtype=torch.float64, device=dev))
        counts = torch.zeros(2, dtype=torch.int64, device=dev)
        n_iter = 0
        while n_iter < most:
            r = pd.nested_step(u, ll, state, B, max_steps=max_steps, n_passes=n_passes, max_shrink=max_shrink, seed=seed, iter=n_iter, dead=dead,
                               dead_first=n_iter * B)
            counts += torch.stack([r["n_eval"].sum(), r["n_stuck"].sum()])
            n_iter += 1
            if float(state.cpu()[4]) < float(dlogz):
                break
        pd.nested_cull(u, ll, state, K, replace=False, seed=seed, iter=n_iter, dead=dead, dead_first=n_iter * B)
        n = n_iter * B + K
        du = dead["u"][:, :n].contiguous()
        theta, theta_t, _ = pd.from_cube(du, logprior_t=False)
        v = float(pd.cube(seed, K, 1)[0, 0])
        torch.cuda.synchronize(dev)
        logz = float(state[0])
        loglike, logwt = dead["loglike"][:n].cpu().numpy(), dead["logwt"][:n].cpu().numpy()
        theta, theta_t = theta.cpu().numpy(), theta_t.cpu().numpy()
        n_evals, n_stuck = (int(c) for c in counts.cpu())
    with np.errstate(all="ignore"):
        p = np.exp(logwt - logz)
        ok = p > 0
        information = float(np.sum(p[ok] * (loglike[ok] - logz)))
    cum = np.cumsum(p)
    pick = np.minimum(np.searchsorted(cum / cum[-1], (v + np.arange(int(n_samples))) / int(n_samples), side="left"), n - 1)
    return dict(logz=logz, logz_err=float(np.sqrt(max(information, 0.0) / K)), information=information, theta=theta, theta_t=theta_t, loglike=loglike,
                logwt=logwt, weights=p, samples=theta[:, pick], samples_t=theta_t[:, pick], ess=float(1.0 / np.sum((p / cum[-1]) ** 2)), n_iter=n_iter,
                n_evals=n_evals + K, n_stuck=n_stuck, names=list(model.names))
