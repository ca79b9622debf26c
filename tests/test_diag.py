"""
The convergence diagnostics on the device (include/octofitter_hip_draws.h: octo_draws_diagnose_device, octo_draws_rank_device; host/draws.py:
PriorDraws.diagnose / ranks; host/callers.py: diagnose_draws_device, octofit_nuts_device(diagnose=True)) against their NumPy restatement
(tests/diag_reference.py) on the cases of tests/diag_cases.py, whose decision margins tests/test_diag_reference.py establishes on the CPU.

Bars: the ranks and the three quantiles bit for bit; z the project's device-transcendental bar TRANS_BAR relative to max(1, |ref|); R̂ and ESS
max(TRANS_BAR, 100 × the statistic's long-double gap of profiles/diag_throughput.txt) relative to max(1, |ref|) — the restatement, never the
device, is the yardstick. Two runs, the same draws at another ld and ls, and a handle that ran other shapes or a cube with non-finite draws
before, give the same bits.
"""
import ctypes as C

import numpy as np
import pytest

import diag_cases as cases
import diag_reference as ref
from draws_device import TRANS_BAR, close, draws_mod, hmc_model, mirror_priors, rel, same_bits      # noqa: F401
import draws_cases

pytestmark = pytest.mark.gpu
BARS = {s: max(TRANS_BAR, 100.0 * cases.LONG_DOUBLE_GAP[s]) for s in cases.STATISTICS}


@pytest.fixture(scope="module")
def pd(pkg, draws_mod):
    """a handle without a model: the calls need none"""
    h = draws_mod.PriorDraws(priors=mirror_priors(pkg, draws_cases.STAT_PRIORS))
    yield h
    h.close()


def on_device(x):
    import torch
    return torch.as_tensor(np.array(x), device="cuda")      # a copy: the cases are read-only


def padded_cube(x, extra_ld=5, extra_rows=2):
    """x [n, K, W] as a view with ld = W + extra_ld and ls = (K + extra_rows)·ld of a buffer that holds NaN everywhere else"""
    import torch
    n, K, W = x.shape
    buf = torch.full((n, K + extra_rows, W + extra_ld), float("nan"), dtype=torch.float64, device="cuda")
    buf[:, :K, :W] = on_device(x)
    return buf[:, :K, :W]


def stats_on_host(d):
    return np.stack([d[name].cpu().numpy() for name in ref.NAMES])


def check_against_reference(name, got_stats, got=None):
    """the statistics (and, if given, the outputs of the rank step by name) of a case against the restatement"""
    want = cases.reference(name)
    ws = want["stats"]
    assert got_stats.shape == ws.shape, (name, got_stats.shape)
    for q in (ref.Q05, ref.Q50, ref.Q95):
        assert np.array_equal(got_stats[q], ws[q], equal_nan=True), (name, ref.NAMES[q], got_stats[q], ws[q])
    for s in cases.STATISTICS:
        q = getattr(ref, s.upper())
        ok = ~np.isnan(ws[q])
        worst = float(np.max(rel(got_stats[q][ok], ws[q][ok]), initial=0.0))
        print(f"{name}: {s} worst relative gap {worst:.3e} (bar {BARS[s]:.1e})")
        assert close(got_stats[q], ws[q], BARS[s]), (name, s, got_stats[q], ws[q])
    for key, arr in (got or {}).items():
        if key.startswith("rank"):
            assert np.array_equal(arr, want[key], equal_nan=True), (name, key)
        else:
            ok = ~np.isnan(want[key])
            print(f"{name}: {key} worst relative gap {float(np.max(rel(arr[ok], want[key][ok]), initial=0.0)):.3e}")
            assert close(arr, want[key], TRANS_BAR), (name, key)


@pytest.mark.parametrize("name", list(cases.CASES))
def test_gpu_diagnose_and_ranks_against_the_restatement(pd, name):
    x = on_device(cases.draws(name))
    first = stats_on_host(pd.diagnose(x))
    r, z = pd.ranks(x)
    rf, zf = pd.ranks(x, fold=True)
    check_against_reference(name, first, dict(rank=r.cpu().numpy(), z=z.cpu().numpy(), rank_folded=rf.cpu().numpy(), z_folded=zf.cpu().numpy()))
    assert np.array_equal(stats_on_host(pd.diagnose(x)), first, equal_nan=True), name      # run to run
    bad = cases.INVALID_ROWS.get(name, [])
    assert np.all(np.isnan(first[:, bad])) and not np.any(np.isnan(np.delete(first, bad, axis=1)[[0, 1, 3, 4, 5, 6, 7]])), name


@pytest.mark.parametrize("name", ["two_blocks", "odd_n", "nan_and_inf", "long_chain", "censored"])
def test_gpu_other_strides_give_the_same_bits(pd, name):
    """ld = W + 5 with NaN beyond column W, ls > K·ld with NaN rows between the samples, and garbage in the unused middle sample"""
    import torch
    x = cases.draws(name)
    n = x.shape[0]
    dense, view = on_device(x), padded_cube(x)
    assert view.stride() == ((x.shape[1] + 2) * (x.shape[2] + 5), x.shape[2] + 5, 1)
    if n % 2:
        view[n // 2] = 1e300
    want = stats_on_host(pd.diagnose(dense))
    assert np.array_equal(stats_on_host(pd.diagnose(view)), want, equal_nan=True), name
    check_against_reference(name, want)
    for fold in (False, True):
        r0, z0 = pd.ranks(dense, fold=fold)
        r1, z1 = pd.ranks(view, fold=fold)
        assert r1.stride() == view.stride() and torch.equal(torch.nan_to_num(r0, nan=-1.0), torch.nan_to_num(r1, nan=-1.0))
        assert torch.equal(torch.nan_to_num(z0, nan=-9.0), torch.nan_to_num(z1, nan=-9.0)), (name, fold)
        if n % 2:
            assert bool(torch.isnan(r1[n // 2]).all()) and bool(torch.isnan(z1[n // 2]).all())      # the unused sample is not written
    r_only, none = pd.ranks(dense, z=False)
    assert none is None and torch.equal(torch.nan_to_num(r_only, nan=-1.0), torch.nan_to_num(pd.ranks(dense)[0], nan=-1.0))


def diagnose_and_folded_ranks(h, name):
    """[stats, r, z] of diagnose and ranks(fold=True) of a case on the handle h, on the host"""
    x = on_device(cases.draws(name))
    stats = stats_on_host(h.diagnose(x))
    r, z = h.ranks(x, fold=True)
    return [stats, r.cpu().numpy(), z.cpu().numpy()]


def test_gpu_one_handle_reused_across_shapes_gives_the_bits_of_a_fresh_one(pkg, draws_mod):
    """The work array is carved again for every shape, larger or smaller than the one before, and the flags of non-finite draws are cleared by
    every call: whatever a handle did before, a call gives the bits of the same call on a handle that has done nothing else."""
    order = ("global_passes", "smallest", "long_chain", "edge_N16_W128", "long_chain")

    def handle():
        return draws_mod.PriorDraws(priors=mirror_priors(pkg, draws_cases.STAT_PRIORS))

    fresh = {}
    for name in sorted(set(order)):
        with handle() as h:
            fresh[name] = diagnose_and_folded_ranks(h, name)
    with handle() as h:
        for step, name in enumerate(order):
            assert same_bits(diagnose_and_folded_ranks(h, name), fresh[name]), (step, name)      # so the second long_chain equals the first
        # a cube that flags rows 1 and 3, then a finite cube of the same shape on the same carving: no flag is left over
        poisoned = stats_on_host(h.diagnose(on_device(cases.draws("nan_and_inf"))))
        assert np.all(np.isnan(poisoned[:, [1, 3]])) and not np.any(np.isnan(poisoned[:, [0, 2]]))
        stats, rf, zf = diagnose_and_folded_ranks(h, "nan_and_inf_finite")
        r, z = (t.cpu().numpy() for t in h.ranks(on_device(cases.draws("nan_and_inf_finite"))))
    assert not np.any(np.isnan(stats)) and not np.any(np.isnan(r)) and not np.any(np.isnan(zf))
    check_against_reference("nan_and_inf_finite", stats, dict(rank=r, z=z, rank_folded=rf, z_folded=zf))
    for name in ("long_chain", "edge_N16_W128"):
        check_against_reference(name, fresh[name][0], dict(rank_folded=fresh[name][1], z_folded=fresh[name][2]))


@pytest.mark.parametrize("name", ["smallest", "global_passes"])
def test_gpu_the_two_dimensional_form(pd, name):
    x = cases.draws(name)
    assert x.shape[1] == 1
    flat = on_device(x[:, 0, :])
    d = pd.diagnose(flat)
    assert all(v.shape == (1,) for v in d.values())
    assert np.array_equal(stats_on_host(d), stats_on_host(pd.diagnose(on_device(x))), equal_nan=True)
    r, z = pd.ranks(flat)
    assert r.shape == flat.shape and np.array_equal(r.cpu().numpy(), cases.reference(name)["rank"][:, 0, :])
    assert close(z.cpu().numpy(), cases.reference(name)["z"][:, 0, :], TRANS_BAR)


def test_gpu_out_argument_and_work_size(pd, draws_mod):
    import torch
    x = on_device(cases.draws("widest_K"))
    out = torch.full((draws_mod.DIAG_N_STATS, 64), -7.0, dtype=torch.float64, device="cuda")
    d = pd.diagnose(x, out=out)
    assert d["ess_bulk"].data_ptr() == out[draws_mod.DIAG_ESS_BULK].data_ptr() and not bool((out == -7.0).any())
    with pytest.raises(ValueError):
        pd.diagnose(x, out=torch.empty((draws_mod.DIAG_N_STATS, 63), dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        pd.diagnose(x.float())
    assert pd.lib.octo_draws_diagnose_work_doubles(16, 2, 64) == ref.work_doubles(16, 2, 64)


def test_gpu_argument_checks_answer_before_any_launch(pkg, pd):
    import torch
    lib, EINVAL, ENOTSUP = pd.lib, pkg.capi.OCTO_EINVAL, pkg.capi.OCTO_ENOTSUP
    n, W, K = 8, 4, 2
    x = torch.zeros((n, K, W), dtype=torch.float64, device="cuda")
    out = torch.full((8, K), -7.0, dtype=torch.float64, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def diag(n_=n, W_=W, ld=W, ls=K * W, K_=K, d_x=x.data_ptr(), d_out=out.data_ptr()):
        return lib.octo_draws_diagnose_device(pd._h, n_, W_, ld, ls, K_, d_x, d_out, st)

    def rank(n_=n, W_=W, ld=W, ls=K * W, K_=K, d_x=x.data_ptr(), d_r=out.data_ptr()):
        return lib.octo_draws_rank_device(pd._h, n_, W_, ld, ls, K_, d_x, 0, d_r, None, st)

    for call in (diag, rank):
        assert call(d_x=None) == EINVAL and call(K_=0) == EINVAL and call(K_=65, ls=65 * W) == EINVAL and call(n_=7) == EINVAL
        assert call(W_=0, ld=0) == EINVAL and call(ld=W - 1) == EINVAL and call(ls=K * W - 1) == EINVAL
        assert b"octo_draws_" in lib.octo_draws_last_error(pd._h)
        assert call(n_=8, W_=(1 << 22) + 1, ld=(1 << 22) + 1, ls=K * ((1 << 22) + 1)) == ENOTSUP      # 2·N·W = 2^25 + 8: refused before any read
        assert call(n_=1 << 26, W_=1, ld=1, ls=K) == ENOTSUP
    assert diag(d_out=None) == EINVAL
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())      # nothing was launched
    assert lib.octo_draws_diagnose_work_doubles(7, 4, 2) == 0 and lib.octo_draws_diagnose_work_doubles(8, 4, 65) == 0
    assert lib.octo_draws_diagnose_work_doubles(1 << 26, 1, 1) == 0


def test_gpu_diagnose_draws_device(pkg):
    x = cases.draws("geyer_far")
    d = pkg.diagnose_draws_device(x)
    want = cases.reference("geyer_far")["stats"]
    assert set(d) == set(ref.NAMES) | {"mcse_mean"} and all(v.shape == (2,) for v in d.values())
    check_against_reference("geyer_far", np.stack([d[name] for name in ref.NAMES]))
    sd = x.transpose(1, 0, 2).reshape(2, -1).std(axis=1, ddof=1)
    assert close(d["mcse_mean"], sd / np.sqrt(want[ref.ESS_BASIC]), max(BARS["ess_basic"], 1e-12))


def test_gpu_octofit_nuts_device_with_diagnose(pkg, draws_mod):
    """the driver at the small shape of tests/test_nuts.py: the new keys are diagnose_draws_device of its own samples_t, and nothing else moves"""
    model = hmc_model(pkg)
    try:
        with draws_mod.PriorDraws(model) as h:
            Cn, nw, ns, seed, D = 256, 40, 40, 61, model.D
            init = h.sample(seed, 0, Cn, theta=False, logprior_t=False)[1].cpu().numpy()
        args = dict(n_chains=Cn, n_warmup=nw, n_samples=ns, max_depth=5, init=init, seed=seed)
        plain = pkg.octofit_nuts_device(model, **args)
        out = pkg.octofit_nuts_device(model, diagnose=True, **args)
        new = {"ess_bulk": "ess_bulk", "ess_tail": "ess_tail", "rhat_rank": "rhat", "ess_basic": "ess_basic"}
        assert set(out) == set(plain) | set(new)
        for k, v in plain.items():
            same = all(np.array_equal(v[j], out[k][j]) for j in v) if isinstance(v, dict) else \
                np.array_equal(v, out[k], equal_nan=True) if isinstance(v, np.ndarray) else v == out[k]
            assert same, k
        table = pkg.diagnose_draws_device(out["samples_t"])
        for k, t in new.items():
            assert out[k].shape == (D,) and np.array_equal(out[k], table[t], equal_nan=True), k
        assert np.all(np.isfinite(out["ess_bulk"])) and np.all(out["rhat_rank"] > 0.9)
        print(f"NUTS driver with diagnose: rank R̂ {out['rhat_rank'].min():.3f} … {out['rhat_rank'].max():.3f}, bulk ESS {out['ess_bulk'].min():.0f} … "
              f"{out['ess_bulk'].max():.0f}, tail ESS {out['ess_tail'].min():.0f} … {out['ess_tail'].max():.0f} of {ns * Cn} draws")
        short = pkg.octofit_nuts_device(model, diagnose=True, **dict(args, n_warmup=4, n_samples=7))
        assert all(short[k].shape == (D,) and np.all(np.isnan(short[k])) for k in new)
    finally:
        model.close()
