"""
octofitter.jl_amd — MI355X-native epoch-loop likelihood path for Octofitter.jl.

The directory name carries a dot (it is the reference's name), so it is loaded by path:
`from __graft_entry__ import load_package; pkg = load_package()` registers it as the module
`octofitter_jl_amd`. Contents: csrc/ (HIP kernels + C ABI), host/ (Python mirror of the
reference's observation / system / ln_like surface over ctypes), julia/ (the ccall shim a
maintainer would drop into Octofitter.jl).
"""
from .host import capi  # noqa: F401
from .host.observations import (  # noqa: F401
    PlanetRelAstromObs, PlanetRelAstromLikelihood, StarAbsoluteRVObs, StarAbsoluteRVLikelihood,
    MarginalizedStarAbsoluteRVObs, PlanetRelativeRVObs, PlanetRelativeRVLikelihood, ObsPriorAstromONeil2019,
    HGCAInstantaneousObs, HGCAInstantaneousLikelihood, AlongScanAstromObs, hipparcos_iad_obs, gaia_epoch_obs,
    CatalogueFitObs, hgca_obs, HGCAObs,
)
from .host.system import Planet, System, make_ln_like, BatchedLnLike, accelerate, not_on_device  # noqa: F401
from .host.sharding import shard_range, ShardedLnLike  # noqa: F401,E402
from .host.tempering import TemperedSwap  # noqa: F401,E402
from .host.ofti import OftiLinearSolver, ofti_linear_solve  # noqa: F401,E402
from .host.priors import (Uniform, LogUniform, Normal, TruncatedNormal, truncated, Sine, UniformCircular,  # noqa: F401,E402
                          θ_at_epoch_to_tperi, variables)
from .host import derived  # noqa: F401,E402
from .host.derived import Derived  # noqa: F401,E402
from .host import gp  # noqa: F401,E402
from .host.gp import RealTerm, ComplexTerm, SHOTerm, Celerite  # noqa: F401,E402
from .host.gp import SqExpTerm, Matern32Term, Matern52Term, PeriodicTerm, QuasiPeriodicTerm, DenseKernel, GP  # noqa: F401,E402
from .host.model import LogDensityModel  # noqa: F401,E402
from .host.callers import (guess_starting_position, octofit_rejection, rejection_evaluate_likelihoods, pointwise_like,  # noqa: F401,E402
                           guess_starting_position_device, octofit_rejection_device, simulate_tables, posterior_predictive,
                           pointwise_like_rows, waic, loo, octofit_pt_device, octofit_pigeons_device, optimize_starting_points_device, pathfinder_device,
                           warmup_windows, hmc_warmup, octofit_hmc_device, octofit_nuts_device, diagnose_draws_device, octofit_nested_device,
                           global_search_device, initialize_device, octofit_ofti_device)
from .host.draws import PriorDraws  # noqa: F401,E402
from .host import predict  # noqa: F401,E402
from .host.predict import Predictor  # noqa: F401,E402
from .host import pointwise  # noqa: F401,E402
from .host.pointwise import Pointwise  # noqa: F401,E402
from .host import psis  # noqa: F401,E402
from .host.psis import Psis  # noqa: F401,E402
