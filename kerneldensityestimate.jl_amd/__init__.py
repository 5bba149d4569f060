"""kdehip -- MI355X-native multiscale-Gibbs KDE products (hot path of KernelDensityEstimate.jl).

This package is the Python host mirror of the reference's interface for that path
(`kde!`, `BallTreeDensity`, `getPoints/getBW/getWeights`, `Npts/Ndim`, `prodAppxMSGibbsS`, `gibbs1`,
`sample/rand/resample`, `evalAvgLogL/entropy/kld/minkld`, `evaluate_log`, `evaluate_tol/setForceEvalDirect`, `marginal`, `getKDERange/getKDEMax/getKDEMean/getKDEfit`,
`intersIntgAppxIS`, and the library's own exact overlap measures `intersIntg/ise/mmd` and joint modes
`evaluate_grad/meanshift/modes/getKDEMode`, their curvature `evaluate_hess/laplace/fit_modes/getKDEModeFit`, conditionals
`condition/conditional_weights/conditional_moments/sample_conditional` and probability masses
`box_mass/cdf/quantile/median/interval/grid_mass`, the exact product of two densities `prod_exact/product_components/log_intersIntg/mul_exact`, nearest neighbours `knn/entropy_knn/kld_knn`, per-point bandwidths `kde_varbw/adaptive_scales/kde_adaptive`, and the joint bandwidth `joint_bandwidth/kde_joint`)
over the C ABI of libkdehip.so (include/kdehip.h).  The directory name contains a dot, so import it
through the top-level `kdehip` module of this repository.
"""
from ._lib import KdeHipError, LIB_PATH, lib as _clib  # noqa: F401  (import fails loudly if the .so is missing)
from .density import (BallTree, BallTreeDensity, Ndim, Npts, density_from_arrays, getBW, getPoints,  # noqa: F401
                      getWeights, kde, kde_b, kde_batch)
from .bandwidth import auto_bandwidth, evaluate_log, evaluateDualTree, kde_auto  # noqa: F401
from .product import (DeviceDensity, GbGlb, MultiProductPlan, ProductBatch, ProductPlan, batch_launches, gibbs1, makeEmptyGbGlb, mul, mul_device, mul_device_batch,  # noqa: F401
                      nlevels, philox_streams, prodAppxMSGibbsS, prodAppxMSGibbsS_batch, prodAppxMSGibbsS_device,
                      prodAppxMSGibbsS_resident)
from .sample import rand, resample, sample, sample_device_batch  # noqa: F401
from .loglik import entropy, eval_avg_logl_device_batch, evalAvgLogL, kld, kld_batch, minkld  # noqa: F401
from .overlap import intersIntg, ise, ise_batch, kernel_sum, kernel_sum_device_batch, mmd, mmd_batch  # noqa: F401
from .modes import evaluate_grad, getKDEMode, meanshift, meanshift_device_batch, modes  # noqa: F401
from .curvature import evaluate_hess, evaluate_hess_device_batch, fit_modes, getKDEModeFit, laplace  # noqa: F401
from .conditional import (condition, conditional_device_batch, conditional_moments, conditional_weights,  # noqa: F401
                          sample_conditional)
from .prodexact import log_intersIntg, mul_exact, prod_exact, prod_exact_device_batch, product_components  # noqa: F401
from .mass import (box_mass, box_mass_device_batch, cdf, grid_mass, interval, median, quantile,  # noqa: F401
                   quantile_device_batch)
from .evaltol import evaluate_tol, getForceEvalDirect, setForceEvalDirect  # noqa: F401
from .knn import entropy_knn, kld_knn, knn  # noqa: F401
from .varbw import adaptive_scales, kde_adaptive, kde_varbw  # noqa: F401
from .bwjoint import joint_bandwidth, joint_bandwidth_device_batch, kde_joint  # noqa: F401
from .summary import (getKDEfit, getKDEMax, getKDEMean, getKDERange, getKDERangeLinspace, intersIntgAppxIS,  # noqa: F401
                      marginal, summary_device_batch)


def device_count() -> int:
    return int(_clib.kdehip_device_count())


def version() -> int:
    return int(_clib.kdehip_version())
