"""Drop-in alias of the reference module of the same name (gibbs/hybrid_gaussian_mrf.py): re-exports the
enumeration half from lhvi.exact and the block Gibbs sampler from lhvi.gibbs (with ``fit_scalar_gms_from_samples``, the batched
device sibling of ``sampling_utils.fit_scalar_gm_from_samples``)."""
from lhvi.exact import (convert_to_bn, get_crv_marg, get_drv_marg, get_drv_marg_map,  # noqa: F401
                        get_rv_marg_map_from_bn_params)
from lhvi.gibbs import HybridGaussianSampler, block_gibbs_sample, fit_scalar_gms_from_samples  # noqa: F401
