"""Drop-in alias of the reference module of the same name (gibbs/hybrid_gaussian_mrf.py): re-exports the
enumeration half from lhvi.exact and the block Gibbs sampler from lhvi.gibbs (with ``fit_scalar_gms_from_samples``, the batched
device sibling of ``sampling_utils.fit_scalar_gm_from_samples``, and ``ais_log_partition`` / ``HybridGaussianSampler.log_partition``,
the annealed importance sampling estimate of ``log Z`` that fills the ``obj`` column of the Gibbs baseline, and
``tempered_gibbs_sample`` / ``HybridGaussianSampler.tempered_gibbs_sample``, the sampler run as ladders of replicas that exchange
their discrete states)."""
from lhvi.exact import (convert_to_bn, get_crv_marg, get_drv_marg, get_drv_marg_map,  # noqa: F401
                        get_rv_marg_map_from_bn_params)
from lhvi.gibbs import (HybridGaussianSampler, ais_log_partition, block_gibbs_sample,  # noqa: F401
                        fit_scalar_gms_from_samples, tempered_gibbs_sample)
