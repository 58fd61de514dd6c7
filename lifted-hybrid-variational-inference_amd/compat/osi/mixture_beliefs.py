"""Drop-in alias of the NumPy half of the reference's ``osi/mixture_beliefs.py`` (:505-867): re-exports
lhvi.mixture.  The symbolic (TensorFlow) half is not provided (docs/widened_rows.md)."""
from lhvi.mixture import (MixtureBelief, _calc_marg_comp_log_prob, calc_cond_mixture_weights,  # noqa: F401
                          calc_marg_comp_log_prob, calc_marg_log_prob, crv_belief_map, drv_belief_map,
                          eval_crvs_comp_log_prob, eval_drvs_comp_prob, get_obs_rvs_domain_types_and_params, joint_map,
                          joint_map_from_belief_params, marginal_map)
