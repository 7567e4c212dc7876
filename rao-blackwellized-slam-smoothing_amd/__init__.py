"""MI355X-native Rao-Blackwellized particle filter / smoother (hot path of
manonkok/Rao-Blackwellized-SLAM-smoothing) -- host-side mirror of the reference interface over the
HIP C-ABI library.  The directory name contains hyphens, so import it with

    import importlib; rbpf = importlib.import_module("rao-blackwellized-slam-smoothing_amd")

(or `import rbpf_amd`, a one-line alias module at the repo root).
"""
from ._build import build, LIBPATH                                    # noqa: F401
from ._ffi import (RBPFError, load_library, EXPORTS,                  # noqa: F401
                   RBPF_OK, RBPF_ERR_INVALID_ARG, RBPF_ERR_UNSUPPORTED, RBPF_ERR_HIP, RBPF_ERR_NO_DEVICE,
                   RBPF_ERR_OUT_OF_MEMORY, RBPF_ERR_CHOL_FAILED, RBPF_ERR_STATE, RBPF_ERR_CALLBACK)
from .host import (particleFilter, particleSmoother, particleSmootherInformationForm,   # noqa: F401
                   DenseMagModel, DenseRadioModel, SparseVisualModel, dense_mag_prior, dense_radio_prior,
                   domain_cartesian_dx, eigenval, PhiloxRNG, ReplayRNG, FilterSession, sample, chol_weights, chol_sweep_probe, pack_whiten_probe, sparse_ext_build_probe, sparse_smoother_timing, quat_helper,
                   GenericDenseModel, GenericSparseModel, DeviceHandles, DeviceSmootherHandles, DeviceSparseHandles, DeviceSparseSmootherHandles, particle_filter_external, chol_refresh_in_use,
                   DenseMagMap, DeviceMap, DeviceLandmarkMap, DeviceTransition, device_map_weights, landmark_map_weights, device_map_backward_step, device_map_backward_workspace_bytes, particleFilterLocalization, LocalizationSession, loc_workspace_bytes,
                   particleSmootherLocalization, loc_backward_step, loc_backward_workspace_bytes,
                   particleMapLocalization, loc_map_step, loc_map_workspace_bytes, device_map_map_step, device_map_map_workspace_bytes,
                   particleMarginalSmootherLocalization, loc_marginal_step, loc_marginal_workspace_bytes, device_map_marginal_step,
                   device_map_marginal_workspace_bytes,
                   particleTransitionStatisticsLocalization, loc_pair_stats_step, loc_pair_stats_workspace_bytes, device_map_pair_stats_step,
                   device_map_pair_stats_workspace_bytes, transition_noise_estimate,
                   particleRunningStatisticsLocalization, loc_forward_stats_step, loc_forward_stats_workspace_bytes,
                   device_map_forward_stats_step, device_map_forward_stats_workspace_bytes, running_noise_estimate,
                   particleFixedLagSmootherLocalization, loc_fixed_lag_step, loc_fixed_lag_workspace_bytes, device_map_fixed_lag_step,
                   device_map_fixed_lag_workspace_bytes, fixed_lag_assemble,
                   loc_backward_reject_step, loc_backward_reject_workspace_bytes, device_map_backward_reject_step, reject_default_max_tries)


def device_count() -> int:
    """Visible HIP devices according to the library (0 without a GPU)."""
    return int(load_library().rbpf_device_count())
