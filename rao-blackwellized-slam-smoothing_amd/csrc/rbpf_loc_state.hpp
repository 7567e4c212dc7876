// State of a localisation context (rbpf_ctx::loc), shared by the filter (rbpf_loc.hip), the backward-simulation smoother
// (rbpf_loc_smooth.hip) and localisation in the map of a generic device-code model (rbpf_loc_generic.hip).
#pragma once
#include "../../include/rbpf.h"
#include "rbpf_devmem.hpp"

namespace rbpf {

struct LocState {
  DevicePool pool;                 // owns the device buffers below; the context-level arrays of a localisation session are in rbpf_ctx::pool
  int n = 0;
  int nN = 7;                      // width of the non-linear state: 7 (pos3 + quat4) in the dense-mag map, the model's in a generic one
  double sigma2 = 0.0;
  double *d_mean = nullptr, *d_V = nullptr, *d_vartab = nullptr, *d_S = nullptr, *d_lse = nullptr, *d_x0 = nullptr;
  int s_pages = 1, x0_cols = 1;
  // generic map (rbpf_loc_generic_create): the caller's handles produce states and Jacobians, the context is driven step by step
  bool generic = false;
  int d = 3;                       // n_y
  int ldx = 0;                     // row stride of the native dy layout
  int drawn_step = -1;             // step whose ancestors rbpf_loc_generic_ancestors_device has drawn
  double *d_R = nullptr;           // [n_y x n_y]
  double *d_H = nullptr;           // [N][n_y][ldx] rows packed from dy layout 0 (allocated on first use)
};

// of rbpf_options a localisation context reads keep_history, trace and on_step only
int loc_validate_options(const rbpf_options* o);

}  // namespace rbpf
