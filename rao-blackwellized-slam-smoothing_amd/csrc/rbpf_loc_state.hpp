// State of a localisation context (rbpf_ctx::loc), shared by the filter (rbpf_loc.hip) and the backward-simulation smoother
// (rbpf_loc_smooth.hip).
#pragma once
#include "rbpf_devmem.hpp"

namespace rbpf {

struct LocState {
  DevicePool pool;                 // owns the device buffers below; the context-level arrays of a localisation session are in rbpf_ctx::pool
  int n = 0;
  double sigma2 = 0.0;
  double *d_mean = nullptr, *d_V = nullptr, *d_vartab = nullptr, *d_S = nullptr, *d_lse = nullptr, *d_x0 = nullptr;
  int s_pages = 1, x0_cols = 1;
};

}  // namespace rbpf
