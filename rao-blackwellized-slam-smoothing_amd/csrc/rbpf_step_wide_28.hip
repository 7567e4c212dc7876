// Full-square step kernels of the generic family at n_y = 2 and n_y = 8 (see launch_step_wide_t in rbpf_step_full.hpp).  gfx950 only.
#include "rbpf_step_full.hpp"

namespace rbpf {

hipError_t launch_step_wide_d2(const StepArgs& a, hipStream_t s) { return launch_step_wide_t<2>(a, s); }
hipError_t launch_step_wide_d8(const StepArgs& a, hipStream_t s) { return launch_step_wide_t<8>(a, s); }

}  // namespace rbpf
