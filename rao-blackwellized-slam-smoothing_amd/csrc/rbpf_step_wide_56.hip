// Full-square step kernels of the generic family at n_y = 5 and n_y = 6 (see launch_step_wide_t in rbpf_step_full.hpp).  gfx950 only.
#include "rbpf_step_full.hpp"

namespace rbpf {

hipError_t launch_step_wide_d5(const StepArgs& a, hipStream_t s) { return launch_step_wide_t<5>(a, s); }
hipError_t launch_step_wide_d6(const StepArgs& a, hipStream_t s) { return launch_step_wide_t<6>(a, s); }

}  // namespace rbpf
