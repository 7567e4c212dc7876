// Full-square step kernels of the generic family at n_y = 4 and n_y = 7 (see launch_step_wide_t in rbpf_step_full.hpp).  gfx950 only.
#include "rbpf_step_full.hpp"

namespace rbpf {

hipError_t launch_step_wide_d4(const StepArgs& a, hipStream_t s) { return launch_step_wide_t<4>(a, s); }
hipError_t launch_step_wide_d7(const StepArgs& a, hipStream_t s) { return launch_step_wide_t<7>(a, s); }

}  // namespace rbpf
