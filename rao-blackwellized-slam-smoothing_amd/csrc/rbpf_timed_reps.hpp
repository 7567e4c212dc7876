// The timed repetitions of the kernel-level probes (rbpf_loc_predict, rbpf_loc_generic_weights, rbpf_loc_landmark_weights,
// rbpf_loc_backward_step, rbpf_loc_generic_backward_pose_step).
#pragma once
#include "rbpf_ctx.hpp"

#include <algorithm>
#include <vector>

namespace rbpf {

// launch() (a hipError_t) max(reps, 1) times in stream s, an event pair around each; waits for the stream; *ms (if not null) <-
// the median of the pairs' times.  The events are destroyed whichever way it returns.
template <class F>
int timed_reps(int reps, hipStream_t s, F&& launch, double* ms) {
  std::vector<hipEvent_t> ev;
  struct Destroy {
    std::vector<hipEvent_t>& ev;
    ~Destroy() { for (hipEvent_t e : ev) hipEventDestroy(e); }
  } destroy{ev};
  const int R = std::max(reps, 1);
  ev.reserve((size_t)2 * R);
  for (int r = 0; r < R; ++r) {
    for (int k = 0; k < 2; ++k) {
      hipEvent_t e;
      HIPCHK(hipEventCreate(&e));
      ev.push_back(e);
    }
    HIPCHK(hipEventRecord(ev[2 * r], s));
    HIPCHK(launch());
    HIPCHK(hipEventRecord(ev[2 * r + 1], s));
  }
  HIPCHK(hipStreamSynchronize(s));
  if (ms) {
    std::vector<float> tt;
    for (int r = 0; r < R; ++r) { float v = 0.f; HIPCHK(hipEventElapsedTime(&v, ev[2 * r], ev[2 * r + 1])); tt.push_back(v); }
    std::sort(tt.begin(), tt.end());
    *ms = tt[tt.size() / 2];
  }
  return RBPF_OK;
}

}  // namespace rbpf
