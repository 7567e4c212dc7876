#!/usr/bin/env python3
"""What a step of the conditional iteration of particleSmoother(..., sparseFeatures=True) costs when the model is device code
(rbpf.DeviceSparseSmootherHandles, rbpf_particle_smoother_sparse_device), at N_P = 8192:

  (n_y, nLin) = (20, 40)   the pinhole camera of examples/slam-sparse-visual at the example's size, N_T = 40, as torch handles
                           (tests/sparse_models_torch.py) AND as the built-in sparse-visual family, in the same run
  (n_y, nLin) = (32, 96)   range-only beacons in 3-D (tests/sparse_models.py), the largest admitted shape, as torch handles, with
                           N_T = 32: M(1) = 31 x 32 = 992 stacked future observations, just under the 1023 the smoother admits

Every output is observed at every step (the most a step can cost); the vehicle stands still up to its process noise, which the
handles draw with torch.randn; the resampling uniforms come from the device Philox generator.  N_K = 2.

Per run the tool records, as medians of WINDOWS runs after a warm-up run,
  ms_per_step       the host clock between the makePlots hooks of iterations 0 and 1 -- the conditional iteration, whole: handles,
                    replicate / pack, build, factorisation, the steps, the trajectory draw -- over N_T (the hook runs once an
                    iteration's outputs are on the host, particleSmoother.m:360-362; the call's set-up is outside)
  build_ms, chol_ms the build kernel's and the batched factorisation's own time per step of that iteration with future observations:
                    HIP events around every launch (rbpf_sparse_smoother_timing), totals over the N_T - 1 such steps / (N_T - 1)
  build_bound_*     what the sizes allow the build kernel, summed over the same steps: bytes = N_P (M n + n^2 + T16(M)) 8 with
                    T16(M) the elements of the 16 x 16 tiles on and below the diagonal, over the HBM peak; multiply-adds =
                    N_P (M n^2 + T16(M) n) over the fp64 matrix-core peak -- and the M^3 / 6 multiply-adds (M^3 / 3 flops) of the factorisation
                    beside it
No ratio is a criterion of anything: the built-in kernel exploits the camera's two non-zeros per Jacobian row and does about
n / 4 times fewer multiply-adds in its build.  Writes one JSON document (default profiles/sparse_device_smoother_bench.json).

Usage: sparse_device_smoother_bench.py [--out FILE] [--particles 8192] [--windows 5]"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
rbpf = importlib.import_module("rao-blackwellized-slam-smoothing_amd")

HBM_PEAK_GBPS = 8000.0                          # MI355X: HBM3E 8 TB/s (as bench.py)
FP64_MATRIX_PEAK_GFMA = 78600.0 / 2             # 78.6 TFLOP/s on the fp64 matrix cores = 39.3 T multiply-adds per second
N_K = 2


def smoother_args(p, N):
    return (p["odometry"], p["y"], p["x0_nonLin"], p["x0_lin"], p["P0_lin"], p["Q"], p["R"], N, N_K, p["dt"])


def device_handles(torch, smt, p):
    """The torch twin (pure in measModel as it stands: tw._meas) with its normals from the device generator."""
    dev = torch.device("cuda", torch.cuda.current_device())
    tw = smt.twin_of(p["model"], dict(p, rng=types.SimpleNamespace(Z=np.zeros((1, 1, 1, 3)))), dev)

    def dyn(xn, dx, dt, Q):
        return xn + dx.reshape(-1, 1) + tw.Lq[0] @ torch.randn(xn.shape, dtype=torch.float64, device=xn.device)

    torch.cuda.synchronize()
    return rbpf.DeviceSparseSmootherHandles(dyn, tw._meas)


def tiles16(M):
    """Elements of the 16 x 16 tiles on and below the diagonal of an M x M matrix: what the build kernel forms and writes."""
    rt = np.arange(M) // 16
    return int(np.sum(rt[:, None] >= rt[None, :]))


def bounds(N, n, Ms):
    byts = sum(N * (M * n + n * n + tiles16(M)) * 8.0 for M in Ms)
    fma = sum(N * (M * n * n + tiles16(M) * n) * 1.0 for M in Ms)
    chol = sum(N * M ** 3 / 6.0 for M in Ms)              # M^3 / 3 flops: M^3 / 6 multiply-adds
    steps = max(len(Ms), 1)
    return {"build_bytes_per_step": byts / steps, "build_fma_per_step": fma / steps, "chol_fma_per_step": chol / steps,
            "build_bound_hbm_ms": byts / steps / (HBM_PEAK_GBPS * 1e9) * 1e3, "build_bound_fma_ms": fma / steps / (FP64_MATRIX_PEAK_GFMA * 1e9) * 1e3,
            "chol_bound_fma_ms": chol / steps / (FP64_MATRIX_PEAK_GFMA * 1e9) * 1e3}


def measure(run, T, windows, timed):
    ms, build, chol = [], [], []
    for w in range(1 + windows):
        stamps = []
        if timed:
            rbpf.sparse_smoother_timing(True)
        out = run(lambda *_a: stamps.append(time.perf_counter()))
        tm = rbpf.sparse_smoother_timing(False) if timed else None
        assert len(stamps) == N_K and np.all(np.isfinite(out[1])), "the smoother returned a non-finite XLK"
        if w >= 1:
            ms.append((stamps[1] - stamps[0]) / T * 1e3)
            if timed:
                assert tm["steps"] == T - 1, tm
                build.append(tm["build_ms"] / tm["steps"])
                chol.append(tm["chol_ms"] / tm["steps"])
    res = {"ms_per_step": statistics.median(ms), "runs_ms_per_step": ms, "N_T": T}
    if timed:
        res.update(build_ms=statistics.median(build), chol_ms=statistics.median(chol), runs_build_ms=build, runs_chol_ms=chol)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse_device_smoother_bench.json"))
    ap.add_argument("--particles", type=int, default=8192)
    ap.add_argument("--windows", type=int, default=5)
    a = ap.parse_args()
    if a.windows < 3:
        ap.error("at least 3 runs per median")
    if rbpf.device_count() < 1:
        raise SystemExit("sparse_device_smoother_bench: no HIP device visible (nothing is measured without one)")
    import torch
    import rbpf_oracle as oracle
    import sparse_models as sm
    import sparse_models_torch as smt
    import sparse_device_bench as sdb
    N = a.particles
    doc = {"tool": "tools/sparse_device_smoother_bench.py", "device": torch.cuda.get_device_name(0), "N_P": N, "N_K": N_K,
           "timing": f"a warm-up run, then medians of {a.windows} runs; per step = host clock between the makePlots hooks of iterations 0 and 1 "
                     "/ N_T; build_ms / chol_ms = HIP events around every launch of the conditional iteration / (N_T - 1)",
           "hbm_peak_GBps": HBM_PEAK_GBPS, "fp64_matrix_peak_Gfma_per_s": FP64_MATRIX_PEAK_GFMA, "runs": []}
    problems = (("pinhole", sdb.pinhole_problem(oracle, 20, 40), 40), ("range_only_3d", sdb.range_only_problem(sm, 32, 32), 32))
    for name, p, T in problems:
        m = p["model"]
        Ms = [m.ny * (T - t) for t in range(1, T)]
        run = {"model": name, "n_y": m.ny, "nLin": m.nLin, "N_T": T, "M_first": Ms[0], "M_last": Ms[-1]}
        handles = device_handles(torch, smt, p)
        run["device_handles"] = measure(lambda hook: rbpf.particleSmoother(handles, None, None, *smoother_args(p, N), True, makePlots=hook,
                                                                           rng=rbpf.PhiloxRNG(1)), T, a.windows, True)
        run["device_handles"].update(bounds(N, m.nLin, Ms))
        if name == "pinhole":
            mdl = rbpf.SparseVisualModel(m.nLand)
            run["builtin_sparse_visual"] = measure(lambda hook: rbpf.particleSmoother(mdl.dynModel, mdl.measModel, [], *smoother_args(p, N), True,
                                                                                      makePlots=hook, rng=rbpf.PhiloxRNG(1)), T, a.windows, False)
        doc["runs"].append(run)
        print(json.dumps(run), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
