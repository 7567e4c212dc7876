#!/usr/bin/env python3
"""What a step of the information-form smoother costs for a generic model whose handles are device code
(rbpf.DeviceSmootherHandles) against the host-callback path and against the built-in dense-mag family: n_y = 3, nLin = 515
(m = 512), N_P = 8192, N_K = 2, block-lower fp64 storage, lazy_depth 3, a short horizon.

The model is the synthetic family of tests/generic_model.py, restated in torch for the device
(tests/generic_model_torch_smoother.py, its dynModel drawing normals from the device generator) and evaluated with numpy on the
host for the host-callback path; the resampling uniforms come from the device Philox generator.

It times four things
  host_callback          the handles on the host, chol_refresh = 1, with fewer steps (they run per particle in Python and the
                         Jacobians cross PCIe every step)
  device_chol_refresh_1  device handles, chol(Imat_i + ImatAddt) from scratch at every step
  device_chol_refresh_32 device handles, carried factors refreshed every 32nd step from information matrices rebuilt through
                         the device measModel: none is stored or copied between the refreshes
  builtin_dense_mag      the recognised family at the same sizes, chol_refresh = 32
The smoothers are one-shot calls, so the clock sits in the makePlots hook, which the library calls after every iteration
once that iteration's outputs are on the host (particleSmoother.m:360-362): the host clock between the hook of iteration 0 and
the hook of iteration 1 is the whole conditional iteration -- measModel along the reference trajectory, N_T steps with their
ancestor weights (with chol_refresh = 32 and N_T = 40: refreshes at t = 1 and t = 33), the trajectory draw and the download of
its outputs -- and nothing of the call's set-up, which allocates tens of GB and varies by more than an iteration takes.
Per step = that time over N_T.  A warm-up run first, then the median of --windows runs.  No ratio between the four is a
criterion of anything: the partners are different code.

Writes one JSON document (default profiles/generic_device_smoother_bench.json).

Usage: generic_device_smoother_bench.py [--out FILE] [--particles 8192] [--windows 5] [--steps 40] [--host-steps 4]

--ny 3 4 8: the measurement-width sweep instead -- per n_y the device handles alone, chol_refresh = 1, on fp64 full squares
rewritten every step (what every n_y from 1 to 8 has), nLin = --ny-nlin (256).  Default output
profiles/generic_device_smoother_ny_bench.json."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
rbpf = importlib.import_module("rao-blackwellized-slam-smoothing_amd")
dg = importlib.import_module("rao-blackwellized-slam-smoothing_amd.datagen")

SHAPE = (4, 3, 4, 3, 515)                       # (n_nonlin, n_w, n_odo, n_y, nLin)
OPTS = dict(storage="fp64sym", lazy_depth=3)
NY_OPTS = dict(storage="fp64", lazy_depth=0)    # the --ny sweep
N_K = 2


def per_step(run, T, windows, warmup=1):
    """run(T, makePlots) -> one smoother call over T steps.  Median over the windows of the conditional iteration's time per
    step [ms]."""
    ms = []
    for w in range(warmup + windows):
        stamps = []
        out = run(T, lambda *_a: stamps.append(time.perf_counter()))
        assert len(stamps) == N_K and np.all(np.isfinite(out[1])), "the smoother returned a non-finite XLK"
        if w >= warmup:
            ms.append((stamps[1] - stamps[0]) / T * 1e3)
    return {"ms_per_step": statistics.median(ms), "windows_ms": ms, "N_T": T}


def generic_args(p, N, T):
    return (p["odometry"][:T - 1], p["y"][:T], p["x0_nonLin"], p["x0_lin"], p["P0_lin"], p["Q"], p["R"], N, N_K, p["dt"])


def device_handles(torch, gms, m, p):
    dev = torch.device("cuda", torch.cuda.current_device())

    class Model(gms.TorchSmootherModel):
        def dynModel(self, xn, dx, dt, Q):
            self.calls += 1
            z = torch.randn((self.G.shape[1], xn.shape[1]), dtype=torch.float64, device=xn.device)
            return self.drift(xn, dx) + self.G @ (self.Lq[0] @ z)

        def measModel(self, xn):
            arg = (self.omega @ xn).t()
            return self.c[None] * torch.cos(arg[:, None, :] + self.phi[None])

        def dynResNorm(self, xnk_t, xn, dx, dt, Q):
            r = self.Gpinv @ (xnk_t.reshape(-1, 1) - self.drift(xn, dx))
            return torch.linalg.solve_triangular(self.Lq[0], r, upper=False)

    tm = Model(m, p, dev)
    torch.cuda.synchronize()
    return rbpf.DeviceSmootherHandles(tm.dynModel, tm.measModel, tm.dynResNorm, dy_layout=2)


def bench_device(torch, gms, m, p, N, chol_refresh, a, opts=OPTS):
    handles = device_handles(torch, gms, m, p)

    def run(T, hook):
        return rbpf.particleSmootherInformationForm(handles, None, None, *generic_args(p, N, T), makePlots=hook, rng=rbpf.PhiloxRNG(1),
                                                    chol_refresh=chol_refresh, **opts)
    return per_step(run, a.steps, a.windows)


def bench_host(m, p, N, a):
    rs = np.random.RandomState(5)
    dyn = lambda xn, dx, dt, Q: m.dynModel(xn, dx, dt, Q, rs.standard_normal(m.nw))[0]          # noqa: E731

    def run(T, hook):
        return rbpf.particleSmootherInformationForm(dyn, m.measModel, m.dynResNorm, *generic_args(p, N, T), makePlots=hook,
                                                    rng=rbpf.PhiloxRNG(1), chol_refresh=1, **OPTS)
    return per_step(run, a.host_steps, 1, warmup=0)                    # one run, no warm-up: seconds per step


def bench_builtin(N, a):
    th = [650.0, 1.2, 200.0, 10.0]                                   # examples/slam-dense-mag/main.m:22-23, as bench.py
    Q = np.diag(np.concatenate((10 ** 2 * np.array([0.05 ** 2, 0.05 ** 2, 0.01 ** 2]), (np.array([0.01, 0.01, 0.3]) * np.pi / 180) ** 2)))
    d = dg.bean_6D(a.steps, Q, th, 0.01, seed=1)
    mdl, x0, P0, R = rbpf.dense_mag_prior(512, d["LL"], th)

    def run(T, hook):
        return rbpf.particleSmootherInformationForm(mdl.dynModel, mdl.measModel, mdl.dynResNorm, d["dx"][:T - 1], d["y"][:T], d["initState"],
                                                    x0, P0, Q, R, N, N_K, 0.01, makePlots=hook, rng=rbpf.PhiloxRNG(1), chol_refresh=32,
                                                    **OPTS)
    return per_step(run, a.steps, a.windows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default: profiles/generic_device_smoother_bench.json (--ny: ..._smoother_ny_bench.json)")
    ap.add_argument("--ny", type=int, nargs="+", default=None, help="measurement widths of the n_y sweep (1 .. 8); replaces the default runs")
    ap.add_argument("--ny-nlin", type=int, default=256)
    ap.add_argument("--particles", type=int, default=8192)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--host-steps", type=int, default=4)
    ap.add_argument("--skip-host", action="store_true")
    a = ap.parse_args()
    if a.windows < 3 or a.steps < 34 or a.host_steps < 3:
        ap.error("at least 3 windows, --steps at least 34 (a refresh of chol_refresh = 32 after the first), --host-steps at least 3")
    if rbpf.device_count() < 1:
        raise SystemExit("generic_device_smoother_bench: no HIP device visible (nothing is measured without one)")
    import torch
    import generic_model as gm
    import generic_model_torch_smoother as gms
    N = a.particles
    free, _total = torch.cuda.mem_get_info()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "generic_device_smoother_ny_bench.json" if a.ny else "generic_device_smoother_bench.json")
    if a.ny:
        doc = {"tool": "tools/generic_device_smoother_bench.py --ny", "device": torch.cuda.get_device_name(0), "N_P": N, "N_K": N_K,
               "nLin": a.ny_nlin, "options": dict(NY_OPTS, chol_refresh=1), "form": "information form, DeviceSmootherHandles, dy layout 2",
               "timing": f"per step = host clock between the makePlots hooks of iterations 0 and 1 / N_T; N_T = {a.steps}, a warm-up run, "
                         f"then the median of {a.windows} runs", "runs": []}
        for ny in a.ny:
            m = gm.GenericModel(4, 3, 4, ny, a.ny_nlin, seed=1)
            p = gm.problem(m, 1, a.steps, N_K=N_K, seed=1)
            doc["runs"].append(dict(bench_device(torch, gms, m, p, N, 1, a, NY_OPTS), n_y=ny))
            print(json.dumps(doc["runs"][-1]), flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(doc, f, indent=1)
                f.write("\n")
        return
    m = gm.GenericModel(*SHAPE, seed=1)
    p = gm.problem(m, 1, a.steps, N_K=N_K, seed=1)
    doc = {"tool": "tools/generic_device_smoother_bench.py", "device": torch.cuda.get_device_name(0), "free_bytes_at_start": free,
           "shape": dict(zip(("n_nonlin", "n_w", "n_odo", "n_y", "nLin"), SHAPE)), "N_P": N, "N_K": N_K, "options": OPTS,
           "timing": f"per step = host clock between the makePlots hooks of iterations 0 and 1 (the conditional iteration, whole) / N_T; "
                     f"N_T = {a.steps}, a warm-up run, then the median of {a.windows} runs; the host-callback path: one run of N_T = {a.host_steps}",
           "runs": {}}

    def record(name, fn):
        doc["runs"][name] = fn()
        print(json.dumps({name: doc["runs"][name]}), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")

    record("builtin_dense_mag_chol_refresh_32", lambda: bench_builtin(N, a))
    record("device_chol_refresh_32", lambda: bench_device(torch, gms, m, p, N, 32, a))
    record("device_chol_refresh_1", lambda: bench_device(torch, gms, m, p, N, 1, a))
    if not a.skip_host:
        record("host_callback_chol_refresh_1", lambda: bench_host(m, p, N, a))


if __name__ == "__main__":
    main()
