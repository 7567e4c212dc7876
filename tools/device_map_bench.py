#!/usr/bin/env python3
"""What localisation in the fixed map of a generic device-code model (rbpf.DeviceMap) costs on one MI355X: the fused weight
kernel alone and the whole step, next to the plain torch evaluation of the same weights and to the SLAM filter step of the same
handles and shape.

The model is the synthetic family of tests/generic_model.py restated in torch (tests/generic_model_torch.py), its dynModel drawing
normals from the device generator; the map is mean = x0_lin + noise, V a random lower factor (tests/device_map_ref.case's scaling).

Per shape (N_P, n_y, nLin) the tool records
  kernel         rbpf_loc_generic_weights on the Jacobians measModel returns at N_P random states: device events around every
                 launch, ROUNDS rounds of REPS launches after a warm-up round, the median of the round medians; ALTERNATING with
  torch          H @ V.T, the Gram blocks, + R, torch.linalg.cholesky, the triangular solve and the log-weight on the same device
                 tensors, device events around every evaluation, the same rounds;
  step           LocalizationSession(DeviceMap) driven by the handles: warm-up, then WINDOWS windows of STEPS steps, each a host
                 clock around work that ends in a synchronise (handles + weight kernel + normalisation + resampling);
  slam_step      FilterSession(DeviceHandles) of the same handles and shape, the same windows (n_y 1 and 3: block-lower fp64
                 storage and lazy_depth 4, the other widths fp64 squares rewritten every step -- the schedules
                 tools/generic_device_bench.py measures); "not measured" when its covariance banks do not fit the device.
From the shapes: the useful flop, N_P n_y nLin (nLin + 1) for Y = V H' on the lower triangle plus N_P nLin n_y (n_y + 1) for the
Gram blocks, over the kernel time and against the 78.6 TF fp64 matrix peak; the bytes of H, N_P n_y nLin 8, over the kernel time
against 8 TB/s (the kernel re-reads the chunks once per 128-row super-block: h_reads_issued says how often); which of the two
bounds the kernel; and the share of the issued MFMA columns that are padding: 1 - N_P n_y / (16 * column tiles issued).

Usage: device_map_bench.py [--out FILE] [--shapes N,ny,n ...] [--rounds 3] [--reps 7] [--windows 5] [--steps 20] [--no-slam]"""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
rbpf = importlib.import_module("rao-blackwellized-slam-smoothing_amd")
host = importlib.import_module("rao-blackwellized-slam-smoothing_amd.host")
_ffi = importlib.import_module("rao-blackwellized-slam-smoothing_amd._ffi")

SHAPES = [(65536, 3, 515), (65536, 1, 128), (65536, 3, 1003), (8192, 3, 256), (8192, 4, 256), (8192, 8, 256)]
FP64_MATRIX_PEAK = 78.6e12
HBM_PEAK = 8.0e12
COLUMN_TILES_PER_WORKGROUP = 8                  # kLgCT of csrc/rbpf_loc_generic.hip


def shape_figures(N, d, n):
    ppt = 16 // d
    tiles = -(-N // (COLUMN_TILES_PER_WORKGROUP * ppt)) * COLUMN_TILES_PER_WORKGROUP
    nsb = -(-n // 128)
    issued = sum(min(n, 128 * (sb + 1)) for sb in range(nsb)) / n
    return {"useful_flop": float(N) * d * n * (n + 1) + float(N) * n * d * (d + 1), "h_bytes": float(N) * d * n * 8,
            "h_reads_issued": issued, "padded_mfma_column_share": 1.0 - float(N) * d / (16.0 * tiles),
            "particles_per_column_tile": ppt}


def handles(torch, gmt, m, p):
    class Model(gmt.TorchGenericModel):
        def dynModel(self, xn, dx, dt, Q):
            z = torch.randn((self.G.shape[1], xn.shape[1]), dtype=torch.float64, device=xn.device)
            return xn + self.bend * torch.sin(xn) + (self.A @ dx.reshape(-1, 1)) + self.G @ (self.Lq[0] @ z)

    tm = Model(m, p, torch.device("cuda", torch.cuda.current_device()))
    torch.cuda.synchronize()
    return tm, rbpf.DeviceHandles(tm.dynModel, tm.measModel)


def windows_ms(advance, sync, warmup, windows, steps):
    advance(warmup)
    sync()
    ms = []
    for _ in range(windows):
        t0 = time.perf_counter()
        advance(steps)
        sync()
        ms.append((time.perf_counter() - t0) / steps * 1e3)
    return {"ms_per_step": statistics.median(ms), "windows_ms": ms}


def torch_weights(torch, dy, Vt, mean, R, y):
    N, d, n = dy.shape
    Y = (dy.reshape(N * d, n) @ Vt).reshape(N, d, n)
    S = Y @ Y.transpose(1, 2) + R
    e = y - dy @ mean
    L = torch.linalg.cholesky(S)
    z = torch.linalg.solve_triangular(L, e.unsqueeze(-1), upper=False).squeeze(-1)
    return -torch.log(torch.diagonal(L, dim1=1, dim2=2)).sum(1) - 0.5 * (z * z).sum(1) - 0.5 * d * np.log(2 * np.pi)


def bench_kernel(torch, tm, p, N, a):
    """The fused kernel and the torch evaluation on the same Jacobians, in alternating rounds."""
    dev = tm.device
    gen = torch.Generator(device=dev).manual_seed(3)
    xn = torch.as_tensor(np.asarray(p["x0_nonLin"]), device=dev).reshape(-1, 1) + 0.3 * torch.randn((tm.A.shape[0], N), dtype=torch.float64, device=dev, generator=gen)
    dy = tm.measModel(xn).contiguous()
    f = dict(dtype=torch.float64, device=dev)
    Vt, mean, R, y = (torch.as_tensor(np.ascontiguousarray(x), **f) for x in (p["V"].T, p["mean"], p["R"], p["y"][0]))
    dy_host = dy.cpu().numpy()
    kernel, torch_ms, logw = [], [], None
    for r in range(a.rounds + 1):                                     # round 0 warms both up
        _, _, logw, ms = rbpf.device_map_weights(dy_host, p["mean"], p["V"], p["R"], p["y"][0], reps=a.reps)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.reps)]
        for e0, e1 in ev:
            e0.record()
            lw = torch_weights(torch, dy, Vt, mean, R, y)
            e1.record()
        torch.cuda.synchronize()
        if r:
            kernel.append(ms)
            torch_ms.append(statistics.median(e0.elapsed_time(e1) for e0, e1 in ev))
    diff = float(np.max(np.abs(lw.cpu().numpy() - logw)) / np.max(np.abs(logw)))
    return {"kernel_ms": statistics.median(kernel), "kernel_round_medians_ms": kernel, "torch_ms": statistics.median(torch_ms),
            "torch_round_medians_ms": torch_ms, "launches_each": a.rounds * a.reps, "logw_rel_distance_kernel_torch": diff}


def bench_step(mp, p, N, a):
    with rbpf.LocalizationSession(mp, p["odometry"], p["y"], p["x0_nonLin"], p["Q"], N, p["dt"], rng=rbpf.PhiloxRNG(1)) as s:
        return windows_ms(s.advance, s.sync, a.warmup, a.windows, a.steps)


def bench_slam(torch, h, m, p, N, a):
    opts = dict(storage="fp64sym", lazy_depth=4) if m.ny in (1, 3) else dict(storage="fp64", lazy_depth=0)
    args = (p["odometry"], p["y"], p["x0_nonLin"], p["x0_lin"], p["P0_lin"], p["Q"], p["R"], N, p["dt"])
    model = host._generic_model(None, None, None, *args[:4], p["Q"], p["dt"])
    prob = host._Problem(model, *args)
    need = C.c_size_t(0)
    opt = _ffi.rbpf_options(storage=host._storage_code(opts["storage"]), lazy_depth=opts["lazy_depth"])
    mdesc = model.descriptor()
    host.check(rbpf.load_library().rbpf_filter_workspace_bytes(C.byref(mdesc), C.byref(prob.c), C.byref(opt), C.byref(need)))
    free, _ = torch.cuda.mem_get_info()
    if need.value > 0.9 * free:
        return {"ms_per_step": "not measured", "reason": f"the SLAM filter's banks need {need.value / 1e9:.0f} GB, {free / 1e9:.0f} GB are free", "options": opts}
    with rbpf.FilterSession(h, *args, rng=rbpf.PhiloxRNG(1), **opts) as s:
        return dict(windows_ms(s.advance, s.sync, a.warmup, a.windows, a.steps), options=opts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_map_bench.json"))
    ap.add_argument("--shapes", nargs="*", default=None, help="N_P,n_y,nLin triples; default: the six shapes of DESIGN.md section 4")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--no-slam", action="store_true", help="skip the SLAM filter step (recorded as not measured)")
    a = ap.parse_args()
    if a.rounds * a.reps < 20 or a.windows < 5:
        ap.error("at least 20 timed launches (rounds x reps) and 5 windows")
    if rbpf.device_count() < 1:
        raise SystemExit("device_map_bench: no HIP device visible (nothing is measured without one)")
    import torch
    import device_map_ref as dm
    import generic_model_torch as gmt
    shapes = [tuple(int(v) for v in s.split(",")) for s in a.shapes] if a.shapes else SHAPES
    T = a.warmup + a.windows * a.steps + 4
    doc = {"tool": "tools/device_map_bench.py", "device": torch.cuda.get_device_name(0),
           "fp64_matrix_peak_TF": FP64_MATRIX_PEAK / 1e12, "hbm_peak_TBps": HBM_PEAK / 1e12,
           "timing": f"kernel and torch: device events, a warm-up round, then {a.rounds} alternating rounds of {a.reps} launches, median of the round "
                     f"medians; steps: warm-up {a.warmup}, median of {a.windows} windows of {a.steps} steps (host clock, each window ends in a synchronise)",
           "runs": []}
    for N, d, n in shapes:
        m, p = dm.case((4, 3, 4, d, n), 1, T, seed=1)
        tm, h = handles(torch, gmt, m, p)
        mp = rbpf.DeviceMap(h, p["mean"], p["V"], p["R"])
        run = dict(N_P=N, n_y=d, nLin=n, **shape_figures(N, d, n))
        run.update(bench_kernel(torch, tm, p, N, a))
        t = run["kernel_ms"] * 1e-3
        run["kernel_TFLOPs"] = run["useful_flop"] / t / 1e12
        run["share_of_fp64_matrix_peak"] = run["useful_flop"] / t / FP64_MATRIX_PEAK
        run["h_TBps"] = run["h_bytes"] / t / 1e12
        run["share_of_hbm_peak"] = run["h_bytes"] / t / HBM_PEAK
        run["bound"] = "fp64 matrix peak" if run["useful_flop"] / FP64_MATRIX_PEAK >= run["h_bytes"] / HBM_PEAK else "HBM bandwidth"
        run["least_time_ms"] = max(run["useful_flop"] / FP64_MATRIX_PEAK, run["h_bytes"] / HBM_PEAK) * 1e3
        run["torch_over_kernel"] = run["torch_ms"] / run["kernel_ms"]
        run["step"] = bench_step(mp, p, N, a)
        run["slam_step"] = {"ms_per_step": "not measured", "reason": "--no-slam"} if a.no_slam else bench_slam(torch, h, m, p, N, a)
        doc["runs"].append(run)
        print(json.dumps(run), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
        del tm, h, mp
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
