#!/usr/bin/env python3
"""What the generic model family costs per step when its handles are device code (rbpf.DeviceHandles) against the
host-callback path and against the built-in dense-mag family, at the headline's sizes: n_y = 3, nLin = 515 (m = 512),
block-lower fp64 storage, lazy_depth 4; N_P = 8192 and the largest N_P that fits the device (65 536 on a free 288 GB GPU).

The model is the synthetic family of tests/generic_model.py, restated in torch for the device (tests/generic_model_torch.py)
and evaluated with numpy on the host for the host-callback path; its dynModel draws its own normals, the resampling uniforms
come from the device Philox generator.

Per N_P the tool records
  host_callback_ms_per_step    few steps: the handles run per particle in Python and 0.8 GB of Jacobians cross PCIe at N_P = 65 536
  device_ms_per_step[layout]   DeviceHandles whose measModel returns MATLAB-order strides (0), fills the native view (1) or
                               returns a C-contiguous tensor (2): handles + pack + step
  builtin_dense_mag_ms_per_step the recognised family at the same N_P, m = 512, same storage and lazy_depth
  pack                         the pack kernels' own launch time (a child run of rbpf_filter_step_device on fixed device inputs
                               under rocprofv3 --kernel-trace --stats) over their bytes N_P n_y (nLin + ldx) 8, next to a
                               device-to-device copy of N_P n_y nLin doubles (read + write: twice that many bytes) timed in
                               the same run of the tool
Timing: a warm-up, then the median of WINDOWS windows of STEPS steps, each window a host clock around work that ends in a
synchronise.  Writes one JSON document (default profiles/generic_device_bench.json).

Usage: generic_device_bench.py [--out FILE] [--particles N ...] [--windows 5] [--steps 20] [--host-steps 2]

--ny 3 4 6 8: the measurement-width sweep instead -- per n_y a DeviceHandles filter (native view filled in place) on fp64 full
squares rewritten every step (lazy_depth 0: what every n_y from 1 to 8 has), at --ny-particles (8192) and --ny-nlin (256);
records the ms per step, the bytes a step must move, N_P (2 nLin^2 + (5 n_y + 2) ldx) 8 (the covariance read and written, H
read, both pending factor pairs read and written, the mean read and written), and that traffic's share of the HBM peak.
Default output profiles/generic_device_ny_bench.json."""
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
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
rbpf = importlib.import_module("rao-blackwellized-slam-smoothing_amd")
dg = importlib.import_module("rao-blackwellized-slam-smoothing_amd.datagen")
host = importlib.import_module("rao-blackwellized-slam-smoothing_amd.host")

SHAPE = (4, 3, 4, 3, 515)                       # (n_nonlin, n_w, n_odo, n_y, nLin)
OPTS = dict(storage="fp64sym", lazy_depth=4)
NY_OPTS = dict(storage="fp64", lazy_depth=0)    # the --ny sweep: the schedule every width has
HBM_PEAK_GBPS = 8000.0                          # MI355X: HBM3E 8 TB/s (as bench.py)


def median_ms_per_step(advance, sync, warmup, windows, steps):
    advance(warmup)
    sync()
    ms = []
    for _ in range(windows):
        t0 = time.perf_counter()
        advance(steps)
        sync()
        ms.append((time.perf_counter() - t0) / steps * 1e3)
    return statistics.median(ms), ms


def filter_args(p, N):
    return (p["odometry"], p["y"], p["x0_nonLin"], p["x0_lin"], p["P0_lin"], p["Q"], p["R"], N, p["dt"])


def device_handles(torch, gmt, m, p, layout):
    """The torch restatement with normals from the device generator, returning dy in the strides of `layout`."""
    dev = torch.device("cuda", torch.cuda.current_device())

    class Model(gmt.TorchGenericModel):
        def dynModel(self, xn, dx, dt, Q):
            z = torch.randn((self.G.shape[1], xn.shape[1]), dtype=torch.float64, device=xn.device)
            return xn + self.bend * torch.sin(xn) + (self.A @ dx.reshape(-1, 1)) + self.G @ (self.Lq[0] @ z)

        def measModel(self, xn, out=None):
            arg = (self.omega @ xn).t()
            if out is not None:
                return torch.mul(self.c[None], torch.cos(arg[:, None, :] + self.phi[None]), out=out)
            dy = self.c[None] * torch.cos(arg[:, None, :] + self.phi[None])
            return dy.permute(2, 1, 0).contiguous().permute(2, 1, 0) if layout == 0 else dy

    tm = Model(m, p, dev)
    torch.cuda.synchronize()
    return rbpf.DeviceHandles(tm.dynModel, tm.measModel, native_out=(layout == 1))


def bench_device(torch, gmt, m, p, N, layout, a, opts=OPTS):
    with rbpf.FilterSession(device_handles(torch, gmt, m, p, layout), *filter_args(p, N), rng=rbpf.PhiloxRNG(1), **opts) as s:
        med, ms = median_ms_per_step(s.advance, s.sync, a.warmup, a.windows, a.steps)
    return {"ms_per_step": med, "windows_ms": ms}


def bench_host(m, p, N, a):
    rs = np.random.RandomState(5)
    dyn = lambda xn, dx, dt, Q: m.dynModel(xn, dx, dt, Q, rs.standard_normal(m.nw))[0]          # noqa: E731
    model = host._generic_model(dyn, m.measModel, None, *filter_args(p, N)[:4], p["Q"], p["dt"])
    with rbpf.FilterSession(model, *filter_args(p, N), rng=rbpf.PhiloxRNG(1), **OPTS) as s:
        s.advance(2)                                                 # t = 0 has no dynModel: warm up past it
        s.sync()
        t0 = time.perf_counter()
        s.advance(a.host_steps)
        s.sync()
        return {"ms_per_step": (time.perf_counter() - t0) / a.host_steps * 1e3, "steps": a.host_steps}


def bench_builtin(N, T, a):
    th = [650.0, 1.2, 200.0, 10.0]                                   # examples/slam-dense-mag/main.m:22-23, as bench.py
    Q = np.diag(np.concatenate((10 ** 2 * np.array([0.05 ** 2, 0.05 ** 2, 0.01 ** 2]), (np.array([0.01, 0.01, 0.3]) * np.pi / 180) ** 2)))
    d = dg.bean_6D(T, Q, th, 0.01, seed=1)
    mdl, x0, P0, R = rbpf.dense_mag_prior(512, d["LL"], th)
    with rbpf.FilterSession(mdl, d["dx"], d["y"], d["initState"], x0, P0, Q, R, N, 0.01, rng=rbpf.PhiloxRNG(1), **OPTS) as s:
        med, ms = median_ms_per_step(s.advance, s.sync, a.warmup, a.windows, a.steps)
    return {"ms_per_step": med, "windows_ms": ms}


def _fixed_inputs(torch, s, m, p, N):
    """A caller-driven context's stream and fixed device inputs in every dy layout (no handle runs)."""
    lib = rbpf.load_library()
    nN, d, n = m.nNonLin, m.ny, m.nLin
    dev = torch.device("cuda", torch.cuda.current_device())
    ldx = C.c_int32(0)
    host.check(lib.rbpf_filter_external_layout(s.ctx, C.byref(ldx)))
    sp = C.c_void_p()
    host.check(lib.rbpf_stream_get(s.ctx, C.byref(sp)))
    stream = torch.cuda.ExternalStream(sp.value, device=dev)
    gen = torch.Generator(device=dev).manual_seed(3)
    xn = torch.as_tensor(np.asarray(p["x0_nonLin"]), device=dev).repeat(N, 1) + 0.01 * torch.randn((N, nN), dtype=torch.float64, device=dev, generator=gen)
    dy = torch.randn((N, d, n), dtype=torch.float64, device=dev, generator=gen) / np.sqrt(n)
    bufs = {2: dy, 0: dy.permute(2, 1, 0).contiguous()}
    torch.cuda.synchronize()
    return lib, ldx.value, stream, xn, bufs


def pack_child(N, steps):
    """Child process of bench_pack, run under rocprofv3 --kernel-trace: `steps` steps through rbpf_filter_step_device in
    layout 0, then in layout 2, on fixed inputs (the pack kernels' time does not depend on the data)."""
    import torch
    import generic_model as gm
    m = gm.GenericModel(*SHAPE, seed=1)
    p = gm.problem(m, 1, 2 * steps + 2, seed=1)
    model = rbpf.GenericDenseModel(m.nNonLin, m.nLin, m.ny, m.nw, m.n_odo)
    with rbpf.FilterSession(model, *filter_args(p, N), rng=rbpf.PhiloxRNG(1), **OPTS) as s:
        lib, _ldx, _stream, xn, bufs = _fixed_inputs(torch, s, m, p, N)
        for layout in (0, 2):
            for _ in range(steps):
                host.check(lib.rbpf_filter_step_device(s.ctx, C.c_void_p(xn.data_ptr()), C.c_void_p(bufs[layout].data_ptr()), layout))
        s.sync()


def bench_pack(torch, m, p, N, a):
    """The pack kernels' own time (rocprofv3 --kernel-trace --stats over a child run of this tool: mean launch time of
    ext_pack_dy_matlab_kernel, layout 0, and ext_pack_dy_rows_kernel, layout 2) against the bytes they move, N_P n_y (nLin + ldx) 8,
    and a device-to-device copy of the same Jacobians on the library's stream in this process (host clock, synchronised)."""
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile
    d, n = m.ny, m.nLin
    model = rbpf.GenericDenseModel(m.nNonLin, n, d, m.nw, m.n_odo)
    with rbpf.FilterSession(model, *filter_args(p, N), rng=rbpf.PhiloxRNG(1), **OPTS) as s:
        _lib, ldx, stream, _xn, bufs = _fixed_inputs(torch, s, m, p, N)
        dst = torch.empty_like(bufs[2])

        def copies(k):
            with torch.cuda.stream(stream):
                for _ in range(10 * k):
                    dst.copy_(bufs[2])
        copy_ms, copy_windows = median_ms_per_step(copies, s.sync, 4, a.windows, a.steps)
    copy_ms, copy_windows = copy_ms / 10, [w / 10 for w in copy_windows]
    pack_bytes = float(N) * d * (n + ldx) * 8
    copy_bytes = 2.0 * N * d * n * 8
    out = {"ldx": ldx, "pack_bytes": pack_bytes, "d2d_copy_ms": copy_ms, "d2d_copy_windows_ms": copy_windows, "d2d_copy_bytes": copy_bytes,
           "d2d_copy_GBps": copy_bytes / (copy_ms * 1e-3) / 1e9, "method": "kernel time: rocprofv3 --kernel-trace --stats over a child run; "
           "copy: torch copy_ (hipMemcpyAsync device to device) on the library's stream, host clock around 10 x steps copies per window"}
    exe = shutil.which("rocprofv3")
    if exe is None:
        out["error"] = "rocprofv3 not on PATH: the pack kernels' time was not measured"
        return out
    tmp = tempfile.mkdtemp(prefix="rbpf_pack_", dir="/tmp")
    try:
        cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "pack", "--", sys.executable,
               os.path.abspath(__file__), "--pack-child", str(N), "--steps", str(max(a.steps, 20))]
        r = subprocess.run(cmd, cwd="/tmp", env=dict(os.environ, TMPDIR="/tmp"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        files = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if r.returncode != 0 or not files:
            out["error"] = f"rocprofv3 child failed (rc {r.returncode}): {r.stdout[-300:]}"
            return out
        for x in csv.DictReader(open(files[0])):
            for kernel, layout in (("ext_pack_dy_matlab_kernel", 0), ("ext_pack_dy_rows_kernel", 2)):
                if kernel in x["Name"]:
                    ms = float(x["AverageNs"]) / 1e6
                    out[f"layout{layout}"] = {"kernel": kernel, "calls": int(x["Calls"]), "avg_launch_ms": ms,
                                              "GBps": pack_bytes / (ms * 1e-3) / 1e9,
                                              "share_of_d2d_copy_rate": (pack_bytes / ms) / (copy_bytes / copy_ms)}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return out


def ny_sweep(a):
    """--ny: ms per step of the DeviceHandles filter per measurement width, with the bytes a step must move."""
    import torch
    import generic_model as gm
    import generic_model_torch as gmt
    N, n = a.ny_particles, a.ny_nlin
    ldx = (n + 1) & ~1
    T = a.warmup + a.windows * a.steps + 4
    doc = {"tool": "tools/generic_device_bench.py --ny", "device": torch.cuda.get_device_name(0), "N_P": N, "nLin": n, "options": NY_OPTS,
           "handles": "rbpf.DeviceHandles, measModel fills the native view (dy layout 1)",
           "timing": f"warm-up {a.warmup} steps, median of {a.windows} windows of {a.steps} steps (host clock, synchronised)",
           "bytes_per_step": "N_P (2 nLin^2 + (5 n_y + 2) ldx) 8", "hbm_peak_GBps": HBM_PEAK_GBPS, "runs": []}
    for ny in a.ny:
        m = gm.GenericModel(4, 3, 4, ny, n, seed=1)
        p = gm.problem(m, 1, T, seed=1)
        run = dict(bench_device(torch, gmt, m, p, N, 1, a, NY_OPTS), n_y=ny)
        run["bytes_per_step"] = float(N) * (2 * n * n + (5 * ny + 2) * ldx) * 8
        run["GBps"] = run["bytes_per_step"] / (run["ms_per_step"] * 1e-3) / 1e9
        run["frac_hbm_peak"] = run["GBps"] / HBM_PEAK_GBPS
        doc["runs"].append(run)
        print(json.dumps(run), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default: profiles/generic_device_bench.json (--ny: profiles/generic_device_ny_bench.json)")
    ap.add_argument("--ny", type=int, nargs="+", default=None, help="measurement widths of the n_y sweep (1 .. 8); replaces the default runs")
    ap.add_argument("--ny-particles", type=int, default=8192)
    ap.add_argument("--ny-nlin", type=int, default=256)
    ap.add_argument("--particles", type=int, nargs="*", default=None, help="default: 8192 and the largest power of two up to 65536 that fits")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--host-steps", type=int, default=2)
    ap.add_argument("--pack-child", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.pack_child:
        return pack_child(a.pack_child, a.steps)
    if a.windows < 5 or a.steps < 20:
        ap.error("at least 5 windows of at least 20 steps")
    if rbpf.device_count() < 1:
        raise SystemExit("generic_device_bench: no HIP device visible (nothing is measured without one)")
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "generic_device_ny_bench.json" if a.ny else "generic_device_bench.json")
    if a.ny:
        return ny_sweep(a)
    import torch
    import generic_model as gm
    import generic_model_torch as gmt
    sizes = a.particles
    free, total = torch.cuda.mem_get_info()
    if not sizes:
        largest = 65536 if free > 200e9 else (32768 if free > 100e9 else 16384)
        sizes = [8192, largest]
    T = a.warmup + 4 * (a.windows * a.steps + 4) + 16               # the longest session: the four passes of bench_pack
    m = gm.GenericModel(*SHAPE, seed=1)
    p = gm.problem(m, 1, T, seed=1)
    doc = {"tool": "tools/generic_device_bench.py", "device": torch.cuda.get_device_name(0), "free_bytes_at_start": free,
           "shape": dict(zip(("n_nonlin", "n_w", "n_odo", "n_y", "nLin"), SHAPE)), "options": OPTS,
           "timing": f"warm-up {a.warmup} steps, median of {a.windows} windows of {a.steps} steps (host clock, synchronised)", "runs": []}
    for N in sizes:
        run = {"N_P": N}
        run["builtin_dense_mag"] = bench_builtin(N, T, a)
        run["device"] = {f"layout{layout}": bench_device(torch, gmt, m, p, N, layout, a) for layout in (0, 1, 2)}
        run["pack"] = bench_pack(torch, m, p, N, a)
        run["host_callback"] = bench_host(m, p, N, a)
        doc["runs"].append(run)
        print(json.dumps(run), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
