#!/usr/bin/env python3
"""What one step of the marginal smoother (the two all-pairs passes of csrc/rbpf_loc_marginal.hpp) costs next to one
backward-simulation step of the same term on the same inputs, at N = M (successors = particles) in {8192, 65 536}, in ONE process,
every shape warmed up first -- the protocol of tools/map_trajectory_bench.py, whose input generators (tools/device_map_backward_bench.py)
this tool takes:

  marginal  the probes rbpf_loc_marginal_step / rbpf_loc_generic_marginal_step: prologue + norm pass + merge + weight pass + merge
            between two device events, log w_{t+1|T} = log w.
  backward  the probes rbpf_loc_backward_step / rbpf_loc_generic_backward_(pose_)step: prologue + all-pairs pass + locate, the
            existing kernels.
  A window is one probe call of REPS event-timed repetitions (its median); the marginal and the backward windows alternate; the
  figure is the median of 5 windows, the spread (max - min) / median over the windows.  Terms: dense-mag; n_res = 1, 3, 6, 8; the
  pose form with 3 plain rows (the dense-mag inputs in model E's form).
  The expectation reported against (no test gate): marginal_ms <= 2 backward_ms + slack_ms, slack_ms = the larger (spread x median)
  of the two -- two all-pairs passes with one exp per surviving pair each, against one such pass plus a locate walk.

  session   one whole LocalizationSession.smoothed_marginals() of N_T = 6 on model A of tests/device_map_smoother_ref.py with a torch
            `mean` handle, host clock, after a warm-up call.

  The compile report is the kernel resource usage (VGPRs, SGPRs, LDS, scratch, occupancy, from hipcc's kernel-resource-usage remarks)
  and the instruction count (the instruction lines of the kernel's body in hipcc's assembly) of every kernel in
  csrc/rbpf_loc_smooth.hip and csrc/rbpf_loc_generic_smooth.hip.  --only-compile-report FILE makes it for the tree the tool stands in,
  or for another checkout with --root DIR (no device needed); a timing run stores the reports handed to it with --this-report (this
  tree) and --parent-report (the parent commit's checkout) and says whether the existing kernels are unchanged.
  Writes profiles/marginal_smoother_bench.json.

Usage: marginal_smoother_bench.py [--out FILE] [--sizes N ...] [--reps 3] [--windows 5] [--steps 6] [--this-report FILE] [--parent-report FILE]
       marginal_smoother_bench.py --only-compile-report FILE [--root DIR]
       marginal_smoother_bench.py --sizes --this-report FILE --parent-report FILE     (no timing, no device: the compile report alone)"""
import argparse
import importlib
import json
import os
import re
import shutil
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

SOURCES = ("rbpf_loc_smooth.hip", "rbpf_loc_generic_smooth.hip")
FIELDS = {"TotalSGPRs": "sgprs", "VGPRs": "vgprs", "AGPRs": "agprs", "ScratchSize [bytes/lane]": "scratch_bytes_per_lane",
          "Occupancy [waves/SIMD]": "occupancy_waves_per_simd", "LDS Size [bytes/block]": "lds_bytes_per_block",
          "SGPRs Spill": "sgpr_spill", "VGPRs Spill": "vgpr_spill"}


def _instruction_counts(asm):
    """{mangled kernel name: instruction lines between its label and its s_endpgm}."""
    out, cur = {}, None
    for line in asm.splitlines():
        m = re.match(r"^(_Z\w+|\w+):\s*(;.*)?$", line)
        if m and cur is None:
            cur = m.group(1)
            out[cur] = 0
            continue
        if cur is None:
            continue
        body = line.strip()
        if re.match(r"^[a-z][a-z0-9_]+(\s|$)", body):
            out[cur] += 1
            if body.startswith("s_endpgm"):
                cur = None
    return out


def compile_report(root=ROOT):
    """{kernel: {vgprs, sgprs, ..., instructions}} of the two smoother sources of the tree at `root`, device code only, nothing is
    kept."""
    import tempfile
    csrc = os.path.join(root, "rao-blackwellized-slam-smoothing_amd", "csrc")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for src in SOURCES:
            asm = os.path.join(tmp, src + ".s")
            cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-value", "-Wno-unused-result",
                   "-I" + os.path.join(root, "include"), "--offload-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", "-c",
                   os.path.join(csrc, src), "-o", asm]
            res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            if res.returncode != 0:
                raise RuntimeError(res.stderr)
            cur = None
            for line in res.stderr.splitlines():
                m = re.search(r"remark: .*?Function Name: (\S+)", line)
                if m:
                    cur = out.setdefault(m.group(1), {})
                    continue
                m = re.search(r"remark:\s+(.+?): (\d+) \[-Rpass", line)
                if m and cur is not None and m.group(1) in FIELDS:
                    cur[FIELDS[m.group(1)]] = int(m.group(2))
            with open(asm) as f:
                counts = _instruction_counts(f.read())
            for name, rec in out.items():
                if name in counts and "instructions" not in rec:
                    rec["instructions"] = counts[name]
    names = sorted(out)
    filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    if filt:
        plain = subprocess.run([filt] + names, stdout=subprocess.PIPE, text=True).stdout.splitlines()
        short = [re.sub(r"\(.*", "", p).replace("void ", "").replace("rbpf::", "") for p in plain]
        out = {s: out[n] for s, n in zip(short, names)}
    return out


def stats(ms, N):
    med = float(np.median(ms))
    return dict(ms=med, windows_ms=[float(v) for v in ms], spread=float((max(ms) - min(ms)) / med), pairs_per_s=float(N) * N / (med * 1e-3))


def compare(name, N, run_marg, run_back, a):
    run_marg(1)                                                            # warm-up
    run_back(1)
    ms_marg, ms_back = [], []
    for _ in range(a.windows):
        ms_marg.append(run_marg(a.reps))
        ms_back.append(run_back(a.reps))
    rec = dict(term=name, marginal=stats(ms_marg, N), backward=stats(ms_back, N))
    slack = max(rec["marginal"]["spread"] * rec["marginal"]["ms"], rec["backward"]["spread"] * rec["backward"]["ms"])
    rec["verdict"] = dict(marginal_ms=rec["marginal"]["ms"], backward_ms=rec["backward"]["ms"], slack_ms=slack,
                          ratio=rec["marginal"]["ms"] / rec["backward"]["ms"],
                          within_two_backward_steps=bool(rec["marginal"]["ms"] <= 2.0 * rec["backward"]["ms"] + slack))
    print(json.dumps(rec), flush=True)
    return rec


def session(rbpf, torch, dev, N, T):
    import device_map_smoother_ref as S
    import generic_model_torch as gmt
    c = S.case("A", N, T)
    p = c.p
    tm = gmt.TorchGenericModel(c.m, p, dev)
    mean = lambda xn, dx, dt, Q: xn + tm.bend * torch.sin(xn) + tm.A @ dx.reshape(-1, 1)       # noqa: E731
    mp = rbpf.DeviceMap(rbpf.DeviceHandles(tm.dynModel, tm.measModel), p["mean"], p["V"], p["R"],
                        transition=rbpf.DeviceTransition(mean, c.cov_of))
    with rbpf.LocalizationSession(mp, p["odometry"], p["y"], p["x0_nonLin"], p["Q"], N, p["dt"], rng=rbpf.PhiloxRNG(3), keep_history=True,
                                  trace=True) as s:
        s.advance(T)
        s.sync()
        s.smoothed_marginals()                                             # warm-up
        t0 = time.perf_counter()
        out = s.smoothed_marginals(want=("w_smooth", "mean", "cov", "ess", "mass"))
        ms = (time.perf_counter() - t0) * 1e3
    return dict(model="A (n_res = 3)", N_T=T, smoothed_marginals_ms=ms, ms_per_step=ms / max(T - 1, 1),
                ess=[float(v) for v in out["ess"]], worst_mass_error=float(np.max(np.abs(out["mass"] - 1.0))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "marginal_smoother_bench.json"))
    ap.add_argument("--sizes", type=int, nargs="*", default=[8192, 65536])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--this-report", default=None)
    ap.add_argument("--parent-report", default=None)
    ap.add_argument("--only-compile-report", default=None)
    ap.add_argument("--root", default=ROOT)
    a = ap.parse_args()
    if a.only_compile_report:
        with open(a.only_compile_report, "w") as f:
            json.dump(compile_report(a.root), f, indent=1)
            f.write("\n")
        return
    doc = dict(tool="tools/marginal_smoother_bench.py", device=None,
               timing=f"median of {a.windows} windows, a window = the median of {a.reps} event-timed repetitions of one step; the marginal and "
                      f"the backward windows alternate in one process, both warmed up first; spread = (max - min) / median over the windows; "
                      f"session: host clock, synchronised",
               expectation="marginal_ms <= 2 backward_ms + slack_ms, slack_ms = max(spread x median) of the two; reported, not a test gate",
               not_measured=["other N", "M != N", "N_T beyond the session's", "hardware counters"], runs=[])
    if a.sizes:                                                            # (--sizes with no value: the compile report alone, no device)
        import torch
        import device_map_backward_bench as B
        rbpf = importlib.import_module("rao-blackwellized-slam-smoothing_amd")
        dev = torch.device("cuda", torch.cuda.current_device())
        doc["device"] = torch.cuda.get_device_name(dev)
    else:
        doc["not_measured"] = ["every timing: this file holds the compile report alone"]
    for N in a.sizes:
        rec = dict(N=N, M=N, terms=[])
        X, w, xs, dx, dt, Q, u = dm_in = B.dense_mag_inputs(N, N)
        with np.errstate(divide="ignore"):
            lw = np.log(w)
        rec["terms"].append(compare("dense_mag", N, lambda r: rbpf.loc_marginal_step(X, lw, xs, lw, dx, dt, Q, reps=r)[2],
                                    lambda r: rbpf.loc_backward_step(*dm_in, reps=r)[2], a))
        for n_res in (1, 3, 6, 8):
            p = B.generic_inputs(n_res, N, N, False)
            lwp = np.log(p["w"])
            rec["terms"].append(compare(
                f"n_res = {n_res}", N,
                lambda r: rbpf.device_map_marginal_step(p["mu"], lwp, p["xs_next"], lwp, p["cov"], angle_rows=p["angle_rows"], reps=r)[2],
                lambda r: rbpf.device_map_backward_step(p["mu"], p["w"], p["xs_next"], p["cov"], p["u"], angle_rows=p["angle_rows"], reps=r)[2], a))
        # the dense-mag inputs in the pose form: mu = (p + dx_pos, qRight(q) dq), cov = blkdiag(dt Q(1:3,1:3), dt Q(4:6,4:6))
        dq, q = dx[3:7], X[3:7]
        mu_q = np.vstack((dq[0] * q[0] - dq[1] * q[1] - dq[2] * q[2] - dq[3] * q[3], dq[0] * q[1] + dq[1] * q[0] + dq[2] * q[3] - dq[3] * q[2],
                          dq[0] * q[2] - dq[1] * q[3] + dq[2] * q[0] + dq[3] * q[1], dq[0] * q[3] + dq[1] * q[2] - dq[2] * q[1] + dq[3] * q[0]))
        mu = np.vstack((X[0:3] + dx[0:3, None], mu_q))
        cov = np.zeros((6, 6))
        cov[0:3, 0:3], cov[3:6, 3:6] = dt * Q[0:3, 0:3], dt * Q[3:6, 3:6]
        rec["terms"].append(compare("pose, 3 plain rows", N,
                                    lambda r: rbpf.device_map_marginal_step(mu, lw, xs, lw, cov, quat_rows=(3, 4, 5, 6), reps=r)[2],
                                    lambda r: rbpf.device_map_backward_step(mu, w, xs, cov, u, quat_rows=(3, 4, 5, 6), reps=r)[2], a))
        rec["all_within_two_backward_steps"] = all(t["verdict"]["within_two_backward_steps"] for t in rec["terms"])
        rec["session"] = session(rbpf, torch, dev, N, a.steps)
        print(json.dumps(rec["session"]), flush=True)
        doc["runs"].append(rec)
    if a.this_report:
        with open(a.this_report) as f:
            doc["compile_report"] = dict(flags="--offload-arch=gfx950 -O3", this_tree=json.load(f))
        if a.parent_report:
            with open(a.parent_report) as f:
                doc["compile_report"]["parent"] = json.load(f)
            new, old = doc["compile_report"]["this_tree"], doc["compile_report"]["parent"]
            doc["compile_report"]["existing_kernels_unchanged"] = all(new.get(k) == v for k, v in old.items())
            doc["compile_report"]["new_kernels_with_scratch"] = [k for k, v in new.items() if k not in old and v["scratch_bytes_per_lane"]]
            doc["compile_report"]["parent"] = "every kernel of the parent commit is in this_tree with the same figures" if \
                doc["compile_report"]["existing_kernels_unchanged"] else old
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
