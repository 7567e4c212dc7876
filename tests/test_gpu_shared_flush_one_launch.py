"""GPU: the shared flush with two covariance banks as ONE launch (step_sym_kernel_shared: the writers' flush body and their read-only
siblings' body in one grid) equals the single-bank flush, which keeps its three launches of step_sym_kernel, bit for bit.

The dense-mag model at m = 512 (nLin = 515: eight tile rows of the block-lower storage), built as bench.py builds it, through
FilterSession with storage="fp64sym", keep_history=True and a fixed Philox seed.  T = 2 * lazy_depth + 2 steps, so that two flush
steps run (t = lazy_depth and t = 2 * lazy_depth).  inplace=-1 (two banks) takes the new launch, inplace=1 (one bank) the untouched
path; the two bank schedules are bit-identical by construction (every workgroup runs the same code on the same data in both), so
every output bench.py's DUMP_WANT names must be equal with np.array_equal -- there is no tolerance to choose.

Two more cases put the flush at its extremes, read back from the ancestor table the library returns (trace_ai):
* R scaled down until the weights collapse: a parent with at least N / 2 children -- one writer, nearly everybody a sibling.
  Below 1e-4 the scale of R changes nothing any more (S = H P H' + R is H P H'; measured from 1e-4 down to 1e-14: the same
  ancestors), and what is left depends on the draw: Philox seed 2024 gives families of at most 23 of 48 at its two flush steps,
  seed 2 families of 42 and 30 (a scan of seeds 1..40 at this scale); this case runs seed 2;
* R scaled up until the weights are flat: N distinct parents -- every particle a writer, no sibling.  The reference draws every
  ancestor on its own (particleFilter.m:106, tools/sample.m:30-32: multinomial), so flat weights alone give about 63 % distinct
  parents and never all N of them (48! / 48^48 = 1e-20); the case therefore replays the device generator's own normals together
  with stratified uniforms u_i = (i + 1/2) / N, which under flat weights pick every parent exactly once.
A case that does not reach its extreme fails.

The last case runs the sharded filter at world 1 with the real collectives (its flush steps come through the same launch builder)
against the single-GPU two-bank run.  traj_max, traj_mean and xl_max are what the step kernels and the normalisation produce and
must be equal bit for bit.  xl_mean, P_max and P_mean are formed at the end by other code in the two sessions: rbpf_shard_finish
adds up a rank's share of the 48 weighted particles and applies the one pending set of the last step (three products per element)
in another order than rbpf_filter_finish.  The same terms in another order differ by at most (terms - 1) roundings of the largest
partial sum, so these three are held to 8 units in the last place of the array's largest magnitude (8 * spacing(max |ref|):
6e-14 at the 35 .. 42 these arrays reach) and no relative slack.  That the difference is the sessions' and not the launch's is on
record: the parent commit, whose flush takes two launches, gives the very same largest differences -- 1.066e-14, 2.842e-14 and
7.105e-15 -- as this one (profiles/r06_shared_flush_one_launch.txt).

Every two-bank run also asserts, from the library's own counter (rbpf_filter_one_launch_flushes), that both of its flush steps
took the one launch, so a case cannot pass through the two launches."""
import importlib
import os
import queue
import socket
import sys

import numpy as np
import pytest
import torch.multiprocessing as mp

import bench

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "rao-blackwellized-slam-smoothing_amd"
M, DT, SEED, SEED_COLLAPSE = 512, 0.01, 2024, 2
R_COLLAPSE, R_FLAT = 1e-6, 1e12           # scales of R for the two extremes (see the module docstring)


def _problem(T):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    pkg = importlib.import_module(PKG)
    dg = importlib.import_module(PKG + ".datagen")
    Q = bench.q_mag()
    d = dg.bean_6D(T, Q, bench.THETA_MAG, DT, seed=1)
    mdl, x0, P0, R = pkg.dense_mag_prior(M, d["LL"], bench.THETA_MAG)
    return pkg, d, mdl, x0, P0, Q, R


def _filter(N, lazy_depth, inplace, r_scale=1.0, rng=None, want=bench.DUMP_WANT + ("trace_ai",), seed=SEED):
    T = 2 * lazy_depth + 2
    pkg, d, mdl, x0, P0, Q, R = _problem(T)
    with pkg.FilterSession(mdl, d["dx"], d["y"], d["initState"], x0, P0, Q, r_scale * R, N, DT,
                           rng=rng if rng is not None else pkg.PhiloxRNG(seed), keep_history=True, trace=True,
                           lazy_depth=lazy_depth, inplace=inplace, storage="fp64sym") as s:
        s.advance(T)
        s.sync()
        assert s.schedule() == ((2 if inplace < 0 else 1), True)      # the banks asked for, the flush shared
        assert s.one_launch_flushes() == (2 if inplace < 0 else 0)    # two banks: both flush steps in the one launch
        return s.finish(want=want)


def _assert_equal(two_banks, one_bank, names):
    for k in names:
        assert np.all(np.isfinite(two_banks[k])), k
        assert np.array_equal(two_banks[k], one_bank[k]), k


def _children(out, lazy_depth):
    """Per flush step: (largest number of children of one parent, number of distinct parents)."""
    ai = out["trace_ai"]
    res = []
    for t in (lazy_depth, 2 * lazy_depth):
        counts = np.bincount(ai[:, t], minlength=ai.shape[0])
        res.append((int(counts.max()), int(np.count_nonzero(counts))))
    return res


@pytest.mark.parametrize("N", [1, 2, 3, 48])
@pytest.mark.parametrize("lazy_depth", [2, 3, 4])
def test_one_launch_equals_the_single_bank_flush(lazy_depth, N):
    a = _filter(N, lazy_depth, -1)
    b = _filter(N, lazy_depth, 1)
    print(f"lazy_depth {lazy_depth} N {N}: flush steps (max children, distinct parents) {_children(a, lazy_depth)}")
    _assert_equal(a, b, bench.DUMP_WANT + ("trace_ai",))


def test_collapsed_weights_few_writers_many_siblings():
    N, lazy_depth = 48, 4
    a = _filter(N, lazy_depth, -1, R_COLLAPSE, seed=SEED_COLLAPSE)
    b = _filter(N, lazy_depth, 1, R_COLLAPSE, seed=SEED_COLLAPSE)
    ch = _children(a, lazy_depth)
    print(f"collapsed weights: flush steps (max children, distinct parents) {ch}")
    assert max(c for c, _ in ch) >= N // 2
    _assert_equal(a, b, bench.DUMP_WANT + ("trace_ai",))


def test_flat_weights_every_particle_a_writer():
    N, lazy_depth = 48, 4
    T = 2 * lazy_depth + 2
    pkg, _, mdl, *_ = _problem(T)
    rng = pkg.PhiloxRNG(SEED).replay(N, T, mdl.nw)
    U = np.broadcast_to((np.arange(N) + 0.5) / N, rng.U.shape)
    rng = pkg.ReplayRNG(U, rng.Z, rng.Ufin)
    a = _filter(N, lazy_depth, -1, R_FLAT, rng)
    b = _filter(N, lazy_depth, 1, R_FLAT, rng)
    ch = _children(a, lazy_depth)
    print(f"flat weights: flush steps (max children, distinct parents) {ch}")
    assert max(p for _, p in ch) == N
    _assert_equal(a, b, bench.DUMP_WANT + ("trace_ai",))


def _sharded_worker(port, N, lazy_depth, q):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1)
    try:
        T = 2 * lazy_depth + 2
        pkg, d, mdl, x0, P0, Q, R = _problem(T)
        mg = importlib.import_module(PKG + ".multigpu")
        with mg.ShardedFilterSession(mdl, d["dx"], d["y"], d["initState"], x0, P0, Q, R, N, DT, rng=pkg.PhiloxRNG(SEED), rank=0,
                                     world=1, lazy_depth=lazy_depth, storage="fp64sym", force_collectives=True) as s:
            s.advance(T)
            out = s.finish(want=bench.DUMP_WANT_SHARDED)
            n_one = s.one_launch_flushes()
        q.put(dict({k: np.asarray(out[k]) for k in bench.DUMP_WANT_SHARDED}, one_launch_flushes=n_one))
    finally:
        dist.destroy_process_group()


def test_sharded_world_one_equals_the_single_gpu_two_bank_run():
    N, lazy_depth = 48, 4
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    p = ctx.Process(target=_sharded_worker, args=(port, N, lazy_depth, q))
    p.start()
    sh = None
    while sh is None:
        try:
            sh = q.get(timeout=1)
        except queue.Empty:
            assert p.is_alive(), f"the sharded run ended with exit code {p.exitcode} and no result"
    p.join(120)
    assert p.exitcode == 0
    ref = _filter(N, lazy_depth, -1, want=bench.DUMP_WANT_SHARDED)
    for k in bench.DUMP_WANT_SHARDED:
        print(f"sharded {k}: max abs difference {np.max(np.abs(sh[k] - ref[k])):.3e}")
    _assert_equal(sh, ref, ("traj_max", "traj_mean", "xl_max"))
    assert sh["one_launch_flushes"] == 2
    for k in ("xl_mean", "P_max", "P_mean"):
        np.testing.assert_allclose(sh[k], ref[k], rtol=0.0, atol=8.0 * np.spacing(np.max(np.abs(ref[k]))), err_msg=k)
