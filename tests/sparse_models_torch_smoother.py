"""The torch twins of tests/sparse_models_torch.py for the smoother's call order: the handles rbpf.DeviceSparseSmootherHandles
takes,

    dynModel(xn (n_nonlin, C), dx (n_odo,), dt, Q (n_w, n_w))  -> (n_nonlin, C)
    measModel(xn (n_nonlin, C), xl (C, nLin))                   -> yhat (C, n_y), dy (C, n_y, nLin)          pure, any C
    dynResNorm(xnk_t (n_nonlin,), xn (n_nonlin, N), dx, dt, Q)  -> (n_w, N)      the additive default, restated as a handle

The twins of sparse_models_torch.py find the step of a measModel call -- for the NaN mask -- by counting calls; under the wider
contract (one call per step plus one per chunk of future times) that breaks, so these are pure in measModel: the rows they
overwrite with NaN are a fixed set of outputs (`nan_rows`), whatever the step.  dynModel is called once per step, N_T - 1 times per
iteration, with C = N_P in iteration 0 and N_P - 1 afterwards (particleSmoother.m:132-137): it finds (k, t) = divmod(calls,
N_T - 1) and replays Z[k, t, :C], what the oracle's dynModel is handed slot by slot (tests/generic_model_torch_smoother.py).
Every call is recorded in `log` as (handle, C)."""
import numpy as np
import torch

import sparse_models_torch as smt


class _SmootherMixin:
    def _init_smoother(self, p, nan_rows=()):
        self.Zk = torch.as_tensor(np.ascontiguousarray(np.asarray(p["rng"].Z)), **self.f)     # [N_K][N_T - 1][N_P][n_w]
        self.T1 = int(self.Zk.shape[1])
        self.nan_rows = torch.as_tensor(np.asarray(sorted(nan_rows), dtype=np.int64), device=self.device)
        self.log = []
        self.calls = 0

    def reset(self):
        self.log = []
        self.calls = 0

    def _lq(self, t):
        return self.Lq[t if len(self.Lq) > 1 else 0]

    def dynModel(self, xn, dx, dt, Q):
        k, t = divmod(self.calls, self.T1)
        self.calls += 1
        C = int(xn.shape[1])
        self.log.append(("dyn", C))
        return xn + dx.reshape(-1, 1) + self._lq(t) @ self.Zk[k, t, :C].t()

    def measModel(self, xn, xl):
        self.log.append(("meas", int(xn.shape[1])))
        yhat, dy = self._meas(xn, xl)
        if self.nan_rows.numel():
            yhat = yhat.clone()
            dy = dy.clone()
            yhat[:, self.nan_rows] = float("nan")
            dy[:, self.nan_rows, :] = float("nan")
        if self.dy_mode == "matlab":
            dy = dy.permute(2, 1, 0).contiguous().permute(2, 1, 0)
        elif self.dy_mode == "slice":
            wide = torch.zeros(dy.shape[0], dy.shape[1], dy.shape[2] + 3, **self.f)
            wide[:, :, :dy.shape[2]] = dy
            dy = wide[:, :, :dy.shape[2]]
        else:
            dy = dy.contiguous()
        yhat = yhat.t().contiguous().t() if self.yhat_mode == "t" else yhat.contiguous()
        return yhat, dy

    def dynResNorm(self, xnk_t, xn, dx, dt, Q):
        """(xnk_t - xn - dx') / chol(dt Q, 'lower')' per column (particleSmoother.m:176-177); the step is that of the last dynModel
        call: dynResNorm of step t follows dynModel of step t."""
        self.log.append(("drn", int(xn.shape[1])))
        t = (self.calls - 1) % self.T1
        r = xnk_t.reshape(-1, 1) - xn - dx.reshape(-1, 1)
        return torch.linalg.solve_triangular(self._lq_chol(t), r, upper=False)

    def _lq_chol(self, t):
        return self.Lq_chol[t if len(self.Lq_chol) > 1 else 0]

    def columns(self, handle):
        return [c for h, c in self.log if h == handle]


def twin_of(model, p, device, nan_rows=(), **kw):
    """The smoother twin of an oracle sparse model (see tests/sparse_models_torch.py for dy_mode / yhat_mode)."""
    base = {"SparseVisualModel": smt.TorchPinhole, "RangeBearingModel": smt.TorchRangeBearing, "RangeOnly3DModel": smt.TorchRangeOnly3D}[type(model).__name__]
    p0 = dict(p, rng=type("R", (), {"Z": np.asarray(p["rng"].Z)[:1]})())           # the base class keeps iteration 0's normals only

    class Twin(_SmootherMixin, base):
        pass

    tw = Twin(model, p0, device, **kw)
    tw._init_smoother(p, nan_rows)
    Q = np.asarray(p["Q"], dtype=np.float64)
    Q = Q[:, :, None] if Q.ndim == 2 else Q
    dt = np.atleast_1d(np.asarray(p["dt"], dtype=np.float64)).ravel()
    pages = tw.T1 if (Q.shape[2] > 1 or dt.size > 1) else min(tw.T1, 1)
    tw.Lq_chol = [torch.as_tensor(np.linalg.cholesky(np.atleast_2d(dt[t if dt.size > 1 else 0] * Q[:, :, t if Q.shape[2] > 1 else 0])), **tw.f)
                  for t in range(pages)]
    return tw
