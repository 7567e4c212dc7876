"""The sparse-branch models (the oracle's SparseVisualModel and tests/sparse_models.py) restated in torch float64 on the device,
batched over the particles: the handles rbpf.DeviceSparseHandles takes,

    dynModel(xn (n_nonlin, N), dx (n_odo,), dt, Q (n_w, n_w)) -> (n_nonlin, N)
    measModel(xn (n_nonlin, N), xl (N, nLin))                 -> yhat (N, n_y), dy (N, n_y, nLin)

The normals Z are replayed from a device tensor in the reference's call order (step t hands slot i the row Z[0, t, i]); the
noise factor of every step is formed once at construction, on the host, as the numpy models form it.  dynModel and measModel
count their calls to find their step; reset() rewinds them.

dy_mode  "c" C-contiguous, "matlab" strides (1, N, N n_y), "slice" a non-contiguous slice of a wider tensor
yhat_mode "c" contiguous, "t" transposed (strides (1, N))
nan_unobserved=True: every row of yhat and dy that belongs to an output with NaN in y at that step is overwritten with NaN."""
import numpy as np
import torch


class _TorchSparseBase:
    def __init__(self, p, device, elementwise_sqrt=False, dy_mode="c", yhat_mode="c", nan_unobserved=False):
        f = dict(dtype=torch.float64, device=device)
        self.f, self.device = f, device
        self.Z = torch.as_tensor(np.asarray(p["rng"].Z)[0], **f)          # [N_T - 1][N_P][n_w]
        Q = np.asarray(p["Q"], dtype=np.float64)
        Q = Q[:, :, None] if Q.ndim == 2 else Q
        dt = np.atleast_1d(np.asarray(p["dt"], dtype=np.float64)).ravel()
        T1 = self.Z.shape[0]
        fac = (lambda a: np.sqrt(a)) if elementwise_sqrt else np.linalg.cholesky
        self.Lq = [torch.as_tensor(fac(np.atleast_2d(dt[t if dt.size > 1 else 0] * Q[:, :, t if Q.shape[2] > 1 else 0])), **f)
                   for t in range(T1 if (Q.shape[2] > 1 or dt.size > 1) else min(T1, 1))]
        self.unobserved = torch.as_tensor(np.isnan(np.asarray(p["y"])), device=device)      # [N_T][n_y]
        self.dy_mode, self.yhat_mode, self.nan_unobserved = dy_mode, yhat_mode, nan_unobserved
        self.dyn_calls = self.meas_calls = 0

    def reset(self):
        self.dyn_calls = self.meas_calls = 0

    def dynModel(self, xn, dx, dt, Q):
        t = self.dyn_calls
        self.dyn_calls += 1
        return xn + dx.reshape(-1, 1) + self.Lq[t if len(self.Lq) > 1 else 0] @ self.Z[t].t()

    def measModel(self, xn, xl):
        t = self.meas_calls
        self.meas_calls += 1
        yhat, dy = self._meas(xn, xl)
        if self.nan_unobserved:
            gone = self.unobserved[t]
            yhat = torch.where(gone[None, :], torch.full_like(yhat, float("nan")), yhat)
            dy = torch.where(gone[None, :, None], torch.full_like(dy, float("nan")), dy)
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


class TorchPinhole(_TorchSparseBase):
    """oracle SparseVisualModel: pfslam.m:81 (element-wise sqrt of dt*Q), measurement.m:32-84."""

    def __init__(self, model, p, device, **kw):
        super().__init__(p, device, elementwise_sqrt=True, **kw)
        self.fl, self.fp = float(model.f), float(model.fp)

    def _meas(self, xn, xl):
        N = xl.shape[0]
        m = xl.reshape(N, -1, 2)
        mx, my = m[:, :, 0], m[:, :, 1]
        px, py, th = xn[0][:, None], xn[1][:, None], xn[2][:, None]
        s, c = torch.sin(th), torch.cos(th)
        t1, t2 = -(c * px + s * py), -(-s * px + c * py)                  # K * [R', -R'*p]
        u1 = (self.fl * c - self.fp * s) * mx + (self.fl * s + self.fp * c) * my + (self.fl * t1 + self.fp * t2)
        u2 = -s * mx + c * my + t2
        div = (my * c - py * c - mx * s + px * s) ** 2
        L = m.shape[1]
        dy = torch.zeros(N, L, 2 * L, **self.f)
        j = torch.arange(L, device=self.device)
        dy[:, j, 2 * j] = (self.fl * (my - py)) / div
        dy[:, j, 2 * j + 1] = -(self.fl * (mx - px)) / div
        return u1 / u2, dy


class TorchRangeBearing(_TorchSparseBase):
    def __init__(self, model, p, device, **kw):
        super().__init__(p, device, **kw)
        self.G = torch.as_tensor(model.G, **self.f)

    def _meas(self, xn, xl):
        N = xl.shape[0]
        m = xl.reshape(N, -1, 2)
        L = m.shape[1]
        dx, dy_ = m[:, :, 0] - xn[0][:, None], m[:, :, 1] - xn[1][:, None]
        r2 = dx * dx + dy_ * dy_
        r = torch.sqrt(r2)
        yhat = torch.empty(N, 2 * L, **self.f)
        yhat[:, 0::2] = r
        yhat[:, 1::2] = torch.atan2(dy_, dx) - xn[2][:, None]
        J = torch.zeros(N, 2 * L, 2 * L, **self.f)
        j = torch.arange(L, device=self.device)
        J[:, 2 * j, 2 * j] = dx / r
        J[:, 2 * j, 2 * j + 1] = dy_ / r
        J[:, 2 * j + 1, 2 * j] = -dy_ / r2
        J[:, 2 * j + 1, 2 * j + 1] = dx / r2
        return yhat + xl @ self.G.t(), J + self.G[None]


class TorchRangeOnly3D(_TorchSparseBase):
    def __init__(self, model, p, device, **kw):
        super().__init__(p, device, **kw)

    def _meas(self, xn, xl):
        N = xl.shape[0]
        dlt = xl.reshape(N, -1, 3) - xn.t()[:, None, :]
        L = dlt.shape[1]
        r = torch.sqrt(torch.sum(dlt * dlt, dim=2))
        J = torch.zeros(N, L, 3 * L, **self.f)
        j = torch.arange(L, device=self.device)
        for a in range(3):
            J[:, j, 3 * j + a] = dlt[:, :, a] / r
        return r, J


def twin_of(model, p, device, **kw):
    name = type(model).__name__
    cls = {"SparseVisualModel": TorchPinhole, "RangeBearingModel": TorchRangeBearing, "RangeOnly3DModel": TorchRangeOnly3D}[name]
    return cls(model, p, device, **kw)
