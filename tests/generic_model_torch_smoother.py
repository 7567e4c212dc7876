"""tests/generic_model.py restated in torch float64 on the device for the smoothers' call order: the handles
rbpf.DeviceSmootherHandles takes.

    dynModel(xn (n_nonlin, n_cols), dx (n_odo,), dt, Q (n_w, n_w)) -> (n_nonlin, n_cols)
    measModel(xn (n_nonlin, n_cols))                               -> (n_cols, n_y, nLin)          pure
    dynResNorm(xnk_t (n_nonlin,), xn (n_nonlin, N), dx, dt, Q)      -> (n_w, N)

dynModel is called once per step, N_T - 1 times per iteration, with n_cols = N_P in iteration 0 and N_P - 1 afterwards
(particleSmoother.m:132-137): it finds (k, t) = divmod(calls, N_T - 1) and replays the normals Z[k, t, :n_cols] -- what the
oracle's dynModel is handed slot by slot.  Every call reads and writes device memory only and is recorded (`log`), so a test
can check the call contract.  chol(dt Q) comes from the base class (numpy's factor, formed once)."""
import numpy as np
import torch

import generic_model_torch as gmt


class TorchSmootherModel(gmt.TorchGenericModel):
    def __init__(self, model, p, device):
        super().__init__(model, p, device)
        f = dict(dtype=torch.float64, device=device)
        self.Zk = torch.as_tensor(np.ascontiguousarray(p["Z"]), **f)          # [N_K][N_T - 1][N_P][n_w]
        self.T1 = int(self.Zk.shape[1])
        self.Gpinv = torch.as_tensor(model.Gpinv, **f)
        self.log = []                                                         # (handle, n_cols) of every call

    def reset(self):
        super().reset()
        self.log = []

    def _lq(self, t):
        return self.Lq[t if len(self.Lq) > 1 else 0]

    def drift(self, xn, dx):
        return xn + self.bend * torch.sin(xn) + (self.A @ dx.reshape(-1, 1))

    def dynModel(self, xn, dx, dt, Q):
        k, t = divmod(self.calls, self.T1)
        self.calls += 1
        n_cols = int(xn.shape[1])
        self.log.append(("dyn", n_cols))
        x = self.drift(xn, dx)
        if self.noise:
            x = x + self.G @ (self._lq(t) @ self.Zk[k, t, :n_cols].t())
        return x

    def measModel(self, xn):
        self.log.append(("meas", int(xn.shape[1])))
        return super().measModel(xn)

    def dynResNorm(self, xnk_t, xn, dx, dt, Q):
        """chol(dt Q)^-1 G^+ (xnk_t - drift(xn)), batched over the columns of xn.  The step is found from the dynModel calls made
        so far: dynResNorm of step t follows dynModel of step t."""
        self.log.append(("drn", int(xn.shape[1])))
        t = (self.calls - 1) % self.T1
        r = self.Gpinv @ (xnk_t.reshape(-1, 1) - self.drift(xn, dx))
        return torch.linalg.solve_triangular(self._lq(t), r, upper=False)

    def count(self, handle):
        return sum(1 for h, _ in self.log if h == handle)

    def columns(self, handle):
        return [c for h, c in self.log if h == handle]
