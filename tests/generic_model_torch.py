"""The synthetic model family of tests/generic_model.py restated in torch float64 on the device: the same A, G, omega, c and
phi, batched over the particles, with the normals Z replayed from a device tensor in the reference's call order (the filter:
step t hands slot i the row Z[0, t, i]).  These are the handles rbpf.DeviceHandles takes:

    dynModel(xn (n_nonlin, N), dx (n_odo,), dt, Q (n_w, n_w)) -> (n_nonlin, N)
    measModel(xn (n_nonlin, N))                               -> (N, n_y, nLin)

Every call reads and writes device memory only.  dynModel counts its calls to find its page of Z; reset() rewinds it.
chol(dt Q, 'lower') of the problem's pages is formed once at construction, as numpy's cholesky forms it for the oracle's
model: torch's factorisation on the device reports its status through the host, and a handle that waits for the host is
what this family is there to avoid."""
import numpy as np
import torch


class TorchGenericModel:
    def __init__(self, model, p, device):
        f = dict(dtype=torch.float64, device=device)
        self.m, self.device = model, device
        self.A, self.G = torch.as_tensor(model.A, **f), torch.as_tensor(model.G, **f)
        self.omega, self.c, self.phi = torch.as_tensor(model.omega, **f), torch.as_tensor(model.c, **f), torch.as_tensor(model.phi, **f)
        self.bend, self.noise = float(model.bend), bool(model.noise)
        self.Z = torch.as_tensor(p["Z"][0], **f)                       # [N_T - 1][N_P][n_w]
        Q = np.asarray(p["Q"], dtype=np.float64)
        Q = Q[:, :, None] if Q.ndim == 2 else Q
        dt = np.atleast_1d(np.asarray(p["dt"], dtype=np.float64)).ravel()
        T1 = self.Z.shape[0]
        self.Lq = [torch.as_tensor(np.linalg.cholesky(np.atleast_2d(dt[t if dt.size > 1 else 0] * Q[:, :, t if Q.shape[2] > 1 else 0])), **f)
                   for t in range(T1 if (Q.shape[2] > 1 or dt.size > 1) else min(T1, 1))]
        self.calls = 0

    def reset(self):
        self.calls = 0

    def dynModel(self, xn, dx, dt, Q):
        t = self.calls
        self.calls += 1
        x = xn + self.bend * torch.sin(xn) + (self.A @ dx.reshape(-1, 1))
        if self.noise:
            x = x + self.G @ (self.Lq[t if len(self.Lq) > 1 else 0] @ self.Z[t].t())
        return x

    def measModel(self, xn):
        arg = (self.omega @ xn).t()                                       # [N x nLin]
        return self.c[None] * torch.cos(arg[:, None, :] + self.phi[None])
