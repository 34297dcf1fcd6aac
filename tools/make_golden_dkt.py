"""Generate tests/golden/g32_dkt.npz: the DKT definition of DESIGN.md section 20 written as a plain torch chain on the
reference's MetaTemplate, run on the CPU.

Build-box only: it needs the reference tree (oracle.make_golden.REF) and imports its ``backbone`` / ``methods.meta_template`` with
oracle.make_golden's recipe; the reference ships no methods/dkt.py, so the class below IS the definition (Deep Kernel Transfer,
Patacchiola et al., NeurIPS 2020: n_way one-vs-rest Gaussian processes on pooled features, trained through the marginal likelihood
of all rows of the episode, scored with the posterior mean conditioned on the support rows).  Like the other golden generators it
stores outputs only; weights and episodes are regenerated from seeds by synthetic.py.

  (a) float64: set_forward scores and set_forward_loss of DKT(ResNet10, 5-way 5-shot, cossim) on
      synthetic.train_episode(32, 5, 5, 16, 84) with synthetic.resnet10_state_dict(seed=32, prefix="feature.") and the
      hyperparameters of synthetic.dkt_head_state(32);
  (b) float64: the three head gradients ("headgrad:<name>"), every BatchNorm gradient, and the gradient norm of every parameter;
  (c) the state-dict keys;
  (d) the step of (a), (b) in torch float32 on the CPU ("f32:<name>"), and for each stored quantity its relative L2 distance to
      the float64 value ("f32err:<name>"): the yardstick of the GPU tests.

    python tools/make_golden_dkt.py
"""
import math
import os
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.make_golden import GOLD, import_reference, make_factory  # noqa: E402
from meta_fine_tuning_amd import synthetic  # noqa: E402

SEED = 32
SIZE = 84
HEAD = ("gp.mean", "gp.raw_outputscale", "gp.raw_noise")
NOISE_FLOOR = 1e-4


def define(MetaTemplate):
    class GPHyperparameters(nn.Module):
        def __init__(self):
            super().__init__()
            self.mean = nn.Parameter(torch.zeros(1))
            self.raw_outputscale = nn.Parameter(torch.zeros(1))
            self.raw_noise = nn.Parameter(torch.full((1,), math.log(math.expm1(0.1 - NOISE_FLOOR))))

    class DKT(MetaTemplate):
        def __init__(self, model_func, n_way, n_support, kernel="cossim"):
            super().__init__(model_func, n_way, n_support)
            self.kernel = kernel
            self.gp = GPHyperparameters()

        def _u(self, z):
            return F.normalize(z, dim=1, eps=1e-12) if self.kernel == "cossim" else z / math.sqrt(z.shape[1])

        def _solve(self, U, per_class):
            """K = s U U^T + noise I over the rows of U (class-major, per_class rows each) -> (A = K^-1 (Y - mean), R, L)."""
            M = U.shape[0]
            s = F.softplus(self.gp.raw_outputscale)
            noise = NOISE_FLOOR + F.softplus(self.gp.raw_noise)
            K = s * (U @ U.t()) + noise * torch.eye(M, dtype=U.dtype)
            Y = 2.0 * F.one_hot(torch.arange(M) // per_class, self.n_way).to(U.dtype) - 1.0
            R = Y - self.gp.mean
            L = torch.linalg.cholesky(K)
            return torch.cholesky_solve(R, L), R, L, s

        def set_forward(self, x, is_feature=False):
            z_support, z_query = self.parse_feature(x, is_feature)
            US = self._u(z_support.contiguous().view(self.n_way * self.n_support, -1))
            UQ = self._u(z_query.contiguous().view(self.n_way * self.n_query, -1))
            A, _, _, s = self._solve(US, self.n_support)
            return self.gp.mean + UQ @ (s * (US.t() @ A))

        def set_forward_loss(self, x):
            z_support, z_query = self.parse_feature(x, False)
            z = torch.cat([z_support, z_query], dim=1).contiguous().view(self.n_way * (self.n_support + self.n_query), -1)
            N, C = z.shape[0], self.n_way
            A, R, L, _ = self._solve(self._u(z), self.n_support + self.n_query)
            logdet = 2.0 * torch.log(torch.diagonal(L)).sum()
            return (0.5 * (R * A).sum() + 0.5 * C * logdet + 0.5 * C * N * math.log(2.0 * math.pi)) / N

    return DKT


def step(DKT, backbone, dtype):
    """One meta-training step in ``dtype`` -> dict of the stored quantities."""
    sd = synthetic.resnet10_state_dict(seed=SEED, prefix="feature.")
    sd.update(synthetic.dkt_head_state(SEED))
    model = DKT(make_factory(backbone, SIZE), n_way=5, n_support=5)
    model.load_state_dict(sd)
    model = model.to(dtype)
    model.train()
    model.n_query = 16
    x = synthetic.train_episode(SEED, 5, 5, 16, SIZE).to(dtype)
    out = {}
    loss = model.set_forward_loss(x)
    loss.backward()
    out["loss"] = np.array(float(loss.detach()), dtype=np.float64)
    named = list(model.named_parameters())
    out["gradnorms"] = np.array([float(p.grad.double().norm()) for _, p in named])
    for name, p in named:
        if name in HEAD:
            out["headgrad:" + name] = p.grad.detach().numpy().copy()
    bn = []
    for mname, mod in model.feature.named_modules():
        if isinstance(mod, nn.BatchNorm2d):
            for pn in ("weight", "bias"):
                key = "feature.%s.%s" % (mname, pn)
                bn.append(key)
                out["bngrad:" + key] = getattr(mod, pn).grad.detach().numpy().copy()
    with torch.no_grad():                       # (after the loss: a train-mode forward moves the running statistics, which neither reads)
        out["scores"] = model.set_forward(x).numpy()
    meta = {"gradnames": np.array([n for n, _ in named]), "bnnames": np.array(bn),
            "state_keys": np.array(list(model.state_dict().keys()))}
    return out, meta


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(b.ravel()), 1e-300))


def main():
    torch.set_num_threads(8)
    import_reference()
    import backbone
    from methods.meta_template import MetaTemplate
    DKT = define(MetaTemplate)
    out, meta = step(DKT, backbone, torch.float64)
    out.update(meta)
    o32, _ = step(DKT, backbone, torch.float32)
    for k, v in o32.items():
        out["f32err:" + k] = np.array(rel(v, out[k]))
        out["f32:" + k] = np.asarray(v, dtype=np.float32)
    path = os.path.join(GOLD, "g32_dkt.npz")
    np.savez(path, **out)
    print("g32 done: %s (%d bytes) loss %.6f" % (path, os.path.getsize(path), float(out["loss"])))
    for k in sorted(out):
        if k.startswith("f32err:"):
            print("  %-60s %.3e" % (k, float(np.max(out[k]))))


if __name__ == "__main__":
    main()
