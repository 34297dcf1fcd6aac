"""Generate tests/golden/g34_mahalanobis.npz: the Mahalanobis head of DESIGN.md section 22 written as a plain torch chain (the dense
definition, torch.linalg.inv on the D x D class covariances) on the reference's MetaTemplate, run on the CPU.

Build-box only: it needs the reference tree (oracle.make_golden.REF) and imports its ``backbone`` / ``methods.meta_template`` with
oracle.make_golden's recipe; the reference ships no methods/mahalanobis.py, so the class below IS the definition (the classifier of
Simple CNAPS, Bateni et al., CVPR 2020: per class a regularised covariance blended from the class's and the task's unbiased sample
covariances, scores = minus half the squared Mahalanobis distance to the class mean).  Weights and the episode are regenerated
from seeds by synthetic.py; the head's own inputs and input gradients are stored.

  (a) float64: set_forward scores and set_forward_loss of Mahalanobis(ResNet10, 5-way 5-shot) on
      synthetic.train_episode(34, 5, 5, 15, 84) with synthetic.resnet10_state_dict(seed=34, prefix="feature.");
  (b) float64 rounded to float32: the head's input "feats" [100, 512] (the trunk's output) and "dfeats", d loss / d feats;
  (c) float64: every BatchNorm gradient and the gradient norm of every parameter;
  (d) the state-dict keys (``feature.*`` only: the head has no parameters);
  (e) the step of (a) - (c) in torch float32 on the CPU ("f32:<name>", but for feats and dfeats), and for each stored quantity its
      relative L2 distance to the float64 value ("f32err:<name>"): the yardstick of the GPU tests.

    python tools/make_golden_mahalanobis.py
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.make_golden import GOLD, import_reference, make_factory  # noqa: E402
from meta_fine_tuning_amd import synthetic  # noqa: E402

SEED = 34
SIZE = 84
N_WAY, N_SUPPORT, N_QUERY = 5, 5, 15
BETA = 1.0


def define(MetaTemplate):
    class Mahalanobis(MetaTemplate):
        def __init__(self, model_func, n_way, n_support):
            super().__init__(model_func, n_way, n_support)
            self.loss_fn = nn.CrossEntropyLoss()

        def head(self, z_support, z_query):
            """z_support [n_way, n, D], z_query [n_way * n_query, D] -> scores [n_way * n_query, n_way]."""
            n_way, n, D = z_support.shape
            S = n_way * n
            lam = n / (n + 1.0)
            eye = torch.eye(D, dtype=z_support.dtype)
            zero = torch.zeros(D, D, dtype=z_support.dtype)
            flat = z_support.reshape(S, D)
            T = flat - flat.mean(0, keepdim=True)
            St = T.t() @ T / (S - 1) if S > 1 else zero
            cols = []
            for c in range(n_way):
                mu = z_support[c].mean(0)
                Tc = z_support[c] - mu
                Sc = Tc.t() @ Tc / (n - 1) if n > 1 else zero
                d = z_query - mu
                Qinv = torch.linalg.inv(lam * Sc + (1.0 - lam) * St + BETA * eye)
                cols.append(-0.5 * ((d @ Qinv) * d).sum(1))
            return torch.stack(cols, dim=1)

        def set_forward(self, x, is_feature=False):
            z_support, z_query = self.parse_feature(x, is_feature)
            self.z_all = torch.cat([z_support, z_query], dim=1)              # the head's input, class-major rows
            self.z_all.retain_grad()
            z = self.z_all
            return self.head(z[:, :self.n_support].contiguous(), z[:, self.n_support:].contiguous().view(self.n_way * self.n_query, -1))

        def set_forward_loss(self, x):
            y_query = torch.arange(self.n_way).repeat_interleave(self.n_query)
            return self.loss_fn(self.set_forward(x), y_query)

    return Mahalanobis


def step(Mahalanobis, backbone, dtype):
    """One meta-training step in ``dtype`` -> dict of the stored quantities."""
    sd = synthetic.resnet10_state_dict(seed=SEED, prefix="feature.")
    model = Mahalanobis(make_factory(backbone, SIZE), n_way=N_WAY, n_support=N_SUPPORT)
    model.load_state_dict(sd)
    model = model.to(dtype)
    model.train()
    model.n_query = N_QUERY
    x = synthetic.train_episode(SEED, N_WAY, N_SUPPORT, N_QUERY, SIZE).to(dtype)
    out = {}
    scores = model.set_forward(x)
    loss = model.loss_fn(scores, torch.arange(N_WAY).repeat_interleave(N_QUERY))
    loss.backward()
    out["scores"] = scores.detach().numpy().copy()
    out["loss"] = np.array(float(loss.detach()), dtype=np.float64)
    out["feats"] = model.z_all.detach().reshape(-1, model.z_all.shape[-1]).numpy().copy()
    out["dfeats"] = model.z_all.grad.detach().reshape(-1, model.z_all.shape[-1]).numpy().copy()
    named = list(model.named_parameters())
    out["gradnorms"] = np.array([float(p.grad.double().norm()) for _, p in named])
    bn = []
    for mname, mod in model.feature.named_modules():
        if isinstance(mod, nn.BatchNorm2d):
            for pn in ("weight", "bias"):
                key = "feature.%s.%s" % (mname, pn)
                bn.append(key)
                out["bngrad:" + key] = getattr(mod, pn).grad.detach().numpy().copy()
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
    Mahalanobis = define(MetaTemplate)
    out, meta = step(Mahalanobis, backbone, torch.float64)
    o32, _ = step(Mahalanobis, backbone, torch.float32)
    for k, v in o32.items():
        out["f32err:" + k] = np.array(rel(v, out[k]))
        if k not in ("feats", "dfeats"):
            out["f32:" + k] = np.asarray(v, dtype=np.float32)
    for k in ("feats", "dfeats"):
        out[k] = out[k].astype(np.float32)
    out.update(meta)
    path = os.path.join(GOLD, "g34_mahalanobis.npz")
    np.savez(path, **out)
    print("g34 done: %s (%d bytes) loss %.6f" % (path, os.path.getsize(path), float(out["loss"])))
    for k in sorted(out):
        if k.startswith("f32err:"):
            print("  %-60s %.3e" % (k, float(np.max(out[k]))))


if __name__ == "__main__":
    main()
