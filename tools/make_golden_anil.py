"""Generate tests/golden/g33_anil.npz: the ANIL definition of DESIGN.md section 21 written as a plain torch chain on the
reference's MetaTemplate, run on the CPU.

Build-box only: it needs the reference tree (oracle.make_golden.REF) and imports its ``backbone`` / ``methods.meta_template`` with
oracle.make_golden's recipe; the reference ships no methods/anil.py, so the class below IS the definition ("Almost No Inner Loop",
Raghu et al., ICLR 2020: per episode a linear classifier takes INNER_STEPS gradient steps from its trained initialisation on the
support rows, the queries are scored by the adapted classifier, and the outer gradient runs through the inner steps).  Like the
other golden generators it stores outputs only; weights and episodes are regenerated from seeds by synthetic.py.

  (a) float64: set_forward scores and set_forward_loss of ANIL(ResNet10, 5-way 5-shot, 5 steps of 0.01) on
      synthetic.train_episode(33, 5, 5, 16, 84) with synthetic.resnet10_state_dict(seed=33, prefix="feature.") and the
      initialisation of synthetic.anil_head_state(33);
  (b) float64: the two head gradients ("headgrad:<name>"), every BatchNorm gradient, and the gradient norm of every parameter;
  (c) the state-dict keys;
  (d) the step of (a), (b) in torch float32 on the CPU ("f32:<name>"), and for each stored quantity its relative L2 distance to
      the float64 value ("f32err:<name>"): the yardstick of the GPU tests.

    python tools/make_golden_anil.py
"""
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

SEED = 33
SIZE = 84
HEAD = ("classifier.weight", "classifier.bias")


def define(MetaTemplate):
    class ANIL(MetaTemplate):
        def __init__(self, model_func, n_way, n_support, inner_steps=5, inner_lr=0.01):
            super().__init__(model_func, n_way, n_support)
            self.inner_steps = inner_steps
            self.inner_lr = float(np.float32(inner_lr))          # the launchers take the step size as a C float
            self.loss_fn = nn.CrossEntropyLoss()
            self.classifier = nn.Linear(self.feat_dim, n_way)
            self.classifier.bias.data.fill_(0)

        def set_forward(self, x, is_feature=False):
            z_support, z_query = self.parse_feature(x, is_feature)
            z_support = z_support.contiguous().view(self.n_way * self.n_support, -1)
            z_query = z_query.contiguous().view(self.n_way * self.n_query, -1)
            y_support = torch.arange(self.n_way).repeat_interleave(self.n_support)
            W, b = self.classifier.weight, self.classifier.bias
            with torch.enable_grad():
                for _ in range(self.inner_steps):
                    inner = F.cross_entropy(z_support @ W.t() + b, y_support)
                    gW, gb = torch.autograd.grad(inner, (W, b), create_graph=True)
                    W, b = W - self.inner_lr * gW, b - self.inner_lr * gb
            return z_query @ W.t() + b

        def set_forward_loss(self, x):
            y_query = torch.arange(self.n_way).repeat_interleave(self.n_query)
            return self.loss_fn(self.set_forward(x), y_query)

    return ANIL


def step(ANIL, backbone, dtype):
    """One meta-training step in ``dtype`` -> dict of the stored quantities."""
    sd = synthetic.resnet10_state_dict(seed=SEED, prefix="feature.")
    sd.update(synthetic.anil_head_state(SEED))
    model = ANIL(make_factory(backbone, SIZE), n_way=5, n_support=5)
    model.load_state_dict(sd)
    model = model.to(dtype)
    model.train()
    model.n_query = 16
    x = synthetic.train_episode(SEED, 5, 5, 16, SIZE).to(dtype)
    out = {}
    scores = model.set_forward(x)
    loss = model.loss_fn(scores, torch.arange(5).repeat_interleave(16))
    loss.backward()
    out["scores"] = scores.detach().numpy().copy()
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
    ANIL = define(MetaTemplate)
    out, meta = step(ANIL, backbone, torch.float64)
    out.update(meta)
    o32, _ = step(ANIL, backbone, torch.float32)
    for k, v in o32.items():
        out["f32err:" + k] = np.array(rel(v, out[k]))
        out["f32:" + k] = np.asarray(v, dtype=np.float32)
    path = os.path.join(GOLD, "g33_anil.npz")
    np.savez(path, **out)
    print("g33 done: %s (%d bytes) loss %.6f" % (path, os.path.getsize(path), float(out["loss"])))
    for k in sorted(out):
        if k.startswith("f32err:"):
            print("  %-60s %.3e" % (k, float(np.max(out[k]))))


if __name__ == "__main__":
    main()
