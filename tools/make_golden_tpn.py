"""Generate tests/golden/g30_tpn.npz: the TPN definition of DESIGN.md section 18 written as a plain torch chain on the
reference's MetaTemplate, run on the CPU.

Build-box only: it needs the reference tree (oracle.make_golden.REF) and imports its ``backbone`` / ``methods.meta_template`` with
oracle.make_golden's recipe; the reference ships no methods/tpn.py, so the class below IS the definition (the label-propagation
head of the Transductive Propagation Network, Liu et al., ICLR 2019, on pooled features, scoring the query nodes).  Like the other
golden generators it stores outputs only; weights and episodes are regenerated from seeds by synthetic.py.

  (a) float64: set_forward scores and set_forward_loss of TPN(ResNet10, 5-way 5-shot) on synthetic.train_episode(30, 5, 5, 16, 84)
      with synthetic.resnet10_state_dict(seed=30, prefix="feature.") and the head of synthetic.tpn_head_state(30); the symmetrised
      neighbour mask [105, 105] (uint8) of that forward;
  (b) float64: the four head gradients ("headgrad:<name>"), every BatchNorm gradient, and the gradient norm of every parameter;
  (c) the state-dict keys;
  (d) the step of (a), (b) in torch float32 on the CPU ("f32:<name>"), and for each stored quantity its relative L2 distance to
      the float64 value ("f32err:<name>"): the yardstick of the GPU tests.  The float32 step takes the float64 step's mask, so
      that the two differ by rounding and not by a neighbour that changed sides.

    python tools/make_golden_tpn.py
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

SEED = 30
SIZE = 84
HEAD = ("relation.fc3.weight", "relation.fc3.bias", "relation.fc4.weight", "relation.fc4.bias")


def define(MetaTemplate):
    class RelationGraph(nn.Module):
        def __init__(self, dim):
            super().__init__()
            self.fc3 = nn.Linear(dim, 8)
            self.fc4 = nn.Linear(8, 1)

        def forward(self, z):
            return self.fc4(torch.relu(self.fc3(z)))

    class TPN(MetaTemplate):
        K, ALPHA, EPS = 20, 0.99, np.finfo(float).eps

        def __init__(self, model_func, n_way, n_support):
            super().__init__(model_func, n_way, n_support)
            self.loss_fn = nn.CrossEntropyLoss()
            self.relation = RelationGraph(self.feat_dim)
            with torch.no_grad():
                self.relation.fc4.bias.fill_(12.0)
            self.forced_mask = None             # the float32 step takes the float64 step's neighbours
            self.last_mask = None

        def set_forward(self, x, is_feature=False):
            z_support, z_query = self.parse_feature(x, is_feature)
            S, Q = self.n_way * self.n_support, self.n_way * self.n_query
            z = torch.cat([z_support.contiguous().view(S, -1), z_query.contiguous().view(Q, -1)])
            N = S + Q
            u = z / (self.relation(z) + self.EPS)
            W = torch.exp(-((u.unsqueeze(1) - u.unsqueeze(0)) ** 2).sum(2) / 2)
            if self.forced_mask is None:
                idx = torch.sort(W.detach(), dim=1, descending=True, stable=True).indices[:, :min(self.K, N)]
                mask = torch.zeros(N, N, dtype=W.dtype).scatter_(1, idx, 1.0)
                mask = ((mask + mask.t()) > 0).to(W.dtype)
            else:
                mask = self.forced_mask.to(W.dtype)
            self.last_mask = mask
            W = W * mask
            D = W.sum(0)
            r = torch.sqrt(1.0 / (D + self.EPS))
            Sn = r.unsqueeze(1) * W * r.unsqueeze(0)
            Y = torch.zeros(N, self.n_way, dtype=W.dtype)
            Y[torch.arange(S), torch.arange(S) // self.n_support] = 1.0
            Fm = torch.linalg.solve(torch.eye(N, dtype=W.dtype) - self.ALPHA * Sn, Y)
            return Fm[S:]

        def set_forward_loss(self, x):
            y_query = torch.from_numpy(np.repeat(range(self.n_way), self.n_query))
            return self.loss_fn(self.set_forward(x), y_query)

    return TPN


def step(TPN, backbone, dtype, mask=None):
    """One meta-training step in ``dtype`` -> dict of the stored quantities."""
    sd = synthetic.resnet10_state_dict(seed=SEED, prefix="feature.")
    sd.update(synthetic.tpn_head_state(SEED))
    model = TPN(make_factory(backbone, SIZE), n_way=5, n_support=5)
    model.load_state_dict(sd)
    model = model.to(dtype)
    model.train()
    model.n_query = 16
    model.forced_mask = mask
    x = synthetic.train_episode(SEED, 5, 5, 16, SIZE).to(dtype)
    out = {}
    with torch.no_grad():
        out["scores"] = model.set_forward(x).numpy()
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
    meta = {"gradnames": np.array([n for n, _ in named]), "bnnames": np.array(bn),
            "state_keys": np.array(list(model.state_dict().keys())), "mask": model.last_mask.numpy().astype(np.uint8)}
    return out, meta


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(b.ravel()), 1e-300))


def main():
    torch.set_num_threads(8)
    import_reference()
    import backbone
    from methods.meta_template import MetaTemplate
    TPN = define(MetaTemplate)
    out, meta = step(TPN, backbone, torch.float64)
    out.update(meta)
    o32, _ = step(TPN, backbone, torch.float32, mask=torch.from_numpy(meta["mask"]))
    for k, v in o32.items():
        out["f32err:" + k] = np.array(rel(v, out[k]))
        out["f32:" + k] = np.asarray(v, dtype=np.float32)
    path = os.path.join(GOLD, "g30_tpn.npz")
    np.savez(path, **out)
    print("g30 done: %s (%d bytes) loss %.6f, %d of %d mask entries set" % (path, os.path.getsize(path), float(out["loss"]),
                                                                            int(meta["mask"].sum()), meta["mask"].size))
    for k in sorted(out):
        if k.startswith("f32err:"):
            print("  %-60s %.3e" % (k, float(np.max(out[k]))))


if __name__ == "__main__":
    main()
