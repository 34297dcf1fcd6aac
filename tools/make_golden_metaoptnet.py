"""Generate tests/golden/g27_metaoptnet.npz: the MetaOptNet definition of DESIGN.md section 14 written with torch's own
cholesky / cholesky_solve on the reference's MetaTemplate, run on the CPU.

Build-box only: it needs the reference tree (oracle.make_golden.REF) and imports its ``backbone`` / ``finetune`` /
``methods.meta_template`` with oracle.make_golden's recipe; the reference ships no methods/metaoptnet.py, so the class below IS the
definition (the ridge-regression head of MetaOptNet, Lee et al., CVPR 2019).  Like the other golden generators it stores outputs
only; weights and episodes are regenerated from seeds by synthetic.py.

  (a) float64: set_forward scores and set_forward_loss of MetaOptNet(ResNet10, 5-way 5-shot) on
      synthetic.train_episode(27, 5, 5, 16, 84) with synthetic.resnet10_state_dict(seed=27, prefix="feature.") and the scale of
      synthetic.metaoptnet_head_state(27);
  (b) float64: d(loss)/d(scale) ("scalegrad"), every BatchNorm gradient, and the gradient norm of every parameter;
  (c) the state-dict keys;
  (d) float32: finetune.finetune() scores with the model on synthetic.test_episode(41, 5, 5, 15, 84, gen_examples=0) at
      fine_tune_epoch 0 and 1 (backbone of synthetic.resnet10_state_dict(seed=13), numpy seeded with 10 -- as G22);
  (e) the step of (a), (b) in torch float32 on the CPU ("f32:<name>"), and for each stored quantity its relative L2 distance to
      the float64 value ("f32err:<name>"): the yardstick of the GPU tests.

    python tools/make_golden_metaoptnet.py
"""
import argparse
import copy
import os
import sys

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.make_golden import GOLD, import_reference, make_factory  # noqa: E402
from meta_fine_tuning_amd import synthetic  # noqa: E402

SEED = 27
SIZE = 84


def define(MetaTemplate):
    class MetaOptNet(MetaTemplate):
        lambda_reg = 50.0

        def __init__(self, model_func, n_way, n_support):
            super().__init__(model_func, n_way, n_support)
            self.loss_fn = nn.CrossEntropyLoss()
            self.scale = nn.Parameter(torch.ones(1))

        def state_dict(self, *args, **kwargs):
            sd = super().state_dict(*args, **kwargs)          # ``scale`` after the feature.* keys
            key = kwargs.get("prefix", args[1] if len(args) > 1 else "") + "scale"
            if key in sd:
                sd.move_to_end(key)
            return sd

        def set_forward(self, x, is_feature=False):
            z_support, z_query = self.parse_feature(x, is_feature)
            z_support = z_support.contiguous().view(self.n_way * self.n_support, -1)
            z_query = z_query.contiguous().view(self.n_way * self.n_query, -1)
            y_s = torch.from_numpy(np.repeat(range(self.n_way), self.n_support))
            Y = torch.zeros(y_s.numel(), self.n_way, dtype=z_support.dtype).scatter_(1, y_s.view(-1, 1), 1.0)
            A = z_support.mm(z_support.t()) + self.lambda_reg * torch.eye(y_s.numel(), dtype=z_support.dtype)
            alpha = 2.0 * torch.cholesky_solve(Y, torch.linalg.cholesky(A))
            W = z_support.t().mm(alpha)
            return self.scale * z_query.mm(W)

        def set_forward_loss(self, x):
            y_query = torch.from_numpy(np.repeat(range(self.n_way), self.n_query))
            return self.loss_fn(self.set_forward(x), y_query)

    return MetaOptNet


def step(MetaOptNet, backbone, dtype):
    """One meta-training step in ``dtype`` -> dict of the stored quantities."""
    sd = synthetic.resnet10_state_dict(seed=SEED, prefix="feature.")
    sd.update(synthetic.metaoptnet_head_state(SEED))
    model = MetaOptNet(make_factory(backbone, SIZE), n_way=5, n_support=5)
    model.load_state_dict(sd)
    model = model.to(dtype)
    model.train()
    model.n_query = 16
    x = synthetic.train_episode(SEED, 5, 5, 16, SIZE).to(dtype)
    out = {}
    with torch.no_grad():
        out["scores"] = model.set_forward(x).numpy()
    loss = model.set_forward_loss(x)
    loss.backward()
    out["loss"] = np.array(float(loss.detach()), dtype=np.float64)
    named = list(model.named_parameters())
    out["gradnorms"] = np.array([float(p.grad.double().norm()) for _, p in named])
    out["scalegrad"] = model.scale.grad.detach().numpy().copy()
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
    import finetune
    from methods.meta_template import MetaTemplate
    MetaOptNet = define(MetaTemplate)
    out, meta = step(MetaOptNet, backbone, torch.float64)
    out.update(meta)
    o32, _ = step(MetaOptNet, backbone, torch.float32)
    for k, v in o32.items():
        out["f32err:" + k] = np.array(rel(v, out[k]))
        out["f32:" + k] = np.asarray(v, dtype=np.float32)

    # (d): test-time finetune() with the MetaOptNet model doing the final scoring (float32, as the reference runs it)
    sd13 = synthetic.resnet10_state_dict(seed=13, prefix="feature.")
    full13 = dict(sd13)
    full13.update(synthetic.metaoptnet_head_state(SEED))
    liz = synthetic.test_episode(41, 5, 5, 15, SIZE, gen_examples=0)
    for E in (0, 1):
        finetune.params = argparse.Namespace(model="ResNet10", fine_tune_epoch=E)
        finetune.model_dict["ResNet10"] = make_factory(backbone, SIZE)
        mm = MetaOptNet(make_factory(backbone, SIZE), n_way=5, n_support=5)
        mm.load_state_dict(full13)
        mm.train()
        np.random.seed(10)
        sc = finetune.finetune(liz, None, mm, copy.deepcopy(sd13), None, n_query=15, n_way=5, n_support=5)
        out["finetune_scores_E%d" % E] = sc.numpy()
    path = os.path.join(GOLD, "g27_metaoptnet.npz")
    np.savez(path, **out)
    print("g27 done: %s (%d bytes) loss %.6f" % (path, os.path.getsize(path), float(out["loss"])))
    for k in sorted(out):
        if k.startswith("f32err:"):
            print("  %-60s %.3e" % (k, float(np.max(out[k]))))


if __name__ == "__main__":
    main()
