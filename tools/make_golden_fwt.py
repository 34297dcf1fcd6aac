"""Generate tests/golden/g28_resnet10_fw.npz: the reference's own ResNet10_FW (backbone.py:90-130,313-350,521-522) under its GnnNet,
run on the CPU.

Build-box only: it needs the reference tree (oracle.make_golden.REF) and imports its ``backbone`` / ``methods.gnnnet`` with
oracle.make_golden's recipe.  Like the other golden generators it stores outputs only; weights and episodes are regenerated from
seeds by synthetic.py.

The feature-wise transformation layers call ``torch.randn`` in every train-mode forward.  During a step that call is wrapped: the
first forward makes every draw in float32 and records it, every later forward of the step replays the recorded draws, each cast to
the model's dtype -- so the stored noise [1, 2, 1856] (row 0 = n_g, row 1 = n_b, the seven layers in draw order at columns 0, 64,
192, 320, 576, 832, 1344) is exactly what the engine consumes through autograd_ops.fwt_forced_noise, and scores, loss and both
backward passes of a step see the same noise.

  (a) float64: set_forward scores and set_forward_loss of GnnNet(ResNet10_FW, 5-way 5-shot, 16 queries) on
      synthetic.train_episode(28, 5, 5, 16, 84) with synthetic.resnet10_fw_state_dict(28, prefix="feature.") and
      synthetic.gnn_head_state_dict(29); the noise;
  (b) float64: every BatchNorm / feature-wise layer's weight and bias gradient, every parameter's gradient norm, and -- from a
      second backward with ``requires_grad = True`` on them -- the gamma / beta gradients ("fwtgrad:<name>");
  (c) the state-dict keys, the parameter names and their ``requires_grad`` flags;
  (d) the step of (a), (b) in torch float32 on the CPU with the same noise ("f32:<name>"), and for each stored quantity its relative
      L2 distance to the float64 value ("f32err:<name>");
  (e) eval-mode features of the episode's first 10 images (float64 "eval_feats", float32 "f32:eval_feats").

    python tools/make_golden_fwt.py
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.make_golden import GOLD, import_reference, pool_for  # noqa: E402
from meta_fine_tuning_amd import synthetic  # noqa: E402
from meta_fine_tuning_amd.backbone import FWT_COLS, FWT_LAYERS  # noqa: E402

SEED = 28
SIZE = 84


def make_factory(backbone, size):
    """oracle.make_golden.make_factory for ResNet10_FW."""
    def f(flatten=True):
        m = backbone.ResNet10_FW(flatten)
        if size != 224:
            m.trunk[8] = nn.AvgPool2d(pool_for(size))
        return m
    return f


class NoiseTape:
    """Stands in for ``torch.randn`` while a step runs: records the 14 float32 draws of the first forward, replays them afterwards."""

    def __init__(self, noise=None):
        self.real = torch.randn
        self.draws = [] if noise is None else self.split(noise)
        self.recording = noise is None
        self.at = 0

    @staticmethod
    def split(noise):
        out = []
        for _, C, col in FWT_LAYERS:
            out += [noise[0, 0, col:col + C].clone(), noise[0, 1, col:col + C].clone()]
        return out

    def noise(self):
        n = torch.zeros(1, 2, FWT_COLS, dtype=torch.float32)
        for i, (_, C, col) in enumerate(FWT_LAYERS):
            n[0, 0, col:col + C], n[0, 1, col:col + C] = self.draws[2 * i], self.draws[2 * i + 1]
        return n

    def __call__(self, *size, dtype=None, device=None, **kw):
        if self.recording:
            d = self.real(*size, dtype=torch.float32)
            self.draws.append(d.reshape(-1).clone())
            if len(self.draws) == 2 * len(FWT_LAYERS):
                self.recording = False
        else:
            d = self.draws[self.at % len(self.draws)].reshape(*size)
            self.at += 1
        return d.to(dtype or torch.get_default_dtype())

    def __enter__(self):
        torch.randn = self
        return self

    def __exit__(self, *exc):
        torch.randn = self.real
        return False


def state():
    sd = synthetic.resnet10_fw_state_dict(SEED, prefix="feature.")
    sd.update(synthetic.gnn_head_state_dict(SEED + 1, 5))
    return sd


def build(GnnNet, backbone, dtype):
    model = GnnNet(make_factory(backbone, SIZE), n_way=5, n_support=5)
    model.load_state_dict(state())
    model = model.to(dtype)
    model.support_label = model.support_label.to(dtype)
    model.n_query = 16
    return model


def step(GnnNet, backbone, dtype, noise=None):
    """One meta-training step in ``dtype`` -> (dict of the stored quantities, names, the noise)."""
    model = build(GnnNet, backbone, dtype)
    model.train()
    x = synthetic.train_episode(SEED, 5, 5, 16, SIZE).to(dtype)
    out = {}
    torch.manual_seed(SEED)
    with NoiseTape(noise) as tape:
        with torch.no_grad():
            out["scores"] = model.set_forward(x).numpy()
        loss = model.set_forward_loss(x)
        loss.backward()
        out["loss"] = np.array(float(loss.detach()), dtype=np.float64)
        named = list(model.named_parameters())
        trainable = [(n, p) for n, p in named if p.requires_grad]
        out["gradnorms"] = np.array([float(p.grad.double().norm()) for _, p in trainable])
        bn = []
        for mname, mod in model.feature.named_modules():
            if isinstance(mod, nn.BatchNorm2d):
                for pn in ("weight", "bias"):
                    key = "feature.%s.%s" % (mname, pn)
                    bn.append(key)
                    out["bngrad:" + key] = getattr(mod, pn).grad.detach().numpy().copy()
        # the learned variant: gamma / beta trainable, same noise
        fw = [(n, p) for n, p in named if n.endswith((".gamma", ".beta"))]
        for _, p in named:
            p.grad = None
        for _, p in fw:
            p.requires_grad = True
        model.set_forward_loss(x).backward()
        for n, p in fw:
            out["fwtgrad:" + n] = p.grad.detach().numpy().copy()
        for _, p in fw:
            p.requires_grad = False
    meta = {"gradnames": np.array([n for n, _ in trainable]), "bnnames": np.array(bn), "fwtnames": np.array([n for n, _ in fw]),
            "state_keys": np.array(list(model.state_dict().keys())), "param_names": np.array([n for n, _ in named]),
            "param_requires_grad": np.array([bool(p.requires_grad) for _, p in named])}
    ev = build(GnnNet, backbone, dtype)
    ev.eval()
    with torch.no_grad():
        out["eval_feats"] = ev.feature(x.reshape(-1, 3, SIZE, SIZE)[:10]).numpy()
    return out, meta, tape.noise()


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(b.ravel()), 1e-300))


def main():
    torch.set_num_threads(8)
    import_reference()
    import backbone
    from methods.gnnnet import GnnNet
    out, meta, noise = step(GnnNet, backbone, torch.float64)
    out.update(meta)
    out["noise"] = noise.numpy()
    o32, _, n32 = step(GnnNet, backbone, torch.float32, noise)
    assert torch.equal(n32, noise)
    for k, v in o32.items():
        out["f32err:" + k] = np.array(rel(v, out[k]))
        out["f32:" + k] = np.asarray(v, dtype=np.float32)
    path = os.path.join(GOLD, "g28_resnet10_fw.npz")
    np.savez(path, **out)
    print("g28 done: %s (%d bytes) loss %.6f" % (path, os.path.getsize(path), float(out["loss"])))
    for k in sorted(out):
        if k.startswith("f32err:"):
            print("  %-60s %.3e" % (k, float(np.max(out[k]))))


if __name__ == "__main__":
    main()
