"""Generate tests/golden/g29_metaoptnet_svm.npz: the MetaOptNet-SVM definition of DESIGN.md section 17 on the reference's
MetaTemplate, run on the CPU, with the contents (a) to (d) of G27 (tools/make_golden_metaoptnet.py) at the same seeds and inputs.

Build-box only: it needs the reference tree (oracle.make_golden.REF).  The head is the float64 oracle of
tests/test_metaoptnet_svm_cpu.py (numpy; it shares nothing with the package), wrapped in its torch.autograd.Function; the class
below puts it on the reference's MetaTemplate.  Like the other golden generators it stores outputs only.

  (a) float64: set_forward scores and set_forward_loss of MetaOptNet-SVM(ResNet10, 5-way 5-shot) on
      synthetic.train_episode(27, 5, 5, 16, 84) with synthetic.resnet10_state_dict(seed=27, prefix="feature.") and the scale of
      synthetic.metaoptnet_head_state(27); "alpha" [25, 5] and "free" [25, 5] of that episode's dual;
  (b) float64: d(loss)/d(scale) ("scalegrad"), every BatchNorm gradient, and the gradient norm of every parameter;
  (c) the state-dict keys;
  (d) float32 backbone, float64 head: finetune.finetune() scores with the model on synthetic.test_episode(41, 5, 5, 15, 84,
      gen_examples=0) at fine_tune_epoch 0 and 1 (backbone of synthetic.resnet10_state_dict(seed=13), numpy seeded with 10).

    python tools/make_golden_metaoptnet_svm.py
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle.make_golden import GOLD, import_reference, make_factory  # noqa: E402
from meta_fine_tuning_amd import synthetic  # noqa: E402
import test_metaoptnet_svm_cpu as T  # noqa: E402

SEED = 27
SIZE = 84


def define(MetaTemplate):
    class MetaOptNetSVM(MetaTemplate):
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
            z = torch.cat([z_support, z_query], dim=1)        # [n_way, n_support + n_query, D]
            scores = T.SvmHead64.apply(z.reshape(-1, z.shape[-1]).double(), self.scale.double(), self.n_way, self.n_support)
            return scores.to(z.dtype)

        def set_forward_loss(self, x):
            y_query = torch.from_numpy(np.repeat(range(self.n_way), self.n_query))
            return self.loss_fn(self.set_forward(x), y_query)

    return MetaOptNetSVM


def main():
    torch.set_num_threads(8)
    import_reference()
    import backbone
    import finetune
    from methods.meta_template import MetaTemplate
    Model = define(MetaTemplate)
    sd = synthetic.resnet10_state_dict(seed=SEED, prefix="feature.")
    sd.update(synthetic.metaoptnet_head_state(SEED))
    model = Model(make_factory(backbone, SIZE), n_way=5, n_support=5)
    model.load_state_dict(sd)
    model = model.double()
    model.train()
    model.n_query = 16
    x = synthetic.train_episode(SEED, 5, 5, 16, SIZE).double()
    out = {}
    with torch.no_grad():
        out["scores"] = model.set_forward(x).numpy()
        zs, zq = model.parse_feature(x, False)
        r = T.head_step(torch.cat([zs, zq], dim=1).numpy(), None, float(model.scale), 5, 5)
        out["alpha"], out["free"] = r["alpha"], r["free"]
    loss = model.set_forward_loss(x)
    loss.backward()
    out["loss"] = np.array(float(loss.detach()), dtype=np.float64)
    named = list(model.named_parameters())
    out["gradnames"] = np.array([n for n, _ in named])
    out["gradnorms"] = np.array([float(p.grad.double().norm()) for _, p in named])
    out["scalegrad"] = model.scale.grad.detach().numpy().copy()
    bn = []
    for mname, mod in model.feature.named_modules():
        if isinstance(mod, nn.BatchNorm2d):
            for pn in ("weight", "bias"):
                key = "feature.%s.%s" % (mname, pn)
                bn.append(key)
                out["bngrad:" + key] = getattr(mod, pn).grad.detach().numpy().copy()
    out["bnnames"] = np.array(bn)
    out["state_keys"] = np.array(list(model.state_dict().keys()))

    sd13 = synthetic.resnet10_state_dict(seed=13, prefix="feature.")
    full13 = dict(sd13)
    full13.update(synthetic.metaoptnet_head_state(SEED))
    liz = synthetic.test_episode(41, 5, 5, 15, SIZE, gen_examples=0)
    for E in (0, 1):
        finetune.params = argparse.Namespace(model="ResNet10", fine_tune_epoch=E)
        finetune.model_dict["ResNet10"] = make_factory(backbone, SIZE)
        mm = Model(make_factory(backbone, SIZE), n_way=5, n_support=5)
        mm.load_state_dict(full13)
        mm.train()
        np.random.seed(10)
        sc = finetune.finetune(liz, None, mm, copy.deepcopy(sd13), None, n_query=15, n_way=5, n_support=5)
        out["finetune_scores_E%d" % E] = sc.detach().numpy()
    path = os.path.join(GOLD, "g29_metaoptnet_svm.npz")
    np.savez(path, **out)
    print("g29 done: %s (%d bytes) loss %.6f, %d of %d entries free" % (path, os.path.getsize(path), float(out["loss"]),
                                                                     int(out["free"].sum()), out["free"].size))


if __name__ == "__main__":
    main()
