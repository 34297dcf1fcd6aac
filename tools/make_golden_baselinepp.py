"""Generate tests/golden/g24_baselinepp.npz by running the REFERENCE's Baseline++ code paths on the CPU.

Build-box only: it needs the reference tree (oracle.make_golden.REF) and imports it with oracle.make_golden's recipe.  The
reference calls ``backbone.distLinear`` (methods/baselinefinetune.py:31, methods/baselinetrain.py:19) but its backbone.py never
defines the class, so this tool adds its own torch statement of it -- the definition of DESIGN.md section 12 with torch's
``WeightNorm`` -- to the reference's ``backbone`` module at run time.  Outputs (and the drawn initial head) only are stored.

  (a) BaselineFinetune(ResNet10, 5, n_shot, loss_type='dist').set_forward_adaptation for n_shot = 5 and 20, n_query = 15, on the
      features abs(RandomState(271 + n_shot).standard_normal((5, n_shot + 15, 512))) as float32, with torch.manual_seed(123) and
      np.random.seed(10): the initial v / g the head drew, the final v / g, the scores, and the next np.random.permutation(7)
      (the position of the numpy stream afterwards);
  (b) one BaselineTrain(ResNet10, 10, loss_type='dist') step on 4 images at 84x84: backbone of
      synthetic.resnet10_state_dict(seed=24, prefix="feature."), images RandomState(24).standard_normal((4, 3, 84, 84)), labels
      (0, 3, 7, 9), head drawn under torch.manual_seed(124): the head's initial v / g, the loss and the gradients of g and v.

    python tools/make_golden_baselinepp.py
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

N_QUERY = 15
TRAIN_LABELS = (0, 3, 7, 9)


class distLinear(nn.Module):
    """Cosine classifier with a class-wise learnable norm: the torch module this project's HIP head is specified against."""
    made = []                       # every instance, in construction order (the reference keeps its head in a local)

    def __init__(self, indim, outdim):
        super().__init__()
        from torch.nn.utils.weight_norm import WeightNorm
        self.L = nn.Linear(indim, outdim, bias=False)
        self.class_wise_learnable_norm = True
        WeightNorm.apply(self.L, 'weight', dim=0)
        self.scale_factor = 2 if outdim <= 200 else 10
        self.initial = {k: v.detach().clone() for k, v in self.L.state_dict().items()}
        distLinear.made.append(self)

    def forward(self, x):
        x_norm = torch.norm(x, p=2, dim=1).unsqueeze(1).expand_as(x)
        return self.scale_factor * self.L(x.div(x_norm + 0.00001))


def features(n_shot):
    z = np.abs(np.random.RandomState(271 + n_shot).standard_normal((5, n_shot + N_QUERY, 512))).astype(np.float32)
    return torch.from_numpy(z)


def main():
    torch.set_num_threads(8)
    import_reference()
    import backbone
    backbone.distLinear = distLinear
    from methods.baselinefinetune import BaselineFinetune
    out = {}

    # (a) test-time adaptation
    for n_shot in (5, 20):
        model = BaselineFinetune(make_factory(backbone, 84), 5, n_shot, loss_type='dist')
        model.n_query = N_QUERY
        torch.manual_seed(123)
        np.random.seed(10)
        scores = model.set_forward_adaptation(features(n_shot))
        head = distLinear.made[-1]
        tag = "_%dshot" % n_shot
        out["v0" + tag] = head.initial["weight_v"].numpy()
        out["g0" + tag] = head.initial["weight_g"].numpy()
        out["v" + tag] = head.L.weight_v.detach().numpy().copy()
        out["g" + tag] = head.L.weight_g.detach().numpy().copy()
        out["scores" + tag] = scores.detach().numpy().copy()
        out["next_perm" + tag] = np.random.permutation(7)

    # (b) one supervised Baseline++ step
    try:
        from methods.baselinetrain import BaselineTrain
        torch.manual_seed(124)
        model = BaselineTrain(make_factory(backbone, 84), 10, loss_type='dist')
        model.feature.load_state_dict({k[len("feature."):]: v for k, v in synthetic.resnet10_state_dict(seed=24, prefix="feature.").items()})
        model.train()
        head = model.classifier
        x = torch.from_numpy(np.random.RandomState(24).standard_normal((4, 3, 84, 84)).astype(np.float32))
        loss = model.forward_loss(x, torch.tensor(TRAIN_LABELS))
        loss.backward()
        out["train_v0"] = head.initial["weight_v"].numpy()
        out["train_g0"] = head.initial["weight_g"].numpy()
        out["train_loss"] = np.array(float(loss.detach()))
        out["train_dv"] = head.L.weight_v.grad.numpy().copy()
        out["train_dg"] = head.L.weight_g.grad.numpy().copy()
    except Exception as e:            # the reference's BaselineTrain does not run through this import: say so, store nothing
        print("BaselineTrain(loss_type='dist') did not run on the CPU: %r -- part (b) left out" % (e,))
    path = os.path.join(GOLD, "g24_baselinepp.npz")
    np.savez_compressed(path, **out)
    print("g24 done: %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
