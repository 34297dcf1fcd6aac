"""Generate tests/golden/g22_protonet.npz by running the REFERENCE ProtoNet (methods/protonet.py) on the CPU.

Build-box only: it needs the reference tree (oracle.make_golden.REF) and imports it with oracle.make_golden's recipe.  Like the
other golden generators it stores outputs only; weights and episodes are regenerated from seeds by synthetic.py.

  (a) set_forward scores and set_forward_loss of ProtoNet(ResNet10, 5-way 5-shot) on synthetic.train_episode(22, 5, 5, 16, 84)
      with synthetic.resnet10_state_dict(seed=22, prefix="feature.");
  (b) the gradients of every BatchNorm weight / bias of that loss, and the L2 norm of every feature parameter's gradient;
  (c) the reference ProtoNet's state_dict keys;
  (d) finetune.finetune() scores with a ProtoNet model on synthetic.test_episode(41, 5, 5, 15, 84, gen_examples=0) at
      fine_tune_epoch 0 and 1 (backbone of synthetic.gnnnet_state_dict(seed=13), numpy seeded with 10 -- as G5).

    python tools/make_golden_protonet.py
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

SEED = 22
SIZE = 84


def main():
    torch.set_num_threads(8)
    import_reference()
    import backbone
    import finetune
    from methods.protonet import ProtoNet
    out = {}

    # (a), (b), (c): one meta-training step
    sd = synthetic.resnet10_state_dict(seed=SEED, prefix="feature.")
    model = ProtoNet(make_factory(backbone, SIZE), n_way=5, n_support=5)
    model.load_state_dict(sd)
    model.train()
    model.n_query = 16
    x = synthetic.train_episode(SEED, 5, 5, 16, SIZE)
    with torch.no_grad():
        out["scores"] = model.set_forward(x).numpy()
    loss = model.set_forward_loss(x)
    loss.backward()
    out["loss"] = np.array(float(loss.detach()))
    names = [n for n, _ in model.named_parameters()]
    out["gradnames"] = np.array(names)
    out["gradnorms"] = np.array([float(p.grad.norm()) for _, p in model.named_parameters()])
    bn = []
    for mname, mod in model.feature.named_modules():
        if isinstance(mod, nn.BatchNorm2d):
            for pn in ("weight", "bias"):
                key = "feature.%s.%s" % (mname, pn)
                bn.append(key)
                out["bngrad:" + key] = getattr(mod, pn).grad.detach().numpy().copy()
    out["bnnames"] = np.array(bn)
    out["state_keys"] = np.array(list(model.state_dict().keys()))

    # (d): test-time finetune() with a ProtoNet model doing the final scoring
    sd13 = synthetic.resnet10_state_dict(seed=13, prefix="feature.")
    liz = synthetic.test_episode(41, 5, 5, 15, SIZE, gen_examples=0)
    for E in (0, 1):
        finetune.params = argparse.Namespace(model="ResNet10", fine_tune_epoch=E)
        finetune.model_dict["ResNet10"] = make_factory(backbone, SIZE)
        pm = ProtoNet(make_factory(backbone, SIZE), n_way=5, n_support=5)
        pm.load_state_dict(sd13)
        pm.train()
        np.random.seed(10)
        sc = finetune.finetune(liz, None, pm, copy.deepcopy(sd13), None, n_query=15, n_way=5, n_support=5)
        out["finetune_scores_E%d" % E] = sc.numpy()
    path = os.path.join(GOLD, "g22_protonet.npz")
    np.savez(path, **out)
    print("g22 done: %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
