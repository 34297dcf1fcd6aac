"""Generate tests/golden/g25_baselinepp_finetune.npz: the REFERENCE's finetune_linear (finetune.py:45-174) with a cosine head.

Build-box only: it needs the reference tree (oracle.make_golden.REF) and imports it with oracle.make_golden's recipe.  The
reference's ``finetune.Classifier`` is replaced at run time by the torch statement of ``distLinear(512, n_way)`` (DESIGN.md
section 12: torch's ``WeightNorm`` on a bias-free ``nn.Linear``), ``finetune.model_dict["ResNet10"]`` by the 84 x 84 factory, and
then the reference's OWN finetune_linear runs: 20 epochs over the 25 original support images in mini-batches of 5,
Adam(0.01, weight_decay=0.001) on the head, Adam(0.01) on trunk.7, scores = softmax(head(features of the queries)).

Inputs: synthetic.gnnnet_state_dict(seed=37); synthetic.test_episode(91 | 92, 5, 5, 15, 84, gen_examples=1);
torch.manual_seed(125) and np.random.seed(10) in front of every run (an episode's head is the nn.Linear draw its first run
below makes after the backbone's own initialisation draws; it is pinned for the other two runs, because a float64 draw from
the same seed gives other numbers).

Stored per episode (suffix _91 / _92): the drawn v0 / g0; scores_f32 (8 ATen threads), scores_f32_1thr, scores_f64 (default dtype
float64, state and images cast); next_perm = np.random.permutation(7) after the run.  Nothing else: no reference code.

The three runs of an episode must agree on every argmax, and the float64 scores must separate their two best classes clearly,
otherwise nothing is written: the GPU test asserts the argmax and a distance measured in units of the fp32-vs-fp64 distance.

    python tools/make_golden_baselinepp_finetune.py
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

EPISODES = (91, 92)


class distLinear(nn.Module):
    """Cosine classifier with a class-wise learnable norm: the torch module this project's HIP head is specified against."""
    pinned = None                   # (v0, g0): the next instance starts from these instead of its own draw
    made = []

    def __init__(self, indim, outdim):
        super().__init__()
        from torch.nn.utils.weight_norm import WeightNorm
        self.L = nn.Linear(indim, outdim, bias=False)
        WeightNorm.apply(self.L, 'weight', dim=0)
        if distLinear.pinned is not None:
            v0, g0 = distLinear.pinned
            with torch.no_grad():
                self.L.weight_v.copy_(v0)
                self.L.weight_g.copy_(g0)
        self.scale_factor = 2 if outdim <= 200 else 10
        self.initial = {k: v.detach().clone() for k, v in self.L.state_dict().items()}
        distLinear.made.append(self)

    def forward(self, x):
        x_norm = torch.norm(x, p=2, dim=1).unsqueeze(1).expand_as(x)
        return self.scale_factor * self.L(x.div(x_norm + 0.00001))


def main():
    mods = import_reference()
    backbone, finetune = mods["backbone"], mods["finetune"]
    finetune.Classifier = distLinear
    finetune.model_dict["ResNet10"] = make_factory(backbone, 84)
    finetune.params = argparse.Namespace(model="ResNet10", fine_tune_epoch=1)
    sd = synthetic.gnnnet_state_dict(seed=37)
    out = {}

    def run(liz, dtype, threads):
        torch.set_num_threads(threads)
        torch.set_default_dtype(dtype)
        try:
            state = {k: (v.to(dtype) if v.is_floating_point() else v.clone()) for k, v in copy.deepcopy(sd).items()}
            torch.manual_seed(125)
            np.random.seed(10)
            sc = finetune.finetune_linear([v.to(dtype) for v in liz], None, state_in=state, linear=True, save_it=None,
                                          n_query=15, n_way=5, n_support=5)
            return sc.numpy().copy(), np.random.permutation(7)
        finally:
            torch.set_default_dtype(torch.float32)
            torch.set_num_threads(8)

    for ep in EPISODES:
        liz = synthetic.test_episode(ep, 5, 5, 15, 84, gen_examples=1)
        distLinear.pinned = None
        s32, nxt = run(liz, torch.float32, 8)
        head = distLinear.made[-1]
        v0, g0 = head.initial["weight_v"].clone(), head.initial["weight_g"].clone()
        distLinear.pinned = (v0, g0)
        s32_1, nxt1 = run(liz, torch.float32, 1)
        s64, nxt64 = run(liz, torch.float64, 8)
        assert (nxt == nxt1).all() and (nxt == nxt64).all()
        top2 = np.sort(s64, 1)
        margin = float((top2[:, -1] - top2[:, -2]).min())
        agree = float(np.mean((s32.argmax(1) == s64.argmax(1)) & (s32_1.argmax(1) == s64.argmax(1))))
        print("episode %d: fp32 vs fp64 %.3e, 8 threads vs 1 thread %.3e, argmax agreement %.3f, smallest top-2 margin (fp64) %.3f"
              % (ep, np.abs(s32 - s64).max(), np.abs(s32 - s32_1).max(), agree, margin), flush=True)
        assert agree == 1.0, "the reference's own variants disagree on an argmax: this episode cannot carry an argmax assertion"
        assert margin >= 0.5, "the float64 scores do not separate their two best classes"
        assert np.abs(s32 - s64).max() > 0, "fp32 and fp64 runs are identical: no yardstick"
        tag = "_%d" % ep
        out["v0" + tag], out["g0" + tag] = v0.numpy(), g0.numpy()
        out["scores_f32" + tag], out["scores_f32_1thr" + tag], out["scores_f64" + tag] = s32, s32_1, s64
        out["next_perm" + tag] = nxt
    path = os.path.join(GOLD, "g25_baselinepp_finetune.npz")
    np.savez_compressed(path, **out)
    print("g25 done: %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
