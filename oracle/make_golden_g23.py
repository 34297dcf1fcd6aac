"""Golden G23: the REFERENCE's GnnNet.set_forward_loss + backward in fp32 at image sizes other than this project's 84 x 84.

Build-container only (imports the reference through make_golden.import_reference).  224 x 224 is the reference's native size (its own
AvgPool2d(7), nothing substituted); 100 x 100 (map sides 50 / 25 / 25 / 13 / 7 / 4: an odd chain) runs through make_factory's pool
substitution.  Per size: the loss, the scores, the norm and the largest |element| of every parameter's gradient, and element slices
of fc.0.weight.grad, feature.trunk.7.C2.weight.grad, feature.trunk.6.C2.weight.grad (256 channels: on the split-precision kernels at
224) and feature.trunk.0.weight.grad.  Weights and episodes are regenerated from the seeds in CASES by ``meta-fine-tuning_amd/synthetic.py``;
the file holds outputs only.

    python oracle/make_golden_g23.py            # writes tests/golden/g23_image_sizes.npz
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as MG  # noqa: E402
from make_golden import synthetic  # noqa: E402

# (image size, weight seed, episode seed), 5-way 5-shot 16-query
CASES = [(224, 7, 21), (100, 8, 22)]
N_WAY, N_SHOT, N_QUERY = 5, 5, 16


def main():
    mods = MG.import_reference()
    gnnnet = mods["methods.gnnnet"]
    torch.set_num_threads(8)
    out = {"cases": np.array(CASES, dtype=np.int64)}
    for size, wseed, xseed in CASES:
        t = str(size)
        sd = synthetic.gnnnet_state_dict(seed=wseed)
        x = synthetic.train_episode(xseed, N_WAY, N_SHOT, N_QUERY, size)
        torch.manual_seed(0)
        model = gnnnet.GnnNet(MG.make_factory(mods["backbone"], size), n_way=N_WAY, n_support=N_SHOT)
        model.load_state_dict(sd)
        model.train()
        model.n_query = N_QUERY
        scores = model.set_forward(x)
        y = torch.from_numpy(np.repeat(range(N_WAY), N_QUERY))
        loss = model.loss_fn(scores, y)          # = set_forward_loss(x) (gnnnet.py:219-224), keeping the scores of the same forward
        loss.backward()
        names = sorted(n for n, _ in model.named_parameters())
        named = dict(model.named_parameters())
        out["scores_" + t] = scores.detach().numpy()
        out["loss_" + t] = np.array(float(loss))
        out["gradnames_" + t] = np.array(names)
        out["gradnorms_" + t] = np.array([float(named[n].grad.norm()) for n in names])
        out["gradmaxs_" + t] = np.array([float(named[n].grad.abs().max()) for n in names])
        out["grad_fc0w_slice_" + t] = named["fc.0.weight"].grad[:4, :8].numpy()
        out["grad_c7c2_slice_" + t] = named["feature.trunk.7.C2.weight"].grad[:2, :4, 1, 1].numpy()
        out["grad_c6c2_slice_" + t] = named["feature.trunk.6.C2.weight"].grad[:4, :8].numpy()
        out["grad_stem_slice_" + t] = named["feature.trunk.0.weight"].grad[:2, :, 3, 3].numpy()
        print(t, "loss %.6f" % float(loss))
    path = os.path.join(MG.GOLD, "g23_image_sizes.npz")
    np.savez(path, **out)
    print("wrote", path)


if __name__ == "__main__":
    main()
