"""Child process of tests/test_matchingnet_gpu.py::test_matchingnet_step_issues_no_aten_device_kernels: one eager MatchingNet meta-training
step under the torch profiler, then one autograd-off head call; prints ONE json line {"n_dev": device kernels of the step, "aten":
[names of ATen device kernels of the step], "head_n_dev": device kernels of the head call, "head_aten": [...]}.  Kept out of the
pytest process for the reason tests/profile_step_worker.py gives."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import meta_fine_tuning_amd  # noqa: E402,F401
from meta_fine_tuning_amd import autograd_ops as AG  # noqa: E402
from meta_fine_tuning_amd import optim, synthetic  # noqa: E402
from meta_fine_tuning_amd.io_utils import model_dict  # noqa: E402
from meta_fine_tuning_amd.methods.matchingnet import MatchingNet  # noqa: E402


def _kernels(prof):
    dev = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    return dev, sorted({n for n in dev if "at::native" in n or n.startswith("void at::")})


def main():
    from torch.profiler import ProfilerActivity, profile
    model = MatchingNet(model_dict['ResNet10'], n_way=5, n_support=5).cuda()
    sd = synthetic.resnet10_state_dict(seed=0, prefix="feature.")
    sd.update(synthetic.matchingnet_head_state(26))
    model.load_state_dict(sd)
    model.train()
    model.n_query = 16
    opt = optim.Adam(model.parameters())
    x = synthetic.train_episode(5, 5, 5, 16, 84).cuda()
    one = torch.ones((), device="cuda")
    for _ in range(2):
        opt.zero_grad()
        model.set_forward_loss(x).backward(one)
        opt.step()
    feats = torch.rand(5 * 21, 512, device="cuda")
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        opt.zero_grad()
        model.set_forward_loss(x).backward(one)
        opt.step()
        torch.cuda.synchronize()
    dev, aten = _kernels(prof)
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        with torch.no_grad():
            AG.matchingnet_head(model, feats, 5, 16)
        torch.cuda.synchronize()
    hdev, haten = _kernels(prof)
    print("RESULT " + json.dumps({"n_dev": len(dev), "aten": aten, "head_n_dev": len(hdev), "head_aten": haten}), flush=True)


if __name__ == "__main__":
    main()
