"""Child process of tests/test_metaoptnet_gpu.py::test_metaoptnet_step_issues_no_aten_device_kernels: one eager MetaOptNet
meta-training step under the torch profiler, one autograd-off head call, and the head's forward + backward launches on fixed
features at two shapes; prints ONE json line {"n_dev": device kernels of the step, "aten": [names of ATen device kernels of the
step], "head_n_dev" / "head_aten": the same for the no-grad head call, "head_step_n_dev" / "head_step_n_dev_50shot": device kernels
of ridge_forward + ridge_backward at (5, 5, 16) and (5, 50, 2), "head_step_aten": ATen kernels of both}.  Kept out of the pytest
process for the reason tests/profile_step_worker.py gives."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import meta_fine_tuning_amd  # noqa: E402,F401
from meta_fine_tuning_amd import autograd_ops as AG  # noqa: E402
from meta_fine_tuning_amd import ops, optim, synthetic  # noqa: E402
from meta_fine_tuning_amd.io_utils import model_dict  # noqa: E402
from meta_fine_tuning_amd.methods.metaoptnet import MetaOptNet  # noqa: E402


def _kernels(prof):
    dev = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    return dev, sorted({n for n in dev if "at::native" in n or n.startswith("void at::")})


def main():
    from torch.profiler import ProfilerActivity, profile
    model = MetaOptNet(model_dict['ResNet10'], n_way=5, n_support=5).cuda()
    sd = synthetic.resnet10_state_dict(seed=0, prefix="feature.")
    sd.update(synthetic.metaoptnet_head_state(27))
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
    scale = model.scale.detach()
    fixed = {}
    for ns, nq in ((5, 16), (50, 2)):
        fixed[ns] = (torch.relu(torch.randn(5 * (ns + nq), 512, device="cuda")), torch.randn(5 * nq, 5, device="cuda"), nq)
        ops.ridge_backward(ops.ridge_forward(fixed[ns][0], scale, 1, 5, ns, nq, save=True)[1], fixed[ns][1])    # (attribute calls done)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        opt.zero_grad()
        model.set_forward_loss(x).backward(one)
        opt.step()
        torch.cuda.synchronize()
    dev, aten = _kernels(prof)
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        with torch.no_grad():
            AG.metaoptnet_head(fixed[5][0], model.scale, 5, 5, 16)
        torch.cuda.synchronize()
    hdev, haten = _kernels(prof)
    counts, step_aten = {}, []
    for ns in (5, 50):
        f, G, nq = fixed[ns]
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            ops.ridge_backward(ops.ridge_forward(f, scale, 1, 5, ns, nq, save=True)[1], G)
            torch.cuda.synchronize()
        d, a = _kernels(prof)
        counts[ns] = len(d)
        step_aten += a
    print("RESULT " + json.dumps({"n_dev": len(dev), "aten": aten, "head_n_dev": len(hdev), "head_aten": haten,
                                  "head_step_n_dev": counts[5], "head_step_n_dev_50shot": counts[50],
                                  "head_step_aten": step_aten}), flush=True)


if __name__ == "__main__":
    main()
