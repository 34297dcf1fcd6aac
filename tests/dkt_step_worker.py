"""Child process of test_dkt_gpu.py::test_dkt_step_issues_no_aten_device_kernels: one eager meta-training step of DKT under the
torch profiler, one autograd-off scoring call on fixed features, and the head's loss forward + backward at (5, 5, 16) and its scores
at (5, 50, 15); prints ONE json line {"n_dev": device kernels of the step, "aten": [names of ATen device kernels of the step],
"head_n_dev": device kernels of the no-grad scoring call, "head_aten": [...], "fwd_n_dev" / "bwd_n_dev": device kernels of
dkt_loss_forward / dkt_loss_backward at (5, 5, 16), "scores_n_dev_50shot": device kernels of dkt_scores at (5, 50, 15),
"head_step_aten": ATen kernels of those}.  Kept out of the pytest process for the reason tests/profile_step_worker.py gives."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import meta_fine_tuning_amd  # noqa: E402,F401
from meta_fine_tuning_amd import ops, optim, synthetic  # noqa: E402
from meta_fine_tuning_amd.io_utils import model_dict  # noqa: E402
from meta_fine_tuning_amd.train import PROBABILISTIC_METHODS  # noqa: E402


def _kernels(prof):
    dev = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    return dev, sorted({n for n in dev if "at::native" in n or n.startswith("void at::")})


def main():
    from torch.profiler import ProfilerActivity, profile
    model = PROBABILISTIC_METHODS["dkt"](model_dict['ResNet10'], n_way=5, n_support=5).cuda()
    sd = synthetic.resnet10_state_dict(seed=0, prefix="feature.")
    sd.update(synthetic.dkt_head_state(32))
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
    hyper = tuple(p.detach() for p in model.head_params())
    draw = lambda *s: torch.relu(torch.randn(*s, device="cuda"))  # noqa: E731
    f5, f50 = draw(5 * 21, 512), draw(5 * 65, 512)
    g1 = torch.ones(1, device="cuda")
    ops.dkt_loss_backward(ops.dkt_loss_forward(f5, hyper, 1, 5, 5, 16, save=True)[1], g1)        # (attribute calls done)
    ops.dkt_scores(f50, hyper, 1, 5, 50, 15)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        opt.zero_grad()
        model.set_forward_loss(x).backward(one)
        opt.step()
        torch.cuda.synchronize()
    dev, aten = _kernels(prof)
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        with torch.no_grad():
            model._head(f5, 16)
        torch.cuda.synchronize()
    hdev, haten = _kernels(prof)
    res = {"n_dev": len(dev), "aten": aten, "head_n_dev": len(hdev), "head_aten": haten, "head_step_aten": []}
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        tape = ops.dkt_loss_forward(f5, hyper, 1, 5, 5, 16, save=True)[1]
        torch.cuda.synchronize()
    d, a = _kernels(prof)
    res["fwd_n_dev"] = len(d)
    res["head_step_aten"] += a
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        ops.dkt_loss_backward(tape, g1)
        torch.cuda.synchronize()
    d, a = _kernels(prof)
    res["bwd_n_dev"] = len(d)
    res["head_step_aten"] += a
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        ops.dkt_scores(f50, hyper, 1, 5, 50, 15)
        torch.cuda.synchronize()
    d, a = _kernels(prof)
    res["scores_n_dev_50shot"] = len(d)
    res["head_step_aten"] += a
    print("RESULT " + json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
