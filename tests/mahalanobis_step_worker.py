"""Child process of test_mahalanobis_gpu.py::test_mahalanobis_step_issues_no_aten_device_kernels: one eager meta-training step of the
Mahalanobis head under the torch profiler, one autograd-off scoring call on fixed features, and the head's forward + backward at
(5, 5, 15) and (5, 50, 15); prints ONE json line {"n_dev": device kernels of the step, "aten": [names of ATen device kernels of the
step], "head_n_dev": device kernels of the no-grad scoring call, "head_aten": [...], "fwd_n_dev" / "bwd_n_dev": {shape: device
kernels of mahalanobis_forward / mahalanobis_backward}, "head_step_aten": ATen kernels of those}.  Kept out of the pytest process
for the reason tests/profile_step_worker.py gives."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import meta_fine_tuning_amd  # noqa: E402,F401
from meta_fine_tuning_amd import ops, optim, synthetic  # noqa: E402
from meta_fine_tuning_amd.io_utils import model_dict  # noqa: E402
from meta_fine_tuning_amd.train import METRIC_METHODS  # noqa: E402

SHAPES = ((5, 5, 15), (5, 50, 15))


def _kernels(prof):
    dev = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    return dev, sorted({n for n in dev if "at::native" in n or n.startswith("void at::")})


def main():
    from torch.profiler import ProfilerActivity, profile
    model = METRIC_METHODS["mahalanobis"](model_dict['ResNet10'], n_way=5, n_support=5).cuda()
    model.load_state_dict(synthetic.resnet10_state_dict(seed=0, prefix="feature."))
    model.train()
    model.n_query = 15
    opt = optim.Adam(model.parameters())
    x = synthetic.train_episode(5, 5, 5, 15, 84).cuda()
    one = torch.ones((), device="cuda")
    for _ in range(2):
        opt.zero_grad()
        model.set_forward_loss(x).backward(one)
        opt.step()
    draw = lambda *s: torch.relu(torch.randn(*s, device="cuda"))  # noqa: E731
    feats = {(5, 5, 15): draw(5 * 20, 512), (5, 50, 15): draw(5 * 65, 512)}
    grads = {s: torch.randn(s[0] * s[2], s[0], device="cuda") for s in SHAPES}
    for s in SHAPES:                                                  # (attribute calls done)
        ops.mahalanobis_backward(ops.mahalanobis_forward(feats[s], 1, *s, save=True)[1], grads[s])
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        opt.zero_grad()
        model.set_forward_loss(x).backward(one)
        opt.step()
        torch.cuda.synchronize()
    dev, aten = _kernels(prof)
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        with torch.no_grad():
            model._head(feats[(5, 5, 15)], 15)
        torch.cuda.synchronize()
    hdev, haten = _kernels(prof)
    res = {"n_dev": len(dev), "aten": aten, "head_n_dev": len(hdev), "head_aten": haten, "head_step_aten": [], "fwd_n_dev": {},
           "bwd_n_dev": {}}
    for s in SHAPES:
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            tape = ops.mahalanobis_forward(feats[s], 1, *s, save=True)[1]
            torch.cuda.synchronize()
        d, a = _kernels(prof)
        res["fwd_n_dev"]["%d_%d_%d" % s] = len(d)
        res["head_step_aten"] += a
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            ops.mahalanobis_backward(tape, grads[s])
            torch.cuda.synchronize()
        d, a = _kernels(prof)
        res["bwd_n_dev"]["%d_%d_%d" % s] = len(d)
        res["head_step_aten"] += a
    print("RESULT " + json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
