"""Child process of test_{protonet,matchingnet,metaoptnet}_gpu.py::test_*_step_issues_no_aten_device_kernels
(``method_step_worker.py METHOD``): one eager meta-training step of that method under the torch profiler, then one autograd-off
head call on fixed features; prints ONE json line {"n_dev": device kernels of the step, "aten": [names of ATen device kernels of the
step], "head_n_dev": device kernels of the head call, "head_aten": [...]}.  For ``metaoptnet`` also the head's forward + backward
launches on fixed features at two shapes: "head_step_n_dev" / "head_step_n_dev_50shot": device kernels of ridge_forward +
ridge_backward at (5, 5, 16) and (5, 50, 2), "head_step_aten": ATen kernels of both.  Kept out of the pytest process for the reason
tests/profile_step_worker.py gives."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import meta_fine_tuning_amd  # noqa: E402,F401
from meta_fine_tuning_amd import ops, optim, synthetic  # noqa: E402
from meta_fine_tuning_amd.io_utils import model_dict  # noqa: E402
from meta_fine_tuning_amd.train import HEAD_METHODS  # noqa: E402

# per method: the head's synthetic state (None: the head has no weights) and the distribution of the fixed features
CASES = {"protonet": (None, torch.randn),
         "matchingnet": (lambda: synthetic.matchingnet_head_state(26), torch.rand),
         "metaoptnet": (lambda: synthetic.metaoptnet_head_state(27), lambda *s, **kw: torch.relu(torch.randn(*s, **kw)))}


def _kernels(prof):
    dev = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    return dev, sorted({n for n in dev if "at::native" in n or n.startswith("void at::")})


def main(method):
    from torch.profiler import ProfilerActivity, profile
    head_state, draw = CASES[method]
    model = HEAD_METHODS[method](model_dict['ResNet10'], n_way=5, n_support=5).cuda()
    sd = synthetic.resnet10_state_dict(seed=0, prefix="feature.")
    if head_state is not None:
        sd.update(head_state())
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
    feats = draw(5 * 21, 512, device="cuda")
    if method == "metaoptnet":
        scale = model.scale.detach()
        fixed = {5: (feats, torch.randn(5 * 16, 5, device="cuda"), 16),
                 50: (draw(5 * 52, 512, device="cuda"), torch.randn(5 * 2, 5, device="cuda"), 2)}
        for ns, (f, G, nq) in fixed.items():
            ops.ridge_backward(ops.ridge_forward(f, scale, 1, 5, ns, nq, save=True)[1], G)    # (attribute calls done)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        opt.zero_grad()
        model.set_forward_loss(x).backward(one)
        opt.step()
        torch.cuda.synchronize()
    dev, aten = _kernels(prof)
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        with torch.no_grad():
            model._head(feats, 16)
        torch.cuda.synchronize()
    hdev, haten = _kernels(prof)
    res = {"n_dev": len(dev), "aten": aten, "head_n_dev": len(hdev), "head_aten": haten}
    if method == "metaoptnet":
        counts, step_aten = {}, []
        for ns, (f, G, nq) in fixed.items():
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                ops.ridge_backward(ops.ridge_forward(f, scale, 1, 5, ns, nq, save=True)[1], G)
                torch.cuda.synchronize()
            d, a = _kernels(prof)
            counts[ns] = len(d)
            step_aten += a
        res.update({"head_step_n_dev": counts[5], "head_step_n_dev_50shot": counts[50], "head_step_aten": step_aten})
    print("RESULT " + json.dumps(res), flush=True)


if __name__ == "__main__":
    main(sys.argv[1])
