#!/usr/bin/env python3
"""Milliseconds per graphed meta-training step (set_forward_loss + backward replayed from one hipGraph, then the fused outer Adam;
MetaTemplate._episode_loop) of MetaOptNet with the SVM head next to the ridge head in the same run, 5-way 5-shot 16 queries at
84 x 84, one episode per step (k = 1) and four in lockstep (k = 4); then the SVM head alone (forward + cross entropy + backward
on fixed class-structured features) at S = 25, 100 and 250 with the products M x [S, n_way] its solve used, and each launch.
    python tools/metaoptnet_svm_time.py [steps]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import meta_fine_tuning_amd  # noqa: E402,F401
from meta_fine_tuning_amd import autograd_ops as AG  # noqa: E402
from meta_fine_tuning_amd import ops, synthetic  # noqa: E402
from meta_fine_tuning_amd.io_utils import model_dict  # noqa: E402
from meta_fine_tuning_amd.methods.metaoptnet import MetaOptNet  # noqa: E402
from graphed_step_timer import time_graphed_step  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 50


def run(head, k):
    torch.manual_seed(0)
    model = MetaOptNet(model_dict["ResNet10"], n_way=5, n_support=5, head=head).cuda()
    sd = synthetic.gnnnet_state_dict(seed=0)
    model.load_state_dict({n: v for n, v in sd.items() if n in model.state_dict()}, strict=False)
    dt, _, loss = time_graphed_step(model, k, steps)
    print("MetaOptNet %-5s k = %d  %7.3f ms per step  %7.1f episodes/s  loss %.5f" % (head, k, dt * 1e3, k / dt, loss), flush=True)


def _time(fn, reps):
    for _ in range(3):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3


def head(n_support, n_query, reps=20):
    n_way, D = 5, 512
    g = torch.Generator().manual_seed(n_support)
    mean = torch.randn(n_way, 1, D, generator=g)
    f = torch.relu(0.5 * torch.randn(n_way, n_support + n_query, D, generator=g) + 0.5 * mean + 0.3).reshape(-1, D).cuda().requires_grad_(True)
    scale = torch.ones(1, device="cuda", requires_grad=True)
    y = torch.arange(n_way, device="cuda").repeat_interleave(n_query)
    loss_fn = AG.CrossEntropyLoss()
    one = torch.ones((), device="cuda")

    def whole():
        f.grad = scale.grad = None
        loss_fn(AG.metaoptnet_svm_head(f, scale, n_way, n_support, n_query), y).backward(one)

    t_whole = _time(whole, reps)
    x, sc = f.detach(), scale.detach()
    G = torch.randn(n_way * n_query, n_way, device="cuda")
    tape = ops.svm_forward(x, sc, 1, n_way, n_support, n_query, save=True)[1]
    t_fwd = _time(lambda: ops.svm_forward(x, sc, 1, n_way, n_support, n_query, save=True), reps)
    t_bwd = _time(lambda: ops.svm_backward(tape, G), reps)
    t_gram = _time(lambda: ops._svm_gram(x, 1, n_way, n_support, n_query), reps)
    print("SVM head alone, 5-way %d-shot %d queries (S = %d): forward + loss + backward %8.1f us; forward (gram, solve, scores) %8.1f us, "
          "backward (gram, query, support) %8.1f us, gram alone %6.1f us; status %d, %d products in the solve"
          % (n_support, n_query, 5 * n_support, t_whole, t_fwd, t_bwd, t_gram, int(tape["status"][0]), int(tape["products"][0])), flush=True)


for k in (1, 4):
    for h in ("ridge", "svm"):
        run(h, k)
for ns, nq in ((5, 16), (20, 16), (50, 16)):
    head(ns, nq)
