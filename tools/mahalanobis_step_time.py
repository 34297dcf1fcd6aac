#!/usr/bin/env python3
"""Milliseconds per graphed meta-training step (set_forward_loss + backward replayed from one hipGraph, then the fused outer Adam;
MetaTemplate._episode_loop) of the Mahalanobis head next to ProtoNet (the same backbone, a negligible head), 5-way 5-shot 15 queries
at 84 x 84, one episode per step (k = 1) and four episodes in lockstep (k = 4, train.py --episodes_per_rank 4); then the head alone
(scores forward + backward on fixed features, eager) at S = 25, 100 and 250 support rows, and each of its five launchers (HIP
events around every launcher call, _lib.LaunchTimer).
    python tools/mahalanobis_step_time.py [steps]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import meta_fine_tuning_amd  # noqa: E402,F401
from meta_fine_tuning_amd import autograd_ops as AG  # noqa: E402
from meta_fine_tuning_amd import _lib, synthetic  # noqa: E402
from meta_fine_tuning_amd.io_utils import model_dict  # noqa: E402
from meta_fine_tuning_amd.methods.mahalanobis import Mahalanobis  # noqa: E402
from meta_fine_tuning_amd.methods.protonet import ProtoNet  # noqa: E402
from graphed_step_timer import time_graphed_step  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 50


def run(cls, k):
    torch.manual_seed(0)
    model = cls(model_dict["ResNet10"], n_way=5, n_support=5).cuda()
    sd = synthetic.gnnnet_state_dict(seed=0)
    model.load_state_dict({n: v for n, v in sd.items() if n in model.state_dict()}, strict=False)
    dt, _, loss = time_graphed_step(model, k, steps)
    print("%-12s k = %d  %7.3f ms per step  %7.1f episodes/s  loss %.5f" % (cls.__name__, k, dt * 1e3, k / dt, loss), flush=True)


def head(n_support, n_query, reps=100):
    """The head alone at 5-way ``n_support``-shot: scores forward + backward through autograd on fixed class-structured features."""
    n_way, D = 5, 512
    N = n_way * (n_support + n_query)
    mean = torch.randn(n_way, 1, D, device="cuda")
    f = torch.relu(0.5 * torch.randn(n_way, n_support + n_query, D, device="cuda") + 0.5 * mean + 0.3).reshape(N, D).requires_grad_(True)
    g = torch.randn(n_way * n_query, n_way, device="cuda")

    def whole():
        f.grad = None
        AG.mahalanobis_scores(f, n_way, n_support, n_query).backward(g)

    for _ in range(5):
        whole()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        whole()
    b.record()
    torch.cuda.synchronize()
    print("head alone, 5-way %d-shot %d queries (S = %d): scores forward + backward %7.1f us"
          % (n_support, n_query, n_way * n_support, a.elapsed_time(b) / reps * 1e3), flush=True)
    with _lib.LaunchTimer(only=lambda n: n.startswith("mft_mahalanobis_")) as t:
        for _ in range(20):
            whole()
    for name, ms in t.collect().items():
        print("    %-32s %7.1f us (mean of %d calls, events around the launch)" % (name, sum(ms) / len(ms) * 1e3, len(ms)), flush=True)
    t.close()


for k in (1, 4):
    for cls in (Mahalanobis, ProtoNet):
        run(cls, k)
for ns, nq in ((5, 15), (20, 15), (50, 15)):
    head(ns, nq)
