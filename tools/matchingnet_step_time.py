#!/usr/bin/env python3
"""Milliseconds per graphed meta-training step (set_forward_loss + backward replayed from one hipGraph, then the fused outer Adam;
MetaTemplate._episode_loop) of MatchingNet next to ProtoNet (whose head is two launches: its step is the backbone's), 5-way 5-shot
16 queries at 84 x 84, one episode per step (k = 1) and four episodes in lockstep (k = 4, train.py --episodes_per_rank 4); then
the MatchingNet head alone (forward + loss + backward on fixed features, replayed from a hipGraph of its own) and its share of
the step.
    python tools/matchingnet_step_time.py [steps]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import meta_fine_tuning_amd  # noqa: E402,F401
from meta_fine_tuning_amd import autograd_ops as AG  # noqa: E402
from meta_fine_tuning_amd import synthetic  # noqa: E402
from meta_fine_tuning_amd.io_utils import model_dict  # noqa: E402
from meta_fine_tuning_amd.methods.matchingnet import MatchingNet  # noqa: E402
from meta_fine_tuning_amd.methods.protonet import ProtoNet  # noqa: E402
from graphed_step_timer import time_graphed_step  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 50


def make(cls):
    torch.manual_seed(0)
    model = cls(model_dict["ResNet10"], n_way=5, n_support=5).cuda()
    sd = synthetic.resnet10_state_dict(seed=0, prefix="feature.")
    sd.update(synthetic.matchingnet_head_state(26))
    model.load_state_dict({n: v for n, v in sd.items() if n in model.state_dict()})
    model.train()
    model.n_query = 16
    return model


def run(cls, k):
    dt, _, loss = time_graphed_step(make(cls), k, steps)
    print("%-11s k = %d  %7.3f ms per step  %7.1f episodes/s  loss %.5f" % (cls.__name__, k, dt * 1e3, k / dt, loss), flush=True)
    return dt * 1e3


def head_alone(k):
    """The head's forward + NLL + backward on fixed features [k * 105, 512], as one hipGraph replay."""
    model = make(MatchingNet)
    g = torch.Generator().manual_seed(1)
    cls = torch.arange(5).repeat_interleave(21).repeat(k).float()
    feats = torch.relu(1 + 0.1 * cls[:, None] + 0.5 * torch.randn(k * 105, 512, generator=g)).cuda().requires_grad_(True)
    y = model._labels(k)
    one = torch.ones((), device="cuda")

    def body():
        feats.grad = None
        loss = model.loss_fn(AG.matchingnet_head(model, feats, 5, 16, episodes=k), y)
        loss.backward(one)
        return loss

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            body()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = body()
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        graph.replay()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps * 1e3
    print("MatchingNet head alone, k = %d: %7.3f ms per forward + loss + backward  (loss %.5f)" % (k, dt, float(loss.detach())), flush=True)
    return dt


for k in (1, 4):
    t_m = run(MatchingNet, k)
    t_p = run(ProtoNet, k)
    t_h = head_alone(k)
    print("k = %d: the head is %.0f%% of the MatchingNet step (%.3f of %.3f ms); ProtoNet's step, i.e. the backbone, takes %.3f ms"
          % (k, 100 * t_h / t_m, t_h, t_m, t_p), flush=True)
