#!/usr/bin/env python3
"""Milliseconds per graphed meta-training step (set_forward_loss + backward replayed from one hipGraph, then the fused outer Adam;
MetaTemplate._episode_loop) of ResNet10_FW next to ResNet10 in the same process, under the ProtoNet and the GnnNet head, 5-way
5-shot 16 queries at 84 x 84: one episode per step (k = 1) and four in lockstep (k = 4, train.py --episodes_per_rank 4).
The yardstick of the feature-wise transformation backbone is the plain ResNet10 step of the same run.
``--launches``: also the per-launcher time of one eager ResNet10_FW ProtoNet step (k = 1), largest first.
``--one MODEL``: only the ProtoNet k = 1 step of that backbone (a run for a kernel trace: rocprofv3 --kernel-trace --stats -- ...).
    python tools/fwt_step_time.py [steps] [--launches | --one ResNet10_FW]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import meta_fine_tuning_amd  # noqa: E402,F401
from meta_fine_tuning_amd import _lib, synthetic  # noqa: E402
from meta_fine_tuning_amd.io_utils import model_dict  # noqa: E402
from meta_fine_tuning_amd.methods.gnnnet import GnnNet  # noqa: E402
from meta_fine_tuning_amd.methods.protonet import ProtoNet  # noqa: E402
from graphed_step_timer import time_graphed_step  # noqa: E402

one = sys.argv[sys.argv.index("--one") + 1] if "--one" in sys.argv else None
args = [a for a in sys.argv[1:] if not a.startswith("--") and a != one]
steps = int(args[0]) if args else 50


def build(cls, name):
    torch.manual_seed(0)
    model = cls(model_dict[name], n_way=5, n_support=5).cuda()
    sd = synthetic.resnet10_fw_state_dict(0, prefix="feature.")
    sd.update(synthetic.gnn_head_state_dict(1, 5))
    model.load_state_dict({n: v for n, v in sd.items() if n in model.state_dict()}, strict=False)
    model.train()
    model.n_query = 16
    return model


def run(cls, name, k):
    best, worst, loss = time_graphed_step(build(cls, name), k, steps, passes=3)      # three timed passes: the minimum and the spread
    print("%-8s %-11s k = %d  %7.3f ms per step (slowest of 3 passes %7.3f)  %7.1f episodes/s  loss %.5f"
          % (cls.__name__, name, k, best * 1e3, worst * 1e3, k / best, loss), flush=True)
    return best


def launches():
    model = build(ProtoNet, "ResNet10_FW")
    x = synthetic.train_episode(5000, 5, 5, 16, 84).cuda()
    for _ in range(3):
        model.set_forward_loss(x).backward()
    with _lib.LaunchTimer() as t:
        model.set_forward_loss(x).backward()
    calls = t.collect()
    t.close()
    tot = sum(sum(v) for v in calls.values())
    print("one eager ResNet10_FW ProtoNet step: %d launcher calls, %.3f ms inside them" % (sum(len(v) for v in calls.values()), tot))
    for name, v in sorted(calls.items(), key=lambda kv: -sum(kv[1])):
        print("    %-36s x%-3d %8.1f us" % (name, len(v), sum(v) * 1e3))


for cls in (() if one else (ProtoNet, GnnNet)):
    for k in (1, 4):
        plain = run(cls, "ResNet10", k)
        fw = run(cls, "ResNet10_FW", k)
        print("    ResNet10_FW - ResNet10: %+.3f ms (%+.2f %% of the plain step)" % ((fw - plain) * 1e3, (fw - plain) / plain * 100), flush=True)
if one:
    run(ProtoNet, one, 1)
if "--launches" in sys.argv:
    launches()
