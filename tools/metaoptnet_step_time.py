#!/usr/bin/env python3
"""Milliseconds per graphed meta-training step (set_forward_loss + backward replayed from one hipGraph, then the fused outer Adam;
MetaTemplate._episode_loop) of MetaOptNet next to ProtoNet (the same backbone, a negligible head), 5-way 5-shot 16 queries at
84 x 84, one episode per step (k = 1) and four episodes in lockstep (k = 4, train.py --episodes_per_rank 4); then the head alone
(forward + cross entropy + backward on fixed features) at S = 25, 100 and 250, and each of its five launches back to back.
    python tools/metaoptnet_step_time.py [steps]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import meta_fine_tuning_amd  # noqa: E402,F401
from meta_fine_tuning_amd import autograd_ops as AG  # noqa: E402
from meta_fine_tuning_amd import _lib, ops, synthetic  # noqa: E402
from meta_fine_tuning_amd.io_utils import model_dict  # noqa: E402
from meta_fine_tuning_amd.methods.metaoptnet import MetaOptNet  # noqa: E402
from meta_fine_tuning_amd.methods.protonet import ProtoNet  # noqa: E402
from graphed_step_timer import time_graphed_step  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 50


def run(cls, k):
    torch.manual_seed(0)
    model = cls(model_dict["ResNet10"], n_way=5, n_support=5).cuda()
    sd = synthetic.gnnnet_state_dict(seed=0)
    model.load_state_dict({n: v for n, v in sd.items() if n in model.state_dict()}, strict=False)
    dt, _, loss = time_graphed_step(model, k, steps)
    print("%-10s k = %d  %7.3f ms per step  %7.1f episodes/s  loss %.5f" % (cls.__name__, k, dt * 1e3, k / dt, loss), flush=True)


def _time(fn, reps):
    for _ in range(5):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3


def head(n_support, n_query, reps=100):
    """The head alone at 5-way ``n_support``-shot: forward + loss + backward through autograd on fixed features, then each launch."""
    n_way, S, Q, D = 5, 5 * n_support, 5 * n_query, 512
    f = torch.relu(torch.randn(n_way * (n_support + n_query), D, device="cuda")).requires_grad_(True)
    scale = torch.ones(1, device="cuda", requires_grad=True)
    y = torch.arange(n_way, device="cuda").repeat_interleave(n_query)
    loss_fn = AG.CrossEntropyLoss()
    one = torch.ones((), device="cuda")

    def whole():
        f.grad = scale.grad = None
        loss_fn(AG.metaoptnet_head(f, scale, n_way, n_support, n_query), y).backward(one)

    t_whole = _time(whole, reps)
    h, p, st = _lib.lib(), ops._p, ops._stream
    x, sc = f.detach(), scale.detach()
    new = lambda *s: torch.empty(s, device="cuda")  # noqa: E731
    A, alpha, W, scores, dW, dx, dscale = new(S, S), new(S, n_way), new(n_way, D), new(Q, n_way), new(n_way, D), new(*x.shape), new(1)
    G = torch.randn(Q, n_way, device="cuda")
    part = torch.empty(8, device="cuda", dtype=torch.float64)
    A0 = new(S, S)
    hd = (1, n_way, n_support, n_query, D)
    h.mft_ridge_gram(p(x), D, *hd, 50.0, p(A0), st())

    def factor():                   # (the factor launch works in place: give it the Gram matrix again; the copy is timed apart)
        A.copy_(A0)
        h.mft_ridge_factor_solve(p(x), D, *hd, p(A), p(alpha), p(W), st())

    launches = [("gram", lambda: h.mft_ridge_gram(p(x), D, *hd, 50.0, p(A0), st())),
                ("copy of A (not a head launch)", lambda: A.copy_(A0)),
                ("factor_solve + copy", factor),
                ("scores", lambda: h.mft_ridge_scores(p(x), D, *hd, p(W), p(sc), p(scores), 0, st())),
                ("backward_query", lambda: h.mft_ridge_backward_query(p(x), D, *hd, p(W), p(sc), p(G), n_way, p(dx), D, p(dW), p(part), st())),
                ("backward_support", lambda: h.mft_ridge_backward_support(p(x), D, *hd, p(A), p(alpha), p(W), p(dW), p(part), p(dx), D,
                                                                          p(dscale), st()))]
    print("head alone, 5-way %d-shot %d queries (S = %d): forward + loss + backward %7.1f us" % (n_support, n_query, S, t_whole), flush=True)
    for name, fn in launches:
        print("    %-32s %7.1f us (back-to-back average)" % (name, _time(fn, reps)), flush=True)


for k in (1, 4):
    for cls in (MetaOptNet, ProtoNet):
        run(cls, k)
for ns, nq in ((5, 16), (20, 16), (50, 16)):
    head(ns, nq)
