#!/usr/bin/env python3
"""Baseline++ timings.

  (1) the head's three launches alone, back to back between two device events after a warm-up: mft_dist_linear_forward and
      mft_dist_linear_backward at the training shape (16 rows, 200 classes, D = 512) and at 64 x 1000; the scoring launch of E
      adapted episodes (E x 75 queries, 5 classes); mft_dist_head_sgd_run for E episodes of 5-way 5-shot (700 steps, support
      rows in LDS) and 5-way 20-shot (2500 steps, support rows from HBM / L2), next to mft_linear_head_sgd_run on the same tables;
  (2) one supervised BaselineTrain step (forward, loss, backward, fused Adam; 16 images at 84 x 84, 200 classes) with
      loss_type='dist' beside the unchanged loss_type='softmax' step, in the same process, alternating windows.

    python tools/baselinepp_step_time.py [repetitions]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import meta_fine_tuning_amd  # noqa: E402,F401
from meta_fine_tuning_amd import backbone, ops, optim  # noqa: E402
from meta_fine_tuning_amd.methods.baselinetrain import BaselineTrain  # noqa: E402
from meta_fine_tuning_amd.methods.meta_template import adaptation_table  # noqa: E402

reps = max(200, int(sys.argv[1])) if len(sys.argv) > 1 else 200


def timed(fn, n=reps, warm=10):
    for _ in range(warm):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3          # microseconds per call


def head_launches():
    for rows, C in ((16, 200), (64, 1000)):
        x = torch.randn(rows, 512, device="cuda").abs()
        v = torch.randn(C, 512, device="cuda") / 22.6
        g = v.norm(dim=1, keepdim=True).contiguous()
        G = torch.randn(rows, C, device="cuda")
        s = ops.dist_scale(C)
        f = timed(lambda: ops.dist_linear_forward(x, g, v, s))
        b = timed(lambda: ops.dist_linear_backward(x, g, v, s, G))
        print("head, %3d rows x %4d classes: forward %6.1f us, backward (dx, dV, dg) %6.1f us (back-to-back average, allocation "
              "of the outputs included)" % (rows, C, f, b), flush=True)
    lib = ops._lib.lib()
    for n_shot, E_list in ((5, (1, 32, 128)), (20, (1, 32))):
        S = 5 * n_shot
        for E in E_list:
            z = torch.randn(E, S, 512, device="cuda").abs()
            zq = torch.randn(E * 75, 512, device="cuda").abs()
            y = torch.from_numpy(np.tile(np.repeat(np.arange(5), n_shot).astype(np.int32), (E, 1))).cuda()
            rs = np.random.RandomState(E)
            table = torch.from_numpy(np.stack([adaptation_table(S, 100, 4, [rs.permutation(S) for _ in range(100)])
                                               for _ in range(E)])).cuda()
            v0 = (torch.rand(E, 5, 512, device="cuda") * 2 - 1) / 22.6
            g0 = v0.norm(dim=2).contiguous()
            b0 = torch.zeros(E, 5, device="cuda")
            v, g, w, b = v0.clone(), g0.clone(), v0.clone(), b0.clone()

            def dist_run():                      # (each call trains on from the last one's head: the same work, no reset launch)
                ops.dist_head_sgd_run(z, y, table, v, g, 2.0)

            def softmax_run():
                ops._lib.check(lib.mft_linear_head_sgd_run(ops._p(z), ops._p(y), ops._p(table), E, S, 512, 5, table.shape[1], 4,
                                                           ops._p(w), ops._p(b), 0.01, 0.9, 0.9, 0.001, ops._stream()), "run")

            td, ts = timed(dist_run, reps, 3), timed(softmax_run, reps, 3)
            tq = timed(lambda: ops.dist_linear_forward(zq, g, v, 2.0, softmax=True))
            print("adaptation, %3d episodes of 5-way %2d-shot (%4d steps): dist run %8.1f us (%5.2f us per step), softmax run %8.1f us; "
                  "scoring %d x 75 queries %6.1f us" % (E, n_shot, table.shape[1], td, td / table.shape[1], ts, E, tq), flush=True)


def train_steps():
    rs = np.random.RandomState(5)
    x = torch.from_numpy(rs.standard_normal((16, 3, 84, 84)).astype(np.float32)).cuda()
    y = torch.from_numpy(rs.randint(0, 200, size=16)).cuda()
    models = {}
    for lt in ("softmax", "dist"):
        torch.manual_seed(3)
        m = BaselineTrain(backbone.ResNet10, 200, loss_type=lt).cuda()
        m.train()
        models[lt] = (m, optim.Adam(m.parameters()))

    def step(lt):
        m, opt = models[lt]
        opt.zero_grad()
        loss = m.forward_loss(x, y)          # (top1 bookkeeping included: one host sync per step, as train_loop has)
        loss.backward()
        opt.step()

    for lt in models:
        for _ in range(5):
            step(lt)
    torch.cuda.synchronize()
    n = max(20, reps // 4)
    windows = {"softmax": [], "dist": []}
    for _ in range(4):                           # alternate the two versions: other work shares the host
        for lt in ("softmax", "dist"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                step(lt)
            torch.cuda.synchronize()
            windows[lt].append((time.perf_counter() - t0) / n * 1e3)
    for lt, w in windows.items():
        print("BaselineTrain step, loss_type=%-8s 16 images 84x84, 200 classes: %s ms per step (4 windows of %d steps), median %.3f"
              % (repr(lt), " ".join("%.3f" % t for t in w), n, float(np.median(w))), flush=True)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is nothing to time without one"
    head_launches()
    train_steps()
