#!/usr/bin/env python3
"""Baseline++ at test time: timings of the fused cosine-head step, in one process.

  (1) mft_dist_head_step alone, back to back between two device events after a warm-up, for E = 1, 32 and 128 episodes of a
      5-way mini-batch of 5 (D = 512), next to mft_linear_head_step on the same features and labels;
  (2) one inner step of FinetuneEngine(mode="dist") at E = 128 (5-way 5-shot, 84 x 84) beside the mode="linear" step: the
      engine's own inner loop (100 steps per pass, two streams), device events around two passes after a warm-up pass,
      alternating windows of the two modes.

    python tools/baselinepp_finetune_time.py [calls per window, >= 200] [E of part 2]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import meta_fine_tuning_amd  # noqa: E402,F401
from meta_fine_tuning_amd import engine as eng  # noqa: E402
from meta_fine_tuning_amd import finetune as ft  # noqa: E402
from meta_fine_tuning_amd import ops, synthetic  # noqa: E402

reps = max(200, int(sys.argv[1])) if len(sys.argv) > 1 else 200
E_STEP = int(sys.argv[2]) if len(sys.argv) > 2 else 128


def timed(fn, n=reps, warm=20):
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
    lib = ops._lib.lib()
    for E in (1, 32, 128):
        feat = torch.randn(E * 5, 512, device="cuda").abs()
        y = torch.from_numpy(np.random.RandomState(E).randint(0, 5, E * 5).astype(np.int32)).cuda()
        dfeat = torch.empty(E * 5, 512, device="cuda")
        loss = torch.empty(E, device="cuda")
        V = (torch.rand(E, 5, 512, device="cuda") * 2 - 1) / 22.6
        g = V.norm(dim=2).contiguous()
        mV, vV, mg, vg = torch.zeros_like(V), torch.zeros_like(V), torch.zeros_like(g), torch.zeros_like(g)
        W, b = V.clone(), torch.zeros_like(g)
        mW, vW, mb, vb = torch.zeros_like(V), torch.zeros_like(V), torch.zeros_like(g), torch.zeros_like(g)
        step = [0, 0]

        def dist():                              # (each call trains on from the last one's head: the same work, no reset launch)
            step[0] += 1
            ops.dist_head_step(feat, y, V, g, mV, vV, mg, vg, 2.0, step[0], dfeat=dfeat, loss=loss)

        def linear():
            step[1] += 1
            ops._lib.check(lib.mft_linear_head_step(ops._p(feat), 512, ops._p(y), 5, E, 5, 512, ops._p(W), ops._p(b), ops._p(mW),
                                                    ops._p(vW), ops._p(mb), ops._p(vb), ops._p(dfeat), 512, ops._p(loss), step[1], 0.01,
                                                    0.9, 0.999, 1e-8, 0.001, ops._stream()), "mft_linear_head_step")

        n = max(reps, 5000)                      # (a launch takes microseconds: enough calls for a window of tens of milliseconds)
        td, tl = timed(dist, n), timed(linear, n)
        print("head step, %3d episodes x 5 rows x 5 classes: mft_dist_head_step %6.1f us, mft_linear_head_step %6.1f us "
              "(back-to-back average of %d calls)" % (E, td, tl, n), flush=True)


def engine_steps(E):
    sd = synthetic.gnnnet_state_dict(seed=37)
    ep = synthetic.test_episode_device(91, torch.device("cuda", 0), 5, 5, 15, 84, 0)
    perms = [eng.draw_perms(25, ft.LINEAR_EPOCHS, np.random.RandomState(1))]
    engines = {}
    with eng.slab_candidates(0):
        for mode in ("linear", "dist"):
            e = eng.FinetuneEngine(sd, n_views=len(ep), fine_tune_epoch=ft.LINEAR_EPOCHS, episodes_per_batch=E, mode=mode)
            e._ingest([ep], False)
            e.adapt.reset(e.W)
            if mode == "linear":
                e.set_classifier(*ft.classifier_init(5), 1)
            else:
                e.set_dist_head(*ft.dist_head_init(5), 1)
            e.prepare_batch()
            engines[mode] = (e, e.step_tables(perms, 1))
    for e, tables in engines.values():
        e.inner_loop(tables)                     # warm-up pass: every arena buffer exists, clocks are up
    torch.cuda.synchronize()
    passes = max(2, (reps + len(tables) - 1) // len(tables))
    windows = {"linear": [], "dist": []}
    for _ in range(3):                           # alternate the two modes: other work shares the machine
        for mode, (e, tables) in engines.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(passes):
                e.inner_loop(tables)
            b.record()
            torch.cuda.synchronize()
            windows[mode].append(a.elapsed_time(b) / (passes * len(tables)))
    for mode, w in windows.items():
        e = engines[mode][0]
        print("inner step, mode=%-8s E = %d, 5-way 5-shot 84x84 (fused next-step forward: %s): %s ms per step (3 windows of %d steps), "
              "median %.3f" % (repr(mode), E, e.fused_last_loop, " ".join("%.3f" % t for t in w), passes * len(engines[mode][1]),
                               float(np.median(w))), flush=True)
    for e, _ in engines.values():
        e.close()


if __name__ == "__main__":
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is nothing to time without one"
    head_launches()
    engine_steps(E_STEP)
