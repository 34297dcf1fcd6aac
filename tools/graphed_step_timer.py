"""The timed loop of the *_step_time.py tools: a graphed meta-training step (set_forward_loss + backward replayed from one hipGraph,
then the fused outer Adam; MetaTemplate._episode_loop) of a model somebody else built, 5-way 5-shot 16 queries at 84 x 84."""
import time

import torch
from meta_fine_tuning_amd import graph_step, optim, synthetic


def time_graphed_step(model, k, steps, passes=1):
    """``k`` episodes per step (k > 1: in lockstep, train.py --episodes_per_rank k), two alternating inputs, six warm-up steps, then
    ``passes`` timed passes of ``steps`` steps.  -> (seconds per step of the fastest pass, of the slowest pass, the last loss)."""
    model.train()
    model.n_query = 16
    opt = optim.Adam(model.parameters())
    eps = [synthetic.train_episode(5000 + i, 5, 5, 16, 84) for i in range(2 * k)]
    xs = [torch.stack(eps[j * k:(j + 1) * k]).cuda() if k > 1 else eps[j].cuda() for j in range(2)]
    loss_fn = model.set_forward_loss_lockstep if k > 1 else model.set_forward_loss
    step = graph_step.for_loop(model, loss_fn)
    assert step is not None, "graphed steps are disabled (MFT_TRAIN_GRAPH)"
    for i in range(6):                                   # eager warm-up, capture, first replays
        step(xs[i % 2], opt)
        opt.step()
    torch.cuda.synchronize()
    assert step.graph is not None and not step.failed
    times = []
    for _ in range(passes):
        t0 = time.perf_counter()
        for i in range(steps):
            loss = step(xs[i % 2], opt)
            opt.step()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) / steps)
    return min(times), max(times), float(loss.detach())
