#!/usr/bin/env python3
"""Episodic evaluation on frozen features: wall times on one MI355X, in one process.

  (1) save_features on the miniImageNet-shaped novel pool (64 classes x 600 images of 84 x 84, stand-in backbone weights): the
      eval-mode backbone over all 38,400 images and the file write, host clock around work that ends in a device synchronise,
      after one warm-up chunk;
  (2) per method, 600 episodes (5-way 5-shot, 15 queries) of `test` sampled from that file: feature_eval.evaluate in lockstep
      batches of 100 beside a loop over the per-episode API (set_forward / set_forward_adaptation, one host read-back per
      episode) from the same seeds; each timed after a warm-up batch, the two alternating, twice.  The accuracies of the two
      must be equal.

    python tools/feature_eval_time.py [episodes, default 600] [images per class, default 600]"""
import os
import random
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import meta_fine_tuning_amd  # noqa: E402,F401
from meta_fine_tuning_amd import configs, feature_eval, save_features, synthetic  # noqa: E402
from meta_fine_tuning_amd import test as test_driver  # noqa: E402
from meta_fine_tuning_amd.data.feature_loader import init_loader  # noqa: E402
from meta_fine_tuning_amd.io_utils import parse_args  # noqa: E402

EPISODES = int(sys.argv[1]) if len(sys.argv) > 1 else 600
PER_CLASS = int(sys.argv[2]) if len(sys.argv) > 2 else 600
CASES = [("baseline", False), ("baseline++", False), ("gnnnet", False), ("protonet", False), ("matchingnet", False),
         ("metaoptnet", False), ("protonet", True)]
N_WAY, N_SHOT, N_QUERY = 5, 5, 15


def seed():
    random.seed(10)
    np.random.seed(10)
    torch.manual_seed(10)


def state_of(method):
    sd = synthetic.resnet10_state_dict(16, prefix="feature.")
    if method == "gnnnet":
        sd.update(synthetic.gnn_head_state_dict(17, N_WAY))
    elif method == "matchingnet":
        sd.update(synthetic.matchingnet_head_state())
    elif method == "metaoptnet":
        sd.update(synthetic.metaoptnet_head_state())
    return sd


def write_checkpoint(method):
    d = save_features.checkpoint_dir(parse_args('save_features', ["--dataset", "miniImageNet", "--method", method]))
    os.makedirs(d, exist_ok=True)
    torch.save({'epoch': 0, 'state': state_of(method)}, os.path.join(d, "0.tar"))


def sequential(model, kind, cl, n_episodes):
    """The per-episode protocol through the existing API: one head call and one host read-back per episode."""
    model.n_way, model.n_support, model.n_query = N_WAY, N_SHOT, N_QUERY
    y = np.repeat(range(N_WAY), N_QUERY)
    acc = []
    for _ in range(n_episodes):
        chosen = random.sample(sorted(cl), N_WAY)
        z_all = []
        for c in chosen:
            perm = np.random.permutation(len(cl[c]))
            z_all.append([cl[c][perm[i]] for i in range(N_SHOT + N_QUERY)])
        z_all = torch.from_numpy(np.array(z_all))
        with torch.no_grad():
            s = model.set_forward_adaptation(z_all, is_feature=True) if kind is not None else model.set_forward(z_all, is_feature=True)
        pred = s.data.topk(1, 1, True, True)[1].cpu().numpy()
        acc.append(np.mean(pred[:, 0] == y) * 100)
    return np.asarray(acc)


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def main():
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is nothing to time without one"
    os.environ["MFT_POOL_PER_CLASS"] = str(PER_CLASS)
    os.environ.pop("MFT_STANDIN_WEIGHTS", None)
    with tempfile.TemporaryDirectory() as d:
        configs.save_dir = d
        for method in sorted({m for m, _ in CASES}):
            write_checkpoint(method)
        # ---- (1) save_features
        argv = ["--dataset", "miniImageNet", "--method", "protonet"]
        p = parse_args('save_features', argv)
        model = save_features.eval_backbone(save_features.resolve_state(p, verbose=False)[0], p.model)
        pool, _ = save_features.split_pool(p, torch.device("cuda", torch.cuda.current_device()))
        save_features.pool_features(model, pool[:1, :min(PER_CLASS, save_features.CHUNK)].contiguous(), 84)        # warm-up: one chunk
        t_feat, (feats, labels) = wall(lambda: save_features.pool_features(model, pool, 84))
        del pool, model
        t_all, featfile = wall(lambda: save_features.main(argv))
        print("save_features, miniImageNet-shaped novel pool, %d images of 84 x 84: backbone pass %.2f s (%.0f images/s); the whole "
              "driver (checkpoint load, pool generation, backbone pass, %.0f MB file) %.2f s"
              % (feats.shape[0], t_feat, feats.shape[0] / t_feat, os.path.getsize(featfile) / 1e6, t_all), flush=True)
        cl = init_loader(featfile)
        table = feature_eval.FeatureTable(cl)
        # ---- (2) test, lockstep beside sequential
        for method, adaptation in CASES:
            margv = ["--dataset", "miniImageNet", "--method", method]
            model, _ = test_driver.load_model(parse_args('test', margv))
            kind = feature_eval.adaptation_kind(method, adaptation)
            seed()
            feature_eval.evaluate(model, method, table, N_WAY, N_SHOT, N_QUERY, 100, 100, adaptation=adaptation)      # warm-up
            sequential(model, kind, cl, 5)
            t_lock, t_seq = [], []
            for _ in range(2):
                seed()
                t, acc_l = wall(lambda: feature_eval.evaluate(model, method, table, N_WAY, N_SHOT, N_QUERY, EPISODES, 100,
                                                              adaptation=adaptation))
                t_lock.append(t)
                seed()
                t, acc_s = wall(lambda: sequential(model, kind, cl, EPISODES))
                t_seq.append(t)
            print("test --method %-11s%s %d episodes: lockstep %s s, sequential %s s; accuracies equal: %s; %s"
                  % (method, " --adaptation" if adaptation else "", EPISODES, " / ".join("%.3f" % t for t in t_lock),
                     " / ".join("%.3f" % t for t in t_seq), bool(np.array_equal(acc_l, acc_s)), feature_eval.accuracy_line(acc_l)),
                  flush=True)


if __name__ == "__main__":
    main()
