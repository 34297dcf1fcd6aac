"""test: episodic evaluation of a trained method on the frozen features `save_features` wrote (the benchmark's standard protocol
for meta-learned methods, CloserLookFewShot / CD-FSL ``test.py``; io_utils.parse_args('test'); definition in DESIGN.md
section 16).  600 episodes are sampled from the feature table and scored by the method's head, 100 episodes per head call.

    python -m meta_fine_tuning_amd.test --dataset miniImageNet --method protonet --train_aug [--adaptation]
"""
import os
import random
import sys

import numpy as np
import torch

from . import feature_eval, save_features, settings
from .data.feature_loader import init_loader
from .io_utils import model_dict, parse_args


def load_model(params):
    """The method's model at --test_n_way / --n_shot on the GPU.  Every method except the two baselines loads its checkpoint (the
    head's weights score the episodes); the baselines train a fresh head per episode.  -> (model, checkpoint file | None)."""
    model = feature_eval.build_model(params.method, model_dict[params.model], params.test_n_way, params.n_shot,
                                     head=getattr(params, "head", "ridge"), kernel=getattr(params, "kernel", None)).cuda()
    loaded = None
    if params.method not in save_features.BASELINES:
        state, loaded = save_features.resolve_state(params)
        if loaded is None:                                # stand-in weights: whatever the model has beyond them keeps its initial value
            own = model.state_dict()
            own.update({k: v for k, v in state.items() if k in own})
            state = own
        model.load_state_dict(state)
    model.eval()
    return model, loaded


def main(argv=None):
    params = parse_args('test', argv)
    save_features.check_method(params.method)
    if params.unsup or params.unsup_cluster:
        raise NotImplementedError("--unsup / --unsup_cluster: the reference defines no unsupervised evaluation for its `test` flags")
    if params.method == 'gnnnet' and params.n_shot == 50:
        raise NotImplementedError("--method gnnnet --n_shot 50: the 50-shot fold lives in methods.gnnnet_copy and is evaluated by "
                                  "finetune_50.main, not by test")
    cfg = settings.current()
    iter_num = feature_eval.ITER_NUM if cfg.episodes is None else cfg.episodes
    per_batch = feature_eval.EPISODES_PER_BATCH if cfg.episodes_per_batch is None else cfg.episodes_per_batch
    featfile = save_features.features_file(params)
    if not os.path.isfile(featfile):
        raise FileNotFoundError("feature file %s not found: run save_features with the same flags first" % featfile)
    model, loaded = load_model(params)
    table = feature_eval.FeatureTable(init_loader(featfile))
    random.seed(10)
    np.random.seed(10)
    torch.manual_seed(10)
    acc_all = feature_eval.evaluate(model, params.method, table, params.test_n_way, params.n_shot, feature_eval.N_QUERY, iter_num,
                                    per_batch, adaptation=params.adaptation)
    standin = loaded is None and params.method not in save_features.BASELINES
    print(feature_eval.accuracy_line(acc_all) + "   [features of a SYNTHETIC dataset-shaped pool]"
          + ("   [SYNTHETIC stand-in weights, MFT_STANDIN_WEIGHTS=1]" if standin else ""))
    sys.stdout.flush()
    return acc_all


if __name__ == '__main__':
    main()
