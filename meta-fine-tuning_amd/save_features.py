"""save_features: the backbone's eval-mode features of a whole split, computed once (the benchmark's standard protocol for
meta-learned methods, CloserLookFewShot / CD-FSL ``save_features.py``; io_utils.parse_args('save_features'); definition in
DESIGN.md section 16).  `test` then samples its episodes from the file this writes.

    python -m meta_fine_tuning_amd.save_features --dataset miniImageNet --method protonet --train_aug
"""
import os
import sys

import numpy as np
import torch

from . import augment, backbone, configs, settings, synthetic
from .data.feature_loader import save_features_file
from .io_utils import get_assigned_file, get_best_file, get_resume_file, method_dir_name, model_dict, parse_args

BASELINES = ('baseline', 'baseline++')
METHODS = BASELINES + ('gnnnet', 'protonet', 'matchingnet', 'metaoptnet', 'tpn', 'feat', 'dkt', 'anil', 'mahalanobis')
SPLIT_SEEDS = {'base': 0, 'val': 2, 'novel': 3}       # miniImageNet-shaped pool per --split; 'base' is train.main's pool (seed 0)
TEST_DATASET_SEED = 1                                 # --test_dataset X: the pool finetune.main evaluates on
CHUNK = 200                                           # images per backbone forward


def check_method(method):
    if method not in METHODS:
        raise NotImplementedError("--method %s: %s are on the HIP path" % (method, ", ".join(repr(m) for m in METHODS)))


def checkpoint_dir(p):
    """The directory train.main writes: <save_dir>/checkpoints/<dataset>/<model>_<method>[_aug][_<train_n_way>way_<n_shot>shot]
    (the two baselines carry no way / shot suffix, train.py:176-180; ``--head svm``: <method> reads metaoptnet_svm; ``--kernel linear``: dkt_linear)."""
    d = '%s/checkpoints/%s/%s_%s' % (configs.save_dir, p.dataset, p.model,
                                     method_dir_name(p.method, getattr(p, "head", "ridge"), getattr(p, "kernel", None)))
    if p.train_aug:
        d += '_aug'
    if p.method not in BASELINES:
        d += '_%dway_%dshot' % (p.train_n_way, p.n_shot)
    return d


def checkpoint_file(p):
    """``--save_iter N``: N.tar; otherwise the newest epoch for the two baselines (get_resume_file) and best_model.tar / the newest
    epoch for every other method (get_best_file).  None: the directory holds no checkpoint."""
    d = checkpoint_dir(p)
    if p.save_iter != -1:
        return get_assigned_file(d, p.save_iter)
    return get_resume_file(d) if p.method in BASELINES else get_best_file(d)


def features_file(p):
    """<checkpoint_dir with "checkpoints" -> "features">/<split>[_<save_iter>].npz"""
    name = p.split if p.save_iter == -1 else '%s_%d' % (p.split, p.save_iter)
    return os.path.join(checkpoint_dir(p).replace("checkpoints", "features"), name + ".npz")


def resolve_state(p, verbose=True):
    """The checkpoint's state dict (finetune._resolve_state: a missing file is a FileNotFoundError unless MFT_STANDIN_WEIGHTS=1
    puts the deterministic stand-in weights in its place) -> (state, file | None)."""
    from .finetune import _resolve_state
    state, loaded = _resolve_state(p.method, checkpoint_file(p), p.test_n_way, p.save_iter != -1, verbose)
    from .train import head_method
    if loaded is None and head_method(p.method) is not None:
        # the stand-in is a GnnNet state: keep its backbone, put the method's own seeded head behind it
        state = type(state)((k, v) for k, v in state.items() if k.startswith("feature."))
        state.update({'matchingnet': synthetic.matchingnet_head_state, 'metaoptnet': synthetic.metaoptnet_head_state,
                      'tpn': synthetic.tpn_head_state, 'feat': synthetic.feat_head_state, 'dkt': synthetic.dkt_head_state,
                      'anil': lambda: synthetic.anil_head_state(n_way=p.test_n_way)}.get(p.method, dict)())
    return state, loaded


def feature_state(state):
    """The ``feature.*`` entries with the prefix stripped; ``feature2.`` / ``feature3.`` (what a --fine_tune run leaves behind) and
    the gamma / beta of ResNet10_FW are dropped: at test time the feature-wise transformation is the identity."""
    sd = type(state)((k[len("feature."):], v) for k, v in state.items() if k.startswith("feature."))
    return backbone.plain_state_dict(sd)


def eval_backbone(state, model_name):
    """``model_dict[model_name]()`` with the checkpoint's backbone weights, on the GPU, in eval mode (running statistics).  An
    eval-mode ResNet10_FW is ResNet10 bit for bit: its gamma / beta keep their initial values and are never read."""
    model = model_dict[model_name]()
    missing, unexpected = model.load_state_dict(feature_state(state), strict=False)
    if unexpected or any(not k.endswith((".gamma", ".beta")) for k in missing):
        raise RuntimeError("checkpoint does not fit %s: missing %s, unexpected %s" % (model_name, missing, unexpected))
    return model.cuda().eval()


def split_pool(p, device):
    """The dataset-shaped resident pool (synthetic.class_pool_u8) the features are computed on -> (pool, its dataset name)."""
    cfg = settings.current()
    if p.test_dataset:
        if p.test_dataset not in synthetic.DATASET_SHAPES or p.test_dataset == "miniImageNet":
            raise ValueError('Unknown test dataset %r (the reference knows ISIC, EuroSAT, CropDisease, ChestX)' % p.test_dataset)
        return synthetic.class_pool_u8(p.test_dataset, device, seed=TEST_DATASET_SEED, n_per_class=cfg.pool_per_class), p.test_dataset
    if p.split not in SPLIT_SEEDS:
        raise ValueError("--split %r: base, val or novel" % (p.split,))
    return synthetic.class_pool_u8("miniImageNet", device, seed=SPLIT_SEEDS[p.split], n_per_class=cfg.pool_per_class), "miniImageNet"


def pool_features(model, pool, size, chunk=CHUNK):
    """pool uint8 [n_classes, n_per_class, Hs, Ws, 3] on the device -> (features [count, feat_dim] float32, labels [count] int32)
    on the host: every image through the non-augmenting view (Resize(1.15 * size) + CenterCrop(size), ImageNet normalisation) and
    the eval-mode backbone, ``chunk`` images per forward."""
    n_classes, per, Hs, Ws, _ = pool.shape
    images = pool.view(n_classes * per, Hs, Ws, 3)
    count = images.shape[0]
    feats = np.empty((count, model.final_feat_dim), dtype=np.float32)
    with torch.no_grad():
        for i0 in range(0, count, chunk):
            src = images[i0:i0 + chunk].contiguous()
            P = augment.sample_train_view_params(None, src.shape[0], Hs, Ws, size, False)
            x = augment.augment_views(src, P, size)[0].permute(0, 3, 1, 2)            # NHWC in memory, NCHW shape
            feats[i0:i0 + src.shape[0]] = model(x).cpu().numpy()
    return feats, np.repeat(np.arange(n_classes, dtype=np.int32), per)


def main(argv=None):
    params = parse_args('save_features', argv)
    check_method(params.method)
    state, loaded = resolve_state(params)
    model = eval_backbone(state, params.model)
    device = torch.device("cuda", torch.cuda.current_device())
    pool, shaped = split_pool(params, device)
    feats, labels = pool_features(model, pool, settings.current().image_size)
    outfile = features_file(params)
    os.makedirs(os.path.dirname(outfile), exist_ok=True)
    save_features_file(outfile, feats, labels)
    print("%d x %d features of split %s -> %s   [SYNTHETIC %s-shaped pool resident in HBM: no image files are read]%s"
          % (feats.shape[0], feats.shape[1], params.split, outfile, shaped,
             "" if loaded is not None else "   [SYNTHETIC stand-in weights, MFT_STANDIN_WEIGHTS=1]"))
    sys.stdout.flush()
    return outfile


if __name__ == '__main__':
    main()
