"""Episodic evaluation on frozen features, E episodes in lockstep: the arithmetic of `test`.

The sequential protocol (CloserLookFewShot / CD-FSL ``test.py``: one ``feature_evaluation`` call per episode) makes every host
draw episode by episode -- ``random.sample`` of the classes, one ``np.random.permutation`` per chosen class, and, where the method
adapts a head, that head's torch-RNG initialisation followed by its 100 permutations.  ``episode_tables`` makes exactly those
draws in exactly that order for a batch of E episodes and only then goes to the device: one mft_gather_rows call assembles
``z_all`` of all E from the resident feature table, the head runs once for all E, mft_episode_top1 counts, and ONE device-to-host
copy per batch brings the E counts back.  Lockstep changes no random number.
"""
import random

import numpy as np
import torch
import torch.nn as nn

from . import autograd_ops as AG
from . import backbone, ops
from .methods.baselinefinetune import BaselineFinetune
from .methods.gnnnet import GnnNet
from .methods.meta_template import ADAPT_MAX_WAY, HeadMethod, dist_head_adapt, linear_head_adapt_episodes

N_QUERY = 15                # the protocol's query images per class
ITER_NUM = 600              # ... and episodes
EPISODES_PER_BATCH = 100
ADAPT_EPOCHS, ADAPT_BATCH = 100, 4          # set_forward_adaptation: 100 epochs of 4-row mini-batches


class FeatureTable:
    """The feature rows of ``data.feature_loader.init_loader`` as one matrix: classes in sorted label order, each class's rows in
    file order.  ``rows[label]`` = the matrix rows of that class (int64); ``device_feats()`` = the matrix on the GPU, uploaded once."""

    def __init__(self, cl_data_file):
        self.classes = sorted(cl_data_file)
        if not self.classes:
            raise ValueError("FeatureTable: the feature file holds no rows")
        self.rows, parts, at = {}, [], 0
        for c in self.classes:
            f = np.asarray(cl_data_file[c], dtype=np.float32)
            if f.ndim != 2 or f.shape[0] < 1:
                raise ValueError("FeatureTable: class %r has no [rows, D] features" % (c,))
            self.rows[c] = np.arange(at, at + f.shape[0], dtype=np.int64)
            parts.append(f)
            at += f.shape[0]
        self.feats = np.ascontiguousarray(np.concatenate(parts, axis=0))
        self._dev = None

    @property
    def dim(self):
        return self.feats.shape[1]

    def device_feats(self, device=None):
        if self._dev is None:
            self._dev = torch.from_numpy(self.feats).to(device if device is not None else torch.device("cuda", torch.cuda.current_device()))
        return self._dev


def adaptation_kind(method, adaptation):
    """Which scorer `test` uses: ``'dist'`` (baseline++: BaselineFinetune(loss_type='dist').set_forward_adaptation), ``'linear'``
    (baseline, and every method under --adaptation: MetaTemplate.set_forward_adaptation) or ``None`` (the method's set_forward)."""
    if method == 'baseline++':
        return 'dist'
    if method == 'baseline' or adaptation:
        return 'linear'
    return None


def draw_head(kind, feat_dim, n_way):
    """The torch-RNG draw set_forward_adaptation makes for its fresh head: nn.Linear(feat_dim, n_way) -> (weight, bias), or
    backbone.distLinear(feat_dim, n_way) -> (weight_v, weight_g)."""
    if kind == 'linear':
        clf = nn.Linear(feat_dim, n_way)
        return clf.weight.data, clf.bias.data
    clf = backbone.distLinear(feat_dim, n_way)
    return clf.L.weight_v.data, clf.L.weight_g.data.view(-1)


def episode_tables(class_rows, n_way, n_support, n_query, n_episodes, adapt=None, feat_dim=512):
    """The host draws of ``n_episodes`` consecutive episodes, in the sequential protocol's order.  ``class_rows``: {label: the
    table rows of that class}.  Per episode: ``random.sample(sorted(labels), n_way)``; per chosen class, in that order,
    ``np.random.permutation(len(rows))`` whose first n_support + n_query entries pick the rows; then, with ``adapt`` ('linear' /
    'dist'), the head's torch-RNG initialisation and the 100 permutations of its support rows; then the next episode.
    -> (classes [E][n_way], rows int64 [E, n_way, n_support + n_query], None | (head tensor A [E, ...], head tensor B [E, ...],
    permutations [E][100] of n_way * n_support rows))."""
    per = n_support + n_query
    labels = sorted(class_rows)
    if n_way > len(labels):
        raise ValueError("%d-way episodes need %d classes, the feature table has %d" % (n_way, n_way, len(labels)))
    short = [c for c in labels if len(class_rows[c]) < per]
    if short:
        raise ValueError("classes %s have fewer than n_support + n_query = %d feature rows" % (short[:5], per))
    classes, rows, heads_a, heads_b, perms = [], np.empty((n_episodes, n_way, per), dtype=np.int64), [], [], []
    for e in range(n_episodes):
        chosen = random.sample(labels, n_way)
        classes.append(chosen)
        for k, c in enumerate(chosen):
            r = np.asarray(class_rows[c])
            rows[e, k] = r[np.random.permutation(len(r))[:per]]
        if adapt is not None:
            a, b = draw_head(adapt, feat_dim, n_way)
            heads_a.append(a)
            heads_b.append(b)
            perms.append([np.random.permutation(n_way * n_support) for _ in range(ADAPT_EPOCHS)])
    if adapt is None:
        return classes, rows, None
    return classes, rows, (torch.stack(heads_a), torch.stack(heads_b), perms)


def check_domain(model, kind, n_way, n_support, n_query):
    """Raise the head's own ValueError for an episode shape outside its launchers' domain, before anything is launched."""
    if kind is not None:
        if not 1 <= int(n_way) <= ADAPT_MAX_WAY:
            raise ValueError("%s-head adaptation: n_way = %d is not supported (1 <= n_way <= %d)"
                             % ("cosine" if kind == 'dist' else "linear", int(n_way), ADAPT_MAX_WAY))
        if n_support < 1 or n_query < 1:
            raise ValueError("head adaptation: n_support = %d, n_query = %d (both must be >= 1)" % (n_support, n_query))
    elif isinstance(model, HeadMethod):
        model._check(n_query)
    elif isinstance(model, GnnNet):
        if n_query != N_QUERY:
            raise ValueError("GnnNet scores features of n_support + 15 rows per class (gnnnet.py:71), got n_query = %d" % n_query)
    else:
        raise TypeError("no feature-evaluation path for %s" % type(model).__name__)
    if not 1 <= int(n_way) <= ops.TOP1_MAX_WAY:
        raise ValueError("mft_episode_top1: n_way = %d is not supported (1 <= n_way <= %d)" % (int(n_way), ops.TOP1_MAX_WAY))


def score_batch(model, kind, z_all, E, n_way, n_support, n_query, heads=None):
    """z_all [E * n_way * (n_support + n_query), D] (class-major rows, one episode after the other) -> scores
    [E * n_way * n_query, n_way] from ONE head call for all E episodes."""
    D = z_all.shape[1]
    if kind is None:
        with torch.no_grad():
            if isinstance(model, HeadMethod):
                return model._head(z_all, n_query, episodes=E)
            return AG.gnnnet_head(model, z_all, model._graph_support(), n_query, fold=model.FOLD50, episodes=E)
    z = z_all.view(E, n_way, n_support + n_query, D)
    z_support = z[:, :, :n_support].reshape(E, n_way * n_support, D)
    z_query = z[:, :, n_support:].reshape(E, n_way * n_query, D)
    y_support = np.repeat(range(n_way), n_support)
    a, b, perms = heads
    if kind == 'dist':
        return dist_head_adapt(z_support, y_support, z_query, a, b, n_way, n_support, epochs=ADAPT_EPOCHS, batch_size=ADAPT_BATCH,
                               perms=perms)[0]
    return linear_head_adapt_episodes(z_support, y_support, z_query, a, b, n_way, n_support, epochs=ADAPT_EPOCHS,
                                      batch_size=ADAPT_BATCH, perms=perms)


def evaluate(model, method, table, n_way, n_support, n_query=N_QUERY, n_episodes=ITER_NUM, episodes_per_batch=EPISODES_PER_BATCH,
             adaptation=False, return_scores=False):
    """``n_episodes`` episodes sampled from ``table`` (a FeatureTable) and scored by ``model``'s head, ``episodes_per_batch`` at a
    time (the last batch may be smaller).  The caller seeds ``random``, ``np.random`` and torch.  -> float64 accuracies
    [n_episodes] in percent (and, with ``return_scores``, the list of per-episode score arrays [n_way * n_query, n_way])."""
    kind = adaptation_kind(method, adaptation)
    if isinstance(model, BaselineFinetune) and (model.loss_type == 'dist') != (kind == 'dist'):
        raise ValueError("--method %s scores with the %s head, the model was built with loss_type=%r" % (method, kind, model.loss_type))
    check_domain(model, kind, n_way, n_support, n_query)
    if table.dim != model.feat_dim:
        raise ValueError("the feature table has %d columns, the model's feat_dim is %d" % (table.dim, model.feat_dim))
    model.n_way, model.n_support, model.n_query = n_way, n_support, n_query
    feats = table.device_feats()
    rows_per_episode = n_way * n_query
    acc_all, scores_all = np.empty((n_episodes,), dtype=np.float64), []
    for e0 in range(0, n_episodes, int(episodes_per_batch)):
        E = min(int(episodes_per_batch), n_episodes - e0)
        _, rows, heads = episode_tables(table.rows, n_way, n_support, n_query, E, adapt=kind, feat_dim=table.dim)
        idx = torch.from_numpy(rows.reshape(-1).astype(np.int32)).to(feats.device)
        z_all = ops.gather_rows(feats, idx)
        scores = score_batch(model, kind, z_all, E, n_way, n_support, n_query, heads)
        correct = ops.episode_top1(scores, E, n_way, n_query).cpu().numpy()           # the batch's one device-to-host copy
        acc_all[e0:e0 + E] = correct.astype(np.float64) / rows_per_episode * 100.0
        if return_scores:
            s = scores.view(E, rows_per_episode, n_way).cpu().numpy()
            scores_all += [s[e] for e in range(E)]
    return (acc_all, scores_all) if return_scores else acc_all


def accuracy_line(acc_all):
    """The reference's line: mean and 1.96 * std / sqrt(iter_num) of the per-episode accuracies, in float64 on the host."""
    acc_all = np.asarray(acc_all, dtype=np.float64)
    iter_num = len(acc_all)
    return '%d Test Acc = %4.2f%% +- %4.2f%%' % (iter_num, np.mean(acc_all), 1.96 * np.std(acc_all) / np.sqrt(iter_num))


def build_model(method, model_func, n_way, n_support, head="ridge", kernel=None):
    """The model `test` scores with: BaselineFinetune for the two baselines, GnnNet, or the method's class of train.HEAD_METHODS
    (``head``: MetaOptNet's, --head; ``kernel``: DKT's, --kernel)."""
    from .io_utils import KERNELS, method_dir_name
    from .train import (ADAPTIVE_METHODS, EMBEDDING_METHODS, HEAD_METHODS, METRIC_METHODS, PROBABILISTIC_METHODS, TRANSDUCTIVE_METHODS,
                        head_method)
    method_dir_name(method, head, kernel)                 # a head / kernel that is unknown or not this method's is a ValueError
    if method == 'baseline':
        return BaselineFinetune(model_func, n_way, n_support)
    if method == 'baseline++':
        return BaselineFinetune(model_func, n_way, n_support, loss_type='dist')
    if method == 'gnnnet':
        return GnnNet(model_func, n_way=n_way, n_support=n_support)
    if head_method(method) is not None:
        kw = dict(head=head) if method == 'metaoptnet' else {}
        if method == 'dkt':
            kw = dict(kernel=KERNELS[0] if kernel is None else kernel)
        return head_method(method)(model_func, n_way=n_way, n_support=n_support, **kw)
    raise NotImplementedError("--method %s: 'baseline', 'baseline++', 'gnnnet', %s are on the HIP path"
                              % (method, ", ".join(repr(m) for m in sorted(list(HEAD_METHODS) + list(TRANSDUCTIVE_METHODS) + list(EMBEDDING_METHODS) + list(PROBABILISTIC_METHODS) + list(ADAPTIVE_METHODS) + list(METRIC_METHODS)))))
