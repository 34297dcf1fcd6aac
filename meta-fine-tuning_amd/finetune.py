"""Test-time fine-tuning driver (mirror of finetune.py:45-328,424-682).

``finetune(liz_x, y, model, state_in, save_it, ...)`` / ``finetune_linear(...)`` keep the reference's signatures and
semantics (module-global ``params`` supplies ``model`` and ``fine_tune_epoch``; permutations come from the global numpy
RNG).  Three ways in, same arithmetic and same permutation stream:

* one call per episode, as the reference's loop does (finetune.py:599-666): an engine with a batch of one;
* ``finetune_batched`` / ``finetune_all_batched``: E independent episodes in lockstep (the throughput path);
* the reference-shaped loop UNCHANGED except that the loader is wrapped in ``LookaheadLoader``: the wrapper reads E
  episodes ahead, runs them as one lockstep batch (drawing their permutations in the order the sequential calls would) and
  the per-episode ``finetune()`` / ``finetune_linear()`` calls of the loop body return the finished scores.

``main`` mirrors the reference's ``__main__``: ``--method gnnnet | baseline | baseline++ | all``, ``--freeze_backbone``,
``--n_shot 50`` (gnnnet_copy, as finetune_50.py:20).  Launched under ``torchrun`` it shards the 600 episodes over the ranks
(parallel.shard_indices, one all-gather of accuracies at the end -- SURVEY.md §8(e)).  Checkpoints are looked up where the reference looks
(``checkpoint_files``, finetune.py:448-527); real datasets are out of scope: episodes are the in-repo
synthetic ones, and without a checkpoint on disk the weights are too (``standin_state``).
"""
import hashlib
import os
import sys

import numpy as np
import torch

from . import engine as eng
from . import parallel
from . import settings
from . import synthetic
from .io_utils import model_dict, parse_args  # noqa: F401  (re-exported like the reference)
from .methods.meta_template import HeadMethod

params = None          # set by main(); finetune() reads params.model / params.fine_tune_epoch (finetune.py:185,261)

LINEAR_EPOCHS = 20     # finetune.py:134 (total_epoch = 20 in finetune_linear)
EPISODIC_METHODS = ("gnnnet", "protonet", "matchingnet", "metaoptnet")     # scored by finetune(): "gnnnet" + train.HEAD_METHODS


# ------------------------------------------------------------------------------------------------ engine cache

def _feature_items(state_in):
    return [(k, v) for k, v in state_in.items() if k.startswith("feature.") and not k.startswith(("feature2.", "feature3."))]


def _state_ident(state_in):
    """Cheap identity of a checkpoint's backbone tensors: (key, address, autograd version).  Valid only while the cache entry
    keeps the tensors alive (it does), so an address cannot be recycled for different weights."""
    return tuple((k, v.data_ptr(), v._version, tuple(v.shape)) for k, v in _feature_items(state_in))


def _state_fingerprint(state_in):
    """Content hash of the backbone tensors (19.6 MB: ~15 ms).  Two checkpoints with equal bytes share one engine -- the
    reference deep-copies the state for every episode (finetune.py:187), callers may too."""
    h = hashlib.blake2b(digest_size=16)
    for k, v in _feature_items(state_in):
        h.update(k.encode())
        h.update(v.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


class _EngineCache:
    """Engines keyed on WHAT the checkpoint contains, not on where the caller's dict lives.  An entry pins the state dict it
    was built from; a miss on the cheap identity falls back to the content hash (and remembers the new identity)."""

    def __init__(self, capacity):
        self.capacity = capacity
        self.entries = []          # dicts: idents (set), fp, cfg, engine, pins (list of state dicts kept alive)

    def get(self, state_in, cfg, build):
        ident = _state_ident(state_in)
        for ent in self.entries:
            if ent["cfg"] == cfg and ident in ent["idents"]:
                return ent["engine"]
        fp = _state_fingerprint(state_in)
        for ent in self.entries:
            if ent["cfg"] == cfg and ent["fp"] == fp:
                if len(ent["pins"]) < 4:                 # remember a few aliases; beyond that just re-hash
                    ent["idents"].add(ident)
                    ent["pins"].append(state_in)
                return ent["engine"]
        while len(self.entries) >= self.capacity:
            old = self.entries.pop(0)
            old["engine"].close()
        e = build()
        self.entries.append({"idents": {ident}, "fp": fp, "cfg": cfg, "engine": e, "pins": [state_in]})
        return e

    def clear(self):
        for ent in self.entries:
            ent["engine"].close()
        self.entries = []


_ENGINES = _EngineCache(3)
_LIN_ENGINES = _EngineCache(2)
_DIST_ENGINES = _EngineCache(2)


def _head_key(model):
    return tuple((p.data_ptr(), p._version) for p in list(model.fc.parameters()) + list(model.gnn.parameters()))


def _engine_for(state_in, model, n_way, n_support, n_query, size, n_views, epochs, E, fold50=False):
    """The finetune() engine for ``model``: a HeadMethod (ProtoNet, MatchingNet, MetaOptNet) scores with its own head -- the
    engine mode it names, keyed on that mode and the (address, version) of each parameter it lists (a ProtoNet lists none) --,
    anything else with the GNN head of its fc / gnn modules."""
    if isinstance(model, HeadMethod):
        mode = model.ENGINE_MODE
        cfg = (mode, *((p.data_ptr(), p._version) for p in model.head_params()), n_way, n_support, n_query, size, n_views, epochs, E)

        def build_head():
            return eng.FinetuneEngine(state_in, n_way, n_support, n_query, size, n_views=n_views, fine_tune_epoch=epochs,
                                      episodes_per_batch=E, mode=mode, head_state=model.head_state())
        return _ENGINES.get(state_in, cfg, build_head)
    cfg = ("gnn", _head_key(model), n_way, n_support, n_query, size, n_views, epochs, E, fold50)

    def build():
        head = {"fc." + k: v for k, v in model.fc.state_dict().items()}
        head.update({"gnn." + k: v for k, v in model.gnn.state_dict().items()})
        return eng.FinetuneEngine(state_in, n_way, n_support, n_query, size, n_views=n_views, fine_tune_epoch=epochs,
                                  episodes_per_batch=E, head_state=head, fold50=fold50)
    return _ENGINES.get(state_in, cfg, build)


def _linear_engine(state_in, n_way, n_support, n_query, size, n_views, E):
    cfg = ("linear", n_way, n_support, n_query, size, n_views, E)

    def build():
        return eng.FinetuneEngine(state_in, n_way, n_support, n_query, size, n_views=n_views, fine_tune_epoch=LINEAR_EPOCHS,
                                  episodes_per_batch=E, mode="linear")
    return _LIN_ENGINES.get(state_in, cfg, build)


def _dist_engine(state_in, n_way, n_support, n_query, size, n_views, E):
    cfg = ("dist", n_way, n_support, n_query, size, n_views, E)

    def build():
        return eng.FinetuneEngine(state_in, n_way, n_support, n_query, size, n_views=n_views, fine_tune_epoch=LINEAR_EPOCHS,
                                  episodes_per_batch=E, mode="dist")
    return _DIST_ENGINES.get(state_in, cfg, build)


# ------------------------------------------------------------------------------------------------ lookahead registry

_READY = {}            # id(first view tensor) -> {"pin": tensor, "gnn" / "linear" / "dist": scores | None, "ctx": {...}}


def _take_ready(liz_x, kind, freeze_backbone=False, state_in=None, model=None):
    """Scores a LookaheadLoader parked for this episode, or None.  An entry was computed for ONE (state dict, model,
    freeze_backbone) combination: a call that asks for anything else raises instead of silently returning the parked result
    (the lookahead has already consumed this episode's permutations, so recomputing here would not be the reference's stream
    either)."""
    ent = _READY.get(id(liz_x[0]))
    if ent is None or ent["pin"] is not liz_x[0] or ent.get(kind) is None:
        return None
    ctx = ent["ctx"]
    want_state = ctx["state_gnn"] if kind == "gnn" else ctx["state_b"]
    if bool(freeze_backbone) != ctx["freeze_backbone"] or (state_in is not None and state_in is not want_state) \
            or (kind == "gnn" and model is not None and model is not ctx["model"]):
        raise RuntimeError("LookaheadLoader parked %s scores for this episode with freeze_backbone=%s and its own state_in / "
                           "model; this call asks for freeze_backbone=%s / another state_in or model -- construct the loader "
                           "with the arguments the loop body passes" % (kind, ctx["freeze_backbone"], bool(freeze_backbone)))
    sc = ent[kind]
    ent[kind] = None
    if ent.get("gnn") is None and ent.get("linear") is None and ent.get("dist") is None:
        del _READY[id(liz_x[0])]
    return sc


# ------------------------------------------------------------------------------------------------ per-episode entry points

def refuse_feature_wise_model(model_name, who):
    if model_name == 'ResNet10_FW':
        raise NotImplementedError("%s --model ResNet10_FW: the feature-wise transformation backbone is a meta-training backbone; at "
                                  "test time the transformation is off, so evaluate the checkpoint with --model ResNet10 after "
                                  "backbone.plain_state_dict(state) dropped its gamma / beta keys" % who)


def refuse_transductive(model=None, method=None, who="finetune"):
    """TPN (methods/tpn.py) scores the queries of an episode together on a graph over support AND query nodes; the test-time engine
    adapts on the support rows and scores each query on its own.  FEAT (methods/feat.py) adapts the prototypes to each other with a
    trained set-to-set function, DKT (methods/dkt.py) conditions a Gaussian process on the support rows, ANIL (methods/anil.py)
    takes gradient steps from a trained classifier initialisation, and Mahalanobis (methods/mahalanobis.py) scores with a covariance
    per class; the engine has no mode for any of them."""
    from .train import ADAPTIVE_METHODS, EMBEDDING_METHODS, METRIC_METHODS, PROBABILISTIC_METHODS, TRANSDUCTIVE_METHODS
    if method in METRIC_METHODS or isinstance(model, tuple(METRIC_METHODS.values())):
        raise NotImplementedError("%s --method %s: the test-time engine has no per-class-covariance mode; score the method with `test` "
                                  "(save_features, then test --method %s)" % ((who,) + 2 * (method or model.METHOD,)))
    if method in ADAPTIVE_METHODS or isinstance(model, tuple(ADAPTIVE_METHODS.values())):
        raise NotImplementedError("%s --method %s: the test-time engine has no trained-initialisation inner-loop mode; score the method "
                                  "with `test` (save_features, then test --method %s)" % ((who,) + 2 * (method or model.METHOD,)))
    if method in PROBABILISTIC_METHODS or isinstance(model, tuple(PROBABILISTIC_METHODS.values())):
        raise NotImplementedError("%s --method %s: the test-time engine has no Gaussian-process mode; score the method with `test` "
                                  "(save_features, then test --method %s)" % ((who,) + 2 * (method or model.METHOD,)))
    if method in EMBEDDING_METHODS or isinstance(model, tuple(EMBEDDING_METHODS.values())):
        raise NotImplementedError("%s --method %s: the test-time engine has no embedding-adaptation mode; score the method with `test` "
                                  "(save_features, then test --method %s)" % ((who,) + 2 * (method or model.METHOD,)))
    if method in TRANSDUCTIVE_METHODS or isinstance(model, tuple(TRANSDUCTIVE_METHODS.values())):
        raise NotImplementedError("%s --method %s: the test-time engine has no transductive mode; score the method with `test` "
                                  "(save_features, then test --method %s)" % ((who,) + 2 * (method or model.METHOD,)))


def _params_of(p):
    if p is not None:
        refuse_feature_wise_model(p.model, "finetune")
    if p is None or p.model != 'ResNet10':
        raise RuntimeError("finetune.params must be set (Namespace(model='ResNet10', fine_tune_epoch=...))")
    return p


def _eval_backbone(state_in, model_name):
    refuse_feature_wise_model(model_name, "finetune")
    eng.refuse_feature_wise(state_in, "finetune")
    feat = model_dict[model_name](flatten=True)
    feat.load_state_dict({k.replace("feature.", "", 1): v for k, v in _feature_items(state_in)})
    return feat.cuda().eval()


def _finetune(P, liz_x, y, model, state_in, save_it, linear=False, flatten=True, n_query=15, ds=False,
              pretrained_dataset='miniImageNet', freeze_backbone=False, n_way=5, n_support=5):
    if linear or not flatten or ds:
        raise NotImplementedError("finetune(): only the GNN scoring branch with a flattened backbone is on the HIP hot path "
                                  "(the linear branch is finetune_linear(); ds = DampNet, out of scope)")
    refuse_transductive(model)
    P = _params_of(P)
    ready = _take_ready(liz_x, "gnn", freeze_backbone, state_in, model)
    if ready is not None:
        model.n_query = liz_x[0].size(1) - n_support               # finetune.py:312
        return ready
    model = model.cuda()
    x0 = liz_x[0]
    n_query = x0.size(1) - n_support
    if freeze_backbone:
        # finetune.py:253-266: eval-mode backbone, no backbone optimiser; the classifier gets no gradient either, so the
        # loop at :270-299 changes nothing -- it only consumes one permutation per epoch.  Scores = GNN on eval features.
        for _ in range(P.fine_tune_epoch):
            np.random.permutation(n_way * n_support * (len(liz_x) + 1))
        feat = _eval_backbone(state_in, P.model)
        with torch.no_grad():
            out_all = feat(x0.cuda().reshape(-1, *x0.shape[2:])).view(n_way, n_support + n_query, -1)
            model.n_query = n_query
            from . import ops
            return ops.softmax_rows(model.set_forward(out_all, is_feature=True).float().contiguous())
    e = _engine_for(state_in, model, n_way, n_support, n_query, x0.size(-1), len(liz_x), P.fine_tune_epoch, 1,
                    fold50=getattr(model, "FOLD50", False))
    model.n_query = n_query                                          # finetune.py:312
    return e.run_batch([liz_x])[0].clone()


def finetune(liz_x, y, model, state_in, save_it, linear=False, flatten=True, n_query=15, ds=False,
             pretrained_dataset='miniImageNet', freeze_backbone=False, n_way=5, n_support=5):
    """One episode: liz_x = [x0, x0, aug_1, ...] each [n_way, n_support+n_query, 3, H, W]; returns softmax scores
    [n_way*n_query, n_way] (finetune.py:182-328)."""
    return _finetune(params, liz_x, y, model, state_in, save_it, linear, flatten, n_query, ds, pretrained_dataset,
                     freeze_backbone, n_way, n_support)


def classifier_init(n_way, dim=512, n=1):
    """Initial weights of ``Classifier(dim, n_way)`` (finetune.py:33-42,65): torch's nn.Linear default draw from the
    global torch RNG, one fresh classifier per episode as in the reference."""
    ws, bs = [], []
    for _ in range(n):
        lin = torch.nn.Linear(dim, n_way)
        ws.append(lin.weight.detach())
        bs.append(lin.bias.detach())
    return torch.stack(ws), torch.stack(bs)


def _finetune_linear_frozen(P, x0, state_in, n_way, n_support, n_query, classifier):
    """finetune_linear(freeze_backbone=True) (finetune.py:45-174, frozen branch): eval-mode features are constants, only the
    Linear(512, n_way) classifier is trained -- 20 epochs of mini-batches of 5 with Adam(lr .01, weight_decay .001), all
    steps in one launch (mft_linear_head_adam_run) -- and the scores are softmax(classifier(features of the queries))."""
    from . import ops
    feat = _eval_backbone(state_in, P.model if P is not None else 'ResNet10')
    support_size, batch_size, epochs = n_way * n_support, 5, LINEAR_EPOCHS
    with torch.no_grad():
        x = x0.cuda()
        za = feat(x[:, :n_support].reshape(support_size, *x.shape[2:])).float().contiguous()
        zb = feat(x[:, n_support:].reshape(n_way * n_query, *x.shape[2:])).float().contiguous()
    w0, b0 = classifier_init(n_way) if classifier is None else (torch.as_tensor(classifier[0]), torch.as_tensor(classifier[1]))
    W = w0.detach().clone().float().cuda().contiguous().view(1, n_way, -1)
    b = b0.detach().clone().float().cuda().contiguous().view(1, n_way)
    steps = []
    for _ in range(epochs):                                          # finetune.py:139-141: one permutation per epoch
        rand_id = np.random.permutation(support_size)
        for j in range(0, support_size, batch_size):
            ids = rand_id[j:min(j + batch_size, support_size)]
            steps.append(np.concatenate([ids, -np.ones(batch_size - len(ids), dtype=ids.dtype)]))
    table = torch.from_numpy(np.stack(steps).astype(np.int32)).cuda()
    y_dev = torch.from_numpy(np.repeat(np.arange(n_way), n_support).astype(np.int32)).cuda()
    ops.linear_head_adam_run(za[None], y_dev[None], table[None], W, b, lr=0.01, weight_decay=0.001)
    return ops.linear_head_scores(zb, W, b)                          # softmax(zb @ W^T + b): one group of all query rows


def _finetune_linear(P, liz_x, y, state_in, save_it, linear=False, flatten=True, n_query=15, ds=False,
                     pretrained_dataset='miniImageNet', freeze_backbone=False, n_way=5, n_support=5, classifier=None):
    if not flatten:
        raise NotImplementedError("finetune_linear(): flatten=False is outside the HIP hot path")
    ready = _take_ready(liz_x, "linear", freeze_backbone, state_in)
    if ready is not None:
        return ready
    x0 = liz_x[0]
    n_query = x0.size(1) - n_support
    if freeze_backbone:
        return _finetune_linear_frozen(P, x0, state_in, n_way, n_support, n_query, classifier)
    e = _linear_engine(state_in, n_way, n_support, n_query, x0.size(-1), len(liz_x), 1)
    w0, b0 = classifier_init(n_way) if classifier is None else (torch.as_tensor(classifier[0]).view(1, n_way, -1),
                                                                 torch.as_tensor(classifier[1]).view(1, n_way))
    return e.run_batch([liz_x], classifier_init=(w0, b0))[0].clone()


def finetune_linear(liz_x, y, state_in, save_it, linear=False, flatten=True, n_query=15, ds=False,
                    pretrained_dataset='miniImageNet', freeze_backbone=False, n_way=5, n_support=5, classifier=None):
    """finetune.finetune_linear (finetune.py:45-174): the "baseline" branch of the README ensemble.  ``classifier`` =
    (w0 [n_way,512], b0 [n_way]) pins the initial Linear weights (default: torch's nn.Linear draw, as the reference)."""
    return _finetune_linear(params, liz_x, y, state_in, save_it, linear, flatten, n_query, ds, pretrained_dataset,
                            freeze_backbone, n_way, n_support, classifier)


def finetune_all(liz_x, y, model, state_baseline, state_gnn, n_way=5, n_support=5, classifier=None, freeze_backbone=False):
    """``--method all`` (finetune.py:634-649): scores_out = finetune_linear(baseline state) + finetune(gnnnet state);
    the numpy permutation stream is consumed in that order."""
    out = finetune_linear(liz_x, y, state_baseline, None, linear=True, n_way=n_way, n_support=n_support,
                          classifier=classifier, freeze_backbone=freeze_backbone)
    out = out + finetune(liz_x, y, model, state_gnn, 600, n_way=n_way, n_support=n_support, freeze_backbone=freeze_backbone)
    return out


# ------------------------------------------------------------------------------------------------ batched entry points

def draw_episode_perms(method, n_way, n_support, n_views, fine_tune_epoch, rng=np.random):
    """The permutations ONE episode consumes, in the reference's order: ``--method all`` / ``baseline`` first draw
    finetune_linear's 20 permutations of the support set (finetune.py:139-141), then ``all`` / ``gnnnet`` draw finetune's
    ``fine_tune_epoch`` permutations of n_way*n_support*(n_views+1) (finetune.py:269-272).  -> (linear perms | None, gnn perms | None)"""
    lin = gnn = None
    if method in ("all", "baseline", "baseline++"):          # (finetune_dist is finetune_linear's loop: the same 20 draws)
        lin = [rng.permutation(n_way * n_support) for _ in range(LINEAR_EPOCHS)]
    if method in ("all",) + EPISODIC_METHODS:
        gnn = [rng.permutation(n_way * n_support * (n_views + 1)) for _ in range(fine_tune_epoch)]
    return lin, gnn


def finetune_batched(episodes, model, state_in, fine_tune_epoch, n_way=5, n_support=5, episodes_per_batch=32,
                     perms=None):
    """Throughput path: ``episodes`` (list of liz_x) processed ``episodes_per_batch`` at a time in lockstep.
    Permutations are drawn episode by episode from the global numpy RNG (the reference's order) unless given."""
    refuse_transductive(model, who="finetune_batched")
    model = model.cuda()
    x0 = episodes[0][0]
    n_query = x0.size(1) - n_support
    e = _engine_for(state_in, model, n_way, n_support, n_query, x0.size(-1), len(episodes[0]), fine_tune_epoch,
                    episodes_per_batch, fold50=getattr(model, "FOLD50", False))
    out = []
    for i in range(0, len(episodes), episodes_per_batch):
        chunk = episodes[i:i + episodes_per_batch]
        p = None if perms is None else perms[i:i + episodes_per_batch]
        out.append(e.run_batch(chunk, perms=p).clone())
    return torch.cat(out)


def finetune_linear_batched(episodes, state_in, n_way=5, n_support=5, episodes_per_batch=32, perms=None, classifiers=None):
    """finetune_linear over a list of episodes in lockstep.  ``classifiers`` = (w0 [n,n_way,512], b0 [n,n_way]); default: one
    nn.Linear draw per episode from torch's global RNG, in episode order."""
    x0 = episodes[0][0]
    n_query = x0.size(1) - n_support
    e = _linear_engine(state_in, n_way, n_support, n_query, x0.size(-1), len(episodes[0]), episodes_per_batch)
    if classifiers is None:
        classifiers = classifier_init(n_way, n=len(episodes))
    out = []
    for i in range(0, len(episodes), episodes_per_batch):
        chunk = episodes[i:i + episodes_per_batch]
        p = None if perms is None else perms[i:i + episodes_per_batch]
        ci = (classifiers[0][i:i + len(chunk)], classifiers[1][i:i + len(chunk)])
        out.append(e.run_batch(chunk, perms=p, classifier_init=ci).clone())
    return torch.cat(out)


BASELINEPP_EPOCHS = 100     # baselinefinetune.py:42


def dist_head_init(n_way, dim=512, n=1):
    """Initial (v0 [n, n_way, dim], g0 [n, n_way, 1]) of ``n`` fresh backbone.distLinear(dim, n_way) heads: one draw per episode
    from torch's global RNG, in episode order, as BaselineFinetune(loss_type='dist') makes them."""
    from . import backbone
    heads = [backbone.distLinear(dim, n_way) for _ in range(n)]
    return torch.stack([h.L.weight_v.data for h in heads]), torch.stack([h.L.weight_g.data for h in heads])


def baselinepp_batched(episodes, state_in, n_way=5, n_support=5, episodes_per_batch=32, perms=None, heads=None):
    """Baseline++ adaptation (BaselineFinetune(loss_type='dist').set_forward on the checkpoint's eval-mode features of view 0)
    over a list of episodes, ``episodes_per_batch`` heads per launch: features through ``_eval_backbone``, then per batch ONE
    mft_dist_head_sgd_run launch (100 epochs of mini-batches of 4 for every head) and ONE scoring launch with its softmax
    epilogue.  ``perms[i]``: the 100 permutations of episode i (default: drawn episode by episode from the global numpy RNG);
    ``heads`` = (v0 [n, n_way, 512], g0 [n, n_way, 1]) (default: ``dist_head_init``).  -> [n * n_way * n_query, n_way]."""
    from .methods.meta_template import dist_head_adapt
    n = len(episodes)
    x0 = episodes[0][0]
    n_query = x0.size(1) - n_support
    S = n_way * n_support
    if perms is None:
        perms = [[np.random.permutation(S) for _ in range(BASELINEPP_EPOCHS)] for _ in range(n)]
    v0, g0 = dist_head_init(n_way, n=n) if heads is None else (torch.as_tensor(heads[0]), torch.as_tensor(heads[1]))
    feat = _eval_backbone(state_in, params.model if params is not None else 'ResNet10')
    y_support = np.repeat(np.arange(n_way), n_support)
    out = []
    for i in range(0, n, episodes_per_batch):
        chunk = episodes[i:i + episodes_per_batch]
        zs, zq = [], []
        with torch.no_grad():
            for liz_x in chunk:
                x = liz_x[0].cuda()
                z = feat(x.reshape(-1, *x.shape[2:])).float().view(n_way, n_support + n_query, -1)
                zs.append(z[:, :n_support].reshape(S, -1))
                zq.append(z[:, n_support:].reshape(n_way * n_query, -1))
        sc, _, _ = dist_head_adapt(torch.stack(zs), y_support, torch.stack(zq), v0[i:i + len(chunk)], g0[i:i + len(chunk)], n_way,
                                   n_support, epochs=BASELINEPP_EPOCHS, perms=perms[i:i + len(chunk)], softmax=True)
        out.append(sc)
    return torch.cat(out)


def _finetune_dist(P, liz_x, y, state_in, save_it, linear=False, flatten=True, n_query=15, ds=False,
                   pretrained_dataset='miniImageNet', freeze_backbone=False, n_way=5, n_support=5, head=None):
    if not flatten:
        raise NotImplementedError("finetune_dist(): flatten=False is outside the HIP hot path")
    ready = _take_ready(liz_x, "dist", freeze_backbone, state_in)
    if ready is not None:
        return ready
    x0 = liz_x[0]
    n_query = x0.size(1) - n_support
    heads = None if head is None else (torch.as_tensor(head[0]).view(1, n_way, -1), torch.as_tensor(head[1]).view(1, n_way, 1))
    if freeze_backbone:
        return baselinepp_batched([liz_x], state_in, n_way, n_support, 1, heads=heads)
    e = _dist_engine(state_in, n_way, n_support, n_query, x0.size(-1), len(liz_x), 1)
    v0, g0 = dist_head_init(n_way) if heads is None else heads
    return e.run_batch([liz_x], classifier_init=(v0, g0))[0].clone()


def finetune_dist(liz_x, y, state_in, save_it, linear=False, flatten=True, n_query=15, ds=False,
                  pretrained_dataset='miniImageNet', freeze_backbone=False, n_way=5, n_support=5, head=None):
    """Baseline++ at test time: the reference's finetune_linear (finetune.py:45-174) with ``Classifier`` replaced by
    ``distLinear(512, n_way)`` -- 20 epochs over the ORIGINAL support images in mini-batches of 5, Adam(0.01,
    weight_decay=0.001) on the head and Adam(0.01) on trunk.7, scores = softmax(head(features of the queries)).  ``head`` =
    (v0 [n_way, 512], g0 [n_way, 1]) pins the initial head (default: one ``dist_head_init`` draw from torch's global RNG).
    ``freeze_backbone=True`` is Baseline++'s OWN protocol instead (``baselinepp_batched``: eval-mode features, 100 epochs of
    SGD on the head alone), not a frozen variant of the loop above."""
    return _finetune_dist(params, liz_x, y, state_in, save_it, linear, flatten, n_query, ds, pretrained_dataset,
                          freeze_backbone, n_way, n_support, head)


def finetune_dist_batched(episodes, state_in, n_way=5, n_support=5, episodes_per_batch=32, perms=None, heads=None):
    """finetune_dist over a list of episodes in lockstep (FinetuneEngine(mode="dist")).  ``perms[i]``: the 20 permutations of the
    support set of episode i (default: drawn episode by episode from the global numpy RNG); ``heads`` = (v0 [n, n_way, 512],
    g0 [n, n_way, 1]); default: one ``dist_head_init`` draw per episode from torch's global RNG, in episode order."""
    x0 = episodes[0][0]
    n_query = x0.size(1) - n_support
    e = _dist_engine(state_in, n_way, n_support, n_query, x0.size(-1), len(episodes[0]), episodes_per_batch)
    if heads is None:
        heads = dist_head_init(n_way, n=len(episodes))
    out = []
    for i in range(0, len(episodes), episodes_per_batch):
        chunk = episodes[i:i + episodes_per_batch]
        p = None if perms is None else perms[i:i + episodes_per_batch]
        hi = (heads[0][i:i + len(chunk)], heads[1][i:i + len(chunk)])
        out.append(e.run_batch(chunk, perms=p, classifier_init=hi).clone())
    return torch.cat(out)


def scores_batched(method, episodes, model, state_gnn, state_b, fine_tune_epoch, n_way=5, n_support=5, episodes_per_batch=32,
                   rngs=None, classifiers=None, parts=False):
    """What the reference's loop body computes for each episode of ``episodes`` (finetune.py:615-619,647-649), in lockstep:
    ``gnnnet`` / ``protonet`` -> finetune(); ``baseline`` -> finetune_linear(); ``baseline++`` -> finetune_dist() (its scores take the
    linear slot, ``classifiers`` = its heads (v0, g0)); ``all`` -> finetune_linear() + finetune().  The permutations of all episodes are
    drawn FIRST, episode by episode in the order the sequential calls would draw them (from the global numpy RNG, or from
    ``rngs[i]`` -- one generator per episode, the rank-count-invariant stream of parallel.episode_rng).
    ``parts``: return (linear scores | None, gnn scores | None) instead of the sum."""
    n = len(episodes)
    n_views = len(episodes[0])
    lin_p, gnn_p = [], []
    for i in range(n):
        lp, gp = draw_episode_perms(method, n_way, n_support, n_views, fine_tune_epoch, np.random if rngs is None else rngs[i])
        lin_p.append(lp)
        gnn_p.append(gp)
    s_lin = s_gnn = None
    if method in ("all", "baseline"):
        s_lin = finetune_linear_batched(episodes, state_b, n_way, n_support, episodes_per_batch, perms=lin_p, classifiers=classifiers)
    if method == "baseline++":
        s_lin = finetune_dist_batched(episodes, state_b, n_way, n_support, episodes_per_batch, perms=lin_p, heads=classifiers)
    if method in ("all",) + EPISODIC_METHODS:
        s_gnn = finetune_batched(episodes, model, state_gnn, fine_tune_epoch, n_way, n_support, episodes_per_batch, perms=gnn_p)
    if parts:
        return s_lin, s_gnn
    return s_gnn if s_lin is None else (s_lin if s_gnn is None else s_lin + s_gnn)


class LookaheadLoader:
    """Wrap the episode loader of the reference's loop (``for idx, elem in enumerate(novel_loader)``, finetune.py:599,634) so
    that the loop body stays as it is and the engine still sees E episodes at a time.

    ``elem`` is the reference's list of (x, y) view tuples.  The wrapper pulls up to ``episodes_per_batch`` elems from the
    underlying loader, runs them as one lockstep batch (``scores_batched``: permutations drawn in the sequential order) and
    parks the per-episode scores in a registry keyed by the identity of the episode's first view tensor; then it yields the
    elems one by one.  ``finetune(liz_x, ...)`` / ``finetune_linear(liz_x, ...)`` called by the loop body with that episode
    return the parked scores instead of running an engine of one -- bit-identical to ``finetune_batched`` because it IS the
    batched run (tests/test_drivers_gpu.py).

    ``freeze_backbone`` must be what the loop body passes (finetune.py:615-619,647-649 pass it on every call).  The frozen
    branches train no backbone, so there is nothing to batch: the wrapper then yields the elems untouched and the per-episode
    calls run their own frozen path (eval-mode features, finetune.py:253-266) -- and a parked result is only ever handed to a
    call with the same freeze_backbone / state_in / model (``_take_ready`` raises otherwise)."""

    def __init__(self, loader, method, model, state_gnn=None, state_b=None, fine_tune_epoch=None, n_way=5, n_support=5,
                 episodes_per_batch=32, classifiers=None, freeze_backbone=False):
        self.loader, self.method, self.model = loader, method, model
        self.freeze_backbone = bool(freeze_backbone)
        self.state_gnn, self.state_b = state_gnn, state_b
        self.epochs = fine_tune_epoch if fine_tune_epoch is not None else _params_of(params).fine_tune_epoch
        self.n_way, self.n_support, self.E = n_way, n_support, episodes_per_batch
        self.classifiers = classifiers

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        if self.freeze_backbone:
            yield from self.loader
            return
        it = iter(self.loader)
        done = False
        k = 0
        issued = []
        ctx = {"freeze_backbone": False, "state_gnn": self.state_gnn, "state_b": self.state_b, "model": self.model}
        while not done:
            for key in issued:                  # scores the loop body never asked for (a skipped episode) must not stay pinned
                _READY.pop(key, None)
            issued = []
            batch = []
            while len(batch) < self.E:
                try:
                    batch.append(next(it))
                except StopIteration:
                    done = True
                    break
            if not batch:
                break
            eps = [[x.cuda() for (x, _y) in elem] for elem in batch]
            cls = None if self.classifiers is None else (self.classifiers[0][k:k + len(batch)], self.classifiers[1][k:k + len(batch)])
            k += len(batch)
            s_lin, s_gnn = scores_batched(self.method, eps, self.model, self.state_gnn, self.state_b, self.epochs, self.n_way,
                                          self.n_support, self.E, classifiers=cls, parts=True)
            for j, elem in enumerate(batch):
                pin = elem[0][0]
                _READY[id(pin)] = {"pin": pin, "gnn": None if s_gnn is None else s_gnn[j],
                                   "dist" if self.method == "baseline++" else "linear": None if s_lin is None else s_lin[j], "ctx": ctx}
                issued.append(id(pin))
            for elem in batch:
                yield elem
        for key in issued:
            _READY.pop(key, None)


# ------------------------------------------------------------------------------------------------ the 600-episode driver

class SyntheticNovelLoader:
    """Stand-in for ``SetDataManager2(...).get_data_loader(num_aug=gen_examples)`` (datasets/EuroSAT_few_shot.py:329-351):
    yields ``elem`` = list of 2+gen_examples (x, y) tuples, views 0 and 1 identical.  ``indices``: the episode ids this rank owns."""

    def __init__(self, indices, n_way, n_shot, n_query, size, gen_examples, seed0=0):
        self.indices, self.a, self.seed0 = list(indices), (n_way, n_shot, n_query, size, gen_examples), seed0

    def __len__(self):
        return len(self.indices)

    def __iter__(self):
        n_way, n_shot, n_query, size, G = self.a
        y = torch.from_numpy(np.repeat(np.arange(n_way), n_shot + n_query).reshape(n_way, n_shot + n_query))
        for i in self.indices:
            views = synthetic.test_episode(self.seed0 + i, n_way, n_shot, n_query, size, G)
            yield [(v, y) for v in views]


FUSED_GAIN = 1.12      # steady-state rate of the fused next-step-forward inner loop over the unfused one (89.5 vs 79-80 episodes/s at E = 120 / 128)


def balanced_batch(n_mine, e_max, fused=False):
    """Episodes per lockstep batch for a rank that owns ``n_mine`` episodes: the engine always runs full batches (a short one is
    padded with copies of its last episode), so 600 episodes at 128 per batch would pay for 640.  Same number of batches, equal
    sizes: 600 -> 5 x 120.

    ``fused``: the engine's fused inner loop (engine.fuse_next_policy: whole waves of its walking kernel need E % 32 == 0) is
    available at this configuration.  Then the equal size is rounded up to the next multiple of 32 when the padded episodes cost
    less than the unfused path would (600 -> 5 x 128 = 640 slots at 1.12x the rate beats 600 unfused slots: the README-shaped
    600-episode job ran wholly unfused in round 5; 75 -> 96 does not pay and stays 75)."""
    if n_mine <= 0:
        return max(1, e_max)
    nb = (n_mine + e_max - 1) // e_max
    e = (n_mine + nb - 1) // nb
    if fused and e >= 32 and e % 32 != 0:
        e32 = (e + 31) // 32 * 32
        if e32 <= e_max and nb * e32 < FUSED_GAIN * nb * e:
            return e32
    return e


def short_job_candidates(n_batches):
    """Slab-placement candidates for an evaluation of ``n_batches`` lockstep batches on this rank (None = the engine's default,
    12).  The scan returns 1.4-2.2 % of a long job's time and costs 0.3-0.8 s of allocation + probing on a good lease -- and
    2.5-3.5 s on a lease whose allocations are slow (round 5, profiles/r05_j_fixed_job_marks.txt: the 5-batch 600-episode job
    7.75 / 7.82 / 8.00 s without it, 7.89 / 8.11 / 8.56 s with the 8-candidate scan round 4 used here, 11.7-12.3 s on a slow
    lease).  So only jobs of more than 8 batches (about 12 s of work) scan."""
    return 0 if n_batches <= 8 else None


def evaluate(model, state, n_episodes, n_way, n_shot, n_query, size, gen_examples, fine_tune_epoch, seed0=0,
             episodes_per_batch=32, verbose=True, method="gnnnet", state_b=None, freeze_backbone=False, rng_seed=None,
             device_episodes=False, balance=False, timings=None, note="", emulate_world=None, sampler=None):
    """The episode loop of finetune.py:599-682 on synthetic episodes; returns per-episode accuracies (all ranks' episodes, in
    episode order, on every rank).

    With torch.distributed initialised the episodes are sharded (episode i -> rank i mod W) and every episode draws its
    permutations from ``parallel.episode_rng(rng_seed, i)`` -- and its classifier initialisation from a torch generator
    seeded the same way -- so the result does not depend on the rank count; pass ``rng_seed`` to get that stream at W = 1 too.
    Without either the global numpy stream is used sequentially, exactly as the reference does.

    The loop is software-pipelined (nothing of it changes a result): the episodes of batch b+2 are generated on a side stream
    while batch b adapts; for ``--method gnnnet`` batch b+1's ingest + stem cache run beside batch b's inner loop and batch b's
    final pass + GNN head beside batch b+1's first steps (FinetuneEngine.run_batch(defer_final=, prefetch=)); accuracies are
    read from the device once, at the end.  ``balance``: equalise the batch sizes (``balanced_batch``).
    ``method="baseline++"`` (``state_b`` = the Baseline++ checkpoint, ``model`` unused): ``finetune_dist`` in lockstep, the heads
    drawn like ``classifier_init``'s; with ``freeze_backbone=True`` it is Baseline++'s own protocol -- eval-mode features and 100
    epochs of SGD on the head alone -- through ONE ``baselinepp_batched`` call per batch.
    ``sampler``: an augment.EpisodeSampler over a uint8 dataset resident in HBM -- episode i is then ``sampler.episode(seed0 + i)``
    (classes = randperm(n_classes)[:n_way], per class n_shot + n_query distinct random images, datasets/EuroSAT_few_shot.py:
    75-124,329-351) and its 2 + gen_examples views are generated on the device (mft_augment_views) straight into the engine's
    stores; without it the synthetic fp32 episodes of synthetic.test_episode(_device) are used.
    ``emulate_world`` = (r, W) (measurement aid, single process only): run exactly rank r's share of a W-rank job -- the same
    episodes, seeds, batch sizes and engine as that rank would -- and return ITS accuracies only (no gather)."""
    import time
    refuse_transductive(model, method, who="finetune.evaluate")
    t_start = time.perf_counter()
    rank, W = parallel.world()
    if emulate_world is not None:
        assert W == 1, "emulate_world is a single-process measurement aid"
        er, eW = emulate_world
        if rng_seed is None:
            rng_seed = 10
        mine = parallel.shard_indices(n_episodes, er, eW)
    else:
        if W > 1 and rng_seed is None:
            rng_seed = 10
        mine = parallel.shard_indices(n_episodes, rank, W)
    if balance:
        # (the fused inner loop exists for --method gnnnet / all at 84 x 84 with the stem cache: engine.fuse_next_policy)
        episodes_per_batch = balanced_batch(len(mine), episodes_per_batch,
                                            fused=(size <= 84 and not freeze_backbone and settings.current().fuse_next != "0"))
    y_query = np.repeat(range(n_way), n_query)
    batches = [mine[c:c + episodes_per_batch] for c in range(0, len(mine), episodes_per_batch)]
    dev = torch.device("cuda", torch.cuda.current_device())
    cur = torch.cuda.current_stream(dev)
    s_gen = torch.cuda.Stream(device=dev) if device_episodes else None
    gens = {}

    def ensure_gen(bi):
        """Episodes of batch ``bi`` -> gens[bi] = (list of liz_x on the device, 'ready' event, views-0/1-differ flag)."""
        if bi >= len(batches) or bi in gens:
            return
        ids = batches[bi]
        if sampler is not None:
            pipe = (method in EPISODIC_METHODS and not freeze_backbone and model is not None)
            eps = []
            for i in ids:
                src, P, _ = sampler.episode(seed0 + i, size, gen_examples)
                if pipe:
                    eps.append((src, P))                  # the engine generates the views itself (run_batch(sources=True))
                else:                                     # per-episode entry points take the list of NCHW views
                    from . import augment
                    v = augment.augment_views(src.view(-1, *src.shape[2:]), P, size)
                    eps.append([v[k].view(n_way, n_shot + n_query, size, size, 3).permute(0, 1, 4, 2, 3).contiguous()
                                for k in range(v.shape[0])])
            ev = torch.cuda.Event()
            ev.record()
            gens[bi] = (eps, ev, torch.zeros((), dtype=torch.bool, device=dev))      # (views 0 and 1 share their parameters)
            return
        if device_episodes:
            # the same synthetic distribution drawn with the device generator straight into HBM (a pure function of the seed as
            # well; not the numpy episodes): 600 19-view episodes are 96 GB of views -- minutes of host time, seconds on the GPU
            s_gen.wait_stream(cur)
            with torch.cuda.stream(s_gen):
                eps = [synthetic.test_episode_device(seed0 + i, dev, n_way, n_shot, n_query, size, gen_examples) for i in ids]
        else:
            # the numpy generator is the slow part (~1 s per 19-view episode): a batch's episodes on a few host threads (each
            # episode is a pure function of its seed)
            from concurrent.futures import ThreadPoolExecutor
            with ThreadPoolExecutor(max_workers=min(8, len(ids))) as ex:
                host = list(ex.map(lambda i: synthetic.test_episode(seed0 + i, n_way, n_shot, n_query, size, gen_examples), ids))
            eps = [[v.cuda() for v in ep] for ep in host]
            del host
        with torch.cuda.stream(s_gen if s_gen is not None else cur):
            bad = torch.stack([(ep[0] != ep[1]).any() for ep in eps]).any()      # finetune.py:606, checked without a sync per episode
            ev = torch.cuda.Event()
            ev.record()
        gens[bi] = (eps, ev, bad)

    pipelined = (method in EPISODIC_METHODS and not freeze_backbone and model is not None)
    n_views = 2 + gen_examples
    engine = None
    flags, score_chunks = [], []
    marks = [] if timings is not None else None

    def mark(name):
        if marks is not None:
            marks.append((name, round(time.perf_counter() - t_start, 3)))

    ensure_gen(0)
    ensure_gen(1)
    mark("first two batches of episodes enqueued")
    for bi, ids in enumerate(batches):
        eps, ev, bad = gens.pop(bi)
        cur.wait_event(ev)
        flags.append(bad)
        if bi + 1 in gens:
            cur.wait_event(gens[bi + 1][1])             # (generated during the previous batch; only batch 0 really waits)
        ensure_gen(bi + 2)                              # runs on the side stream beside this batch's inner loop
        rngs = cls = None
        if rng_seed is not None:
            rngs = [parallel.episode_rng(rng_seed, i) for i in ids]
            if method in ("all", "baseline", "baseline++"):
                ws, bs = [], []
                for i in ids:
                    with torch.random.fork_rng(devices=[]):
                        torch.manual_seed(parallel.episode_torch_seed(rng_seed, i))
                        w, b = dist_head_init(n_way) if method == "baseline++" else classifier_init(n_way)
                    ws.append(w[0]); bs.append(b[0])
                cls = (torch.stack(ws), torch.stack(bs))
        if freeze_backbone and method == "baseline++":
            S = n_way * n_shot
            perms = [[(np.random if rngs is None else rngs[k]).permutation(S) for _ in range(BASELINEPP_EPOCHS)] for k in range(len(eps))]
            sc = baselinepp_batched(eps, state_b, n_way, n_shot, episodes_per_batch, perms=perms, heads=cls)
            sc = sc.view(len(eps), n_way * n_query, n_way)
        elif freeze_backbone:
            sc = []
            for k, ep in enumerate(eps):
                st = np.random.get_state()
                if rngs is not None:                                  # the frozen branches draw from the global stream
                    np.random.set_state(rngs[k].get_state())
                sc.append(_score_one(method, ep, model, state, state_b, n_way, n_shot, fine_tune_epoch,
                                     None if cls is None else (cls[0][k], cls[1][k]), True))
                if rngs is not None:
                    np.random.set_state(st)
            sc = torch.stack(sc)
        elif pipelined:
            if engine is None:
                with eng.slab_candidates(short_job_candidates(len(batches))):        # a short job: the cheaper placement scan, or none
                    engine = _engine_for(state, model.cuda(), n_way, n_shot, n_query, size, n_views, fine_tune_epoch,
                                         episodes_per_batch, fold50=getattr(model, "FOLD50", False))
                mark("engine built (host)")
                if timings is not None:
                    torch.cuda.synchronize(dev)
                    timings["engine_ready_s"] = time.perf_counter() - t_start
                    mark("engine built + episodes generated (device)")
            perms = [draw_episode_perms(method, n_way, n_shot, n_views, fine_tune_epoch, np.random if rngs is None else rngs[k])[1]
                     for k, ep in enumerate(eps)]
            nxt = gens.get(bi + 1)
            sc = engine.run_batch(eps, perms=perms, defer_final=True, prefetch=None if nxt is None else nxt[0],
                                  sources=sampler is not None)
        else:
            with eng.slab_candidates(short_job_candidates(len(batches))):            # (engines are built on the first batch)
                sc = scores_batched(method, eps, model, state, state_b, fine_tune_epoch, n_way, n_shot, episodes_per_batch,
                                    rngs=rngs, classifiers=cls)
        score_chunks.append(sc)
        del eps
        mark("batch %d enqueued" % bi)
    torch.cuda.synchronize(dev)                          # deferred final passes included
    mark("device done")
    assert not bool(torch.stack(flags).any()) if flags else True                 # finetune.py:606
    accs = []
    for sc in score_chunks:
        pred = sc.argmax(2).cpu().numpy()
        for p in pred:
            accs.append(float(np.mean(p == y_query)) * 100)
    gdev = "cuda" if (torch.distributed.is_initialized() and torch.distributed.get_backend() == "nccl") else "cpu"
    accs = np.asarray(accs) if emulate_world is not None else parallel.gather_episode_values(accs, n_episodes, device=gdev)
    if timings is not None:
        timings["total_s"] = time.perf_counter() - t_start
        timings["episodes_per_batch"] = episodes_per_batch
        timings["batches"] = len(batches)
        timings["marks"] = marks
    if verbose and rank == 0:
        print('%d Test Acc = %4.2f%% +- %4.2f%%' % (len(accs), accs.mean(), 1.96 * accs.std() / np.sqrt(len(accs))) + note)
    return accs


def _score_one(method, liz_x, model, state, state_b, n_way, n_shot, fine_tune_epoch, classifier, freeze_backbone):
    """Loop body of finetune.py:615-619 / :647-649 for one episode (per-episode entry points)."""
    global params
    import argparse
    if params is None:
        params = argparse.Namespace(model='ResNet10', fine_tune_epoch=fine_tune_epoch)
    if method == "baseline":
        return finetune_linear(liz_x, None, state_b, None, linear=True, freeze_backbone=freeze_backbone, n_way=n_way,
                               n_support=n_shot, classifier=classifier)
    if method == "baseline++":
        return finetune_dist(liz_x, None, state_b, None, linear=True, freeze_backbone=freeze_backbone, n_way=n_way,
                             n_support=n_shot, head=classifier)
    if method == "all":
        return finetune_all(liz_x, None, model, state_b, state, n_way, n_shot, classifier=classifier, freeze_backbone=freeze_backbone)
    return finetune(liz_x, None, model, state, None, freeze_backbone=freeze_backbone, n_way=n_way, n_support=n_shot)


def _init_distributed():
    """Under torchrun (WORLD_SIZE > 1): one process per GPU, RCCL.  Must run before anything touches the GPU."""
    W = int(os.environ.get("WORLD_SIZE", "1"))
    forced = settings.current().force_collectives and "RANK" in os.environ      # one rank, real collectives (tests)
    if (W <= 1 and not forced) or torch.distributed.is_initialized():
        return
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    if settings.current().one_device:            # test hook: W ranks share device 0, gloo for the gather
        torch.cuda.set_device(0)
        torch.distributed.init_process_group("gloo")
    else:
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
        torch.distributed.init_process_group("nccl")


PRETRAINED_DATASET = "miniImageNet"          # finetune.py:431,448,468,488: hard-coded, NOT params.dataset


def checkpoint_files(p):
    """The checkpoint files the reference's ``__main__`` opens (finetune.py:448-527), as (gnnnet file | None, baseline file | None):

    * ``--method baseline`` / ``all``: <save_dir>/checkpoints/miniImageNet/<model>_baseline[_aug]/ -- ``400.tar`` when
      ``--save_iter`` is given (the literal 400 of :455,472), else the newest epoch for ``baseline`` (get_resume_file) or
      best_model.tar / newest for ``all`` (get_best_file);
    * ``--method all``: the GNN checkpoint is ALWAYS <model>_gnnnet_aug_<n>way_<k>shot/600.tar (:469,510-514: ``_aug`` and 600
      are literals there, whatever --train_aug / --save_iter say);
    * any other method: <model>_<method>[_aug]_<n>way_<k>shot/<save_iter>.tar, or best_model.tar / newest with --save_iter -1."""
    from . import configs
    from .io_utils import get_assigned_file, get_best_file, get_resume_file
    f_gnn = f_b = None
    if p.method in ("baseline", "all"):
        d = '%s/checkpoints/%s/%s_%s' % (configs.save_dir, PRETRAINED_DATASET, p.model, "baseline")
        if p.train_aug:
            d += '_aug'
        if p.save_iter != -1:
            f_b = get_assigned_file(d, 400)
        elif p.method in ('baseline', 'baseline++'):
            f_b = get_resume_file(d)
        else:
            f_b = get_best_file(d)
    if p.method == "all":
        d2 = '%s/checkpoints/%s/%s_%s' % (configs.save_dir, 'miniImageNet', p.model, "gnnnet") + '_aug'
        d2 += '_%dway_%dshot' % (p.train_n_way, p.n_shot)
        f_gnn = get_assigned_file(d2, 600)
    elif p.method != "baseline":
        d = '%s/checkpoints/%s/%s_%s' % (configs.save_dir, 'miniImageNet', p.model, p.method)
        if p.train_aug:
            d += '_aug'
        d += '_%dway_%dshot' % (p.train_n_way, p.n_shot)
        f_gnn = get_assigned_file(d, p.save_iter) if p.save_iter != -1 else get_best_file(d)
    return f_gnn, f_b


def baselinepp_checkpoint_file(p):
    """The checkpoint ``--method baseline++`` evaluates: <save_dir>/checkpoints/miniImageNet/<model>_baseline++[_aug]/<save_iter>.tar,
    or the newest epoch there (get_resume_file) with ``--save_iter -1`` -- the directory ``train.main --method baseline++``
    writes.  The reference's own lookup for this method (finetune.py:519-527, the last case of ``checkpoint_files``) appends
    ``_<n>way_<k>shot`` to the directory name, which its train.py never does for the two baselines (train.py:176-180): it can
    never find the checkpoint, so this is a separate function and ``checkpoint_files`` stays the reference's."""
    from . import configs
    from .io_utils import get_assigned_file, get_resume_file
    d = '%s/checkpoints/%s/%s_%s' % (configs.save_dir, PRETRAINED_DATASET, p.model, "baseline++")
    if p.train_aug:
        d += '_aug'
    return get_assigned_file(d, p.save_iter) if p.save_iter != -1 else get_resume_file(d)


def load_checkpoint_state(modelfile):
    """``torch.load(modelfile)['state']`` minus the ``feature2.`` / ``feature3.`` entries a --fine_tune run leaves behind
    (finetune.py:498-512,531-540; train.py:197-202).  Tensors stay on the host: the engine packs its own device copies."""
    tmp = torch.load(modelfile, map_location="cpu")
    state = tmp['state']
    for key in list(state.keys()):
        if "feature2." in key or "feature3." in key:
            state.pop(key)
    return state


def standin_state(kind, n_way):
    """No checkpoint on this box (the reference's logs.zip cannot be fetched offline): deterministic stand-ins.  ``gnn``: the
    seeded backbone + the GNN head that was meta-trained with the REFERENCE's set_forward_loss for accuracy golden G9
    (tests/golden/g9_head.npz) -- the printed accuracy is then a real one (~90 % on the synthetic episodes at the README
    settings), not the below-chance score of a random head.  ``baseline``: a seeded backbone (finetune_linear trains its own
    classifier); ``baseline++``: the same seeded backbone (finetune_dist trains its own head)."""
    if kind in ("baseline", "baseline++"):
        return synthetic.gnnnet_state_dict(seed=400, n_way=n_way)
    head = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "g9_head.npz")
    if n_way == 5 and os.path.isfile(head):
        sd = synthetic.gnnnet_state_dict(seed=31, n_way=n_way)
        hz = np.load(head)
        for k in hz.files:
            sd[k] = torch.from_numpy(hz[k])
        return sd
    return synthetic.gnnnet_state_dict(seed=0, n_way=n_way)


def standin_allowed():
    """Stand-in weights are an explicit opt-in (``MFT_STANDIN_WEIGHTS=1``): a mis-pointed ``configs.save_dir`` must not print a
    plausible accuracy (the reference's torch.load raises on a missing file, finetune.py:498)."""
    return settings.current().standin_weights


def _resolve_state(kind, modelfile, n_way, explicit, verbose):
    """Load ``modelfile`` if it exists.  A missing checkpoint is an ERROR, as it is in the reference (torch.load raises,
    finetune.py:498) -- whether the user named the epoch (``explicit``) or get_best_file / get_resume_file found nothing.  Only
    under ``MFT_STANDIN_WEIGHTS=1`` are the deterministic stand-in weights used instead; the caller then tags its stdout."""
    if modelfile is not None and os.path.isfile(modelfile):
        if verbose:
            print("loading %s checkpoint %s" % (kind, modelfile), file=sys.stderr)          # (stdout keeps the reference's lines only)
        return load_checkpoint_state(modelfile), modelfile
    if not standin_allowed():
        from . import configs
        raise FileNotFoundError("%s checkpoint %s not found (configs.save_dir = %r%s); set MFT_STANDIN_WEIGHTS=1 to evaluate the "
                                "synthetic stand-in weights instead" % (kind, "<none: empty checkpoint directory>" if modelfile is None
                                                                        else modelfile, configs.save_dir,
                                                                        ", epoch named on the command line" if explicit else ""))
    if verbose:
        print("no %s checkpoint%s: synthetic stand-in weights (MFT_STANDIN_WEIGHTS=1)" % (kind, "" if modelfile is None else " at " + modelfile),
              file=sys.stderr)
    return standin_state(kind, n_way), None


def main(argv=None, model_cls=None, n_episodes=600, episodes_per_batch=None):
    """finetune.py:424-682.  ``--method gnnnet`` (and gnnnet at ``--n_shot 50`` through gnnnet_copy, finetune_50.py),
    ``--method baseline`` (finetune_linear on the baseline checkpoint), ``--method all`` (their sum), ``--method baseline++``
    (finetune_dist on the Baseline++ checkpoint).  Checkpoints are looked up exactly where the reference looks
    (``checkpoint_files``; ``baselinepp_checkpoint_file`` for baseline++, whose reference lookup cannot succeed): what
    ``train.main --dataset miniImageNet`` wrote under ``configs.save_dir`` is what this evaluates."""
    global params
    np.random.seed(10)                                               # finetune.py:425
    params = parse_args('train', argv)
    refuse_feature_wise_model(params.model, "finetune.main")
    parallel.limit_host_threads()
    _init_distributed()
    rank, _W = parallel.world()
    from .methods.gnnnet import GnnNet
    from .methods import gnnnet_copy
    refuse_transductive(method=params.method, who="finetune.main")
    if params.method not in ('gnnnet', 'baseline', 'baseline++', 'all'):
        raise NotImplementedError("--method %s: 'gnnnet', 'baseline', 'baseline++' and 'all' are on the HIP hot path (protonet / "
                                  "relationnet / dampnet are out of scope, SURVEY.md §2.1)" % params.method)
    cfg = settings.current()
    size = cfg.image_size
    n_episodes = n_episodes if cfg.episodes is None else cfg.episodes
    if model_cls is None:
        model_cls = gnnnet_copy.GnnNet if params.n_shot == 50 else GnnNet
    if episodes_per_batch is None:
        episodes_per_batch = cfg.episodes_per_batch if cfg.episodes_per_batch is not None else {5: 128, 20: 96, 50: 64}.get(params.n_shot, 32)
    model = state = state_b = None
    f_gnn, f_b = (None, baselinepp_checkpoint_file(params)) if params.method == 'baseline++' else checkpoint_files(params)
    main.loaded = {"gnnnet": None, "baseline": None, "baseline++": None}       # what was actually read (tests, logs)
    if params.method in ('gnnnet', 'all'):
        model = model_cls(model_dict[params.model], n_way=params.test_n_way, n_support=params.n_shot).cuda()
        # `all` names 600.tar by literal, gnnnet names <save_iter>.tar: both explicit unless --save_iter is -1 for gnnnet
        state, main.loaded["gnnnet"] = _resolve_state("gnnnet", f_gnn, params.test_n_way,
                                                      params.method == 'all' or params.save_iter != -1, rank == 0)
        model.load_state_dict(state)                                 # finetune.py:512,540
    if params.method in ('baseline', 'all'):
        state_b, main.loaded["baseline"] = _resolve_state("baseline", f_b, params.test_n_way, params.save_iter != -1, rank == 0)
    if params.method == 'baseline++':
        state_b, main.loaded["baseline++"] = _resolve_state("baseline++", f_b, params.test_n_way, params.save_iter != -1, rank == 0)
    used = ["baseline++"] if params.method == 'baseline++' else [k for k in ("gnnnet", "baseline") if params.method in (k, "all")]
    print(params.freeze_backbone)                                    # finetune.py:591
    tm = {} if cfg.timings else None
    if tm is not None:
        import time
        t_main = time.time()
        try:
            import psutil
            print("[timings] process start -> evaluate: %.2f s" % (t_main - psutil.Process().create_time()), file=sys.stderr)
        except Exception:
            pass
    sampler = None
    if params.test_dataset:
        # finetune.py:558-579: --test_dataset picks the novel-class loader.  Here: a dataset-SHAPED synthetic pool resident in HBM
        # (synthetic.class_pool_u8; e.g. EuroSAT: 10 classes x 2700 images x 64x64 uint8) sampled per episode on the device
        from . import augment
        if params.test_dataset not in synthetic.DATASET_SHAPES or params.test_dataset == "miniImageNet":
            raise ValueError('Unknown test dataset %r (the reference knows ISIC, EuroSAT, CropDisease, ChestX)' % params.test_dataset)
        if rank == 0:
            # (the reference prints "Loading <dataset>" and reads an ImageFolder, finetune.py:559-577; there is no ImageFolder path
            # here -- the pool below is SYNTHETIC and only dataset-SHAPED, and both printed lines say so: ADVICE r05)
            print("Loading %s   [SYNTHETIC %s-shaped pool resident in HBM: no image files are read]" % (params.test_dataset, params.test_dataset))
        pool = synthetic.class_pool_u8(params.test_dataset, torch.device("cuda", torch.cuda.current_device()), seed=1,
                                       n_per_class=cfg.pool_per_class)
        sampler = augment.EpisodeSampler(pool, params.test_n_way, params.n_shot + 15, seed=10)
    accs = evaluate(model, state, n_episodes, params.test_n_way, params.n_shot, 15, size, params.gen_examples,
                    params.fine_tune_epoch, method=params.method, state_b=state_b, freeze_backbone=params.freeze_backbone,
                    sampler=sampler,
                    episodes_per_batch=episodes_per_batch, device_episodes=not cfg.synth_on_host,
                    balance=cfg.balance_batches, timings=tm,
                    note=("" if all(main.loaded[k] is not None for k in used) else "   [SYNTHETIC stand-in weights, MFT_STANDIN_WEIGHTS=1]") +
                         ("   [SYNTHETIC %s-shaped pool]" % params.test_dataset if params.test_dataset else ""))
    if tm is not None:
        print("[timings] evaluate: %s" % tm, file=sys.stderr)
    if torch.distributed.is_initialized():
        torch.distributed.barrier()
    return accs


if __name__ == '__main__':
    main()
