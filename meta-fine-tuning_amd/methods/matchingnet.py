"""MatchingNet with full context embeddings (the MatchingNet of "A Closer Look at Few-shot Classification"; definition in
DESIGN.md section 13): ResNet10 features -> bidirectional LSTM over the support set (G_encoder) -> attention LSTM over the
queries (FCE) -> softmax over 100 * relu(cosine) to every support row -> class sums -> log-probabilities, NLL loss.

``FCE.lstmcell`` (nn.LSTMCell(2D, D)) and ``G_encoder`` (nn.LSTM(D, D, 1, batch_first=True, bidirectional=True)) are parameter
containers with torch's names, shapes and gate order (i, f, g, o); their own ``forward`` is never called.  The head runs on
csrc/matchingnet.hip through autograd_ops.matchingnet_head (hand-written backward), the loss through autograd_ops.NLLLoss.
"""
import numpy as np
import torch
import torch.nn as nn

from .. import autograd_ops as AG
from .. import ops
from .meta_template import MetaTemplate

MAX_N_WAY = ops.MN_MAX_WAY          # the launchers' domain: n_way 1..32, S = n_way * n_support <= 256, D = 512
MAX_S = ops.MN_MAX_S


class FullyContextualEmbedding(nn.Module):
    """Holder of the FCE's LSTMCell(2D, D); the recurrence itself is ops.matching_forward."""

    def __init__(self, feat_dim):
        super().__init__()
        self.lstmcell = nn.LSTMCell(feat_dim * 2, feat_dim)

    def forward(self, f, G):
        raise NotImplementedError("FullyContextualEmbedding is a parameter container: the FCE runs inside MatchingNet.set_forward "
                                  "(autograd_ops.matchingnet_head)")


class MatchingNet(MetaTemplate):
    def __init__(self, model_func, n_way, n_support):
        ops.mn_check(1, n_way, n_support, 1)
        super().__init__(model_func, n_way, n_support)
        if self.feat_dim != ops.MN_D:
            raise ValueError("MatchingNet head: feat_dim = %d is not supported (D = %d)" % (self.feat_dim, ops.MN_D))
        self.loss_fn = AG.NLLLoss()                                  # nn.NLLLoss() on mft_nll_mean
        self.FCE = FullyContextualEmbedding(self.feat_dim)
        self.G_encoder = nn.LSTM(self.feat_dim, self.feat_dim, 1, batch_first=True, bidirectional=True)

    # ------------------------------------------------------------------ forward
    def _head(self, feats, n_query, episodes=1):
        ops.mn_check(episodes, self.n_way, self.n_support, n_query, feats.size(-1))
        return AG.matchingnet_head(self, feats, self.n_support, n_query, episodes=episodes)

    def set_forward(self, x, is_feature=False):
        """x [n_way, n_support+n_query, 3,H,W] (or features [n_way, n_support+n_query, D]) -> log-probabilities
        [n_way*n_query, n_way], row = class*n_query + q.  With ``freeze_backbone`` the backbone parameters stop requiring
        gradients (parse_feature)."""
        x = x.cuda()
        n_query = x.size(1) - self.n_support
        ops.mn_check(1, self.n_way, self.n_support, n_query)
        if is_feature:
            feats = x.reshape(-1, x.size(-1))
        else:
            if self.freeze_backbone:
                for p in self.feature.parameters():
                    p.requires_grad = False
            feats = self.feature(x.reshape(-1, *x.size()[2:]))
        return self._head(feats, n_query)

    def set_forward_loss(self, x):
        return self.loss_fn(self.set_forward(x), self._labels(1))

    # ------------------------------------------------------------------ k episodes in lockstep (opt-in, train.py --episodes_per_rank k)
    def set_forward_lockstep(self, xs):
        """xs [k, n_way, n_support+n_query, 3,H,W]: k episodes through one sequence of launches (per-episode BatchNorm statistics
        in the backbone, every head launch for all k).  Log-probabilities [k*n_way*n_query, n_way], episode after episode."""
        xs = xs.cuda()
        k = xs.size(0)
        feats = AG.resnet10_module_forward(self.feature, xs.reshape(-1, *xs.size()[3:]), groups=k)
        return self._head(feats, xs.size(2) - self.n_support, episodes=k)

    def set_forward_loss_lockstep(self, xs):
        """Mean over the k episodes of ``set_forward_loss``: its backward leaves the average of the k episodes' gradients."""
        return self.loss_fn(self.set_forward_lockstep(xs), self._labels(xs.size(0)))

    def _labels(self, k):
        """np.tile(np.repeat(range(n_way), n_query), k) on the device, uploaded once per shape (a per-step upload is a synchronous
        copy, which a hipGraph capture of the step refuses)."""
        key = (self.n_way, self.n_query, k, torch.cuda.current_device())
        cache = self.__dict__.setdefault("_yq_cache", {})
        y = cache.get(key)
        if y is None:
            y = cache[key] = torch.from_numpy(np.tile(np.repeat(range(self.n_way), self.n_query), k)).cuda()
        return y

    # ------------------------------------------------------------------ first-order MAML (not on the HIP path)
    def MAML_update(self):
        raise NotImplementedError("MatchingNet.MAML_update: the --fine_tune (first-order MAML) meta-training of matchingnet is not "
                                  "on the HIP path; meta-train with train.py --method matchingnet without --fine_tune")

    def set_forward_finetune(self, x):
        raise NotImplementedError("MatchingNet.set_forward_finetune: the --fine_tune (first-order MAML) meta-training of matchingnet "
                                  "is not on the HIP path; meta-train with train.py --method matchingnet without --fine_tune")

    def set_forward_loss_finetune(self, x):
        return self.set_forward_finetune(x)
