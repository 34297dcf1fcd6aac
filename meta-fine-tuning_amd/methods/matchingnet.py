"""MatchingNet with full context embeddings (the MatchingNet of "A Closer Look at Few-shot Classification"; definition in
DESIGN.md section 13): ResNet10 features -> bidirectional LSTM over the support set (G_encoder) -> attention LSTM over the
queries (FCE) -> softmax over 100 * relu(cosine) to every support row -> class sums -> log-probabilities, NLL loss.

``FCE.lstmcell`` (nn.LSTMCell(2D, D)) and ``G_encoder`` (nn.LSTM(D, D, 1, batch_first=True, bidirectional=True)) are parameter
containers with torch's names, shapes and gate order (i, f, g, o); their own ``forward`` is never called.  The head runs on
csrc/matchingnet.hip through autograd_ops.matchingnet_head (hand-written backward), the loss through autograd_ops.NLLLoss.
"""
import torch.nn as nn

from .. import autograd_ops as AG
from .. import ops
from .meta_template import HeadMethod

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


class MatchingNet(HeadMethod):
    METHOD, ENGINE_MODE = "matchingnet", "matching"

    def __init__(self, model_func, n_way, n_support):
        ops.mn_check(1, n_way, n_support, 1)
        super().__init__(model_func, n_way, n_support)
        if self.feat_dim != ops.MN_D:
            raise ValueError("MatchingNet head: feat_dim = %d is not supported (D = %d)" % (self.feat_dim, ops.MN_D))
        self.loss_fn = AG.NLLLoss()                                  # nn.NLLLoss() on mft_nll_mean
        self.FCE = FullyContextualEmbedding(self.feat_dim)
        self.G_encoder = nn.LSTM(self.feat_dim, self.feat_dim, 1, batch_first=True, bidirectional=True)

    def _check(self, n_query):
        ops.mn_check(1, self.n_way, self.n_support, n_query)

    def _head(self, feats, n_query, episodes=1):
        ops.mn_check(episodes, self.n_way, self.n_support, n_query, feats.size(-1))
        return AG.matchingnet_head(self, feats, self.n_support, n_query, episodes=episodes)

    def head_params(self):
        return AG.matchingnet_params(self)

    def head_state(self):
        return {k: p.detach() for k, p in zip(ops.MN_KEYS, self.head_params())}
