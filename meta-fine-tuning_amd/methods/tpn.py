"""TPN: the Transductive Propagation Network of Liu et al. (ICLR 2019) on the reference's MetaTemplate, on pooled ResNet10 features
(definition in DESIGN.md section 18): sigma = fc4(relu(fc3 z)), u = z / (sigma + EPS), W = exp(-|u_i - u_j|^2 / 2) on the K nearest
neighbours of every node (support and query nodes of the episode together), S = D^-1/2 W D^-1/2, F = (I - ALPHA S)^-1 Y; the scores
are the query rows of F, the loss is cross entropy on them.

``relation`` holds the two nn.Linear and nothing else; its four tensors follow the ``feature.*`` keys in the state dict.  ``K`` and
``ALPHA`` are constant attributes.  The head runs on csrc/tpn.hip through autograd_ops.tpn_head (hand-written backward), the loss
through autograd_ops.CrossEntropyLoss.  The first-order-MAML ``--fine_tune`` path is not on the HIP path and raises, and the
test-time engine has no transductive mode (finetune.py refuses the method).
"""
import torch
import torch.nn as nn

from .. import autograd_ops as AG
from .. import ops
from .meta_template import HeadMethod

MAX_N_WAY = ops.TPN_MAX_WAY         # the launchers' domain: n_way 1..32, N = n_way * (n_support + n_query) <= 256, D = 512
MAX_N = ops.TPN_MAX_N
FC4_BIAS = 12.0                     # the constructor's relation.fc4.bias (with torch's draw every affinity is 0)


class RelationGraph(nn.Module):
    """Holder of the two layers that give every node its length scale; the arithmetic is in csrc/tpn.hip."""

    def __init__(self, dim):
        super().__init__()
        self.fc3 = nn.Linear(dim, 8)
        self.fc4 = nn.Linear(8, 1)


class TPN(HeadMethod):
    METHOD, ENGINE_MODE = "tpn", None
    K = ops.TPN_K
    ALPHA = ops.TPN_ALPHA

    def __init__(self, model_func, n_way, n_support):
        ops.tpn_check(1, n_way, n_support, 1)
        super().__init__(model_func, n_way, n_support)
        if self.feat_dim != ops.TPN_D:
            raise ValueError("TPN head: feat_dim = %d is not supported (D = %d)" % (self.feat_dim, ops.TPN_D))
        self.loss_fn = AG.CrossEntropyLoss()                         # nn.CrossEntropyLoss() on mft_cross_entropy_mean
        self.relation = RelationGraph(self.feat_dim)                 # torch's default draws (the RNG stream of two nn.Linear) ...
        with torch.no_grad():
            self.relation.fc4.bias.fill_(FC4_BIAS)                   # ... then the one deliberate deviation

    def _check(self, n_query):
        ops.tpn_check(1, self.n_way, self.n_support, n_query)

    def head_params(self):
        r = self.relation
        return [r.fc3.weight, r.fc3.bias, r.fc4.weight, r.fc4.bias]

    def _head(self, feats, n_query, episodes=1):
        return AG.tpn_head(feats, *self.head_params(), self.n_way, self.n_support, n_query, episodes=episodes)

    def head_state(self):
        return {k: p.detach() for k, p in zip(("fc3_w", "fc3_b", "fc4_w", "fc4_b"), self.head_params())}
