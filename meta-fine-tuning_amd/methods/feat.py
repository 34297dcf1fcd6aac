"""FEAT: few-shot learning via embedding adaptation with a set-to-set function (Ye et al., CVPR 2020) on the reference's
MetaTemplate, on pooled ResNet10 features (definition in DESIGN.md section 19).  The class prototypes of an episode are one set of
n_way tokens; one single-head self-attention block A (d_k = d_v = 512, residual, LayerNorm) adapts them to each other and the scores
are minus the squared distances of the queries to the adapted prototypes over TEMPERATURE.  In train mode every class's support and
query rows are a set too: the distances of every row to the centres of the adapted sets, over TEMPERATURE2, give the auxiliary
cross-entropy term that BALANCE weighs, and the attention / output dropouts (P_ATT, P_OUT) are on.

``slf_attn`` holds the seven tensors and nothing else; they follow the ``feature.*`` keys in the state dict.  The five constants are
class attributes.  The head runs on csrc/feat.hip through autograd_ops.feat_head (hand-written backward), the two-term loss through
autograd_ops.feat_loss.  The dropout multipliers come from the library's Philox generator at a device-resident draw index
(``feat_draw_index``, not in the state dict), so a replayed hipGraph draws fresh masks.  The first-order-MAML ``--fine_tune`` path
is not on the HIP path and raises, and the test-time engine has no FEAT mode (finetune.py refuses the method).
"""
import math

import torch
import torch.nn as nn

from .. import autograd_ops as AG
from .. import ops
from .meta_template import HeadMethod

MAX_N_WAY = ops.FEAT_MAX_WAY        # the launchers' domain: n_way 1..32, T = n_support + n_query <= 128, D = 512
MAX_T = ops.FEAT_MAX_T


class SetAttention(nn.Module):
    """Holder of the set-to-set function's seven tensors, drawn in state-dict order; the arithmetic is in csrc/feat.hip."""

    def __init__(self, dim):
        super().__init__()
        skip = nn.utils.skip_init
        self.w_qs = skip(nn.Linear, dim, dim, bias=False)
        self.w_ks = skip(nn.Linear, dim, dim, bias=False)
        self.w_vs = skip(nn.Linear, dim, dim, bias=False)
        for m in (self.w_qs, self.w_ks, self.w_vs):
            nn.init.normal_(m.weight, mean=0.0, std=math.sqrt(2.0 / (dim + dim)))
        self.layer_norm = nn.LayerNorm(dim)                          # ones and zeros, eps 1e-5: no draw
        self.fc = skip(nn.Linear, dim, dim)
        nn.init.xavier_normal_(self.fc.weight)
        nn.init.uniform_(self.fc.bias, -1.0 / math.sqrt(dim), 1.0 / math.sqrt(dim))      # nn.Linear's bias draw

    def forward(self, *args, **kwargs):
        raise NotImplementedError("SetAttention holds parameters; FEAT._head runs the set-to-set function on csrc/feat.hip")


class FEAT(HeadMethod):
    METHOD, ENGINE_MODE = "feat", None
    TEMPERATURE = ops.FEAT_TEMPERATURE
    TEMPERATURE2 = ops.FEAT_TEMPERATURE2
    BALANCE = ops.FEAT_BALANCE
    P_ATT = ops.FEAT_P_ATT
    P_OUT = ops.FEAT_P_OUT

    def __init__(self, model_func, n_way, n_support):
        ops.feat_check(1, n_way, n_support, 1)
        super().__init__(model_func, n_way, n_support)
        if self.feat_dim != ops.FEAT_D:
            raise ValueError("FEAT head: feat_dim = %d is not supported (D = %d)" % (self.feat_dim, ops.FEAT_D))
        self.loss_fn = AG.CrossEntropyLoss()                         # keeper of the running sum of the main term (loss_sum)
        self.slf_attn = SetAttention(self.feat_dim)
        self.feat_seed = 0
        self.register_buffer("feat_draw_index", torch.zeros(1, dtype=torch.int64), persistent=False)
        self._reg = None
        self.last_terms = None                                       # (main, auxiliary) term of the last loss, 0-dim device tensors

    def _check(self, n_query):
        ops.feat_check(1, self.n_way, self.n_support, n_query)

    def head_params(self):
        a = self.slf_attn
        return [a.w_qs.weight, a.w_ks.weight, a.w_vs.weight, a.layer_norm.weight, a.layer_norm.bias, a.fc.weight, a.fc.bias]

    def _seed(self):
        from .. import parallel
        return (int(self.feat_seed) + 0x9E3779B97F4A7C15 * parallel.world()[0]) & 0xFFFFFFFFFFFFFFFF

    def _head(self, feats, n_query, episodes=1):
        kw = dict(episodes=episodes, temperature=self.TEMPERATURE, temperature2=self.TEMPERATURE2)
        if not (self.training and torch.is_grad_enabled()):
            self._reg = None
            return AG.feat_head(feats, self.head_params(), self.n_way, self.n_support, n_query, **kw)
        masks = ops.feat_draw(episodes, self.n_way, self.n_support, n_query, self._seed(), self.feat_draw_index, self.P_ATT, self.P_OUT,
                              masks_in=AG.feat_forced())
        scores, self._reg = AG.feat_head(feats, self.head_params(), self.n_way, self.n_support, n_query, train=True, masks=masks, **kw)
        return scores

    def head_state(self):
        return None

    def _loss(self, scores, n_query, episodes):
        reg, self._reg = self._reg, None
        loss, main, aux = AG.feat_loss(scores, reg, episodes, self.n_way, self.n_support, n_query, self.BALANCE,
                                       loss_sum=self.loss_fn.loss_sum(scores.device))
        self.last_terms = (main, aux)
        return loss

    def set_forward_loss(self, x):
        """CE(scores, y_query) + BALANCE * CE(reg, y_all) in train mode, the main term alone otherwise."""
        return self._loss(self.set_forward(x), x.size(1) - self.n_support, 1)

    def set_forward_loss_lockstep(self, xs):
        return self._loss(self.set_forward_lockstep(xs), xs.size(2) - self.n_support, xs.size(0))

    def _loss_item(self, loss):
        """The episode loops print the running mean of the main term."""
        return self.last_terms[0].item()
