"""MetaOptNet with the ridge-regression head (MetaOptNet-RR of Lee et al., CVPR 2019, on the reference's MetaTemplate; definition
in DESIGN.md section 14): ResNet10 features -> A = Z_S Z_S^T + lambda_reg I -> alpha = 2 A^-1 Y -> W = Z_S^T alpha ->
scores = scale * Z_Q W, cross-entropy loss.

``scale`` (nn.Parameter(torch.ones(1))) is the head's one learnable parameter and the last state-dict key; ``lambda_reg`` is a
constant attribute.  The head runs on csrc/ridge.hip through autograd_ops.metaoptnet_head (hand-written backward), the loss
through autograd_ops.CrossEntropyLoss.  The first-order-MAML ``--fine_tune`` path is not on the HIP path and raises.
"""
import numpy as np
import torch
import torch.nn as nn

from .. import autograd_ops as AG
from .. import ops
from .meta_template import MetaTemplate

MAX_N_WAY = ops.RIDGE_MAX_WAY       # the launchers' domain: n_way 1..32, S = n_way * n_support <= 256, D = 512
MAX_S = ops.RIDGE_MAX_S


class MetaOptNet(MetaTemplate):
    lambda_reg = ops.RIDGE_LAMBDA

    def __init__(self, model_func, n_way, n_support):
        ops.ridge_check(1, n_way, n_support, 1)
        super().__init__(model_func, n_way, n_support)
        if self.feat_dim != ops.RIDGE_D:
            raise ValueError("MetaOptNet head: feat_dim = %d is not supported (D = %d)" % (self.feat_dim, ops.RIDGE_D))
        self.loss_fn = AG.CrossEntropyLoss()                         # nn.CrossEntropyLoss() on mft_cross_entropy_mean
        self.scale = nn.Parameter(torch.ones(1))

    def state_dict(self, *args, **kwargs):
        """``scale`` after the ``feature.*`` keys (a module's own parameters otherwise precede its children's): the checkpoint
        layout of DESIGN.md section 14."""
        sd = super().state_dict(*args, **kwargs)
        key = kwargs.get("prefix", args[1] if len(args) > 1 else "") + "scale"
        if key in sd:
            sd.move_to_end(key)
        return sd

    # ------------------------------------------------------------------ forward
    def _head(self, feats, n_query, episodes=1):
        return AG.metaoptnet_head(feats, self.scale, self.n_way, self.n_support, n_query, episodes=episodes)

    def set_forward(self, x, is_feature=False):
        """x [n_way, n_support+n_query, 3,H,W] (or features [n_way, n_support+n_query, D]) -> scores [n_way*n_query, n_way],
        row = class*n_query + q.  With ``freeze_backbone`` the backbone parameters stop requiring gradients (parse_feature)."""
        x = x.cuda()
        n_query = x.size(1) - self.n_support
        ops.ridge_check(1, self.n_way, self.n_support, n_query)
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
        in the backbone, every head launch for all k).  Scores [k*n_way*n_query, n_way], episode after episode."""
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
        raise NotImplementedError("MetaOptNet.MAML_update: the --fine_tune (first-order MAML) meta-training of metaoptnet is not "
                                  "on the HIP path; meta-train with train.py --method metaoptnet without --fine_tune")

    def set_forward_finetune(self, x):
        raise NotImplementedError("MetaOptNet.set_forward_finetune: the --fine_tune (first-order MAML) meta-training of metaoptnet "
                                  "is not on the HIP path; meta-train with train.py --method metaoptnet without --fine_tune")

    def set_forward_loss_finetune(self, x):
        return self.set_forward_finetune(x)
