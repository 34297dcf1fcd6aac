"""MetaOptNet with the ridge-regression head (MetaOptNet-RR of Lee et al., CVPR 2019, on the reference's MetaTemplate; definition
in DESIGN.md section 14): ResNet10 features -> A = Z_S Z_S^T + lambda_reg I -> alpha = 2 A^-1 Y -> W = Z_S^T alpha ->
scores = scale * Z_Q W, cross-entropy loss.

``scale`` (nn.Parameter(torch.ones(1))) is the head's one learnable parameter and the last state-dict key; ``lambda_reg`` is a
constant attribute.  The head runs on csrc/ridge.hip through autograd_ops.metaoptnet_head (hand-written backward), the loss
through autograd_ops.CrossEntropyLoss.  The first-order-MAML ``--fine_tune`` path is not on the HIP path and raises.

``head="svm"`` (MetaOptNet-SVM, the method's published head) puts W = Z_S^T alpha of the Crammer-Singer dual
(csrc/svm.hip, autograd_ops.metaoptnet_svm_head) in the place of the ridge regression; parameters and state-dict keys are the same.
"""
import torch
import torch.nn as nn

from .. import autograd_ops as AG
from .. import ops
from ..io_utils import HEADS
from .meta_template import HeadMethod

MAX_N_WAY = ops.RIDGE_MAX_WAY       # the launchers' domain: n_way 1..32, S = n_way * n_support <= 256, D = 512
MAX_S = ops.RIDGE_MAX_S


class MetaOptNet(HeadMethod):
    METHOD, ENGINE_MODE = "metaoptnet", "ridge"
    lambda_reg = ops.RIDGE_LAMBDA

    def __init__(self, model_func, n_way, n_support, head="ridge"):
        if head not in HEADS:
            raise ValueError("MetaOptNet: head = %r (%s)" % (head, " or ".join(repr(h) for h in HEADS)))
        ops.ridge_check(1, n_way, n_support, 1)
        super().__init__(model_func, n_way, n_support)
        self.head = head
        if head != "ridge":
            self.ENGINE_MODE = head                                  # on the instance: the class keeps ("metaoptnet", "ridge")
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

    def _check(self, n_query):
        ops.ridge_check(1, self.n_way, self.n_support, n_query)

    def _head(self, feats, n_query, episodes=1):
        fn = AG.metaoptnet_svm_head if self.head == "svm" else AG.metaoptnet_head
        return fn(feats, self.scale, self.n_way, self.n_support, n_query, episodes=episodes)

    def head_params(self):
        return [self.scale]

    def head_state(self):
        return {"scale": self.scale.detach(), "head": self.head}
