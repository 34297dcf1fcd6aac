"""ProtoNet: ResNet10 features -> class prototypes (mean of the support features) -> scores = minus the squared euclidean
distance of every query to every prototype (mirror of methods/protonet.py), with the reference's constructor, attributes and
state_dict keys (``feature.*`` only).

The head is one HIP launch each way for all episodes of a step (autograd_ops.protonet_head: mft_proto_scores /
mft_proto_backward), the loss is autograd_ops.CrossEntropyLoss.  The reference's first-order-MAML ``--fine_tune`` path
(set_forward_finetune / MAML_update) is not on the HIP path and raises.
"""
import numpy as np
import torch

from .. import autograd_ops as AG
from .meta_template import MetaTemplate

MAX_N_WAY = 64          # mft_proto_scores / mft_proto_backward: n_way 1..64, D <= 512


class ProtoNet(MetaTemplate):
    def __init__(self, model_func, n_way, n_support):
        if not 1 <= int(n_way) <= MAX_N_WAY:
            raise ValueError("ProtoNet head: n_way = %d is not supported (1 <= n_way <= %d)" % (int(n_way), MAX_N_WAY))
        super().__init__(model_func, n_way, n_support)
        self.loss_fn = AG.CrossEntropyLoss()                         # nn.CrossEntropyLoss() on mft_cross_entropy_mean
        self.first = True

    # ------------------------------------------------------------------ forward
    def set_forward(self, x, is_feature=False):
        """x [n_way, n_support+n_query, 3,H,W] (or features [n_way, n_support+n_query, D]) -> scores [n_way*n_query, n_way],
        row = class*n_query + q.  With ``freeze_backbone`` the backbone parameters stop requiring gradients (parse_feature)."""
        x = x.cuda()
        n_query = x.size(1) - self.n_support
        if is_feature:
            feats = x.reshape(-1, x.size(-1))
        else:
            if self.freeze_backbone:
                for p in self.feature.parameters():
                    p.requires_grad = False
            feats = self.feature(x.reshape(-1, *x.size()[2:]))
        return AG.protonet_head(feats, self.n_way, self.n_support, n_query)

    def set_forward_loss(self, x):
        return self.loss_fn(self.set_forward(x), self._labels(1))

    # ------------------------------------------------------------------ k episodes in lockstep (opt-in, train.py --episodes_per_rank k)
    def set_forward_lockstep(self, xs):
        """xs [k, n_way, n_support+n_query, 3,H,W]: k episodes through one sequence of launches (per-episode BatchNorm statistics
        in the backbone, one head launch for all k).  Scores [k*n_way*n_query, n_way], episode after episode."""
        xs = xs.cuda()
        k = xs.size(0)
        feats = AG.resnet10_module_forward(self.feature, xs.reshape(-1, *xs.size()[3:]), groups=k)
        return AG.protonet_head(feats, self.n_way, self.n_support, xs.size(2) - self.n_support, episodes=k)

    def set_forward_loss_lockstep(self, xs):
        """Mean over the k episodes of ``set_forward_loss``: its backward leaves the average of the k episodes' gradients."""
        return self.loss_fn(self.set_forward_lockstep(xs), self._labels(xs.size(0)))

    def _labels(self, k):
        """np.tile(np.repeat(range(n_way), n_query), k) on the device, uploaded once per shape: a per-step upload is a
        synchronous copy, which a hipGraph capture of the step refuses."""
        key = (self.n_way, self.n_query, k, torch.cuda.current_device())
        cache = self.__dict__.setdefault("_yq_cache", {})
        y = cache.get(key)
        if y is None:
            y = cache[key] = torch.from_numpy(np.tile(np.repeat(range(self.n_way), self.n_query), k)).cuda()
        return y

    # ------------------------------------------------------------------ first-order MAML (not on the HIP path)
    def MAML_update(self):
        raise NotImplementedError("ProtoNet.MAML_update: the --fine_tune (first-order MAML) meta-training of protonet is not on "
                                  "the HIP path; meta-train with train.py --method protonet without --fine_tune")

    def set_forward_finetune(self, x):
        raise NotImplementedError("ProtoNet.set_forward_finetune: the --fine_tune (first-order MAML) meta-training of protonet is "
                                  "not on the HIP path; meta-train with train.py --method protonet without --fine_tune")

    def set_forward_loss_finetune(self, x):
        return self.set_forward_finetune(x)
