"""ProtoNet: ResNet10 features -> class prototypes (mean of the support features) -> scores = minus the squared euclidean
distance of every query to every prototype (mirror of methods/protonet.py), with the reference's constructor, attributes and
state_dict keys (``feature.*`` only).

The head is one HIP launch each way for all episodes of a step (autograd_ops.protonet_head: mft_proto_scores /
mft_proto_backward), the loss is autograd_ops.CrossEntropyLoss.  The reference's first-order-MAML ``--fine_tune`` path
(set_forward_finetune / MAML_update) is not on the HIP path and raises.
"""
from .. import autograd_ops as AG
from .meta_template import HeadMethod

MAX_N_WAY = 64          # mft_proto_scores / mft_proto_backward: n_way 1..64, D <= 512


class ProtoNet(HeadMethod):
    METHOD, ENGINE_MODE = "protonet", "proto"

    def __init__(self, model_func, n_way, n_support):
        if not 1 <= int(n_way) <= MAX_N_WAY:
            raise ValueError("ProtoNet head: n_way = %d is not supported (1 <= n_way <= %d)" % (int(n_way), MAX_N_WAY))
        super().__init__(model_func, n_way, n_support)
        self.loss_fn = AG.CrossEntropyLoss()                         # nn.CrossEntropyLoss() on mft_cross_entropy_mean
        self.first = True

    def _head(self, feats, n_query, episodes=1):
        return AG.protonet_head(feats, self.n_way, self.n_support, n_query, episodes=episodes)
