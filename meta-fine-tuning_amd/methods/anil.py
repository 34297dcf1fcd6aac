"""ANIL: "Almost No Inner Loop" (Raghu et al., "Rapid Learning or Feature Reuse? Towards Understanding the Effectiveness of MAML",
ICLR 2020) on the reference's MetaTemplate, on pooled ResNet10 features (definition in DESIGN.md section 21): the member of the
gradient-based meta-learning family whose inner loop adapts only a linear classifier.  Per episode the classifier starts from the
trained initialisation (W0, b0) and takes INNER_STEPS gradient steps of size INNER_LR on the mean cross entropy of the support rows;
the scores are the adapted classifier's on the query rows, the loss is cross entropy on them, and the outer gradient is the exact
second-order one through the inner steps: it reaches W0, b0 and the trunk through both the support and the query features.

``classifier`` is an nn.Linear(512, n_way) that only stores the initialisation (torch's default draw for the weight, a zero bias);
its two tensors follow the ``feature.*`` keys in the state dict.  The same steps and step size hold in train and eval mode; there is
no dropout and no first-order switch.  The head runs on csrc/anil.hip through autograd_ops.anil_scores (hand-written backward), the
loss through autograd_ops.CrossEntropyLoss.  The first-order-MAML ``--fine_tune`` path is not on the HIP path and raises, and the
test-time engine has no mode for the method (finetune.py refuses it).
"""
import torch
import torch.nn as nn

from .. import autograd_ops as AG
from .. import ops
from .meta_template import HeadMethod

MAX_N_WAY = ops.ANIL_MAX_WAY        # the launchers' domain: n_way 1..32, S = n_way * n_support <= 256, any n_query, D = 512
MAX_S = ops.ANIL_MAX_S
MAX_STEPS = ops.ANIL_MAX_STEPS      # inner_steps 1..16


class ANIL(HeadMethod):
    METHOD, ENGINE_MODE = "anil", None

    def __init__(self, model_func, n_way, n_support, inner_steps=5, inner_lr=0.01):
        ops.anil_check(1, n_way, n_support, 1, inner_steps, inner_lr)
        super().__init__(model_func, n_way, n_support)
        if self.feat_dim != ops.ANIL_D:
            raise ValueError("ANIL head: feat_dim = %d is not supported (D = %d)" % (self.feat_dim, ops.ANIL_D))
        self.inner_steps, self.inner_lr = int(inner_steps), float(inner_lr)
        self.loss_fn = AG.CrossEntropyLoss()                         # nn.CrossEntropyLoss() on mft_cross_entropy_mean
        self.classifier = nn.Linear(self.feat_dim, n_way)            # holder of (W0, b0): torch's default draw for the weight ...
        with torch.no_grad():
            self.classifier.bias.zero_()                             # ... and a zero bias

    def load_state_dict(self, state_dict, *args, **kwargs):
        """The trained initialisation fixes n_way: a checkpoint of another n_way is refused by name, not by a shape error."""
        w = state_dict.get("classifier.weight")
        if w is not None and w.shape[0] != self.classifier.out_features:
            raise ValueError("ANIL: the checkpoint's classifier has %d classes and the model was built for n_way = %d; ANIL's trained "
                             "initialisation fixes n_way (--train_n_way and --test_n_way must agree)"
                             % (w.shape[0], self.classifier.out_features))
        return super().load_state_dict(state_dict, *args, **kwargs)

    def _check(self, n_query):
        ops.anil_check(1, self.n_way, self.n_support, n_query, self.inner_steps, self.inner_lr)

    def head_params(self):
        return [self.classifier.weight, self.classifier.bias]

    def _head(self, feats, n_query, episodes=1):
        return AG.anil_scores(feats, *self.head_params(), self.n_way, self.n_support, n_query, episodes=episodes,
                              inner_steps=self.inner_steps, inner_lr=self.inner_lr)
