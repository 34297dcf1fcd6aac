"""Mahalanobis: the classifier of Simple CNAPS (Bateni et al., "Improved Few-Shot Visual Classification", CVPR 2020) on the
reference's MetaTemplate, on pooled ResNet10 features (definition in DESIGN.md section 22): the first head here that estimates a
metric per class from the support set.  A query is scored by minus half its squared Mahalanobis distance to each class mean, under
the class's regularised covariance Q_c = lambda S_c + (1 - lambda) S_t + beta I: the class's and the task's unbiased sample
covariances blended with lambda = n_support / (n_support + 1), and beta = 1.  The loss is cross entropy on the scores; the gradient
reaches the trunk through the support rows (class means, task mean, both covariances) and the query rows, exactly.

The head has no parameters and no train / eval difference: the state dict holds ``feature.*`` only, as ProtoNet's, and the head
scores the features of any checkpoint.  It runs on csrc/mahalanobis.hip through autograd_ops.mahalanobis_scores (hand-written
backward), the loss through autograd_ops.CrossEntropyLoss.  The first-order-MAML ``--fine_tune`` path is not on the HIP path and
raises, and the test-time engine has no mode for the method (finetune.py refuses it).
"""
from .. import autograd_ops as AG
from .. import ops
from .meta_template import HeadMethod

MAX_N_WAY = ops.MAHALANOBIS_MAX_WAY     # the launchers' domain: n_way 1..32, S = n_way * n_support <= 256, any n_query, D = 512
MAX_S = ops.MAHALANOBIS_MAX_S


class Mahalanobis(HeadMethod):
    METHOD, ENGINE_MODE = "mahalanobis", None

    def __init__(self, model_func, n_way, n_support):
        ops.mahalanobis_check(1, n_way, n_support, 1)
        super().__init__(model_func, n_way, n_support)
        if self.feat_dim != ops.MAHALANOBIS_D:
            raise ValueError("Mahalanobis head: feat_dim = %d is not supported (D = %d)" % (self.feat_dim, ops.MAHALANOBIS_D))
        self.loss_fn = AG.CrossEntropyLoss()                         # nn.CrossEntropyLoss() on mft_cross_entropy_mean

    def _check(self, n_query):
        ops.mahalanobis_check(1, self.n_way, self.n_support, n_query)

    def _head(self, feats, n_query, episodes=1):
        return AG.mahalanobis_scores(feats, self.n_way, self.n_support, n_query, episodes=episodes)
