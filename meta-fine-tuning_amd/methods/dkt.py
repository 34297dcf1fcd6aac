"""DKT: Deep Kernel Transfer (Patacchiola et al., NeurIPS 2020) on the reference's MetaTemplate, on pooled ResNet10 features
(definition in DESIGN.md section 20).  n_way one-vs-rest Gaussian processes share the kernel k(i, j) = s <u_i, u_j> on the
normalised features (KERNEL "cossim": u = z / |z|; "linear": u = z / sqrt(D)), a constant mean and a noise level.  Training
minimises the negative marginal log-likelihood of ALL rows of the episode, support and query together, with targets +1 / -1:
there is no cross entropy and there are no scores on the training path.  The scores are the posterior mean at the queries of the
processes conditioned on the support rows.

``gp`` holds the three one-element parameters and nothing else; they follow the ``feature.*`` keys in the state dict.  The loss
runs on csrc/dkt.hip through autograd_ops.dkt_loss (hand-written backward), the scores through autograd_ops.dkt_scores: a
prediction, whose tensor never requires grad.  The first-order-MAML ``--fine_tune`` path is not on the HIP path and raises, and
the test-time engine has no Gaussian-process mode (finetune.py refuses the method).
"""
import math

import torch
import torch.nn as nn

from .. import autograd_ops as AG
from .. import ops
from .meta_template import HeadMethod

MAX_N_WAY = ops.DKT_MAX_WAY         # the launchers' domain: n_way 1..32, D = 512; loss N <= 256, scores S <= 256 with any n_query
MAX_M = ops.DKT_MAX_M
KERNELS = ops.DKT_KERNELS
RAW_NOISE_INIT = math.log(math.expm1(ops.DKT_NOISE_INIT - ops.DKT_NOISE_FLOOR))     # softplus^-1(0.1 - 1e-4): noise = 0.1


class GPHyperparameters(nn.Module):
    """Holder of the constant mean and the two raw (pre-softplus) kernel hyperparameters; the arithmetic is in csrc/dkt.hip.
    Nothing is drawn: mean 0, outputscale softplus(0) = ln 2, noise 1e-4 + softplus(raw_noise) = 0.1."""

    def __init__(self):
        super().__init__()
        self.mean = nn.Parameter(torch.zeros(1))
        self.raw_outputscale = nn.Parameter(torch.zeros(1))
        self.raw_noise = nn.Parameter(torch.full((1,), RAW_NOISE_INIT))

    def forward(self, *args, **kwargs):
        raise NotImplementedError("GPHyperparameters holds parameters; DKT runs the Gaussian process on csrc/dkt.hip")


class _LossSum:
    """The float64 device scalar the loss launch adds every step's loss to (AG.CrossEntropyLoss.loss_sum): the graphed episode loop
    prints its running mean from differences of it."""
    loss_sum = AG.CrossEntropyLoss.loss_sum


class DKT(HeadMethod):
    METHOD, ENGINE_MODE = "dkt", None

    def __init__(self, model_func, n_way, n_support, kernel="cossim"):
        ops.dkt_check(1, n_way, n_support, 1, loss=False)
        ops.dkt_kernel_id(kernel)
        super().__init__(model_func, n_way, n_support)
        if self.feat_dim != ops.DKT_D:
            raise ValueError("DKT head: feat_dim = %d is not supported (D = %d)" % (self.feat_dim, ops.DKT_D))
        self.kernel = kernel
        self.loss_fn = _LossSum()                                    # keeper of the running loss sum; there is no loss module
        self.gp = GPHyperparameters()

    def _check(self, n_query, loss=False):
        """Scores condition on the support rows (S <= 256, any n_query); the loss on all rows of the episode (N <= 256)."""
        ops.dkt_check(1, self.n_way, self.n_support, n_query, loss=loss)

    def head_params(self):
        return [self.gp.mean, self.gp.raw_outputscale, self.gp.raw_noise]

    def _head(self, feats, n_query, episodes=1):
        return AG.dkt_scores(feats, *self.head_params(), self.n_way, self.n_support, n_query, episodes=episodes, kernel=self.kernel)

    def _loss(self, feats, n_query, episodes):
        return AG.dkt_loss(feats, *self.head_params(), self.n_way, self.n_support, n_query, episodes=episodes, kernel=self.kernel,
                           loss_sum=self.loss_fn.loss_sum(feats.device))

    def set_forward_loss(self, x):
        """The negative marginal log-likelihood of the episode's rows (a refused shape raises before the trunk pass)."""
        n_query = x.size(1) - self.n_support
        self._check(n_query, loss=True)
        x = x.cuda()
        if self.freeze_backbone:
            for p in self.feature.parameters():
                p.requires_grad = False
        return self._loss(self.feature(x.reshape(-1, *x.size()[2:])), n_query, 1)

    def set_forward_loss_lockstep(self, xs):
        """Mean over the k episodes of ``set_forward_loss``: its backward leaves the average of the k episodes' gradients."""
        k, n_query = xs.size(0), xs.size(2) - self.n_support
        self._check(n_query, loss=True)
        xs = xs.cuda()
        feats = AG.resnet10_module_forward(self.feature, xs.reshape(-1, *xs.size()[3:]), groups=k)
        return self._loss(feats, n_query, k)

    def _loss_item(self, loss):
        """The eager episode loop adds the loss itself to its running sum, as the graphed loop's device sum does."""
        return loss.item()
