"""ResNet10 backbone with the reference's module tree / state_dict contract and a HIP forward+backward.

Mirror of backbone.{init_layer, Flatten, SimpleBlock, ResNet, ResNet10} (backbone.py:9-23,216-261,
401-439,519-520).  The nn.Conv2d / nn.BatchNorm2d children exist as *parameter containers* so that
key names, ``named_parameters()`` order (the last 9 names are the inner-loop-adaptable set,
finetune.py:236-252), ``load_state_dict``, ``copy.deepcopy`` and optimisers behave exactly as in the
reference; their own ``forward`` is never used -- ``ResNet.forward`` runs the gfx950 kernels of
libmft_hip.so on NHWC activations.  There is no CPU path: a CPU input raises.
"""
import math

import torch
import torch.nn as nn

from . import functional as Fn
from . import ops
from . import autograd_ops as AG


def init_layer(L):
    """Fan-out initialisation (backbone.py:9-16)."""
    if isinstance(L, nn.Conv2d):
        n = L.kernel_size[0] * L.kernel_size[1] * L.out_channels
        L.weight.data.normal_(0, math.sqrt(2.0 / float(n)))
    elif isinstance(L, nn.BatchNorm2d):
        L.weight.data.fill_(1)
        L.bias.data.fill_(0)


class Flatten(nn.Module):
    def forward(self, x):
        return x.view(x.size(0), -1)


class SimpleBlock(nn.Module):
    """Residual block container (backbone.py:216-261); children registered in the reference's order."""
    maml = False

    def __init__(self, indim, outdim, half_res):
        super().__init__()
        self.indim, self.outdim, self.half_res = indim, outdim, half_res
        self.C1 = nn.Conv2d(indim, outdim, kernel_size=3, stride=2 if half_res else 1, padding=1, bias=False)
        self.BN1 = nn.BatchNorm2d(outdim)
        self.C2 = nn.Conv2d(outdim, outdim, kernel_size=3, padding=1, bias=False)
        self.BN2 = nn.BatchNorm2d(outdim)
        self.relu1 = nn.ReLU(inplace=True)
        self.relu2 = nn.ReLU(inplace=True)
        self.parametrized_layers = [self.C1, self.C2, self.BN1, self.BN2]
        if indim != outdim:
            self.shortcut = nn.Conv2d(indim, outdim, 1, 2 if half_res else 1, bias=False)
            self.BNshortcut = nn.BatchNorm2d(outdim)
            self.parametrized_layers += [self.shortcut, self.BNshortcut]
            self.shortcut_type = '1x1'
        else:
            self.shortcut_type = 'identity'
        for layer in self.parametrized_layers:
            init_layer(layer)

    def forward(self, x):
        raise RuntimeError("SimpleBlock is executed by ResNet.forward on the HIP path, not on its own")


class FeatureWiseTransformation2d_fw(nn.BatchNorm2d):
    """Feature-wise transformation layer of Tseng et al. (ICLR 2020; backbone.py:313-350): a BatchNorm2d whose train-mode output is
    perturbed per channel, y = (1 + n_g softplus(gamma)) bn(x) + n_b softplus(beta), n_g, n_b ~ N(0, 1) drawn per call.  A parameter
    container like the other children: ``gamma`` / ``beta`` [1, C, 1, 1] (0.3 / 0.5, frozen unless the user turns their
    ``requires_grad`` on) sit behind ``weight`` / ``bias``; the arithmetic runs in csrc/fwt.hip through ResNet.forward."""
    feature_augment = True

    def __init__(self, num_features, momentum=0.1, track_running_stats=True):
        super().__init__(num_features, momentum=momentum, track_running_stats=track_running_stats)
        self.gamma = nn.Parameter(torch.ones(1, num_features, 1, 1) * 0.3)
        self.beta = nn.Parameter(torch.ones(1, num_features, 1, 1) * 0.5)
        self.gamma.requires_grad = False
        self.beta.requires_grad = False

    def forward(self, x):
        raise RuntimeError("FeatureWiseTransformation2d_fw is executed by ResNet.forward on the HIP path, not on its own")


class SimpleBlock2(SimpleBlock):
    """SimpleBlock whose BN2 and BNshortcut are feature-wise transformation layers (backbone.py:90-130); BN1 stays plain.  Same
    children in the same registration order, hence the reference's state-dict keys."""

    def __init__(self, indim, outdim, half_res):
        super().__init__(indim, outdim, half_res)
        self.BN2 = FeatureWiseTransformation2d_fw(outdim)              # (assigning to a registered name keeps its position)
        init_layer(self.BN2)
        self.parametrized_layers[3] = self.BN2
        if indim != outdim:
            self.BNshortcut = FeatureWiseTransformation2d_fw(outdim)
            init_layer(self.BNshortcut)
            self.parametrized_layers[5] = self.BNshortcut


# the noise layout of one ResNet10_FW forward: [groups, 2, FWT_COLS], row 0 = n_g, row 1 = n_b, the seven
# layers in the reference's draw order at these column offsets
FWT_LAYERS = (("trunk.4.BN2", 64, 0), ("trunk.5.BN2", 128, 64), ("trunk.5.BNshortcut", 128, 192), ("trunk.6.BN2", 256, 320),
              ("trunk.6.BNshortcut", 256, 576), ("trunk.7.BN2", 512, 832), ("trunk.7.BNshortcut", 512, 1344))
FWT_COLS = 1856


def plain_state_dict(sd):
    """A ResNet10_FW (or method-on-ResNet10_FW) state dict without the feature-wise transformation parameters: what is left
    loads into the same model built on ResNet10, where the transformation is the identity it is at test time."""
    out = type(sd)()
    for k, v in sd.items():
        head, _, leaf = k.rpartition(".")
        if leaf in ("gamma", "beta") and head.rpartition(".")[2] in ("BN2", "BNshortcut"):
            continue
        out[k] = v
    return out


def has_fwt_keys(sd):
    return len(plain_state_dict(sd)) != len(sd)


class ResNet(nn.Module):
    """ResNet container (backbone.py:401-439).  ``trunk`` keeps the reference's Sequential indices
    0 Conv2d, 1 BatchNorm2d, 2 ReLU, 3 MaxPool2d, 4-7 SimpleBlock, 8 AvgPool2d, 9 Flatten."""
    maml = False

    def __init__(self, block, list_of_num_layers, list_of_out_dims, flatten=False):
        super().__init__()
        assert len(list_of_num_layers) == 4, 'Can have only four stages'
        if list(list_of_num_layers) != [1, 1, 1, 1] or list(list_of_out_dims) != [64, 128, 256, 512]:
            raise NotImplementedError("only the ResNet10 geometry is built on the HIP path (SURVEY.md §2.1)")
        conv1 = nn.Conv2d(3, 64, kernel_size=7, stride=2, padding=3, bias=False)
        bn1 = nn.BatchNorm2d(64)
        init_layer(conv1)
        init_layer(bn1)
        trunk = [conv1, bn1, nn.ReLU(), nn.MaxPool2d(kernel_size=3, stride=2, padding=1)]
        indim = 64
        for i in range(4):
            for j in range(list_of_num_layers[i]):
                half_res = (i >= 1) and (j == 0)
                trunk.append(block(indim, list_of_out_dims[i], half_res))
                indim = list_of_out_dims[i]
        if flatten:
            # the reference's nn.AvgPool2d(7) is a *global* pool at 224x224; executed as a global average
            # pool so that 84x84 inputs (3x3 map) work too
            trunk.append(nn.AvgPool2d(7))
            trunk.append(Flatten())
            self.final_feat_dim = indim
        else:
            self.final_feat_dim = [indim, 7, 7]
        self.flatten = flatten
        self.trunk = nn.Sequential(*trunk)
        self.feature_wise = block is SimpleBlock2
        if self.feature_wise:
            # the generator's state (csrc/fwt.hip): a 64-bit seed (plain attribute) and the draw index, advanced on the device by
            # every train-mode forward (a buffer, so that it moves with .cuda() and copies with deepcopy; not in the state dict)
            self.fwt_seed = 0
            self.register_buffer("fwt_draw_index", torch.zeros(1, dtype=torch.int64), persistent=False)

    def forward(self, x):
        if not self.flatten:
            raise NotImplementedError("flatten=False feature maps are off the GNN hot path")
        return AG.resnet10_module_forward(self, x)


def ResNet10(flatten=True):
    return ResNet(SimpleBlock, [1, 1, 1, 1], [64, 128, 256, 512], flatten)


def ResNet10_FW(flatten=True):
    """ResNet10 with a feature-wise transformation layer at the end of every residual block (backbone.py:521-522)."""
    return ResNet(SimpleBlock2, [1, 1, 1, 1], [64, 128, 256, 512], flatten)


class _WeightNormLinear(nn.Module):
    """Parameter container with the keys, shapes and registration order of
    ``WeightNorm.apply(nn.Linear(indim, outdim, bias=False), 'weight', dim=0)``: ``weight_g`` [outdim, 1], ``weight_v``
    [outdim, indim].  No hook recomposes a ``weight``: the head kernels read g and v directly."""

    def __init__(self, indim, outdim):
        super().__init__()
        self.in_features, self.out_features = indim, outdim
        v = nn.Linear(indim, outdim, bias=False).weight.data        # the draw the torch class makes from the global RNG
        self.weight_g = nn.Parameter(torch.norm_except_dim(v, 2, 0).data)
        self.weight_v = nn.Parameter(v)

    def forward(self, x):
        raise RuntimeError("distLinear.L is executed by distLinear.forward on the HIP path, not on its own")


class distLinear(nn.Module):
    """Baseline++ cosine classifier ("A Closer Look at Few-shot Classification"): scores = scale_factor * cos-similarity of
    x / (||x|| + 1e-5) and the weight-normalised rows g_c v_c / ||v_c||, scale_factor 2 up to 200 classes and 10 above, no bias.
    The state dict is the torch weight-norm module's (``L.weight_g``, ``L.weight_v``); forward and backward are one HIP launch
    each (autograd_ops.dist_linear)."""

    def __init__(self, indim, outdim):
        super().__init__()
        self.L = _WeightNormLinear(indim, outdim)
        self.class_wise_learnable_norm = True
        self.scale_factor = 2 if outdim <= 200 else 10

    def forward(self, x):
        return AG.dist_linear(x, self.L.weight_g, self.L.weight_v, self.scale_factor)
