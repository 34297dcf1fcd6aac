"""Baseline++ without a GPU: the module contract of backbone.distLinear against torch's weight-norm Linear, and the golden G24
(the reference's BaselineFinetune(loss_type='dist') run on the CPU, tools/make_golden_baselinepp.py) against a float64
restatement of the head's definition that replays G24's permutation stream."""
import os
import warnings

import numpy as np
import pytest
import torch
import torch.nn as nn

import meta_fine_tuning_amd  # noqa: F401
from meta_fine_tuning_amd import backbone
from meta_fine_tuning_amd.methods.baselinefinetune import BaselineFinetune
from meta_fine_tuning_amd.methods.baselinetrain import BaselineTrain

torch.set_num_threads(8)


class TorchDistHead(nn.Module):
    """The parameter layout distLinear has to match: a bias-free Linear under torch's weight-norm hook, as child ``L``."""

    def __init__(self, indim, outdim):
        super().__init__()
        from torch.nn.utils.weight_norm import WeightNorm
        self.L = nn.Linear(indim, outdim, bias=False)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            WeightNorm.apply(self.L, 'weight', dim=0)


def dist_scores64(x, g, v, s):
    """score[r,c] = s * (x_r / (||x_r|| + 1e-5)) . (g_c v_c / ||v_c||) in float64."""
    x, g, v = x.double(), g.double().reshape(-1, 1), v.double()
    xh = x / (x.norm(dim=1, keepdim=True) + 1e-5)
    return s * xh @ (g * v / v.norm(dim=1, keepdim=True)).t()


def adapt64(z_support, y_support, z_query, v0, g0, perms, batch_size=4):
    """baselinefinetune.py:35-58 with the head above, in float64: SGD(0.01, 0.9, 0.9, 0.001) over the given permutations."""
    n_way = v0.shape[0]
    s = 2.0 if n_way <= 200 else 10.0
    v = torch.from_numpy(np.asarray(v0)).double().requires_grad_(True)
    g = torch.from_numpy(np.asarray(g0)).double().reshape(n_way, 1).requires_grad_(True)
    opt = torch.optim.SGD([g, v], lr=0.01, momentum=0.9, dampening=0.9, weight_decay=0.001)
    y = torch.from_numpy(np.asarray(y_support)).long()
    S = z_support.shape[0]
    for rand_id in perms:
        for i in range(0, S, batch_size):
            ids = torch.from_numpy(np.asarray(rand_id[i:min(i + batch_size, S)])).long()
            opt.zero_grad()
            torch.nn.functional.cross_entropy(dist_scores64(z_support[ids], g, v, s), y[ids]).backward()
            opt.step()
    return g.detach(), v.detach(), dist_scores64(z_query, g.detach(), v.detach(), s)


def g24_features(n_shot):
    return torch.from_numpy(np.abs(np.random.RandomState(271 + n_shot).standard_normal((5, n_shot + 15, 512))).astype(np.float32))


# ---------------------------------------------------------------------------------------------------- module contract
@pytest.mark.parametrize("C", [5, 200, 201])
def test_distlinear_has_the_torch_weight_norm_contract(C):
    torch.manual_seed(7 + C)
    ours = backbone.distLinear(512, C)
    after_ours = torch.rand(1)
    torch.manual_seed(7 + C)
    ref = TorchDistHead(512, C)
    after_ref = torch.rand(1)
    assert torch.equal(after_ours, after_ref)                  # one draw each from the global torch RNG
    a, b = ours.state_dict(), ref.state_dict()
    assert list(a.keys()) == list(b.keys()) == ["L.weight_g", "L.weight_v"]
    assert [n for n, _ in ours.named_parameters()] == [n for n, _ in ref.named_parameters()]
    assert a["L.weight_g"].shape == (C, 1) and a["L.weight_v"].shape == (C, 512)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert ours.class_wise_learnable_norm is True
    assert ours.scale_factor == (2 if C <= 200 else 10)
    assert not ours.L._forward_pre_hooks                       # no torch weight-norm hook: the kernels read g and v
    # strict loads, both ways
    torch.manual_seed(99)
    other_ours, other_ref = backbone.distLinear(512, C), TorchDistHead(512, C)
    other_ref.load_state_dict(a, strict=True)
    other_ours.load_state_dict(ref.state_dict(), strict=True)
    for k in a:
        assert torch.equal(other_ref.state_dict()[k], a[k]) and torch.equal(other_ours.state_dict()[k], a[k])


def test_distlinear_exported_by_the_dropin_backbone():
    import importlib.util
    path = os.path.join(os.path.dirname(os.path.abspath(backbone.__file__)), "dropin", "backbone.py")
    spec = importlib.util.spec_from_file_location("_dropin_backbone_under_test", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.distLinear is backbone.distLinear


def test_loss_type_is_checked_and_cpu_forward_raises():
    with pytest.raises(ValueError):
        BaselineTrain(backbone.ResNet10, 10, loss_type='cosine')
    with pytest.raises(ValueError):
        BaselineFinetune(backbone.ResNet10, 5, 5, loss_type='cosine')
    m = BaselineTrain(backbone.ResNet10, 10, loss_type='dist')
    assert isinstance(m.classifier, backbone.distLinear)
    assert list(m.classifier.state_dict().keys()) == ["L.weight_g", "L.weight_v"]
    assert [k for k in m.state_dict() if k.startswith("classifier.")] == ["classifier.L.weight_g", "classifier.L.weight_v"]
    f = BaselineFinetune(backbone.ResNet10, 5, 5, loss_type='dist')
    assert f.loss_type == 'dist'
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.classifier(torch.randn(4, 512))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        from meta_fine_tuning_amd import autograd_ops
        autograd_ops.dist_linear(torch.randn(4, 512), m.classifier.L.weight_g, m.classifier.L.weight_v, 2)


# ---------------------------------------------------------------------------------------------------- fixture consistency
@pytest.mark.parametrize("n_shot", [5, 20])
def test_g24_is_the_float64_restatement_on_its_permutation_stream(golden_dir, n_shot):
    g24 = np.load(os.path.join(golden_dir, "g24_baselinepp.npz"))
    tag = "_%dshot" % n_shot
    z = g24_features(n_shot)
    S = 5 * n_shot
    # the head's draw: one nn.Linear(512, 5, bias=False) under torch.manual_seed(123)
    torch.manual_seed(123)
    head = backbone.distLinear(512, 5)
    assert torch.equal(head.L.weight_v.data, torch.from_numpy(g24["v0" + tag]))
    assert torch.equal(head.L.weight_g.data, torch.from_numpy(g24["g0" + tag]))
    np.random.seed(10)
    perms = [np.random.permutation(S) for _ in range(100)]
    assert np.array_equal(np.random.permutation(7), g24["next_perm" + tag])
    g, v, sc = adapt64(z[:, :n_shot].reshape(S, 512), np.repeat(np.arange(5), n_shot), z[:, n_shot:].reshape(75, 512),
                       g24["v0" + tag], g24["g0" + tag], perms)
    eg = float((g - torch.from_numpy(g24["g" + tag]).double()).abs().max())
    ev = float((v - torch.from_numpy(g24["v" + tag]).double()).abs().max())
    es = float((sc - torch.from_numpy(g24["scores" + tag]).double()).abs().max())
    print("G24 %d-shot: fp32 reference vs float64 restatement: max|dg| %.2e  max|dv| %.2e  max|dscore| %.2e" % (n_shot, eg, ev, es))
    assert eg < 2e-5 and ev < 2e-5 and es < 2e-5, (eg, ev, es)
    assert g24["scores" + tag].shape == (75, 5)
