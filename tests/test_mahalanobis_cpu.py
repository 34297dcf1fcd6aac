"""The Mahalanobis head (methods/mahalanobis.py) on the CPU: the span form and the hand-written backward the
kernels run against the dense float64 definition and its autograd gradients (tests/mahalanobis_reference.py), the golden G34, the
shape checks, the registration beside the five pinned method tables and the refusals of the paths that are not on the HIP path."""
import argparse
import os

import numpy as np
import pytest
import torch

import meta_fine_tuning_amd  # noqa: F401
from meta_fine_tuning_amd import autograd_ops as AG
from meta_fine_tuning_amd import feature_eval, finetune, ops, save_features, synthetic, train
from meta_fine_tuning_amd.io_utils import method_dir_name, model_dict, parse_args
from meta_fine_tuning_amd.methods.anil import ANIL
from meta_fine_tuning_amd.methods.mahalanobis import Mahalanobis
from meta_fine_tuning_amd.methods.meta_template import HeadMethod
from meta_fine_tuning_amd.methods.protonet import ProtoNet
from oracle import mft_oracle as O

from mahalanobis_reference import closed_form, dense_chain, rel

SHAPES = [(5, 5, 15), (2, 1, 1), (3, 2, 2), (1, 3, 2), (1, 1, 1)]         # (n_way, n_support, n_query)
_id = lambda s: "w%d_s%d_q%d" % s  # noqa: E731


def _g34(golden_dir):
    return np.load(os.path.join(golden_dir, "g34_mahalanobis.npz"))


def _inputs(kind, shape, episodes=1):
    n_way, ns, nq = shape
    g = torch.Generator().manual_seed(131 * n_way + 17 * ns + nq + (0 if kind == "randn" else 500000))
    # "randn" at a quarter of unit scale: |scores| is about 20 and cond(Q_c) at most 16.  At unit scale the scores reach 400, the
    # cross entropy saturates and the dense chain's autograd gradient is itself only good to 1e-12 (measured: 1.6e-12 at (2, 1, 1))
    f = 0.25 * torch.randn(episodes, n_way, ns + nq, 512, generator=g, dtype=torch.float64)
    if kind == "relu":
        f = 4.0 * f
        f = torch.relu(0.5 * f + 0.5 * torch.randn(episodes, n_way, 1, 512, generator=g, dtype=torch.float64) + 0.3)
    return f.reshape(-1, 512)


@pytest.mark.parametrize("kind", ["randn", "relu"])
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_closed_form_equals_the_dense_chain_and_its_autograd(shape, kind):
    n_way, ns, nq = shape
    torch.set_num_threads(8)
    f = _inputs(kind, shape).requires_grad_(True)
    loss, scores = dense_chain(f, n_way, ns, nq)
    scores.retain_grad()
    loss.backward()
    # the backward is compared behind the dense chain's own d loss / d scores: softmax - onehot of well-separated scores cancels, so
    # two chains whose scores agree to 1e-14 of |scores| ~ 250 disagree in that gradient by more than the 1e-12 this test is about
    cl, cs, dfeats = closed_form(f, n_way, ns, nq, dscores=scores.grad)
    assert scores.shape == cs.shape == (n_way * nq, n_way)
    assert rel(cs, scores.detach()) < 1e-12 and abs(float(cl) - float(loss.detach())) <= 1e-12 * max(1.0, abs(float(loss.detach())))
    if n_way == 1:          # one class: the loss and its gradient are exactly zero
        assert float(loss.detach()) == 0.0 and float(cl) == 0.0 and not bool(f.grad.any()) and not bool(dfeats.any())
        assert not bool(closed_form(f, n_way, ns, nq)[2].any())
    else:
        assert rel(dfeats, f.grad) < 1e-12
        assert rel(closed_form(f, n_way, ns, nq)[2], f.grad) < 1e-9      # its own cross-entropy gradient: see above
    # an upstream gradient of its own (the only gradient there is at n_way = 1), two episodes
    f2 = _inputs(kind, shape, episodes=2).requires_grad_(True)
    G = torch.randn(2 * n_way * nq, n_way, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    _, scores = dense_chain(f2, n_way, ns, nq, 2)
    (scores * G).sum().backward()
    _, cs, dfeats = closed_form(f2, n_way, ns, nq, 2, dscores=G)
    assert rel(cs, scores.detach()) < 1e-12 and rel(dfeats, f2.grad) < 1e-12


def test_one_support_row_scores_with_the_identity():
    f = _inputs("relu", (1, 1, 3))
    _, scores = dense_chain(f, 1, 1, 3)
    assert torch.allclose(scores[:, 0], -0.5 * ((f[1:] - f[0]) ** 2).sum(1), rtol=1e-14, atol=0.0)


def test_float64_chain_reproduces_g34(golden_dir):
    g = _g34(golden_dir)
    torch.set_num_threads(8)
    sd = O.clone_state(synthetic.resnet10_state_dict(seed=34, prefix="feature."), torch.float64)
    x = synthetic.train_episode(34, 5, 5, 15, 84).double()
    with torch.no_grad():
        feats = O.resnet10_forward(sd, x.reshape(-1, *x.shape[2:]), prefix="feature.")
    assert feats.shape == g["feats"].shape == (100, 512) and g["feats"].dtype == np.float32
    assert rel(torch.from_numpy(g["feats"]), feats) < 1e-7                    # stored rounded to float32
    feats.requires_grad_(True)
    loss, scores = dense_chain(feats, 5, 5, 15)
    ref = torch.from_numpy(g["scores"]).double()
    assert scores.shape == ref.shape == (75, 5)
    assert rel(scores.detach(), ref) < 1e-9
    assert abs(float(loss.detach()) - float(g["loss"])) < 1e-9
    loss.backward()
    assert rel(torch.from_numpy(g["dfeats"]), feats.grad) < 1e-7
    cl, cs, dfeats = closed_form(feats, 5, 5, 15)
    assert rel(cs, ref) < 1e-9 and abs(float(cl) - float(g["loss"])) < 1e-9 and rel(dfeats, feats.grad) < 1e-9
    assert 0.0 < float(g["f32err:loss"]) < 1e-5 and 0.0 < float(g["f32err:scores"]) < 1e-5 and 0.0 < float(g["f32err:dfeats"]) < 1e-4
    assert all(str(k).startswith("feature.") for k in g["state_keys"])
    assert os.path.getsize(os.path.join(golden_dir, "g34_mahalanobis.npz")) < 1 << 20


def test_state_dict_has_feature_keys_only(golden_dir):
    keys = [str(k) for k in _g34(golden_dir)["state_keys"]]
    model = Mahalanobis(model_dict['ResNet10'], n_way=5, n_support=5)
    assert list(model.state_dict().keys()) == keys == list(ProtoNet(model_dict['ResNet10'], 5, 5).state_dict().keys())
    assert all(n.startswith("feature.") for n, _ in model.named_parameters())
    assert isinstance(model, HeadMethod) and model.head_params() == [] and model.head_state() is None
    assert (Mahalanobis.METHOD, Mahalanobis.ENGINE_MODE) == ("mahalanobis", None)
    model.load_state_dict(synthetic.resnet10_state_dict(seed=34, prefix="feature."))


def test_mahalanobis_check_bounds():
    assert (ops.MAHALANOBIS_D, ops.MAHALANOBIS_MAX_WAY, ops.MAHALANOBIS_MAX_S, ops.MAHALANOBIS_BETA) == (512, 32, 256, 1.0)
    assert (ops.MAHALANOBIS_FORWARD_LAUNCHES, ops.MAHALANOBIS_BACKWARD_LAUNCHES) == (3, 3)
    for args in [(1, 5, 5, 15), (4, 5, 20, 15), (1, 5, 50, 15), (1, 32, 8, 1000), (1, 1, 1, 1), (1, 1, 256, 1), (1, 32, 1, 1)]:
        assert ops.mahalanobis_check(*args) is None
    for args, word in [((1, 0, 5, 15), "n_way"), ((1, 33, 1, 1), "n_way"), ((1, 5, 0, 15), "n_support"), ((1, 5, 5, 0), "n_query"),
                       ((0, 5, 5, 15), "episodes"), ((1, 1, 257, 1), "S = n_way"), ((1, 32, 9, 1), "S = n_way")]:
        with pytest.raises(ValueError, match=word):
            ops.mahalanobis_check(*args)
    with pytest.raises(ValueError, match="D = 512"):
        ops.mahalanobis_check(1, 5, 5, 15, D=256)
    # the rest of the launchers' domain: one grid dimension counts the episodes, and row offsets are 32-bit element counts
    assert (ops.MAHALANOBIS_MAX_EPISODES, ops.MAHALANOBIS_MAX_ROWS) == (65535, 2 ** 31 // 512)
    assert ops.mahalanobis_check(65535, 1, 1, 1) is None and ops.mahalanobis_check(1, 1, 1, 2 ** 22 - 2) is None
    for args in [(65536, 1, 1, 1), (1, 1, 1, 2 ** 22 - 1), (4096, 32, 8, 24)]:
        with pytest.raises(ValueError, match="rows"):
            ops.mahalanobis_check(*args)
    for kw in (dict(n_way=33, n_support=1), dict(n_way=1, n_support=257), dict(n_way=0, n_support=5)):
        with pytest.raises(ValueError):
            Mahalanobis(model_dict['ResNet10'], **kw)
    model = Mahalanobis(model_dict['ResNet10'], n_way=5, n_support=50)
    assert model._check(15) is None and model._check(1000) is None
    with pytest.raises(ValueError, match="n_query"):
        model._check(0)
    model.n_support = 52                                   # (set_forward calls _check before the trunk pass)
    with pytest.raises(ValueError, match="S = n_way"):
        model._check(15)


def test_tables_are_unchanged_and_mahalanobis_resolves_through_the_lookup():
    assert list(train.HEAD_METHODS) == ["protonet", "matchingnet", "metaoptnet"]
    assert finetune.EPISODIC_METHODS == ("gnnnet",) + tuple(train.HEAD_METHODS)
    assert train.ADAPTIVE_METHODS == {"anil": ANIL} and train.METRIC_METHODS == {"mahalanobis": Mahalanobis}
    assert train.head_method("mahalanobis") is Mahalanobis and train.head_method("anil") is ANIL
    assert train.head_method("protonet") is ProtoNet and train.head_method("gnnnet") is None and train.head_method("maml") is None
    model = feature_eval.build_model("mahalanobis", model_dict['ResNet10'], 5, 5)
    assert type(model) is Mahalanobis and (model.n_way, model.n_support) == (5, 5)
    assert (type(Mahalanobis(model_dict['ResNet10_FW'], 5, 5).feature).__name__
            == type(ProtoNet(model_dict['ResNet10_FW'], 5, 5).feature).__name__)
    assert save_features.check_method("mahalanobis") is None and "mahalanobis" in save_features.METHODS
    assert method_dir_name("mahalanobis") == "mahalanobis"
    for script in ("train", "save_features", "test"):
        assert parse_args(script, ["--method", "mahalanobis"]).method == "mahalanobis"
    p = argparse.Namespace(dataset="miniImageNet", model="ResNet10", method="mahalanobis", head="ridge", kernel="cossim", train_aug=True,
                           train_n_way=5, n_shot=5, save_iter=-1, split="novel")
    assert save_features.checkpoint_dir(p).endswith("checkpoints/miniImageNet/ResNet10_mahalanobis_aug_5way_5shot")
    with pytest.raises(ValueError):
        feature_eval.build_model("mahalanobis", model_dict['ResNet10'], 5, 5, head="svm")
    with pytest.raises(ValueError):
        feature_eval.build_model("mahalanobis", model_dict['ResNet10'], 5, 5, kernel="linear")


def test_refusals():
    with pytest.raises(NotImplementedError, match="first-order-MAML"):
        train.main(["--method", "mahalanobis", "--fine_tune", "--stop_epoch", "1"])
    with pytest.raises(ValueError, match="metaoptnet"):
        train.main(["--method", "mahalanobis", "--head", "svm", "--stop_epoch", "1"])
    with pytest.raises(ValueError, match="dkt"):
        train.main(["--method", "mahalanobis", "--kernel", "linear", "--stop_epoch", "1"])
    model = Mahalanobis(model_dict['ResNet10'], n_way=5, n_support=5)
    for call in (model.MAML_update, lambda: model.set_forward_finetune(torch.zeros(5, 20, 3, 84, 84)),
                 lambda: model.set_forward_loss_finetune(torch.zeros(5, 20, 3, 84, 84))):
        with pytest.raises(NotImplementedError):
            call()
    liz = [torch.zeros(5, 20, 3, 84, 84)] * 2
    finetune.params = argparse.Namespace(model="ResNet10", fine_tune_epoch=1)
    with pytest.raises(NotImplementedError, match="test --method mahalanobis"):
        finetune.finetune(liz, None, model, {}, None, n_way=5, n_support=5)
    with pytest.raises(NotImplementedError, match="test --method mahalanobis"):
        finetune.finetune_batched([liz], model, {}, 1, 5, 5)
    with pytest.raises(NotImplementedError, match="test --method mahalanobis"):
        finetune.evaluate(model, {}, 1, 5, 5, 15, 84, 0, 1, method="mahalanobis")
    with pytest.raises(NotImplementedError, match="test --method mahalanobis"):
        finetune.main(["--method", "mahalanobis"])


def test_dropin_alias_exports_mahalanobis():
    import importlib.util
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.path.join(here, "meta-fine-tuning_amd", "dropin", "methods", "mahalanobis.py")
    spec = importlib.util.spec_from_file_location("_dropin_mahalanobis", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.Mahalanobis is Mahalanobis


def test_cpu_tensors_raise_runtime_error():
    feats = torch.zeros(5 * 20, 512)
    with pytest.raises(RuntimeError):
        AG.mahalanobis_scores(feats, 5, 5, 15)
    with pytest.raises(RuntimeError):
        ops.mahalanobis_forward(feats, 1, 5, 5, 15)
    with pytest.raises(RuntimeError):
        ops.mahalanobis_backward(dict(feats=feats, T=feats, Mu=feats, W=feats, shape=(1, 5, 5, 15)), torch.ones(75, 5))
