"""DKT (methods/dkt.py) on the CPU: the definition restated in float64 (tests/dkt_reference.py) against the
golden G32, its autograd gradients against the closed forms the kernels use, the module's state-dict keys and initial values, the
shape checks, the registration beside the three pinned method tables and the refusals of the paths that are not on the HIP path."""
import argparse
import math
import os

import numpy as np
import pytest
import torch

import meta_fine_tuning_amd  # noqa: F401
from meta_fine_tuning_amd import autograd_ops as AG
from meta_fine_tuning_amd import feature_eval, finetune, ops, save_features, synthetic, train
from meta_fine_tuning_amd.io_utils import method_dir_name, model_dict, parse_args
from meta_fine_tuning_amd.methods.dkt import DKT, GPHyperparameters
from meta_fine_tuning_amd.methods.feat import FEAT
from meta_fine_tuning_amd.methods.protonet import ProtoNet
from meta_fine_tuning_amd.methods.tpn import TPN
from oracle import mft_oracle as O

from dkt_reference import HEAD, RAW_NOISE_INIT, dkt_chain, dkt_closed_form, hyper_values, raw_noise_for, rel


def _g32(golden_dir):
    return np.load(os.path.join(golden_dir, "g32_dkt.npz"))


def test_float64_chain_reproduces_g32(golden_dir):
    g = _g32(golden_dir)
    torch.set_num_threads(8)
    sd = O.clone_state(synthetic.resnet10_state_dict(seed=32, prefix="feature."), torch.float64)
    hs = synthetic.dkt_head_state(32)
    hyper = [hs[k].double().requires_grad_(True) for k in HEAD]
    x = synthetic.train_episode(32, 5, 5, 16, 84).double()
    with torch.no_grad():
        feats = O.resnet10_forward(sd, x.reshape(-1, *x.shape[2:]), prefix="feature.")
    feats.requires_grad_(True)
    loss, scores, per = dkt_chain(feats, hyper, 5, 5, 16)
    ref = torch.from_numpy(g["scores"]).double()
    assert scores.shape == ref.shape == (80, 5) and per.shape == (1,)
    assert rel(scores, ref) < 1e-9
    assert abs(float(loss.detach()) - float(g["loss"])) < 1e-9
    loss.backward()
    for k, p in zip(HEAD, hyper):
        want = torch.from_numpy(g["headgrad:" + k])
        assert p.grad.shape == want.shape == (1,)
        assert float((p.grad - want).norm()) <= 1e-8 * float(want.norm()), k
    # every query of this class-structured episode is scored highest for its own class, and the stored float32 step is close
    assert torch.equal(ref.argmax(1), torch.arange(5).repeat_interleave(16))
    assert 0.0 < float(g["f32err:loss"]) < 1e-5 and 0.0 < float(g["f32err:scores"]) < 1e-4
    assert [str(k) for k in g["state_keys"]][-3:] == HEAD


@pytest.mark.parametrize("kernel", ["cossim", "linear"])
@pytest.mark.parametrize("shape", [(1, 5, 5, 16), (3, 3, 2, 3), (2, 1, 1, 1)], ids=lambda s: "E%d_w%d_s%d_q%d" % s)
def test_autograd_gradients_equal_the_closed_forms(kernel, shape):
    E, n_way, ns, nq = shape
    g = torch.Generator().manual_seed(11 + E)
    feats = torch.relu(torch.randn(E * n_way * (ns + nq), 512, generator=g, dtype=torch.float64) + 0.3).requires_grad_(True)
    hyper = [torch.tensor([v], dtype=torch.float64, requires_grad=True) for v in (0.05, 0.3, raw_noise_for(0.01))]
    loss, _, _ = dkt_chain(feats, hyper, n_way, ns, nq, E, kernel, scores=False)
    loss.backward()
    dz, dmean, dos, dnoise = dkt_closed_form(feats.detach(), [h.detach() for h in hyper], n_way, ns, nq, E, kernel)
    assert rel(dz, feats.grad) < 1e-12
    for got, p in zip((dmean, dos, dnoise), hyper):
        assert abs(float(got) - float(p.grad)) <= 1e-12 * max(1.0, abs(float(p.grad)))


def test_zero_row_under_cossim_is_finite_in_the_chain():
    g = torch.Generator().manual_seed(3)
    feats = torch.randn(2 * 3, 512, generator=g, dtype=torch.float64)
    feats[2] = 0.0
    feats.requires_grad_(True)
    hyper = [torch.tensor([v], dtype=torch.float64) for v in (0.0, 0.0, RAW_NOISE_INIT)]
    loss, scores, _ = dkt_chain(feats, hyper, 2, 1, 2)
    loss.backward()
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(scores).all()) and bool(torch.isfinite(feats.grad).all())
    dz = dkt_closed_form(feats.detach(), hyper, 2, 1, 2)[0]
    assert rel(dz, feats.grad) < 1e-12 and float(feats.grad[2].abs().max()) > 1e6       # dU / 1e-12 on the clamped row


def test_state_dict_keys_initial_values_and_rng_position(golden_dir):
    g = _g32(golden_dir)
    keys = [str(k) for k in g["state_keys"]]
    torch.manual_seed(1234)
    model = DKT(model_dict['ResNet10'], n_way=5, n_support=5)
    after = torch.get_rng_state()
    assert list(model.state_dict().keys()) == keys
    assert keys[-3:] == HEAD and all(k.startswith("feature.") for k in keys[:-3])
    assert [n for n, _ in model.named_parameters() if not n.startswith("feature.")] == HEAD
    assert [tuple(model.state_dict()[k].shape) for k in HEAD] == [(1,), (1,), (1,)]
    assert isinstance(model.gp, GPHyperparameters) and list(model.gp.children()) == []
    assert float(model.gp.mean.detach()) == 0.0 and float(model.gp.raw_outputscale.detach()) == 0.0
    mean, s, noise = hyper_values([p.detach().double() for p in model.head_params()])
    assert abs(float(s) - math.log(2.0)) < 1e-12 and abs(float(noise) - 0.1) < 1e-7
    assert abs(float(model.gp.raw_noise.detach()) - math.log(math.expm1(0.1 - 1e-4))) < 1e-6
    assert (DKT.METHOD, DKT.ENGINE_MODE, model.kernel) == ("dkt", None, "cossim")
    assert DKT(model_dict['ResNet10'], 5, 5, kernel="linear").kernel == "linear"
    with pytest.raises(ValueError, match="kernel"):
        DKT(model_dict['ResNet10'], 5, 5, kernel="rbf")
    assert [p is q for p, q in zip(model.head_params(), (model.gp.mean, model.gp.raw_outputscale, model.gp.raw_noise))] == [True] * 3
    # constructing the head draws nothing: the torch RNG stands where the backbone alone leaves it
    torch.manual_seed(1234)
    model_dict['ResNet10']()
    assert torch.equal(torch.get_rng_state(), after)
    sd = synthetic.resnet10_state_dict(seed=32, prefix="feature.")
    sd.update(synthetic.dkt_head_state(32))
    assert list(sd.keys()) == keys
    fresh = DKT(model_dict['ResNet10'], n_way=5, n_support=5)
    fresh.load_state_dict(sd)
    assert all(torch.equal(getattr(fresh.gp, k[3:]).detach(), sd[k]) for k in HEAD)


def test_dkt_check_bounds():
    assert ops.dkt_check(1, 5, 5, 16) is None and ops.dkt_check(4, 5, 20, 15) is None and ops.dkt_check(1, 4, 49, 15) is None
    assert ops.dkt_check(1, 32, 7, 1) is None and ops.dkt_check(1, 1, 1, 1) is None
    with pytest.raises(ValueError, match="N = n_way"):             # 5-way 50-shot with 15 queries: N = 325 cannot be trained ...
        ops.dkt_check(1, 5, 50, 15)
    assert ops.dkt_check(1, 5, 50, 15, loss=False) is None         # ... but S = 250 can be scored
    assert ops.dkt_check(1, 32, 8, 1000, loss=False) is None
    for loss in (True, False):
        for args, word in [((1, 0, 5, 16), "n_way"), ((1, 33, 1, 1), "n_way"), ((1, 5, 0, 16), "n_support"), ((1, 5, 5, 0), "n_query"),
                           ((0, 5, 5, 16), "episodes"), ((1, 1, 257, 1), "256")]:
            with pytest.raises(ValueError, match=word):
                ops.dkt_check(*args, loss=loss)
        with pytest.raises(ValueError, match="D = 512"):
            ops.dkt_check(1, 5, 5, 16, D=256, loss=loss)
    with pytest.raises(ValueError, match="S = n_way"):
        ops.dkt_check(1, 1, 257, 1, loss=False)
    with pytest.raises(ValueError):
        DKT(model_dict['ResNet10'], n_way=33, n_support=1)
    with pytest.raises(ValueError):
        DKT(model_dict['ResNet10'], n_way=1, n_support=257)
    model = DKT(model_dict['ResNet10'], n_way=5, n_support=50)
    assert model._check(15) is None and model._check(1, loss=True) is None
    with pytest.raises(ValueError, match="N = n_way"):
        model._check(15, loss=True)
    # set_forward_loss refuses the shape before the trunk pass (and before any device is touched)
    model.feature = None
    with pytest.raises(ValueError, match="N = n_way"):
        model.set_forward_loss(torch.zeros(5, 65, 1))
    with pytest.raises(ValueError, match="N = n_way"):
        model.set_forward_loss_lockstep(torch.zeros(2, 5, 65, 1))


def test_directory_names_and_kernel_flag():
    assert method_dir_name("dkt") == "dkt" and method_dir_name("dkt", kernel="cossim") == "dkt"
    assert method_dir_name("dkt", kernel="linear") == "dkt_linear"
    assert method_dir_name("protonet", kernel="cossim") == "protonet" and method_dir_name("metaoptnet", "svm") == "metaoptnet_svm"
    with pytest.raises(ValueError, match="dkt"):
        method_dir_name("protonet", kernel="linear")
    with pytest.raises(ValueError, match="kernel"):
        method_dir_name("dkt", kernel="rbf")
    with pytest.raises(ValueError, match="metaoptnet"):
        method_dir_name("dkt", "svm")
    assert parse_args("train", ["--method", "dkt"]).kernel == "cossim"
    for script in ("train", "save_features", "test"):
        assert parse_args(script, ["--method", "dkt", "--kernel", "linear"]).kernel == "linear"
    p = argparse.Namespace(dataset="miniImageNet", model="ResNet10", method="dkt", head="ridge", kernel="cossim", train_aug=True,
                           train_n_way=5, n_shot=5, save_iter=-1, split="novel")
    assert save_features.checkpoint_dir(p).endswith("checkpoints/miniImageNet/ResNet10_dkt_aug_5way_5shot")
    assert save_features.features_file(p).endswith("features/miniImageNet/ResNet10_dkt_aug_5way_5shot/novel.npz")
    p.kernel = "linear"
    assert save_features.checkpoint_dir(p).endswith("checkpoints/miniImageNet/ResNet10_dkt_linear_aug_5way_5shot")
    assert save_features.check_method("dkt") is None and "dkt" in save_features.METHODS
    with pytest.raises(ValueError):
        feature_eval.build_model("dkt", model_dict['ResNet10'], 5, 5, head="svm")
    with pytest.raises(ValueError):
        feature_eval.build_model("tpn", model_dict['ResNet10'], 5, 5, kernel="linear")


def test_tables_are_unchanged_and_dkt_resolves_through_the_lookup():
    assert list(train.HEAD_METHODS) == ["protonet", "matchingnet", "metaoptnet"]
    assert finetune.EPISODIC_METHODS == ("gnnnet",) + tuple(train.HEAD_METHODS)
    assert train.TRANSDUCTIVE_METHODS == {"tpn": TPN} and train.EMBEDDING_METHODS == {"feat": FEAT}
    assert train.PROBABILISTIC_METHODS == {"dkt": DKT}
    assert train.head_method("dkt") is DKT and train.head_method("tpn") is TPN and train.head_method("feat") is FEAT
    assert train.head_method("protonet") is ProtoNet and train.head_method("gnnnet") is None and train.head_method("baseline") is None
    model = feature_eval.build_model("dkt", model_dict['ResNet10'], 5, 5)
    assert type(model) is DKT and model.n_way == 5 and model.n_support == 5 and model.kernel == "cossim"
    assert feature_eval.build_model("dkt", model_dict['ResNet10'], 5, 5, kernel="linear").kernel == "linear"
    assert type(DKT(model_dict['ResNet10_FW'], 5, 5).feature).__name__ == type(ProtoNet(model_dict['ResNet10_FW'], 5, 5).feature).__name__


def test_refusals():
    with pytest.raises(NotImplementedError, match="first-order-MAML"):
        train.main(["--method", "dkt", "--fine_tune", "--stop_epoch", "1"])
    with pytest.raises(ValueError, match="metaoptnet"):
        train.main(["--method", "dkt", "--head", "svm", "--stop_epoch", "1"])
    with pytest.raises(ValueError, match="dkt"):
        train.main(["--method", "protonet", "--kernel", "linear", "--stop_epoch", "1"])
    with pytest.raises(ValueError, match="kernel"):
        train.main(["--method", "dkt", "--kernel", "rbf", "--stop_epoch", "1"])
    model = DKT(model_dict['ResNet10'], n_way=5, n_support=5)
    for call in (model.MAML_update, lambda: model.set_forward_finetune(torch.zeros(5, 21, 3, 84, 84)),
                 lambda: model.set_forward_loss_finetune(torch.zeros(5, 21, 3, 84, 84))):
        with pytest.raises(NotImplementedError):
            call()
    with pytest.raises(NotImplementedError):
        model.gp()
    liz = [torch.zeros(5, 20, 3, 84, 84)] * 2
    finetune.params = argparse.Namespace(model="ResNet10", fine_tune_epoch=1)
    with pytest.raises(NotImplementedError, match="test --method dkt"):
        finetune.finetune(liz, None, model, {}, None, n_way=5, n_support=5)
    with pytest.raises(NotImplementedError, match="test --method dkt"):
        finetune.finetune_batched([liz], model, {}, 1, 5, 5)
    with pytest.raises(NotImplementedError, match="test --method dkt"):
        finetune.evaluate(model, {}, 1, 5, 5, 15, 84, 0, 1, method="dkt")
    with pytest.raises(NotImplementedError, match="test --method dkt"):
        finetune.main(["--method", "dkt"])


def test_dropin_alias_exports_dkt():
    import importlib.util
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.path.join(here, "meta-fine-tuning_amd", "dropin", "methods", "dkt.py")
    spec = importlib.util.spec_from_file_location("_dropin_dkt", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.DKT is DKT


def test_cpu_tensors_raise_runtime_error():
    feats = torch.zeros(5 * 21, 512)
    hyper = tuple(synthetic.dkt_head_state(32)[k] for k in HEAD)
    with pytest.raises(RuntimeError):
        AG.dkt_loss(feats, *hyper, 5, 5, 16)
    with pytest.raises(RuntimeError):
        AG.dkt_scores(feats, *hyper, 5, 5, 16)
    with pytest.raises(RuntimeError):
        ops.dkt_loss_forward(feats, hyper, 1, 5, 5, 16)
    with pytest.raises(RuntimeError):
        ops.dkt_scores(feats, hyper, 1, 5, 5, 16)
    with pytest.raises(RuntimeError):
        ops.dkt_loss_backward(dict(U=feats, nrm=feats, L=feats, A=feats, stats=feats, hyper=hyper, linear=0, shape=(1, 5, 5, 16)),
                              torch.ones(1))
