"""MetaOptNet (methods/metaoptnet.py) on the CPU: the ridge-regression head restated in float64 against the
golden G27, the module's state-dict keys, the shape checks and the refusals of the paths that are not on the HIP path."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import meta_fine_tuning_amd  # noqa: F401
from meta_fine_tuning_amd import autograd_ops as AG
from meta_fine_tuning_amd import ops, synthetic
from meta_fine_tuning_amd.io_utils import model_dict
from meta_fine_tuning_amd.methods.metaoptnet import MetaOptNet
from oracle import mft_oracle as O


def ridge_head64(feats, scale, n_way, n_support, n_query, lambda_reg=50.0):
    """DESIGN.md section 14 on features [n_way, n_support + n_query, D] in float64, by an explicit inverse-free solve:
    A = Z_S Z_S^T + lambda I, alpha = 2 A^-1 Y, W = Z_S^T alpha, scores = scale Z_Q W; query rows class-major."""
    z = feats.double()
    zs = z[:, :n_support].reshape(n_way * n_support, -1)
    zq = z[:, n_support:].reshape(n_way * n_query, -1)
    Y = torch.zeros(n_way * n_support, n_way, dtype=torch.float64)
    Y[torch.arange(n_way * n_support), torch.arange(n_way * n_support) // n_support] = 1.0
    A = zs @ zs.t() + lambda_reg * torch.eye(n_way * n_support, dtype=torch.float64)
    alpha = 2.0 * torch.linalg.solve(A, Y)
    return float(scale) * (zq @ (zs.t() @ alpha))


def _g27(golden_dir):
    return np.load(os.path.join(golden_dir, "g27_metaoptnet.npz"))


def test_float64_head_matches_g27_scores_and_loss(golden_dir):
    g = _g27(golden_dir)
    torch.set_num_threads(8)
    sd = O.clone_state(synthetic.resnet10_state_dict(seed=27, prefix="feature."), torch.float64)
    scale = synthetic.metaoptnet_head_state(27)["scale"]
    assert scale.shape == (1,) and abs(float(scale) - 1.0) > 0.04
    x = synthetic.train_episode(27, 5, 5, 16, 84).double()
    with torch.no_grad():
        feats = O.resnet10_forward(sd, x.reshape(-1, *x.shape[2:]), prefix="feature.").view(5, 21, -1)
    scores = ridge_head64(feats, scale, 5, 5, 16)
    ref = torch.from_numpy(g["scores"]).double()
    assert scores.shape == ref.shape == (80, 5)
    assert float((scores - ref).norm() / ref.norm()) < 1e-9
    assert float((scores - ref).abs().max()) < 1e-9 * float(ref.abs().max())
    loss = float(F.cross_entropy(scores, torch.from_numpy(np.repeat(np.arange(5), 16))))
    assert abs(loss - float(g["loss"])) < 1e-9


def test_state_dict_keys_equal_g27_and_load(golden_dir):
    g = _g27(golden_dir)
    keys = [str(k) for k in g["state_keys"]]
    model = MetaOptNet(model_dict['ResNet10'], n_way=5, n_support=5)
    assert list(model.state_dict().keys()) == keys
    assert keys[-1] == "scale" and all(k.startswith("feature.") for k in keys[:-1])
    assert [n for n, _ in model.named_parameters() if not n.startswith("feature.")] == ["scale"]
    assert float(model.scale.detach()) == 1.0 and model.lambda_reg == 50.0 and "lambda_reg" not in dict(model.named_parameters())
    assert type(model.loss_fn).__name__ == "CrossEntropyLoss"
    sd = synthetic.resnet10_state_dict(seed=27, prefix="feature.")
    sd.update(synthetic.metaoptnet_head_state(27))
    assert list(sd.keys()) == keys
    fresh = MetaOptNet(model_dict['ResNet10'], n_way=5, n_support=5)
    fresh.load_state_dict(sd)
    assert float(fresh.scale.detach()) == float(sd["scale"])


def test_dropin_alias_exports_metaoptnet():
    import importlib.util
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.path.join(here, "meta-fine-tuning_amd", "dropin", "methods", "metaoptnet.py")
    spec = importlib.util.spec_from_file_location("_dropin_metaoptnet", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.MetaOptNet is MetaOptNet


@pytest.mark.parametrize("n_way,n_support", [(0, 5), (33, 1), (5, 0), (5, 52)])
def test_out_of_range_shapes_raise_value_error(n_way, n_support):
    with pytest.raises(ValueError):
        MetaOptNet(model_dict['ResNet10'], n_way=n_way, n_support=n_support)
    with pytest.raises(ValueError):
        ops.ridge_check(1, n_way, n_support, 3)
    assert ops.ridge_check(1, 5, 50, 2) is None and ops.ridge_check(2, 32, 8, 1) is None
    for bad in (dict(n_query=0), dict(episodes=0), dict(D=510)):
        a = dict(episodes=1, n_way=5, n_support=5, n_query=16, D=512)
        a.update(bad)
        with pytest.raises(ValueError):
            ops.ridge_check(a["episodes"], a["n_way"], a["n_support"], a["n_query"], a["D"])


def test_cpu_tensor_into_the_head_raises_runtime_error():
    feats = torch.zeros(5 * 21, 512)
    with pytest.raises(RuntimeError):
        AG.metaoptnet_head(feats, torch.ones(1), 5, 5, 16)
    with pytest.raises(RuntimeError):
        ops.ridge_forward(feats, torch.ones(1), 1, 5, 5, 16)
    with pytest.raises(RuntimeError):
        ops.ridge_backward(dict(feats=feats, scale=torch.ones(1), shape=(1, 5, 5, 16)), torch.zeros(80, 5))


def test_maml_paths_are_refused():
    model = MetaOptNet(model_dict['ResNet10'], n_way=5, n_support=5)
    with pytest.raises(NotImplementedError):
        model.MAML_update()
    with pytest.raises(NotImplementedError):
        model.set_forward_finetune(torch.zeros(5, 21, 3, 84, 84))
    with pytest.raises(NotImplementedError):
        model.set_forward_loss_finetune(torch.zeros(5, 21, 3, 84, 84))


def test_train_main_refuses_metaoptnet_fine_tune():
    from meta_fine_tuning_amd import train
    with pytest.raises(NotImplementedError, match="metaoptnet"):
        train.main(["--method", "metaoptnet", "--fine_tune", "--stop_epoch", "1"])
