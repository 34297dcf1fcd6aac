"""FEAT (methods/feat.py) on the CPU: the definition restated in float64 against the golden G31, the
module's state-dict keys, initial draws and constants, the shape checks, the registration beside the two pinned method tables, the
refusals of the paths that are not on the HIP path, and the host restatement of the dropout generator."""
import argparse
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

import meta_fine_tuning_amd  # noqa: F401
from meta_fine_tuning_amd import autograd_ops as AG
from meta_fine_tuning_amd import feature_eval, finetune, ops, save_features, synthetic, train
from meta_fine_tuning_amd.io_utils import method_dir_name, model_dict
from meta_fine_tuning_amd.methods.feat import FEAT
from oracle import mft_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import feat_reference as R  # noqa: E402
import test_fwt_cpu as FW  # noqa: E402  (the Philox restatement tests/test_fwt_cpu.py pins with known answers)

HEAD = R.HEAD


def _g31(golden_dir):
    return np.load(os.path.join(golden_dir, "g31_feat.npz"))


def test_float64_chain_reproduces_g31(golden_dir):
    g = _g31(golden_dir)
    torch.set_num_threads(8)
    sd = O.clone_state(synthetic.resnet10_state_dict(seed=31, prefix="feature."), torch.float64)
    hs = synthetic.feat_head_state(31)
    x = synthetic.train_episode(31, 5, 5, 16, 84).double()
    # eval mode: running statistics, no multipliers, no auxiliary term
    with torch.no_grad():
        feats = O.resnet10_forward(sd, x.reshape(-1, *x.shape[2:]), prefix="feature.", train=False)
    scores, reg = R.feat_chain(feats, [hs[k].double() for k in HEAD], 5, 5, 16)
    ref = torch.from_numpy(g["eval_scores"])
    assert reg is None and scores.shape == ref.shape == (80, 5)
    assert float((scores - ref).norm() / ref.norm()) < 1e-9
    # train mode on the forced multipliers
    head = [hs[k].double().requires_grad_(True) for k in HEAD]
    with torch.no_grad():
        feats = O.resnet10_forward(sd, x.reshape(-1, *x.shape[2:]), prefix="feature.")
    feats.requires_grad_(True)
    masks = synthetic.feat_masks(31, 1, 5, 5, 16)
    scores, reg = R.feat_chain(feats, head, 5, 5, 16, train=True, masks=masks)
    for got, key, shape in ((scores, "scores", (80, 5)), (reg, "reg", (105, 5))):
        ref = torch.from_numpy(g[key])
        assert got.shape == ref.shape == shape
        assert float((got.detach() - ref).norm() / ref.norm()) < 1e-9, key
    total, main, aux = R.feat_loss(scores, reg, 5, 5, 16)
    for got, key in ((total, "loss"), (main, "loss_main"), (aux, "loss_aux")):
        assert abs(float(got.detach()) - float(g[key])) < 1e-9, key
    assert abs(float(g["loss"]) - (float(g["loss_main"]) + 0.01 * float(g["loss_aux"]))) < 1e-12
    total.backward()
    names = [str(n) for n in g["gradnames"]]
    for k, p in zip(HEAD, head):
        if p.dim() == 2:
            want, got = torch.from_numpy(g["headgrad_rows:" + k]), p.grad[::32]
        else:
            want, got = torch.from_numpy(g["headgrad:" + k]), p.grad
        assert float((got - want).norm()) <= 1e-8 * float(want.norm()), k
        assert abs(float(p.grad.norm()) - float(g["gradnorms"][names.index(k)])) <= 1e-8 * float(p.grad.norm()), k
    # nothing underflows: the scores are of order ten and every head gradient has a usable size
    assert -20.0 < float(g["eval_scores"].min()) and float(g["eval_scores"].max()) < -1.0
    assert all(1e-3 < float(p.grad.norm()) < 2.0 for p in head)


def test_multipliers_and_one_token_sets():
    g = torch.Generator().manual_seed(5)
    hs = synthetic.feat_head_state(31)
    head = [hs[k].double() for k in HEAD]
    X = torch.randn(3, 1, 512, generator=g, dtype=torch.float64)
    taps = []
    R.set_to_set(X.clone().requires_grad_(True), [h.clone().requires_grad_(True) for h in head], taps=taps)
    assert torch.equal(taps[0]["o"], taps[0]["v"]) and bool((taps[0]["P"] == 1).all())         # t = 1 is the identity
    X = torch.randn(2, 4, 512, generator=g, dtype=torch.float64)
    A = R.set_to_set(X, head, m_out=torch.zeros(2, 4, 512, dtype=torch.float64))
    assert torch.allclose(A, torch.nn.functional.layer_norm(X, (512,), head[3], head[4], 1e-5), rtol=0, atol=1e-12)
    m_att, m_out = synthetic.feat_masks(31, 1, 5, 5, 16)
    assert m_att.shape == (25 + 5 * 21 * 21,) and m_out.shape == (5 + 105, 512)
    assert set(np.unique(m_out.numpy())) == {np.float32(0), np.float32(2)}
    assert set(np.unique(m_att.numpy())) == {np.float32(0), np.float32(1.0 / (1.0 - float(np.float32(0.1))))}
    again = synthetic.feat_masks(31, 1, 5, 5, 16)
    assert torch.equal(again[0], m_att) and torch.equal(again[1], m_out)


def test_state_dict_keys_initial_values_and_rng_position(golden_dir):
    g = _g31(golden_dir)
    keys = [str(k) for k in g["state_keys"]]
    torch.manual_seed(1234)
    model = FEAT(model_dict['ResNet10'], n_way=5, n_support=5)
    after = torch.get_rng_state()
    assert list(model.state_dict().keys()) == keys
    assert keys[-7:] == HEAD == list(synthetic.FEAT_HEAD_KEYS) and all(k.startswith("feature.") for k in keys[:-7])
    assert [n for n, _ in model.named_parameters() if not n.startswith("feature.")] == HEAD
    assert [tuple(model.state_dict()[k].shape) for k in HEAD] == [(512, 512)] * 3 + [(512,), (512,), (512, 512), (512,)]
    a = model.slf_attn
    assert bool((a.layer_norm.weight == 1).all()) and bool((a.layer_norm.bias == 0).all()) and a.layer_norm.eps == 1e-5
    assert a.w_qs.bias is None and a.w_ks.bias is None and a.w_vs.bias is None
    with pytest.raises(NotImplementedError):
        a(torch.zeros(1, 5, 512))
    # the constants are class attributes and not state-dict entries
    assert (FEAT.TEMPERATURE, FEAT.TEMPERATURE2, FEAT.BALANCE, FEAT.P_ATT, FEAT.P_OUT) == (64.0, 32.0, 0.01, 0.1, 0.5)
    assert (FEAT.METHOD, FEAT.ENGINE_MODE) == ("feat", None)
    assert not any(c in k for k in keys for c in ("TEMPERATURE", "BALANCE", "P_ATT", "P_OUT", "draw_index"))
    assert type(model.loss_fn).__name__ == "CrossEntropyLoss"
    # the torch RNG stands where the backbone's draws followed by the head's five random draws, in state-dict order, leave it
    torch.manual_seed(1234)
    model_dict['ResNet10']()
    std = math.sqrt(2.0 / 1024.0)
    drawn = [nn.init.normal_(torch.empty(512, 512), 0.0, std) for _ in range(3)]
    drawn.append(nn.init.xavier_normal_(torch.empty(512, 512)))
    drawn.append(nn.init.uniform_(torch.empty(512), -1.0 / math.sqrt(512.0), 1.0 / math.sqrt(512.0)))
    assert torch.equal(torch.get_rng_state(), after)
    for t, p in zip(drawn, (a.w_qs.weight, a.w_ks.weight, a.w_vs.weight, a.fc.weight, a.fc.bias)):
        assert torch.equal(t, p.detach())
    for w in drawn[:4]:
        assert abs(float(w.std()) - std) < 0.02 * std
    sd = synthetic.resnet10_state_dict(seed=31, prefix="feature.")
    sd.update(synthetic.feat_head_state(31))
    assert list(sd.keys()) == keys
    fresh = FEAT(model_dict['ResNet10'], n_way=5, n_support=5)
    fresh.load_state_dict(sd)
    assert torch.equal(fresh.slf_attn.fc.weight.detach(), sd["slf_attn.fc.weight"])


def test_feat_check_bounds():
    for args in [(1, 5, 5, 16), (4, 5, 20, 15), (1, 5, 50, 16), (1, 5, 50, 15), (1, 5, 20, 16), (1, 5, 5, 15), (1, 32, 1, 1), (1, 1, 1, 1),
                 (100, 5, 5, 15), (1, 1, 127, 1)]:
        assert ops.feat_check(*args) is None
    for args, word in [((1, 0, 5, 16), "n_way"), ((1, 33, 1, 1), "n_way"), ((1, 5, 0, 16), "n_support"), ((1, 5, 5, 0), "n_query"),
                       ((0, 5, 5, 16), "episodes"), ((1, 5, 113, 16), "128"), ((1, 1, 128, 1), "128"), ((4000, 32, 64, 64), "token rows")]:
        with pytest.raises(ValueError, match=word):
            ops.feat_check(*args)
    with pytest.raises(ValueError, match="D = 512"):
        ops.feat_check(1, 5, 5, 16, D=256)
    with pytest.raises(ValueError):
        FEAT(model_dict['ResNet10'], n_way=33, n_support=1)
    model = FEAT(model_dict['ResNet10'], n_way=5, n_support=50)
    assert model._check(16) is None and model._check(78) is None
    with pytest.raises(ValueError, match="T = n_support"):
        model._check(79)
    assert ops.feat_counts(1, 5, 5, 16, True) == (5 + 105, 25 + 5 * 441) and ops.feat_counts(2, 5, 5, 16, False) == (10, 50)


def test_directory_names_and_head_flag():
    assert method_dir_name("feat") == "feat"
    with pytest.raises(ValueError, match="metaoptnet"):
        method_dir_name("feat", "svm")
    p = argparse.Namespace(dataset="miniImageNet", model="ResNet10", method="feat", head="ridge", train_aug=True, train_n_way=5, n_shot=5,
                           save_iter=-1, split="novel")
    assert save_features.checkpoint_dir(p).endswith("checkpoints/miniImageNet/ResNet10_feat_aug_5way_5shot")
    assert save_features.features_file(p).endswith("features/miniImageNet/ResNet10_feat_aug_5way_5shot/novel.npz")
    assert save_features.check_method("feat") is None and "feat" in save_features.METHODS
    with pytest.raises(ValueError):
        feature_eval.build_model("feat", model_dict['ResNet10'], 5, 5, head="svm")


def test_the_pinned_tables_are_unchanged_and_feat_resolves_through_the_lookup():
    assert list(train.HEAD_METHODS) == ["protonet", "matchingnet", "metaoptnet"]
    assert finetune.EPISODIC_METHODS == ("gnnnet",) + tuple(train.HEAD_METHODS)
    assert list(train.TRANSDUCTIVE_METHODS) == ["tpn"]
    assert train.EMBEDDING_METHODS == {"feat": FEAT}
    assert train.head_method("feat") is FEAT and train.head_method("tpn") is train.TRANSDUCTIVE_METHODS["tpn"]
    assert train.head_method("protonet") is train.HEAD_METHODS["protonet"]
    assert train.head_method("gnnnet") is None and train.head_method("baseline") is None
    model = feature_eval.build_model("feat", model_dict['ResNet10'], 5, 5)
    assert type(model) is FEAT and model.n_way == 5 and model.n_support == 5


def test_refusals():
    with pytest.raises(NotImplementedError, match="first-order-MAML"):
        train.main(["--method", "feat", "--fine_tune", "--stop_epoch", "1"])
    with pytest.raises(ValueError, match="metaoptnet"):
        train.main(["--method", "feat", "--head", "svm", "--stop_epoch", "1"])
    model = FEAT(model_dict['ResNet10'], n_way=5, n_support=5)
    for call in (model.MAML_update, lambda: model.set_forward_finetune(torch.zeros(5, 21, 3, 84, 84)),
                 lambda: model.set_forward_loss_finetune(torch.zeros(5, 21, 3, 84, 84))):
        with pytest.raises(NotImplementedError):
            call()
    liz = [torch.zeros(5, 20, 3, 84, 84)] * 2
    finetune.params = argparse.Namespace(model="ResNet10", fine_tune_epoch=1)
    with pytest.raises(NotImplementedError, match="score the method with `test`"):
        finetune.finetune(liz, None, model, {}, None, n_way=5, n_support=5)
    with pytest.raises(NotImplementedError, match="score the method with `test`"):
        finetune.finetune_batched([liz], model, {}, 1, 5, 5)
    with pytest.raises(NotImplementedError, match="score the method with `test`"):
        finetune.evaluate(model, {}, 1, 5, 5, 15, 84, 0, 1, method="feat")
    with pytest.raises(NotImplementedError, match="score the method with `test`"):
        finetune.main(["--method", "feat"])


def test_dropin_alias_exports_feat():
    import importlib.util
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.path.join(here, "meta-fine-tuning_amd", "dropin", "methods", "feat.py")
    spec = importlib.util.spec_from_file_location("_dropin_feat", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.FEAT is FEAT


def test_cpu_tensors_raise_runtime_error():
    feats = torch.zeros(5 * 21, 512)
    hs = synthetic.feat_head_state(31)
    head = tuple(hs[k] for k in HEAD)
    with pytest.raises(RuntimeError):
        AG.feat_head(feats, head, 5, 5, 16)
    with pytest.raises(RuntimeError):
        ops.feat_forward(feats, head, 1, 5, 5, 16, False)
    with pytest.raises(RuntimeError):
        ops.feat_draw(1, 5, 5, 16, 0, torch.zeros(1, dtype=torch.int64))


def test_host_philox_restatement_agrees_with_the_trusted_one():
    rs = np.random.RandomState(3)
    ctr = rs.randint(0, 2 ** 32, size=(16, 4), dtype=np.uint64).astype(np.uint32)
    key = rs.randint(0, 2 ** 32, size=(16, 2), dtype=np.uint64).astype(np.uint32)
    assert np.array_equal(R.philox4x32_10(ctr, key), FW.philox4x32_10(ctr, key))
    got = ["%08x" % v for v in R.philox4x32_10(np.array([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], dtype=np.uint32),
                                                np.array([0xA4093822, 0x299F31D0], dtype=np.uint32))]
    assert got == ["d16cfe09", "94fdcceb", "5001e420", "24126ea1"]
    # the draw's counter layout: (element low, element high | mask id << 31, index low, index high), key = seed; word 0
    seed, index = 0x0123456789ABCDEF, (7 << 32) | 9
    for mask_id in (0, 1):
        w = R.draw_words(seed, index, mask_id, 4)
        for i in range(4):
            one = FW.philox4x32_10(np.array([i, mask_id << 31, 9, 7], dtype=np.uint32), np.array([0x89ABCDEF, 0x01234567], dtype=np.uint32))
            assert int(w[i]) == int(one[0])
    m_att, m_out = R.draw_masks(seed, index, 1, 3, 2, 3)
    assert m_att.shape == (9 + 75,) and m_out.shape == (18, 512)
    assert 0.4 < float((m_out == 0).mean()) < 0.6 and 0.0 < float((m_att == 0).mean()) < 0.3
