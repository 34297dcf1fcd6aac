"""ProtoNet on a real MI355X: the prototype-head kernels (mft_proto_scores / mft_proto_backward) against float64, the
meta-training step against the float64 oracle and the reference's golden G22, lockstep episodes, the graphed episode loop, the
test-time engine (FinetuneEngine(mode="proto")) and the train.main --method protonet driver."""
import argparse
import copy
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import meta_fine_tuning_amd  # noqa: F401
from meta_fine_tuning_amd import _lib, ops, synthetic
from meta_fine_tuning_amd import finetune as ft
from meta_fine_tuning_amd.io_utils import model_dict
from meta_fine_tuning_amd.methods.protonet import ProtoNet
from oracle import mft_oracle as O

pytestmark = pytest.mark.gpu
torch.set_num_threads(8)


def _g22(golden_dir):
    return np.load(os.path.join(golden_dir, "g22_protonet.npz"))


def head64(feats, n_way, n_support, n_query, episodes=1):
    """protonet.py set_forward on feature rows [episodes*n_way*(n_support+n_query), D], in float64 (direct form)."""
    z = feats.double().view(episodes, n_way, n_support + n_query, -1)
    out = []
    for e in range(episodes):
        proto = z[e, :, :n_support].mean(1)
        q = z[e, :, n_support:].reshape(n_way * n_query, -1)
        out.append(-((q[:, None, :] - proto[None, :, :]) ** 2).sum(2))
    return torch.cat(out)


# ------------------------------------------------------------------------------------------------ kernels
SHAPES = [(5, 5, 15, 1), (5, 5, 16, 3), (2, 1, 1, 1), (20, 5, 16, 1), (32, 1, 16, 2), (64, 5, 5, 1)]


@pytest.mark.parametrize("n_way,ns,nq,E", SHAPES)
def test_kernels_match_float64(n_way, ns, nq, E):
    g = torch.Generator().manual_seed(n_way * 1000 + ns * 100 + nq * 10 + E)
    rows = E * n_way * (ns + nq)
    f_cpu = torch.randn(rows, 512, generator=g)
    f = f_cpu.cuda()
    sc = ops.proto_scores(f, E, n_way, ns, nq)
    ref = head64(f_cpu, n_way, ns, nq, E)
    assert sc.shape == (E * n_way * nq, n_way)
    err = (sc.cpu().double() - ref).abs() / ref.abs()
    assert float(err.max()) < 5e-6, float(err.max())
    # backward: d(sum(scores * G)) / d(feats) against float64 autograd, relative L2 per episode
    G = torch.randn(E * n_way * nq, n_way, generator=g)
    d = ops.proto_backward(f, G.cuda(), E, n_way, ns, nq)
    f64 = f_cpu.double().requires_grad_(True)
    (head64(f64, n_way, ns, nq, E) * G.double()).sum().backward()
    per = n_way * (ns + nq)
    for e in range(E):
        want = f64.grad[e * per:(e + 1) * per]
        got = d[e * per:(e + 1) * per].cpu().double()
        assert float((got - want).norm() / want.norm()) < 1e-5, e
    # two calls: bit-identical
    assert torch.equal(sc, ops.proto_scores(f, E, n_way, ns, nq))
    assert torch.equal(d, ops.proto_backward(f, G.cuda(), E, n_way, ns, nq))
    # softmax epilogue (features scaled so that the softmax is not one-hot)
    fs_cpu = f_cpu * 0.05
    sm = ops.proto_scores(fs_cpu.cuda(), E, n_way, ns, nq, softmax=True)
    want = torch.softmax(head64(fs_cpu, n_way, ns, nq, E), dim=1)
    assert float((sm.cpu().double() - want).abs().max()) < 2e-5
    assert torch.equal(sm, ops.proto_scores(fs_cpu.cuda(), E, n_way, ns, nq, softmax=True))


def test_out_of_range_shapes_are_refused():
    lib = _lib.lib()
    f = torch.zeros(66 * 2, 520, device="cuda")
    s = torch.zeros(66 * 66, device="cuda")
    ok = lib.mft_proto_scores(ops._p(f), 512, 1, 5, 5, 16, 512, ops._p(s), 0, ops._stream(f))
    assert ok == 0
    bad = [dict(n_way=65), dict(n_way=0), dict(ns=0), dict(nq=0), dict(D=516, ld=520), dict(D=510), dict(ld=500), dict(ld=514),
           dict(E=0)]
    for b in bad:
        a = dict(ld=512, E=1, n_way=5, ns=5, nq=16, D=512)
        a.update(b)
        rc = lib.mft_proto_scores(ops._p(f), a["ld"], a["E"], a["n_way"], a["ns"], a["nq"], a["D"], ops._p(s), 0, ops._stream(f))
        assert rc == -22, b
        rc = lib.mft_proto_backward(ops._p(f), a["ld"], a["E"], a["n_way"], a["ns"], a["nq"], a["D"], ops._p(s), max(a["n_way"], 1),
                                    ops._p(f), a["ld"], ops._stream(f))
        assert rc == -22, b
    with pytest.raises(ValueError):
        ops.proto_scores(torch.zeros(100, 512, device="cuda"), 1, 5, 5, 16)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ meta-training step
def _oracle(sd32, xs):
    """float64 loss (mean over the episodes of xs [k, n_way, S+Q, 3, H, W]) and gradients of every feature parameter."""
    sd = O.clone_state(sd32, torch.float64)
    pkeys = [k for k, v in sd.items() if v.is_floating_point() and "running" not in k]
    for k in pkeys:
        sd[k].requires_grad_(True)
    n_way, per = xs.shape[1], xs.shape[2]
    losses = []
    for x in xs:
        feats = O.resnet10_forward(sd, x.double().reshape(-1, *x.shape[2:]), prefix="feature.")
        sc = head64(feats, n_way, 5, per - 5)
        losses.append(F.cross_entropy(sc, torch.from_numpy(np.repeat(np.arange(n_way), per - 5))))
    loss = torch.stack(losses).mean()
    grads = torch.autograd.grad(loss, [sd[k] for k in pkeys])
    return float(loss.detach()), dict(zip(pkeys, grads))


def _check_grads(named, ref):
    # bounds of test_metatrain_gpu.py::test_set_forward_loss_backward_all_parameters (a ReLU whose pre-activation is ~1e-6 may
    # flip in fp32 and perturb a handful of entries)
    for k, gr in ref.items():
        got = named[k].grad
        assert got is not None, k
        nrm = float(gr.norm())
        if nrm < 1e-9:
            assert float(got.norm()) < 1e-5, k
            continue
        rel = float((got.cpu().double() - gr).norm()) / nrm
        mx = float((got.cpu().double() - gr).abs().max()) / float(gr.abs().max())
        assert rel < 3e-2 and mx < 0.15, (k, rel, mx)


def _model(sd, n_way=5):
    m = ProtoNet(model_dict['ResNet10'], n_way=n_way, n_support=5)
    m.load_state_dict(sd)
    m = m.cuda()
    m.train()
    m.n_query = 16
    return m


def test_set_forward_loss_backward_vs_oracle_and_g22(golden_dir):
    g = _g22(golden_dir)
    sd = synthetic.resnet10_state_dict(seed=22, prefix="feature.")
    model = _model(sd)
    x = synthetic.train_episode(22, 5, 5, 16, 84)
    with torch.no_grad():
        sc = model.set_forward(x)
    np.testing.assert_allclose(sc.cpu().numpy(), g["scores"], rtol=1e-3, atol=1e-3)
    loss = model.set_forward_loss(x)
    loss.backward()
    assert abs(float(loss.detach()) - float(g["loss"])) < 2e-4
    ref_loss, ref = _oracle(sd, x[None])
    assert abs(float(loss.detach()) - ref_loss) < 2e-4
    named = dict(model.named_parameters())
    assert set(ref) == set(named)
    _check_grads(named, ref)
    # the reference's own fp32 run: BatchNorm gradients and every gradient's norm
    for name in g["bnnames"]:
        name = str(name)
        want = g["bngrad:" + name]
        got = named[name].grad.cpu().numpy()
        assert np.linalg.norm(got - want) <= 3e-2 * np.linalg.norm(want) + 1e-9, name
    gn = {k: float(p.grad.norm()) for k, p in named.items()}
    for name, refn in zip(g["gradnames"], g["gradnorms"]):
        assert abs(gn[str(name)] - refn) <= 1e-2 * refn + 1e-9, name


def test_lockstep_two_episodes_equal_float64_mean():
    sd = synthetic.resnet10_state_dict(seed=23, prefix="feature.")
    xs = torch.stack([synthetic.train_episode(400 + i, 5, 5, 16, 84) for i in range(2)])
    model = _model(sd)
    scores = model.set_forward_lockstep(xs.cuda())
    assert scores.shape == (2 * 80, 5)
    loss = model.set_forward_loss_lockstep(xs.cuda())
    loss.backward()
    ref_loss, ref = _oracle(sd, xs)
    assert abs(float(loss.detach()) - ref_loss) < 2e-4
    _check_grads(dict(model.named_parameters()), ref)


def test_graphed_episode_loop_is_bit_identical(capsys, monkeypatch):
    from meta_fine_tuning_amd import graph_step, optim
    eps = [synthetic.train_episode(800 + i, 5, 5, 16, 84) for i in range(6)]

    class Loader:
        def __len__(self):
            return len(eps)

        def __iter__(self):
            for x in eps:
                yield x, None

    def run(graphed):
        monkeypatch.setattr(graph_step, "ENABLED", graphed)
        model = _model(synthetic.resnet10_state_dict(seed=27, prefix="feature."))
        opt = optim.Adam(model.parameters())
        capsys.readouterr()
        model.train_loop(0, Loader(), opt)
        out = capsys.readouterr().out
        st = model.__dict__.get("_mft_graph_steps", {}).get("set_forward_loss")
        return out, [p.detach().clone() for p in model.parameters()], [b.detach().clone() for b in model.buffers()], st

    out_e, par_e, buf_e, st_e = run(False)
    out_g, par_g, buf_g, st_g = run(True)
    assert st_e is None and st_g is not None and st_g.graph is not None and not st_g.failed
    assert out_g == out_e and out_e.count("Loss") == 1
    assert all(torch.equal(a, b) for a, b in zip(par_e, par_g))
    assert all(torch.equal(a, b) for a, b in zip(buf_e, buf_g))


def test_protonet_step_issues_no_aten_device_kernels():
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "method_step_worker.py")
    r = subprocess.run([sys.executable, worker, "protonet"], capture_output=True, text=True, timeout=900)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert lines, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    res = json.loads(lines[-1][len("RESULT "):])
    assert res["n_dev"] > 0 and res["head_n_dev"] == 1, res
    assert not res["aten"] and not res["head_aten"], res


# ------------------------------------------------------------------------------------------------ evaluation
def _proto_model(sd):
    m = ProtoNet(model_dict['ResNet10'], n_way=5, n_support=5)
    m.load_state_dict(sd)
    m.train()
    return m


@pytest.mark.parametrize("E", [0, 1])
def test_finetune_with_protonet_matches_g22(golden_dir, E):
    g = _g22(golden_dir)
    sd = synthetic.resnet10_state_dict(seed=13, prefix="feature.")
    ft.params = argparse.Namespace(model="ResNet10", fine_tune_epoch=E)
    model = _proto_model(sd)
    liz = synthetic.test_episode(41, 5, 5, 15, 84, gen_examples=0)
    np.random.seed(10)
    sc = ft.finetune(liz, None, model, copy.deepcopy(sd), None, n_query=15, n_way=5, n_support=5)
    assert sc.shape == (75, 5) and model.n_query == 15
    ref = g["finetune_scores_E%d" % E]
    if E == 0:
        np.testing.assert_allclose(sc.cpu().numpy(), ref, atol=1e-4)          # forward only: G5's bar
    else:
        # 15 Adam steps on the last block: no two fp32 implementations agree step for step, so G5's bar after adaptation
        # (tests/test_modules_gpu.py::test_finetune_dropin; measured here: 7.7e-4 at most)
        err = np.abs(sc.cpu().numpy() - ref)
        assert err.max() < 3e-2 and (sc.argmax(1).cpu().numpy() == ref.argmax(1)).mean() >= 0.96, err.max()


def test_finetune_batched_equals_single_episode_calls():
    sd = synthetic.resnet10_state_dict(seed=13, prefix="feature.")
    model = _proto_model(sd)
    eps = [synthetic.test_episode(60 + i, 5, 5, 15, 84, gen_examples=1) for i in range(4)]
    ft.params = argparse.Namespace(model="ResNet10", fine_tune_epoch=1)
    np.random.seed(3)
    single = [ft.finetune(ep, None, model, sd, None, n_way=5, n_support=5) for ep in eps]
    np.random.seed(3)
    batched = ft.finetune_batched(eps, model, sd, 1, 5, 5, episodes_per_batch=4)
    assert batched.shape == (4, 75, 5)
    # the same arithmetic per episode, but an engine of one groups the frozen trunk's launches differently (trunk_chunk) and may
    # pick other kernel forms, which moves fp32 rounding through the 20 Adam steps: G5's bar after adaptation
    # (tests/test_modules_gpu.py::test_finetune_dropin; measured up to 2.9e-3 here, and the same 2.9e-3 for a GnnNet model)
    for a, b in zip(single, batched):
        err = float((a - b).abs().max())
        assert err < 3e-2 and float((a.argmax(1) == b.argmax(1)).float().mean()) >= 0.96, err
    # the proto engines are cached apart from gnn engines of the same backbone
    assert any(ent["cfg"][0] == "proto" for ent in ft._ENGINES.entries)


def test_frozen_backbone_branch_runs():
    sd = synthetic.resnet10_state_dict(seed=13, prefix="feature.")
    model = _proto_model(sd)
    ft.params = argparse.Namespace(model="ResNet10", fine_tune_epoch=1)
    liz = synthetic.test_episode(41, 5, 5, 15, 84, gen_examples=0)
    sc = ft.finetune(liz, None, model, sd, None, freeze_backbone=True, n_way=5, n_support=5)
    assert sc.shape == (75, 5)
    torch.testing.assert_close(sc.sum(1).cpu(), torch.ones(75), atol=1e-5, rtol=0)
    # the same scores as the ProtoNet head on the eval-mode features, softmaxed
    feat = ft._eval_backbone(sd, "ResNet10")
    with torch.no_grad():
        f = feat(liz[0].cuda().reshape(-1, 3, 84, 84))
    want = torch.softmax(head64(f.cpu(), 5, 5, 15), dim=1)
    assert float((sc.cpu().double() - want).abs().max()) < 1e-4


def test_evaluate_protonet_with_device_sampler():
    from meta_fine_tuning_amd import augment
    sd = synthetic.resnet10_state_dict(seed=13, prefix="feature.")
    model = _proto_model(sd).cuda()
    pool = synthetic.class_pool_u8("EuroSAT", "cuda:0", seed=1, n_per_class=40)
    sampler = augment.EpisodeSampler(pool, 5, 20, seed=10)
    np.random.seed(10)
    accs = ft.evaluate(model, sd, 2, 5, 5, 15, 84, 2, 1, episodes_per_batch=2, verbose=False, method="protonet", sampler=sampler)
    assert accs.shape == (2,) and np.all((accs >= 0) & (accs <= 100))


# ------------------------------------------------------------------------------------------------ CLI
def test_train_main_protonet_writes_a_loadable_checkpoint(golden_dir, tmp_path, monkeypatch):
    from meta_fine_tuning_amd import configs, train
    g = _g22(golden_dir)
    monkeypatch.setattr(configs, "save_dir", str(tmp_path))
    train.main(["--dataset", "miniImageNet", "--method", "protonet", "--model", "ResNet10", "--stop_epoch", "1"], n_episode=2, size=84)
    f = tmp_path / "checkpoints" / "miniImageNet" / "ResNet10_protonet_5way_5shot" / "0.tar"
    assert f.is_file()
    state = torch.load(str(f), map_location="cpu")["state"]
    assert list(state.keys()) == [str(k) for k in g["state_keys"]]
    fresh = ProtoNet(model_dict['ResNet10'], n_way=5, n_support=5)
    fresh.load_state_dict(state)
    assert list(fresh.state_dict().keys()) == [str(k) for k in g["state_keys"]]
