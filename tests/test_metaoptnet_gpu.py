"""MetaOptNet on a real MI355X: the ridge-regression head kernels (csrc/ridge.hip) against float64 with the float32 CPU chain as
the yardstick, the meta-training step against the float64 oracle and the golden G27, lockstep episodes, the graphed episode loop,
the test-time engine (FinetuneEngine(mode="ridge")) and the train.main --method metaoptnet driver."""
import argparse
import copy
import functools
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
from meta_fine_tuning_amd.methods.metaoptnet import MetaOptNet
from oracle import mft_oracle as O

pytestmark = pytest.mark.gpu
torch.set_num_threads(8)

LAMBDA = 50.0


def _g27(golden_dir):
    return np.load(os.path.join(golden_dir, "g27_metaoptnet.npz"))


def head_chain(feats, scale, n_way, n_support, n_query, episodes=1):
    """DESIGN.md section 14 on feature rows [episodes*n_way*(n_support+n_query), D] in the dtype of ``feats`` (float64: the
    reference; float32: the yardstick), with torch's cholesky / cholesky_solve; differentiable in feats and scale."""
    z = feats.view(episodes, n_way, n_support + n_query, -1)
    S = n_way * n_support
    Y = torch.zeros(S, n_way, dtype=feats.dtype)
    Y[torch.arange(S), torch.arange(S) // n_support] = 1.0
    out = []
    for e in range(episodes):
        zs = z[e, :, :n_support].reshape(S, -1)
        zq = z[e, :, n_support:].reshape(n_way * n_query, -1)
        A = zs @ zs.t() + LAMBDA * torch.eye(S, dtype=feats.dtype)
        alpha = 2.0 * torch.cholesky_solve(Y, torch.linalg.cholesky(A))
        out.append(scale * (zq @ (zs.t() @ alpha)))
    return torch.cat(out)


def head64(feats, scale, n_way, n_support, n_query, episodes=1):
    with torch.no_grad():
        return head_chain(feats.double(), torch.as_tensor(scale).double(), n_way, n_support, n_query, episodes)


# ------------------------------------------------------------------------------------------------ kernels
# (E, n_way, n_support, n_query): every tile edge of the Gram launch, S = 1, the 64 boundary, the packed-triangle limit S = 256,
# n_way = 32 and the multi-episode stride
SHAPES = [(1, 5, 5, 16), (1, 2, 1, 1), (2, 1, 1, 2), (3, 3, 2, 3), (2, 5, 1, 15), (1, 5, 13, 2), (1, 5, 20, 3), (1, 5, 50, 2),
          (1, 32, 8, 1), (1, 32, 1, 1)]
KINDS = ["randn", "relu"]
DRAWS = 3
SCALE = 0.8125


def _features(kind, shape, draw):
    E, n_way, ns, nq = shape
    g = torch.Generator().manual_seed(1000003 * draw + 7919 * E + 131 * n_way + 17 * ns + nq + (0 if kind == "randn" else 500000))
    f = torch.randn(E, n_way, ns + nq, 512, generator=g)
    if kind == "relu":          # non-negative and class-structured, as trunk outputs are
        mean = torch.randn(E, n_way, 1, 512, generator=g)
        f = torch.relu(0.5 * f + 0.5 * mean + 0.3)
    G = torch.randn(E * n_way * nq, n_way, generator=g)
    return f.reshape(-1, 512).contiguous(), G


def _chain_step(f, G, shape, dtype):
    E, n_way, ns, nq = shape
    x = f.to(dtype).requires_grad_(True)
    sc = torch.tensor([SCALE], dtype=dtype, requires_grad=True)
    scores = head_chain(x, sc, n_way, ns, nq, E)
    (scores * G.to(dtype)).sum().backward()
    return scores.detach().double(), x.grad.double(), float(sc.grad.double())


def _rel_per_episode(got, want, E):
    got, want = got.reshape(E, -1), want.reshape(E, -1)
    return [float((got[e] - want[e]).norm() / want[e].norm()) for e in range(E)]


@functools.lru_cache(maxsize=None)
def _references():
    """Every (shape, kind, draw): inputs, the float64 step and the yardstick = the distance of the float32 CPU chain to float64.
    Computed once for the module and never modified."""
    refs, dscale_yard = {}, 0.0
    for shape in SHAPES:
        E = shape[0]
        for kind in KINDS:
            for draw in range(DRAWS):
                f, G = _features(kind, shape, draw)
                s64, d64, ds64 = _chain_step(f, G, shape, torch.float64)
                s32, d32, ds32 = _chain_step(f, G, shape, torch.float32)
                denom = float((G.double() * s64 / SCALE).abs().sum())
                refs[(shape, kind, draw)] = dict(f=f, G=G, scores=s64, dfeats=d64, dscale=ds64, dscale_denom=denom,
                                                 y_scores=max(_rel_per_episode(s32, s64, E)),
                                                 y_dfeats=max(_rel_per_episode(d32, d64, E)))
                dscale_yard = max(dscale_yard, abs(ds32 - ds64) / denom)
    return refs, dscale_yard


def _run_head(f, G, shape):
    E, n_way, ns, nq = shape
    scale = torch.tensor([SCALE], device="cuda")
    scores, tape = ops.ridge_forward(f, scale, E, n_way, ns, nq, save=True)
    dfeats, dscale = ops.ridge_backward(tape, G)
    return scores, dfeats, dscale


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "E%d_w%d_s%d_q%d" % s)
def test_kernels_match_float64_within_4x_the_float32_chain(shape, kind):
    refs, dscale_yard = _references()
    E, n_way, ns, nq = shape
    y_scores = max(refs[(shape, kind, d)]["y_scores"] for d in range(DRAWS))
    y_dfeats = max(refs[(shape, kind, d)]["y_dfeats"] for d in range(DRAWS))
    for draw in range(DRAWS):
        r = refs[(shape, kind, draw)]
        scores, dfeats, dscale = _run_head(r["f"].cuda(), r["G"].cuda(), shape)
        assert scores.shape == (E * n_way * nq, n_way) and dfeats.shape == r["f"].shape and dscale.shape == (1,)
        e_s = max(_rel_per_episode(scores.cpu().double(), r["scores"], E))
        e_d = max(_rel_per_episode(dfeats.cpu().double(), r["dfeats"], E))
        e_c = abs(float(dscale.cpu().double()) - r["dscale"]) / r["dscale_denom"]
        print("ridge %s %s draw %d: scores %.3e (yardstick %.3e, ratio %.2f)  dfeats %.3e (yardstick %.3e, ratio %.2f)  "
              "dscale %.3e (yardstick %.3e, ratio %.2f)" % (shape, kind, draw, e_s, y_scores, e_s / y_scores, e_d, y_dfeats,
                                                            e_d / y_dfeats, e_c, dscale_yard, e_c / dscale_yard))
        assert e_s <= 4.0 * y_scores, (draw, e_s, y_scores)
        assert e_d <= 4.0 * y_dfeats, (draw, e_d, y_dfeats)
        assert e_c <= 4.0 * dscale_yard, (draw, e_c, dscale_yard)


@pytest.mark.parametrize("shape", [(3, 3, 2, 3), (1, 5, 50, 2), (1, 32, 8, 1)], ids=lambda s: "E%d_w%d_s%d_q%d" % s)
def test_two_calls_are_bit_identical(shape):
    r = _references()[0][(shape, "relu", 0)]
    f, G = r["f"].cuda(), r["G"].cuda()
    a, b = _run_head(f, G, shape), _run_head(f, G, shape)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    E, n_way, ns, nq = shape
    scale = torch.tensor([SCALE], device="cuda")
    s1 = ops.ridge_forward(f, scale, E, n_way, ns, nq, softmax=True)[0]
    assert torch.equal(s1, ops.ridge_forward(f, scale, E, n_way, ns, nq, softmax=True)[0])


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "E%d_w%d_s%d_q%d" % s)
def test_softmax_epilogue(shape):
    r = _references()[0][(shape, "relu", 1)]
    E, n_way, ns, nq = shape
    sm = ops.ridge_forward(r["f"].cuda(), torch.tensor([SCALE], device="cuda"), E, n_way, ns, nq, softmax=True)[0]
    want = torch.softmax(r["scores"], dim=1)
    assert float((sm.cpu().double() - want).abs().max()) < 2e-5
    if n_way > 1:               # scores of these features stay small: the softmax is not one-hot
        assert float(want.max()) < 0.999


def test_non_finite_features_give_non_finite_output():
    f = _references()[0][((1, 5, 5, 16), "relu", 0)]["f"].clone()
    f[3, 7] = float("nan")
    scores = ops.ridge_forward(f.cuda(), torch.tensor([SCALE], device="cuda"), 1, 5, 5, 16)[0]
    torch.cuda.synchronize()
    assert not bool(torch.isfinite(scores).all())


def test_out_of_range_arguments_are_refused():
    lib = _lib.lib()
    f = torch.zeros(300, 520, device="cuda")
    ws = torch.zeros(7, 1 << 16, device="cuda")         # A, alpha, W, scores, dscores, dW, dfeats of the one accepted call
    part = torch.zeros(64, device="cuda", dtype=torch.float64)
    scale = torch.ones(1, device="cuda")
    st = ops._stream(f)

    def call_all(a):
        p = ops._p
        head = (p(f), a["ld"], a["E"], a["n_way"], a["ns"], a["nq"], a["D"])
        A, alpha, W, scores, G, dW, dfeats = ws
        return [lib.mft_ridge_gram(*head, 50.0, p(A), st),
                lib.mft_ridge_factor_solve(*head, p(A), p(alpha), p(W), st),
                lib.mft_ridge_scores(*head, p(W), p(scale), p(scores), 0, st),
                lib.mft_ridge_backward_query(*head, p(W), p(scale), p(G), max(a["n_way"], 1), p(dfeats), 512, p(dW), p(part), st),
                lib.mft_ridge_backward_support(*head, p(A), p(alpha), p(W), p(dW), p(part), p(dfeats), 512, p(scale), st)]

    good = dict(ld=520, E=1, n_way=5, ns=5, nq=16, D=512)
    assert call_all(good) == [0, 0, 0, 0, 0]
    bad = [dict(n_way=0), dict(n_way=33, ns=1), dict(n_way=1, ns=257), dict(n_way=16, ns=17), dict(nq=0), dict(E=0), dict(D=510),
           dict(D=516), dict(ld=500), dict(ld=514), dict(ns=0)]
    for b in bad:
        a = dict(good)
        a.update(b)
        assert call_all(a) == [-22] * 5, b
    torch.cuda.synchronize()
    z = lambda *s: torch.zeros(*s, device="cuda")  # noqa: E731
    for args in [(z(0, 512), 1, 0, 5, 16), (z(33 * 2, 512), 1, 33, 1, 1), (z(258, 512), 1, 1, 257, 1), (z(25, 512), 1, 5, 5, 0),
                 (z(0, 512), 0, 5, 5, 16), (z(105, 510), 1, 5, 5, 16), (z(105, 516), 1, 5, 5, 16),
                 (z(105, 514)[:, :512], 1, 5, 5, 16), (z(100, 512), 1, 5, 5, 16)]:
        with pytest.raises(ValueError):
            ops.ridge_forward(args[0], scale, *args[1:])
    tape = ops.ridge_forward(z(105, 512), scale, 1, 5, 5, 16, save=True)[1]
    with pytest.raises(ValueError):
        ops.ridge_backward(tape, z(80, 4))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ meta-training step
def _oracle(sd32, scale, xs):
    """float64 loss (mean over the episodes of xs [k, n_way, S+Q, 3, H, W]) and gradients of every parameter, ``scale`` included."""
    sd = O.clone_state(sd32, torch.float64)
    sd["scale"] = scale.double().clone()
    pkeys = [k for k, v in sd.items() if v.is_floating_point() and "running" not in k]
    for k in pkeys:
        sd[k].requires_grad_(True)
    n_way, per = xs.shape[1], xs.shape[2]
    losses = []
    for x in xs:
        feats = O.resnet10_forward(sd, x.double().reshape(-1, *x.shape[2:]), prefix="feature.")
        sc = head_chain(feats, sd["scale"], n_way, 5, per - 5)
        losses.append(F.cross_entropy(sc, torch.from_numpy(np.repeat(np.arange(n_way), per - 5))))
    loss = torch.stack(losses).mean()
    grads = torch.autograd.grad(loss, [sd[k] for k in pkeys])
    return float(loss.detach()), dict(zip(pkeys, grads))


def _check_grads(named, ref):
    # bounds of tests/test_protonet_gpu.py::_check_grads (the trunk backward is the same code)
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


def _state(seed):
    sd = synthetic.resnet10_state_dict(seed=seed, prefix="feature.")
    sd.update(synthetic.metaoptnet_head_state(27))
    return sd


def _model(sd, n_way=5):
    m = MetaOptNet(model_dict['ResNet10'], n_way=n_way, n_support=5)
    m.load_state_dict(sd)
    m = m.cuda()
    m.train()
    m.n_query = 16
    return m


def test_set_forward_loss_backward_vs_oracle_and_g27(golden_dir):
    g = _g27(golden_dir)
    sd = _state(27)
    model = _model(sd)
    x = synthetic.train_episode(27, 5, 5, 16, 84)
    with torch.no_grad():
        sc = model.set_forward(x)
    np.testing.assert_allclose(sc.cpu().numpy(), g["scores"], rtol=1e-3, atol=1e-3)
    loss = model.set_forward_loss(x)
    loss.backward()
    assert abs(float(loss.detach()) - float(g["loss"])) < 2e-4
    ref_loss, ref = _oracle(sd, sd["scale"], x[None])
    assert abs(ref_loss - float(g["loss"])) < 1e-9
    assert abs(float(loss.detach()) - ref_loss) < 2e-4
    named = dict(model.named_parameters())
    assert set(ref) == set(named)
    _check_grads(named, ref)
    # d(loss)/d(scale): within 4x the distance of the float32 CPU step to float64 (G27 (e))
    want = float(g["scalegrad"][0])
    assert abs(float(ref["scale"]) - want) < 1e-9 * abs(want)
    err = abs(float(model.scale.grad.cpu().double()) - want) / abs(want)
    print("metaoptnet step: dscale rel err %.3e, G27 float32 distance %.3e, ratio %.2f"
          % (err, float(g["f32err:scalegrad"]), err / float(g["f32err:scalegrad"])))
    assert err <= 4.0 * float(g["f32err:scalegrad"]), (err, float(g["f32err:scalegrad"]))
    # G27 (b): BatchNorm gradients and every gradient's norm
    for name in g["bnnames"]:
        name = str(name)
        want = g["bngrad:" + name]
        got = named[name].grad.cpu().numpy()
        assert np.linalg.norm(got - want) <= 3e-2 * np.linalg.norm(want) + 1e-9, name
    gn = {k: float(p.grad.norm()) for k, p in named.items()}
    for name, refn in zip(g["gradnames"], g["gradnorms"]):
        assert abs(gn[str(name)] - refn) <= 1e-2 * refn + 1e-9, name


def test_lockstep_two_episodes_equal_float64_mean():
    sd = _state(23)
    xs = torch.stack([synthetic.train_episode(400 + i, 5, 5, 16, 84) for i in range(2)])
    model = _model(sd)
    scores = model.set_forward_lockstep(xs.cuda())
    assert scores.shape == (2 * 80, 5)
    loss = model.set_forward_loss_lockstep(xs.cuda())
    loss.backward()
    ref_loss, ref = _oracle(sd, sd["scale"], xs)
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
        model = _model(_state(27))
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
    assert float(par_g[0].cpu()) != float(_state(27)["scale"])          # ``scale`` is the first parameter, and it was trained


def test_metaoptnet_step_issues_no_aten_device_kernels():
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "method_step_worker.py")
    r = subprocess.run([sys.executable, worker, "metaoptnet"], capture_output=True, text=True, timeout=900)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert lines, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    res = json.loads(lines[-1][len("RESULT "):])
    assert res["n_dev"] > 0 and res["head_n_dev"] == 3, res
    assert not res["aten"] and not res["head_aten"], res
    assert res["head_step_n_dev"] == res["head_step_n_dev_50shot"] > res["head_n_dev"] and not res["head_step_aten"], res


# ------------------------------------------------------------------------------------------------ evaluation
def _eval_model(sd):
    m = MetaOptNet(model_dict['ResNet10'], n_way=5, n_support=5)
    full = dict(sd)
    full.update(synthetic.metaoptnet_head_state(27))
    m.load_state_dict(full)
    m.train()
    return m


@pytest.mark.parametrize("E", [0, 1])
def test_finetune_with_metaoptnet_matches_g27(golden_dir, E):
    g = _g27(golden_dir)
    sd = synthetic.resnet10_state_dict(seed=13, prefix="feature.")
    ft.params = argparse.Namespace(model="ResNet10", fine_tune_epoch=E)
    model = _eval_model(sd)
    liz = synthetic.test_episode(41, 5, 5, 15, 84, gen_examples=0)
    np.random.seed(10)
    sc = ft.finetune(liz, None, model, copy.deepcopy(sd), None, n_query=15, n_way=5, n_support=5)
    assert sc.shape == (75, 5) and model.n_query == 15
    ref = g["finetune_scores_E%d" % E]
    if E == 0:
        np.testing.assert_allclose(sc.cpu().numpy(), ref, atol=1e-4)          # forward only: G5's bar
    else:
        # 15 Adam steps on the last block: G5's bar after adaptation (tests/test_modules_gpu.py::test_finetune_dropin)
        err = np.abs(sc.cpu().numpy() - ref)
        print("metaoptnet finetune E=1: max err %.3e" % err.max())
        assert err.max() < 3e-2 and (sc.argmax(1).cpu().numpy() == ref.argmax(1)).mean() >= 0.96, err.max()


def test_finetune_batched_equals_single_episode_calls():
    sd = synthetic.resnet10_state_dict(seed=13, prefix="feature.")
    model = _eval_model(sd)
    eps = [synthetic.test_episode(60 + i, 5, 5, 15, 84, gen_examples=1) for i in range(4)]
    ft.params = argparse.Namespace(model="ResNet10", fine_tune_epoch=1)
    np.random.seed(3)
    single = [ft.finetune(ep, None, model, sd, None, n_way=5, n_support=5) for ep in eps]
    np.random.seed(3)
    batched = ft.finetune_batched(eps, model, sd, 1, 5, 5, episodes_per_batch=4)
    assert batched.shape == (4, 75, 5)
    for a, b in zip(single, batched):                    # G5's bar after adaptation, as the ProtoNet test
        err = float((a - b).abs().max())
        assert err < 3e-2 and float((a.argmax(1) == b.argmax(1)).float().mean()) >= 0.96, err
    # the ridge engines are cached apart from gnn engines of the same backbone, keyed on the scale parameter
    mine = ("ridge", (model.scale.data_ptr(), model.scale._version))
    assert any(ent["cfg"][:2] == mine for ent in ft._ENGINES.entries)
    assert not any(ent["cfg"][0] == "gnn" and ent["engine"].mode == "ridge" for ent in ft._ENGINES.entries)


def test_frozen_backbone_branch_equals_the_head_on_eval_features():
    sd = synthetic.resnet10_state_dict(seed=13, prefix="feature.")
    model = _eval_model(sd)
    ft.params = argparse.Namespace(model="ResNet10", fine_tune_epoch=1)
    liz = synthetic.test_episode(41, 5, 5, 15, 84, gen_examples=0)
    sc = ft.finetune(liz, None, model, sd, None, freeze_backbone=True, n_way=5, n_support=5)
    assert sc.shape == (75, 5)
    feat = ft._eval_backbone(sd, "ResNet10")
    with torch.no_grad():
        f = feat(liz[0].cuda().reshape(-1, 3, 84, 84))
    want = torch.softmax(head64(f.cpu(), model.scale.detach().cpu(), 5, 5, 15), dim=1)
    assert float((sc.cpu().double() - want).abs().max()) < 1e-4


def test_evaluate_metaoptnet_with_device_sampler():
    from meta_fine_tuning_amd import augment
    sd = synthetic.resnet10_state_dict(seed=13, prefix="feature.")
    model = _eval_model(sd).cuda()
    pool = synthetic.class_pool_u8("EuroSAT", "cuda:0", seed=1, n_per_class=40)
    sampler = augment.EpisodeSampler(pool, 5, 20, seed=10)
    np.random.seed(10)
    accs = ft.evaluate(model, sd, 2, 5, 5, 15, 84, 2, 1, episodes_per_batch=2, verbose=False, method="metaoptnet", sampler=sampler)
    assert accs.shape == (2,) and np.all((accs >= 0) & (accs <= 100))


# ------------------------------------------------------------------------------------------------ CLI
@pytest.mark.parametrize("extra", [[], ["--episodes_per_rank", "2"]], ids=["plain", "lockstep2"])
def test_train_main_metaoptnet_writes_a_loadable_checkpoint(golden_dir, tmp_path, monkeypatch, extra):
    from meta_fine_tuning_amd import configs, train
    g = _g27(golden_dir)
    monkeypatch.setattr(configs, "save_dir", str(tmp_path))
    train.main(["--dataset", "miniImageNet", "--method", "metaoptnet", "--model", "ResNet10", "--stop_epoch", "1"] + extra,
               n_episode=2, size=84)
    f = tmp_path / "checkpoints" / "miniImageNet" / "ResNet10_metaoptnet_5way_5shot" / "0.tar"
    assert f.is_file()
    state = torch.load(str(f), map_location="cpu")["state"]
    assert list(state.keys()) == [str(k) for k in g["state_keys"]]
    fresh = MetaOptNet(model_dict['ResNet10'], n_way=5, n_support=5)
    fresh.load_state_dict(state)
    assert list(fresh.state_dict().keys()) == [str(k) for k in g["state_keys"]]
