"""MetaOptNet-SVM on a real MI355X: the dual solve and its adjoint (csrc/svm.hip) against the float64
oracle of tests/test_metaoptnet_svm_cpu.py -- status, KKT of the returned alpha, the free mask, scores / dfeats / dscale within
4x the problem's own sensitivity to one fp32 rounding of its inputs --, bit-identical reruns and lockstep episodes, the
meta-training step against the golden G29, the graphed episode loop, FinetuneEngine(mode="svm") and the `test` driver."""
import argparse
import copy
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import meta_fine_tuning_amd  # noqa: F401
from meta_fine_tuning_amd import _lib, configs, ops, synthetic
from meta_fine_tuning_amd import autograd_ops as AG
from meta_fine_tuning_amd import finetune as ft
from meta_fine_tuning_amd.io_utils import model_dict
from meta_fine_tuning_amd.methods.metaoptnet import MetaOptNet
from oracle import mft_oracle as O
from test_metaoptnet_svm_cpu import C_REG, KINDS, SHAPES, SvmHead64, episodes_step, features, g29, kkt

pytestmark = pytest.mark.gpu
torch.set_num_threads(8)

SCALE = 0.8125
DRAWS = 2
EPS = 2.0 ** -24


def _rel_per_episode(got, want, E):
    got, want = np.asarray(got).reshape(E, -1), np.asarray(want).reshape(E, -1)
    return [float(np.linalg.norm(got[e] - want[e]) / max(np.linalg.norm(want[e]), 1e-300)) for e in range(E)]


@functools.lru_cache(maxsize=None)
def _references(shape, kind):
    """Per draw: the inputs, the oracle's step on them, and the yardstick y = the distance of the oracle at inputs multiplied by
    1 + 2^-24 u (u uniform in [-1, 1]) to the oracle at the inputs -- the problem's own sensitivity to one fp32 rounding.
    Computed once per (shape, kind) and never modified."""
    E = shape[0]
    refs = []
    for draw in range(DRAWS):
        f, G = features(kind, shape, draw)
        f64, G64 = f.double().numpy(), G.double().numpy()
        scores, dfeats, dscale, eps = episodes_step(f64, G64, SCALE, shape)
        rs = np.random.RandomState(9176 + draw)
        fp = f64 * (1.0 + EPS * rs.uniform(-1.0, 1.0, f64.shape))
        Gp = G64 * (1.0 + EPS * rs.uniform(-1.0, 1.0, G64.shape))
        s2, d2, c2, _ = episodes_step(fp, Gp, SCALE * (1.0 + EPS * rs.uniform(-1.0, 1.0)), shape)
        denom = float(np.abs(G64 * scores / SCALE).sum())
        refs.append(dict(f=f, G=G, scores=scores, dfeats=dfeats, dscale=dscale, eps=eps, dscale_denom=denom,
                         y_scores=max(_rel_per_episode(s2, scores, E)), y_dfeats=max(_rel_per_episode(d2, dfeats, E)),
                         y_dscale=abs(c2 - dscale) / max(denom, 1e-300)))
    return refs


def _run_head(f, G, shape):
    E, n_way, ns, nq = shape
    scale = torch.tensor([SCALE], device="cuda")
    scores, tape = ops.svm_forward(f, scale, E, n_way, ns, nq, save=True)
    dfeats, dscale = ops.svm_backward(tape, G)
    return scores, dfeats, dscale, tape


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "E%d_w%d_s%d_q%d" % s)
def test_kernels_match_the_oracle(shape, kind):
    """Reached on an MI355X (largest over shapes, kinds and draws; DESIGN.md section 17 has the table): stationarity
    1.20 x 2^-24 (|M| |alpha|) against the bound of 8; scores 2.5e-7, dfeats 7.2e-8, dscale 1.1e-7 against bounds of 4.8e-7 (every
    yardstick y is below the 2^-23 floor: the largest are 8.6e-8, 9.7e-8 and 2.4e-8)."""
    refs = _references(shape, kind)
    E, n_way, ns, nq = shape
    y_s, y_d, y_c = (max(r[k] for r in refs) for k in ("y_scores", "y_dfeats", "y_dscale"))
    for draw, r in enumerate(refs):
        # the condition on the inputs, on the ORACLE: no entry of the optimum sits within rounding of changing sides
        for ep in r["eps"]:
            k = kkt(ep["M"], ep["alpha"], n_way, ns)
            assert k["min_slack"] >= 1e-8 * C_REG, (draw, k["min_slack"])
            assert k["min_multiplier"] >= 1e-8 * k["gmax"], (draw, k["min_multiplier"], k["gmax"])
        assert max(r["y_scores"], r["y_dfeats"], r["y_dscale"]) <= 1e-3, (draw, r["y_scores"], r["y_dfeats"], r["y_dscale"])
        scores, dfeats, dscale, tape = _run_head(r["f"].cuda(), r["G"].cuda(), shape)
        assert scores.shape == (E * n_way * nq, n_way) and dfeats.shape == r["f"].shape and dscale.shape == (1,)
        # (i) every episode converged
        assert tape["status"].cpu().tolist() == [0] * E
        alpha = tape["alpha"].cpu().double().numpy()
        free = tape["free"].cpu().numpy().astype(bool)
        assert alpha.shape == free.shape == (E, n_way * ns, n_way) and tape["alpha"].dtype == torch.float32
        worst = 0.0
        for e, ep in enumerate(r["eps"]):
            # (ii) KKT of the stored fp32 alpha, in float64
            k = kkt(ep["M"], alpha[e], n_way, ns, free=free[e])
            assert k["over"] == 0.0
            assert k["rowsum"] <= n_way * EPS * C_REG, (draw, e, k["rowsum"])
            bound = 8.0 * EPS * k["scale"]
            assert (np.abs(k["res"])[free[e]] <= bound[free[e]]).all(), (draw, e)
            assert (-k["res"][~free[e]] >= -bound[~free[e]]).all(), (draw, e)
            worst = max(worst, float((np.abs(k["res"])[free[e]] / np.maximum(k["scale"][free[e]], 1e-300)).max()) / EPS)
            # (iii) the free set is the oracle's
            assert (free[e] == ep["free"]).all(), (draw, e, int((free[e] != ep["free"]).sum()))
        # (iv) against the oracle, within 4x the problem's sensitivity to one fp32 rounding
        e_s = max(_rel_per_episode(scores.cpu().double().numpy(), r["scores"], E))
        e_d = max(_rel_per_episode(dfeats.cpu().double().numpy(), r["dfeats"], E))
        e_c = abs(float(dscale.cpu().double()) - r["dscale"]) / max(r["dscale_denom"], 1e-300)
        print("svm %s %s draw %d: stationarity %.2f x 2^-24  scores %.3e (y %.3e)  dfeats %.3e (y %.3e)  dscale %.3e (y %.3e)"
              % (shape, kind, draw, worst, e_s, y_s, e_d, y_d, e_c, y_c))
        assert e_s <= 4.0 * max(y_s, 2.0 ** -23), (draw, e_s, y_s)
        assert e_d <= 4.0 * max(y_d, 2.0 ** -23), (draw, e_d, y_d)
        assert e_c <= 4.0 * max(y_c, 2.0 ** -23), (draw, e_c, y_c)


@pytest.mark.parametrize("shape", [(3, 3, 2, 3), (2, 5, 1, 15), (1, 5, 50, 2), (1, 32, 8, 1)], ids=lambda s: "E%d_w%d_s%d_q%d" % s)
def test_reruns_and_lockstep_episodes_are_bit_identical(shape):
    E, n_way, ns, nq = shape
    f, G = features("relu", shape, 0)
    f, G = f.cuda(), G.cuda()
    a, b = _run_head(f, G, shape), _run_head(f, G, shape)
    for x, y in zip(a[:3], b[:3]):
        assert torch.equal(x, y)
    for key in ("alpha", "free", "W", "status"):
        assert torch.equal(a[3][key], b[3][key])
    scale = torch.tensor([SCALE], device="cuda")
    sm = ops.svm_forward(f, scale, E, n_way, ns, nq, softmax=True)[0]
    assert torch.equal(sm, torch.softmax(a[0], dim=1)) or float((sm - torch.softmax(a[0], dim=1)).abs().max()) < 2e-6
    if E > 1:       # every episode alone gives the bits it gives in the batch (dscale is a sum over episodes: not compared)
        per, q = n_way * (ns + nq), n_way * nq
        for e in range(E):
            s1, d1, _, t1 = _run_head(f[e * per:(e + 1) * per], G[e * q:(e + 1) * q], (1, n_way, ns, nq))
            assert torch.equal(s1, a[0][e * q:(e + 1) * q]) and torch.equal(d1, a[1][e * per:(e + 1) * per])
            assert torch.equal(t1["alpha"][0], a[3]["alpha"][e]) and torch.equal(t1["free"][0], a[3]["free"][e])


def test_non_finite_features_give_non_finite_output_and_status_one():
    f, G = features("relu", (1, 5, 5, 16), 0)
    f = f.clone()
    f[3, 7] = float("nan")              # a support row
    scores, tape = ops.svm_forward(f.cuda(), torch.tensor([SCALE], device="cuda"), 1, 5, 5, 16, save=True)
    torch.cuda.synchronize()
    assert tape["status"].cpu().tolist() == [1] and not bool(torch.isfinite(scores).any())
    f[3, 7] = float("inf")
    scores, tape = ops.svm_forward(f.cuda(), torch.tensor([SCALE], device="cuda"), 1, 5, 5, 16, save=True)
    torch.cuda.synchronize()
    assert tape["status"].cpu().tolist() == [1] and not bool(torch.isfinite(scores).all())


def test_out_of_range_arguments_are_refused():
    lib = _lib.lib()
    f = torch.zeros(300, 520, device="cuda")
    ws = torch.zeros(5, 1 << 16, device="cuda")
    M = torch.zeros(1 << 16, device="cuda", dtype=torch.float64)
    work = torch.zeros(1 << 14, device="cuda", dtype=torch.float64)
    part = torch.zeros(64, device="cuda", dtype=torch.float64)
    free = torch.ones(1 << 14, device="cuda", dtype=torch.uint8)
    status = torch.zeros(4, device="cuda", dtype=torch.int32)
    scale = torch.ones(1, device="cuda")
    st = ops._stream(f)

    def call_all(a):
        p = ops._p
        head = (p(f), a["ld"], a["E"], a["n_way"], a["ns"], a["nq"], a["D"])
        alpha, W, dW, dfeats, _ = ws
        return [lib.mft_svm_gram(*head, p(M), st),
                lib.mft_svm_solve(*head, p(M), p(work), p(alpha), p(free), p(W), p(status), st),
                lib.mft_svm_backward_support(*head, p(M), p(alpha), p(free), p(W), p(dW), p(part), p(dfeats), 512, p(scale), st)]

    good = dict(ld=520, E=1, n_way=5, ns=5, nq=16, D=512)
    assert call_all(good) == [0, 0, 0]
    for b in [dict(n_way=0), dict(n_way=33, ns=1), dict(n_way=1, ns=257), dict(n_way=16, ns=17), dict(nq=0), dict(E=0), dict(D=510),
              dict(D=516), dict(ld=500), dict(ld=514), dict(ns=0)]:
        a = dict(good)
        a.update(b)
        assert call_all(a) == [-22] * 3, b
    torch.cuda.synchronize()
    z = lambda *s: torch.zeros(*s, device="cuda")  # noqa: E731
    for args in [(z(0, 512), 1, 0, 5, 16), (z(33 * 2, 512), 1, 33, 1, 1), (z(258, 512), 1, 1, 257, 1), (z(25, 512), 1, 5, 5, 0),
                 (z(105, 510), 1, 5, 5, 16), (z(105, 514)[:, :512], 1, 5, 5, 16), (z(100, 512), 1, 5, 5, 16)]:
        with pytest.raises(ValueError):
            ops.svm_forward(args[0], scale, *args[1:])
    tape = ops.svm_forward(z(105, 512), scale, 1, 5, 5, 16, save=True)[1]
    with pytest.raises(ValueError):
        ops.svm_backward(tape, z(80, 4))
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
        sc = SvmHead64.apply(feats, sd["scale"], n_way, 5)
        losses.append(F.cross_entropy(sc, torch.from_numpy(np.repeat(np.arange(n_way), per - 5))))
    loss = torch.stack(losses).mean()
    grads = torch.autograd.grad(loss, [sd[k] for k in pkeys])
    return float(loss.detach()), dict(zip(pkeys, grads))


def _check_grads(named, ref):
    # bounds of tests/test_metaoptnet_gpu.py::_check_grads (the trunk backward is the same code)
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


def _model(sd, train=True):
    m = MetaOptNet(model_dict['ResNet10'], n_way=5, n_support=5, head="svm")
    m.load_state_dict(sd)
    m = m.cuda() if train else m
    m.train()
    m.n_query = 16
    return m


def test_set_forward_loss_backward_vs_oracle_and_g29(golden_dir):
    g = g29(golden_dir)
    sd = _state(27)
    model = _model(sd)
    x = synthetic.train_episode(27, 5, 5, 16, 84)
    with torch.no_grad():
        sc = model.set_forward(x)
    assert AG.metaoptnet_svm_status().cpu().tolist() == [0]
    np.testing.assert_allclose(sc.cpu().numpy(), g["scores"], rtol=1e-3, atol=1e-3)
    loss = model.set_forward_loss(x)
    loss.backward()
    assert AG.metaoptnet_svm_status().cpu().tolist() == [0]
    assert abs(float(loss.detach()) - float(g["loss"])) < 2e-4
    ref_loss, ref = _oracle(sd, sd["scale"], x[None])
    assert abs(ref_loss - float(g["loss"])) < 1e-9
    named = dict(model.named_parameters())
    assert set(ref) == set(named)
    _check_grads(named, ref)
    want = float(g["scalegrad"][0])
    assert abs(float(ref["scale"]) - want) < 1e-9 * abs(want)
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
    loss = model.set_forward_loss_lockstep(xs.cuda())
    loss.backward()
    assert AG.metaoptnet_svm_status().cpu().tolist() == [0, 0]
    ref_loss, ref = _oracle(sd, sd["scale"], xs)
    assert abs(float(loss.detach()) - ref_loss) < 2e-4
    _check_grads(dict(model.named_parameters()), ref)


def test_graphed_episode_loop_is_bit_identical(capsys, monkeypatch):
    from meta_fine_tuning_amd import graph_step, optim
    eps = [synthetic.train_episode(800 + i, 5, 5, 16, 84) for i in range(6)]        # three eager warm-up steps, three replayed

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


# ------------------------------------------------------------------------------------------------ evaluation
@pytest.mark.parametrize("E", [0, 1])
def test_finetune_with_the_svm_head_matches_g29(golden_dir, E):
    g = g29(golden_dir)
    sd = synthetic.resnet10_state_dict(seed=13, prefix="feature.")
    ft.params = argparse.Namespace(model="ResNet10", fine_tune_epoch=E)
    full = dict(sd)
    full.update(synthetic.metaoptnet_head_state(27))
    model = _model(full, train=False)
    liz = synthetic.test_episode(41, 5, 5, 15, 84, gen_examples=0)
    np.random.seed(10)
    sc = ft.finetune(liz, None, model, copy.deepcopy(sd), None, n_query=15, n_way=5, n_support=5)
    assert sc.shape == (75, 5) and model.n_query == 15
    mine = [ent["engine"] for ent in ft._ENGINES.entries if ent["cfg"][0] == "svm"]
    assert mine and mine[-1].mode == "svm" and mine[-1].svm_status.cpu().tolist() == [0]
    ref = g["finetune_scores_E%d" % E]
    if E == 0:
        np.testing.assert_allclose(sc.cpu().numpy(), ref, atol=1e-4)          # forward only: the bar G27 (d) gets
    else:
        err = np.abs(sc.cpu().numpy() - ref)
        print("metaoptnet-svm finetune E=1: max err %.3e" % err.max())
        assert err.max() < 3e-2 and (sc.argmax(1).cpu().numpy() == ref.argmax(1)).mean() >= 0.96, err.max()


def test_test_driver_with_head_svm_in_lockstep_equals_the_per_episode_loop(tmp_path, monkeypatch):
    from meta_fine_tuning_amd import feature_eval, save_features
    from meta_fine_tuning_amd import test as test_driver
    from meta_fine_tuning_amd.data.feature_loader import init_loader
    from meta_fine_tuning_amd.io_utils import parse_args
    from test_feature_eval_gpu import EPISODES, N_QUERY, N_SHOT, N_WAY, PER_BATCH, POOL, _env, _seed, _sequential, _state as fe_state
    monkeypatch.setattr(configs, "save_dir", str(tmp_path))
    _env(monkeypatch)
    argv = ["--dataset", "miniImageNet", "--method", "metaoptnet", "--head", "svm", "--test_dataset", POOL]
    d = save_features.checkpoint_dir(parse_args('save_features', argv))
    assert d.endswith("ResNet10_metaoptnet_svm_5way_5shot")
    os.makedirs(d)
    torch.save({'epoch': 0, 'state': fe_state("metaoptnet")}, os.path.join(d, "0.tar"))
    featfile = save_features.main(argv)
    assert "ResNet10_metaoptnet_svm_5way_5shot" in featfile
    acc_main = test_driver.main(argv)
    model, loaded = test_driver.load_model(parse_args('test', argv))
    assert loaded is not None and model.head == "svm"
    cl = init_loader(featfile)
    _seed()
    acc_lock, s_lock = feature_eval.evaluate(model, "metaoptnet", feature_eval.FeatureTable(cl), N_WAY, N_SHOT, N_QUERY, EPISODES,
                                             PER_BATCH, return_scores=True)
    s_seq, acc_seq, _ = _sequential(model, "metaoptnet", False, cl)
    for e, (a, b) in enumerate(zip(s_lock, s_seq)):
        assert a.shape == b.shape == (N_WAY * N_QUERY, N_WAY) and np.array_equal(a, b), (e, float(np.abs(a - b).max()))
    assert np.array_equal(acc_lock, acc_seq) and np.array_equal(acc_main, acc_seq)
    # and it is the SVM head that scored: the ridge head gives other scores on the same episode
    ridge = MetaOptNet(model_dict['ResNet10'], n_way=N_WAY, n_support=N_SHOT).cuda()
    ridge.load_state_dict(model.state_dict())
    ridge.n_query = N_QUERY
    _seed()
    _, s_ridge = feature_eval.evaluate(ridge, "metaoptnet", feature_eval.FeatureTable(cl), N_WAY, N_SHOT, N_QUERY, EPISODES,
                                       PER_BATCH, return_scores=True)
    assert not np.array_equal(s_ridge[0], s_lock[0])


def test_train_main_with_head_svm_writes_a_loadable_checkpoint(golden_dir, tmp_path, monkeypatch):
    from meta_fine_tuning_amd import train
    g = g29(golden_dir)
    monkeypatch.setattr(configs, "save_dir", str(tmp_path))
    model = train.main(["--dataset", "miniImageNet", "--method", "metaoptnet", "--head", "svm", "--model", "ResNet10", "--stop_epoch", "1",
                        "--episodes_per_rank", "2"], n_episode=2, size=84)
    assert model.head == "svm" and AG.metaoptnet_svm_status().cpu().tolist() == [0, 0]
    f = tmp_path / "checkpoints" / "miniImageNet" / "ResNet10_metaoptnet_svm_5way_5shot" / "0.tar"
    assert f.is_file()
    state = torch.load(str(f), map_location="cpu")["state"]
    assert list(state.keys()) == [str(k) for k in g["state_keys"]]
