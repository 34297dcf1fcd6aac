"""Baseline++ on a real MI355X: the cosine-head kernels (mft_dist_linear_forward / mft_dist_linear_backward /
mft_dist_head_sgd_run) against a float64 restatement of the head's definition, the test-time adaptation
against the reference's golden G24, the training head inside a BaselineTrain step, the fused optimiser, the
train.main --method baseline++ driver and finetune.baselinepp_batched."""
import argparse
import os
import warnings

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import meta_fine_tuning_amd  # noqa: F401
from meta_fine_tuning_amd import _lib, backbone, ops, synthetic
from meta_fine_tuning_amd import finetune as ft
from meta_fine_tuning_amd.methods.baselinefinetune import BaselineFinetune
from meta_fine_tuning_amd.methods.baselinetrain import BaselineTrain
from meta_fine_tuning_amd.methods.meta_template import dist_head_adapt

pytestmark = pytest.mark.gpu
torch.set_num_threads(8)


def _g24(golden_dir):
    return np.load(os.path.join(golden_dir, "g24_baselinepp.npz"))


def g24_features(n_shot):
    return torch.from_numpy(np.abs(np.random.RandomState(271 + n_shot).standard_normal((5, n_shot + 15, 512))).astype(np.float32))


def dist_scores64(x, g, v, s):
    """score[r,c] = s * (x_r / (||x_r|| + 1e-5)) . (g_c v_c / ||v_c||) in float64."""
    x, g, v = x.double(), g.double().reshape(-1, 1), v.double()
    xh = x / (x.norm(dim=1, keepdim=True) + 1e-5)
    return s * xh @ (g * v / v.norm(dim=1, keepdim=True)).t()


def adapt64(z_support, y_support, v0, g0, perms, batch_size=4, z_query=None):
    """baselinefinetune.py:35-58 with the head above, in float64: torch.optim.SGD(0.01, 0.9, 0.9, 0.001) over ``perms``."""
    n_way = v0.shape[0]
    s = 2.0 if n_way <= 200 else 10.0
    v = torch.as_tensor(v0).double().clone().requires_grad_(True)
    g = torch.as_tensor(g0).double().reshape(n_way, 1).clone().requires_grad_(True)
    opt = torch.optim.SGD([g, v], lr=0.01, momentum=0.9, dampening=0.9, weight_decay=0.001)
    y = torch.as_tensor(np.asarray(y_support)).long()
    S = z_support.shape[0]
    for rand_id in perms:
        for i in range(0, S, batch_size):
            ids = torch.from_numpy(np.asarray(rand_id[i:min(i + batch_size, S)])).long()
            opt.zero_grad()
            F.cross_entropy(dist_scores64(z_support[ids], g, v, s), y[ids]).backward()
            opt.step()
    sc = None if z_query is None else dist_scores64(z_query, g.detach(), v.detach(), s)
    return g.detach(), v.detach(), sc


def _rel(got, want):
    return float((got.cpu().double() - want).norm() / want.norm())


# ------------------------------------------------------------------------------------------------ forward / backward
#         rows, C, D, ldx, an all-zero row
CASES = [(16, 200, 512, 512, None), (1, 5, 512, 512, None), (3, 257, 512, 516, 1), (75, 5, 512, 512, None), (16, 201, 64, 64, None)]


@pytest.mark.parametrize("rows,C,D,ldx,zero_row", CASES)
def test_forward_backward_match_float64_autograd(rows, C, D, ldx, zero_row):
    gen = torch.Generator().manual_seed(rows * 100000 + C * 100 + D)
    x_cpu = torch.randn(rows, D, generator=gen).abs()
    if zero_row is not None:
        x_cpu[zero_row] = 0
    v_cpu = torch.randn(C, D, generator=gen).abs() / D ** 0.5
    g_cpu = torch.rand(C, 1, generator=gen) + 0.5
    G_cpu = torch.randn(rows, C, generator=gen)
    s = ops.dist_scale(C)
    assert s == (2.0 if C <= 200 else 10.0)
    xbuf = torch.zeros(rows, ldx, device="cuda")
    xbuf[:, :D] = x_cpu.cuda()
    x = xbuf[:, :D]
    assert x.stride(0) == ldx
    v, g, G = v_cpu.cuda(), g_cpu.cuda(), G_cpu.cuda()
    x64, g64, v64 = (t.double().requires_grad_(True) for t in (x_cpu, g_cpu, v_cpu))
    ref = dist_scores64(x64, g64, v64, s)
    (ref * G_cpu.double()).sum().backward()
    ref = ref.detach()

    sc = ops.dist_linear_forward(x, g, v, s)
    assert sc.shape == (rows, C)
    err = float(((sc.cpu().double() - ref).abs() / ref.abs().clamp(min=1.0)).max())
    dx, dv, dg = ops.dist_linear_backward(x, g, v, s, G)
    assert dx.shape == (rows, D) and dv.shape == (C, D) and dg.shape == (C, 1)
    e_dx, e_dv, e_dg = _rel(dx, x64.grad), _rel(dv, v64.grad), _rel(dg, g64.grad)
    print("rows %d C %d D %d: score err %.2e, rel L2 dx %.2e dV %.2e dg %.2e" % (rows, C, D, err, e_dx, e_dv, e_dg))
    assert err < 5e-6, err
    assert e_dx < 1e-5 and e_dv < 1e-5 and e_dg < 1e-5, (e_dx, e_dv, e_dg)
    for t in (sc, dx, dv, dg):
        assert bool(torch.isfinite(t).all())
    if zero_row is not None:
        # a zero row: score 0, dx = dxh / eps (it dominates the norm above, so the other rows are compared apart as well)
        assert float(sc[zero_row].abs().max()) == 0.0
        keep = [r for r in range(rows) if r != zero_row]
        assert _rel(dx[keep], x64.grad[keep]) < 1e-5
        assert _rel(dx[zero_row], x64.grad[zero_row]) < 1e-5
    # dx not wanted: the same dV and dg
    none_dx, dv2, dg2 = ops.dist_linear_backward(x, g, v, s, G, need_dx=False)
    assert none_dx is None and torch.equal(dv2, dv) and torch.equal(dg2, dg)
    # two calls: bit-identical
    assert torch.equal(sc, ops.dist_linear_forward(x, g, v, s))
    dx3, dv3, dg3 = ops.dist_linear_backward(x, g, v, s, G)
    assert torch.equal(dx3, dx) and torch.equal(dv3, dv) and torch.equal(dg3, dg)
    # softmax epilogue
    sm = ops.dist_linear_forward(x, g, v, s, softmax=True)
    assert float((sm.cpu().double() - torch.softmax(ref, dim=1)).abs().max()) < 2e-5
    assert torch.equal(sm, ops.dist_linear_forward(x, g, v, s, softmax=True))


def test_grouped_forward_scores_each_group_with_its_own_head():
    gen = torch.Generator().manual_seed(37)
    x_cpu = torch.randn(3 * 7, 512, generator=gen).abs()
    v_cpu = torch.randn(3, 5, 512, generator=gen).abs() / 512 ** 0.5
    g_cpu = torch.rand(3, 5, generator=gen) + 0.5
    ref = torch.cat([dist_scores64(x_cpu[7 * e:7 * e + 7], g_cpu[e], v_cpu[e], 2.0) for e in range(3)])
    sc = ops.dist_linear_forward(x_cpu.cuda(), g_cpu.cuda(), v_cpu.cuda(), 2.0)
    assert sc.shape == (21, 5)
    assert float(((sc.cpu().double() - ref).abs() / ref.abs().clamp(min=1.0)).max()) < 5e-6
    sm = ops.dist_linear_forward(x_cpu.cuda(), g_cpu.cuda(), v_cpu.cuda(), 2.0, softmax=True)
    assert float((sm.cpu().double() - torch.softmax(ref, dim=1)).abs().max()) < 2e-5
    assert torch.equal(sc, ops.dist_linear_forward(x_cpu.cuda(), g_cpu.cuda(), v_cpu.cuda(), 2.0))


def test_autograd_function_returns_the_three_gradients():
    from meta_fine_tuning_amd import autograd_ops as AG
    gen = torch.Generator().manual_seed(5)
    x_cpu, v_cpu, g_cpu = torch.randn(6, 512, generator=gen).abs(), torch.randn(10, 512, generator=gen) / 22.6, torch.rand(10, 1, generator=gen) + 0.5
    y = torch.tensor([0, 3, 9, 1, 1, 7])
    x, g, v = (t.cuda().requires_grad_(True) for t in (x_cpu, g_cpu, v_cpu))
    F.cross_entropy(AG.dist_linear(x, g, v, 2), y.cuda()).backward()
    x64, g64, v64 = (t.double().requires_grad_(True) for t in (x_cpu, g_cpu, v_cpu))
    F.cross_entropy(dist_scores64(x64, g64, v64, 2.0), y).backward()
    assert _rel(x.grad, x64.grad) < 1e-5 and _rel(g.grad, g64.grad) < 1e-5 and _rel(v.grad, v64.grad) < 1e-5
    with torch.no_grad():
        assert not AG.dist_linear(x, g, v, 2).requires_grad


def test_out_of_range_shapes_are_refused():
    lib = _lib.lib()
    x = torch.zeros(20, 520, device="cuda")
    V = torch.zeros(1025, 520, device="cuda")
    g = torch.ones(1025, device="cuda")
    out = torch.zeros(20 * 1025, device="cuda")
    dV = torch.zeros(1025, 520, device="cuda")
    dg = torch.zeros(1025, device="cuda")
    dx = torch.zeros(20, 520, device="cuda")
    base = dict(ld=512, rows=4, C=5, D=512)

    def fwd(a):
        return lib.mft_dist_linear_forward(ops._p(x), a["ld"], a.get("groups", 1), a["rows"], ops._p(V), ops._p(g), a["C"], a["D"], 2.0,
                                           ops._p(out), 0, ops._stream(x))

    def bwd(a):
        return lib.mft_dist_linear_backward(ops._p(x), a["ld"], a["rows"], ops._p(V), ops._p(g), a["C"], a["D"], 2.0, ops._p(out),
                                            max(a["C"], 1), ops._p(dx), a.get("ldd", a["ld"]), ops._p(dV), ops._p(dg), ops._stream(x))

    V[:5, :512] = 1.0
    assert fwd(base) == 0 and bwd(base) == 0
    for b in [dict(C=0), dict(C=1025), dict(D=510), dict(D=516, ld=520), dict(ld=508), dict(ld=514), dict(rows=0)]:
        a = dict(base)
        a.update(b)
        assert fwd(a) == -22, b
        assert bwd(a) == -22, b
    assert fwd(dict(base, groups=0)) == -22
    assert bwd(dict(base, ldd=508)) == -22
    # the run: n_way and batch_size are bounded as in the softmax run
    z = torch.ones(1, 25, 512, device="cuda")
    y = torch.zeros(1, 25, dtype=torch.int32, device="cuda")
    tab = torch.zeros(1, 2, 17, dtype=torch.int32, device="cuda")
    Vr = torch.ones(1, 17, 512, device="cuda")
    gr = torch.ones(1, 17, device="cuda")

    def run(n_way=5, bs=4, D=512, steps=2, groups=1, S=25):
        return lib.mft_dist_head_sgd_run(ops._p(z), ops._p(y), ops._p(tab), groups, S, D, n_way, steps, bs, ops._p(Vr), ops._p(gr), 2.0,
                                         0.01, 0.9, 0.9, 0.001, ops._stream(z))

    assert run() == 0
    for kw in [dict(n_way=17), dict(n_way=0), dict(bs=17), dict(bs=0), dict(D=510), dict(D=516), dict(steps=0), dict(groups=0),
               dict(S=0)]:
        assert run(**kw) == -22, kw
    with pytest.raises(ValueError):
        ops.dist_linear_forward(torch.zeros(4, 512, device="cuda"), torch.ones(5, device="cuda"), torch.ones(6, 512, device="cuda"), 2.0)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the SGD run
@pytest.mark.parametrize("groups,S,epochs", [(2, 25, 6), (1, 100, 3)])       # LDS form (ragged tail); HBM form (5-way 20-shot)
def test_head_sgd_run_matches_torch_sgd_float64(groups, S, epochs):
    gen = torch.Generator().manual_seed(S + groups)
    rs = np.random.RandomState(S)
    n_way, D, bs = 5, 512, 4
    z = torch.randn(groups, S, D, generator=gen).abs()
    y = np.stack([rs.permutation(np.repeat(np.arange(n_way), S // n_way)) for _ in range(groups)]).astype(np.int32)
    v0 = (torch.rand(groups, n_way, D, generator=gen) * 2 - 1) / D ** 0.5
    g0 = v0.norm(dim=2)
    perms = [[rs.permutation(S) for _ in range(epochs)] for _ in range(groups)]
    from meta_fine_tuning_amd.methods.meta_template import adaptation_table
    table = torch.from_numpy(np.stack([adaptation_table(S, epochs, bs, p) for p in perms])).cuda()
    assert table.shape == (groups, epochs * ((S + bs - 1) // bs), bs)
    assert (S % bs == 0) or int((table[0, S // bs] < 0).sum()) == bs - S % bs       # the ragged tail is -1 padded
    v, g = v0.clone().cuda(), g0.clone().cuda()
    ops.dist_head_sgd_run(z.cuda(), torch.from_numpy(y).cuda(), table, v, g, 2.0, 0.01, 0.9, 0.9, 0.001)
    for e in range(groups):
        g64, v64, _ = adapt64(z[e], y[e], v0[e], g0[e], perms[e], bs)
        eg = float((g[e].cpu().double() - g64.view(-1)).abs().max())
        ev = float((v[e].cpu().double() - v64).abs().max())
        print("group %d of S=%d: max|dg| %.2e max|dv| %.2e" % (e, S, eg, ev))
        assert eg < 2e-5 and ev < 2e-5, (e, eg, ev)
        assert float((v64 - v0[e].double()).abs().max()) > 1e-3                     # the head did move
    # a second run from the same start: bit-identical
    v2, g2 = v0.clone().cuda(), g0.clone().cuda()
    ops.dist_head_sgd_run(z.cuda(), torch.from_numpy(y).cuda(), table, v2, g2, 2.0, 0.01, 0.9, 0.9, 0.001)
    assert torch.equal(v2, v) and torch.equal(g2, g)


# ------------------------------------------------------------------------------------------------ adaptation vs G24
@pytest.mark.parametrize("n_shot", [5, 20])
def test_baselinefinetune_dist_set_forward_matches_g24(golden_dir, n_shot):
    g24 = _g24(golden_dir)
    tag = "_%dshot" % n_shot
    model = BaselineFinetune(backbone.ResNet10, 5, n_shot, loss_type='dist')
    model.n_query = 15
    torch.manual_seed(123)
    np.random.seed(10)
    sc = model.set_forward(g24_features(n_shot).cuda())
    assert np.array_equal(np.random.permutation(7), g24["next_perm" + tag])
    ref = g24["scores" + tag]
    assert sc.shape == (75, 5)
    err = float(np.abs(sc.cpu().numpy() - ref).max())
    print("%d-shot set_forward vs G24: max|dscore| %.2e" % (n_shot, err))
    assert err < 2e-5, err
    assert np.array_equal(sc.argmax(1).cpu().numpy(), ref.argmax(1))


def test_dist_head_adapt_two_episodes_g24_and_float64(golden_dir):
    """E = 2 in one run launch and one scoring launch: episode 0 is G24's 5-shot episode, episode 1 another one (other features,
    head and permutations) checked against the float64 restatement; the permutations are drawn episode by episode."""
    g24 = _g24(golden_dir)
    z0 = g24_features(5)
    gen = torch.Generator().manual_seed(77)
    z1 = torch.randn(5, 20, 512, generator=gen).abs()
    v1 = (torch.rand(5, 512, generator=gen) * 2 - 1) / 512 ** 0.5
    g1 = v1.norm(dim=1, keepdim=True)
    z = torch.stack([z0, z1])
    y = np.repeat(np.arange(5), 5)
    v0 = torch.stack([torch.from_numpy(g24["v0_5shot"]), v1])
    g0 = torch.stack([torch.from_numpy(g24["g0_5shot"]), g1])
    np.random.seed(10)
    sc, v, g = dist_head_adapt(z[:, :, :5].reshape(2, 25, 512).cuda(), y, z[:, :, 5:].reshape(2, 75, 512).cuda(), v0, g0, 5, 5)
    after = np.random.permutation(7)
    np.random.seed(10)
    for _ in range(100):
        np.random.permutation(25)                     # episode 0's: G24's stream
    p1 = [np.random.permutation(25) for _ in range(100)]
    assert np.array_equal(after, np.random.permutation(7))
    assert sc.shape == (150, 5) and v.shape == (2, 5, 512) and g.shape == (2, 5)
    ref = g24["scores_5shot"]
    got = sc[:75].cpu().numpy()
    assert float(np.abs(got - ref).max()) < 2e-5 and np.array_equal(got.argmax(1), ref.argmax(1))
    assert float(np.abs(v[0].cpu().numpy() - g24["v_5shot"]).max()) < 2e-5
    assert float(np.abs(g[0].cpu().numpy() - g24["g_5shot"].reshape(-1)).max()) < 2e-5
    g64, v64, sc64 = adapt64(z1[:, :5].reshape(25, 512), y, v1, g1, p1, 4, z_query=z1[:, 5:].reshape(75, 512))
    assert float((sc[75:].cpu().double() - sc64).abs().max()) < 2e-5
    assert np.array_equal(sc[75:].argmax(1).cpu().numpy(), sc64.argmax(1).numpy())
    assert float((g[1].cpu().double() - g64.view(-1)).abs().max()) < 2e-5 and float((v[1].cpu().double() - v64).abs().max()) < 2e-5
    # the caller's initial heads are not modified
    assert torch.equal(v0[0], torch.from_numpy(g24["v0_5shot"]))


# ------------------------------------------------------------------------------------------------ training
def _dist_model(num_class, seed=3):
    torch.manual_seed(seed)
    m = BaselineTrain(backbone.ResNet10, num_class, loss_type='dist').cuda()
    m.train()
    return m


def test_training_head_inside_the_step_matches_float64():
    """BaselineTrain(loss_type='dist') on 16 images: with the HIP features as a float64 leaf, the loss and the gradients of g, v
    and of the features (what the trunk backward receives) against float64 autograd of the restatement."""
    m = _dist_model(200)
    rs = np.random.RandomState(21)
    x = torch.from_numpy(rs.standard_normal((16, 3, 84, 84)).astype(np.float32))
    y = torch.from_numpy(rs.randint(0, 200, size=16))
    seen = {}
    trunk_forward = m.feature.forward

    def forward(inp):
        out = trunk_forward(inp)
        seen["feat"] = out.detach().clone()
        out.register_hook(lambda d: seen.__setitem__("dfeat", d.detach().clone()))
        return out

    m.feature.forward = forward
    loss = m.forward_loss(x, y)
    loss.backward()
    assert m.top1.count == 16 and seen["feat"].shape == (16, 512)
    f64 = seen["feat"].cpu().double().requires_grad_(True)
    g64 = m.classifier.L.weight_g.detach().cpu().double().requires_grad_(True)
    v64 = m.classifier.L.weight_v.detach().cpu().double().requires_grad_(True)
    ref = F.cross_entropy(dist_scores64(f64, g64, v64, 2.0), y)
    ref.backward()
    assert abs(float(loss) - float(ref)) < 1e-4
    dg, dv = m.classifier.L.weight_g.grad, m.classifier.L.weight_v.grad
    assert dg.shape == (200, 1) and dv.shape == (200, 512)
    assert float((dg.cpu().double() - g64.grad).abs().max()) < 2e-5 * max(1.0, float(g64.grad.abs().max()))
    assert float((dv.cpu().double() - v64.grad).abs().max()) < 2e-5 * max(1.0, float(v64.grad.abs().max()))
    assert _rel(seen["dfeat"], f64.grad) < 1e-5
    assert all(p.grad is not None for p in m.feature.parameters())


def test_training_step_matches_the_reference_g24(golden_dir):
    """The reference's own BaselineTrain(loss_type='dist') step on the CPU (G24 part (b): 4 images, 10 classes): loss within the
    2e-4 of the ProtoNet G22 step, head gradients within its event bound (3e-2 relative L2: a ReLU pre-activation of ~1e-7 may
    fall on the other side of zero in another fp32 implementation of the trunk)."""
    g24 = _g24(golden_dir)
    m = _dist_model(10)
    m.feature.load_state_dict({k[len("feature."):]: v for k, v in synthetic.resnet10_state_dict(seed=24, prefix="feature.").items()})
    m.classifier.load_state_dict({"L.weight_g": torch.from_numpy(g24["train_g0"]), "L.weight_v": torch.from_numpy(g24["train_v0"])})
    x = torch.from_numpy(np.random.RandomState(24).standard_normal((4, 3, 84, 84)).astype(np.float32))
    loss = m.forward_loss(x, torch.tensor([0, 3, 7, 9]))
    loss.backward()
    assert abs(float(loss) - float(g24["train_loss"])) < 2e-4
    for got, want in ((m.classifier.L.weight_g.grad, g24["train_dg"]), (m.classifier.L.weight_v.grad, g24["train_dv"])):
        want = torch.from_numpy(want).double()
        assert _rel(got, want) < 3e-2


def test_fused_adam_sees_fresh_head_weights_loss_falls_every_step():
    from meta_fine_tuning_amd import optim
    m = _dist_model(10)
    opt = optim.Adam(m.parameters())
    rs = np.random.RandomState(5)
    x = torch.from_numpy(rs.standard_normal((16, 3, 84, 84)).astype(np.float32))
    y = torch.from_numpy(rs.randint(0, 10, size=16))
    g_before = m.classifier.L.weight_g.detach().clone()
    losses = []
    for _ in range(4):
        opt.zero_grad()
        loss = m.forward_loss(x, y)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert all(b < a for a, b in zip(losses, losses[1:])), losses
    assert not torch.equal(g_before, m.classifier.L.weight_g.detach())


def test_train_driver_baselinepp_method(tmp_path, monkeypatch):
    from meta_fine_tuning_amd import configs, train as tr
    monkeypatch.setattr(configs, "save_dir", str(tmp_path))
    torch.manual_seed(0)
    m = tr.main(["--method", "baseline++", "--model", "ResNet10", "--num_classes", "10", "--stop_epoch", "2", "--save_freq", "1"],
                n_episode=3, size=84)
    dirs = os.listdir(os.path.join(str(tmp_path), "checkpoints"))
    assert len(dirs) == 1
    d = os.path.join(str(tmp_path), "checkpoints", dirs[0], "ResNet10_baseline++")
    ck = torch.load(os.path.join(d, "1.tar"), map_location="cpu")
    assert ck["epoch"] == 1
    state = ck["state"]
    assert "feature.trunk.0.weight" in state
    assert state["classifier.L.weight_g"].shape == (10, 1) and state["classifier.L.weight_v"].shape == (10, 512)
    assert [k for k in state if k.startswith("classifier.")] == ["classifier.L.weight_g", "classifier.L.weight_v"]

    class TorchHead(nn.Module):
        def __init__(self):
            super().__init__()
            from torch.nn.utils.weight_norm import WeightNorm
            self.L = nn.Linear(512, 10, bias=False)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                WeightNorm.apply(self.L, 'weight', dim=0)

    head = TorchHead()
    head.load_state_dict({k[len("classifier."):]: v for k, v in state.items() if k.startswith("classifier.")}, strict=True)
    assert torch.equal(head.L.weight_v.data, state["classifier.L.weight_v"])
    assert m.top1.count == 2 * 3 * 16 == 96
    # the head trained: g is no longer the row norm of v it was initialised to
    assert float((state["classifier.L.weight_g"].view(-1) - state["classifier.L.weight_v"].norm(dim=1)).abs().max()) > 1e-5


# ------------------------------------------------------------------------------------------------ evaluation
def test_baselinepp_batched_equals_one_episode_at_a_time():
    sd = synthetic.resnet10_state_dict(seed=13, prefix="feature.")
    ft.params = argparse.Namespace(model="ResNet10", fine_tune_epoch=0)
    eps = [synthetic.test_episode(60 + i, 5, 5, 15, 84, gen_examples=0) for i in range(3)]
    rs = np.random.RandomState(8)
    perms = [[rs.permutation(25) for _ in range(100)] for _ in range(3)]
    torch.manual_seed(11)
    heads = ft.dist_head_init(5, n=3)
    assert heads[0].shape == (3, 5, 512) and heads[1].shape == (3, 5, 1)
    sc = ft.baselinepp_batched(eps, sd, 5, 5, episodes_per_batch=2, perms=perms, heads=heads)
    assert sc.shape == (225, 5)
    torch.testing.assert_close(sc.sum(1).cpu(), torch.ones(225), atol=1e-5, rtol=0)
    for i in range(3):
        one = ft.baselinepp_batched(eps[i:i + 1], sd, 5, 5, episodes_per_batch=1, perms=perms[i:i + 1],
                                    heads=(heads[0][i:i + 1], heads[1][i:i + 1]))
        assert one.shape == (75, 5)
        assert torch.equal(one, sc[75 * i:75 * i + 75]), float((one - sc[75 * i:75 * i + 75]).abs().max())
    # the defaults draw: one head per episode from torch's RNG, 100 permutations per episode from numpy's
    torch.manual_seed(11)
    np.random.seed(4)
    sc2 = ft.baselinepp_batched(eps[:2], sd, 5, 5, episodes_per_batch=2)
    np.random.seed(4)
    p2 = [[np.random.permutation(25) for _ in range(100)] for _ in range(2)]
    want = ft.baselinepp_batched(eps[:2], sd, 5, 5, episodes_per_batch=2, perms=p2, heads=(heads[0][:2], heads[1][:2]))
    assert torch.equal(sc2, want)
