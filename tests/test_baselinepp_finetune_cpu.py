"""Baseline++ at test time without a GPU: a float64 restatement of the fused head step (mft_dist_head_step: scores, mean cross
entropy, the gradients of DESIGN.md section 12, Adam with L2 weight decay) against torch autograd + torch.optim.Adam on the
WeightNorm statement of the head, the same restatement replayed through finetune_linear's loop against golden G25, and the
host-side surface (permutation stream, checkpoint lookup)."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import meta_fine_tuning_amd  # noqa: F401
from meta_fine_tuning_amd import finetune as ft
from meta_fine_tuning_amd import io_utils, synthetic
from oracle import mft_oracle as O

EPS_N = 1e-5


def head_step64(x, y, V, g, mom, step, s=2.0, lr=0.01, b1=0.9, b2=0.999, eps=1e-8, wd=0.001):
    """One head step in float64.  x [k, D], y [k], V [C, D], g [C]; ``mom`` = dict(mV, vV, mg, vg), updated in place together with
    V and g.  -> (loss, dx, dV, dg): the loss and the gradients (without weight decay) at the PRE-update head."""
    k = x.shape[0]
    n = x.norm(dim=1, keepdim=True)
    ie = 1.0 / (n + EPS_N)
    xh = x * ie
    nv = V.norm(dim=1)
    u = xh @ V.t() / nv                                                   # [k, C]
    score = s * g * u
    lse = torch.logsumexp(score, dim=1)
    loss = (lse - score[torch.arange(k), y]).mean()
    G = (torch.softmax(score, dim=1) - F.one_hot(y, V.shape[0]).to(x.dtype)) / k
    P = (G * u).sum(0)                                                    # sum_r G[r,c] u[r,c]
    dg = s * P
    dV = (s * g / nv)[:, None] * (G.t() @ xh - (P / nv)[:, None] * V)
    dxh = s * G @ (g[:, None] * V / nv[:, None])
    k2 = torch.where(n > 0, (dxh * x).sum(1, keepdim=True) * ie * ie / n.clamp(min=1e-300), torch.zeros_like(n))
    dx = dxh * ie - x * k2
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    for w, gr, m, v in ((V, dV, mom["mV"], mom["vV"]), (g, dg, mom["mg"], mom["vg"])):
        gr = gr + wd * w
        m.mul_(b1).add_(gr, alpha=1.0 - b1)
        v.mul_(b2).add_(gr * gr, alpha=1.0 - b2)
        w.sub_((lr / bc1) * m / (v.sqrt() / bc2 ** 0.5 + eps))
    return loss, dx, dV, dg


def zero_moments(V, g):
    return {"mV": torch.zeros_like(V), "vV": torch.zeros_like(V), "mg": torch.zeros_like(g), "vg": torch.zeros_like(g)}


class DistLinearTorch(nn.Module):
    """The torch statement of distLinear: WeightNorm on a bias-free nn.Linear."""

    def __init__(self, v0, g0):
        super().__init__()
        import warnings
        from torch.nn.utils.weight_norm import WeightNorm
        self.L = nn.Linear(v0.shape[1], v0.shape[0], bias=False).to(v0.dtype)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            WeightNorm.apply(self.L, 'weight', dim=0)
        with torch.no_grad():
            self.L.weight_v.copy_(v0)
            self.L.weight_g.copy_(g0.reshape(-1, 1))

    def forward(self, x):
        x_norm = torch.norm(x, p=2, dim=1).unsqueeze(1).expand_as(x)
        return 2 * self.L(x.div(x_norm + 0.00001))


def _close(a, b, tol=1e-12):
    return float((a - b).abs().max()) <= tol * max(float(b.abs().max()), 1e-300)


@pytest.mark.parametrize("k,n_way", [(5, 5), (1, 2)])
def test_head_step_restatement_matches_torch_autograd_and_adam(k, n_way):
    rs = np.random.RandomState(1000 * k + n_way)
    V = torch.from_numpy(rs.uniform(-1, 1, (n_way, 512)) / np.sqrt(512))
    g = V.norm(dim=1).clone()
    head = DistLinearTorch(V, g)
    opt = torch.optim.Adam(head.parameters(), lr=0.01, weight_decay=0.001)
    mom = zero_moments(V, g)
    for step in (1, 2, 3):
        x = torch.from_numpy(np.abs(rs.standard_normal((k, 512))))
        y = torch.from_numpy(rs.randint(0, n_way, k)).long()
        xt = x.clone().requires_grad_(True)
        opt.zero_grad()
        loss_t = F.cross_entropy(head(xt), y)
        loss_t.backward()
        dV_t, dg_t = head.L.weight_v.grad.clone(), head.L.weight_g.grad.reshape(-1).clone()
        opt.step()
        loss, dx, dV, dg = head_step64(x, y, V, g, mom, step)
        assert abs(float(loss) - float(loss_t.detach())) <= 1e-12 * abs(float(loss_t.detach()))
        assert _close(dx, xt.grad) and _close(dV, dV_t) and _close(dg, dg_t), step
        assert _close(V, head.L.weight_v.detach()) and _close(g, head.L.weight_g.detach().reshape(-1)), step
        st = opt.state[head.L.weight_v]
        assert _close(mom["mV"], st["exp_avg"]) and _close(mom["vV"], st["exp_avg_sq"]), step


def test_zero_feature_row_has_a_finite_gradient():
    rs = np.random.RandomState(3)
    V = torch.from_numpy(rs.uniform(-1, 1, (5, 512)) / np.sqrt(512))
    g = V.norm(dim=1).clone()
    x = torch.from_numpy(np.abs(rs.standard_normal((4, 512))))
    x[2] = 0
    y = torch.tensor([0, 1, 2, 3])
    xt = x.clone().requires_grad_(True)
    F.cross_entropy(DistLinearTorch(V, g)(xt), y).backward()
    _, dx, _, _ = head_step64(x, y, V.clone(), g.clone(), zero_moments(V, g), 1)
    assert bool(torch.isfinite(dx).all()) and _close(dx, xt.grad)
    assert float(dx[2].abs().max()) > 1.0                                  # dxh / eps_n


@pytest.fixture(scope="module")
def g25(golden_dir):
    return np.load(os.path.join(golden_dir, "g25_baselinepp_finetune.npz"))


def finetune_dist_episode64(sd, liz, v0, g0, n_way=5, n_support=5, epochs=20, batch_size=5):
    """finetune_linear's loop (finetune.py:45-174) in float64 with the head step above: oracle backbone, oracle Adam on trunk.7."""
    dt = torch.float64
    fsd = O.feature_state(O.clone_state(sd, dt))
    x0 = liz[0].to(dt)
    n_query = x0.shape[1] - n_support
    xa = x0[:, :n_support].contiguous().view(n_way * n_support, *x0.shape[2:])
    xb = x0[:, n_support:].contiguous().view(n_way * n_query, *x0.shape[2:])
    ya = torch.from_numpy(np.repeat(np.arange(n_way), n_support))
    S = n_way * n_support
    V = torch.as_tensor(v0).to(dt).clone()
    g = torch.as_tensor(g0).to(dt).reshape(-1).clone()
    mom = zero_moments(V, g)
    params = [fsd[k] for k in O.ADAPT_KEYS]
    adam_blk = O.adam_init(params)
    step = 0
    for _ in range(epochs):
        rand_id = np.random.permutation(S)
        for j in range(0, S, batch_size):
            sel = torch.from_numpy(rand_id[j:min(j + batch_size, S)])
            for t in params:
                t.requires_grad_(True)
            feat = O.resnet10_forward(fsd, xa[sel], "", train=True)
            step += 1
            _, dfeat, _, _ = head_step64(feat.detach(), ya[sel], V, g, mom, step)
            grads = torch.autograd.grad(feat, params, grad_outputs=dfeat)
            for t in params:
                t.requires_grad_(False)
            O.adam_step(params, list(grads), adam_blk, lr=0.01)
    with torch.no_grad():
        out = O.resnet10_forward(fsd, torch.cat([xa, xb], 0), "", train=True)[S:]
        xh = out / (out.norm(dim=1, keepdim=True) + EPS_N)
        return torch.softmax(2.0 * xh @ (g[:, None] * V / V.norm(dim=1, keepdim=True)).t(), dim=1)


def test_g25_fixture_is_a_usable_yardstick(g25):
    """What tools/make_golden_baselinepp_finetune.py asserts before it writes: the reference's three runs of an episode agree on
    every argmax, and its fp32 run is a finite, non-zero distance from its float64 run."""
    for ep in (91, 92):
        f32, f32_1, f64 = (g25["%s_%d" % (k, ep)] for k in ("scores_f32", "scores_f32_1thr", "scores_f64"))
        assert f64.shape == (75, 5) and g25["v0_%d" % ep].shape == (5, 512) and g25["g0_%d" % ep].shape == (5, 1)
        assert (f32.argmax(1) == f64.argmax(1)).all() and (f32_1.argmax(1) == f64.argmax(1)).all()
        top2 = np.sort(f64, 1)
        assert float((top2[:, -1] - top2[:, -2]).min()) >= 0.67
        assert 0.0 < np.abs(f32 - f64).max() < 5e-2
        assert np.allclose(np.linalg.norm(g25["v0_%d" % ep], axis=1), g25["g0_%d" % ep][:, 0], rtol=1e-6)


def test_float64_restatement_replays_g25(g25):
    """Episode 91: the same algorithm in float64 lands orders of magnitude inside 1 / 100 of the reference's own fp32-vs-fp64
    distance; another algorithm (another gradient, another optimiser epilogue, another draw order) does not."""
    sd = synthetic.gnnnet_state_dict(seed=37)
    liz = synthetic.test_episode(91, 5, 5, 15, 84, gen_examples=1)
    np.random.seed(10)
    sc = finetune_dist_episode64(sd, liz, g25["v0_91"], g25["g0_91"]).numpy()
    assert (np.random.permutation(7) == g25["next_perm_91"]).all()
    d = float(np.abs(sc - g25["scores_f64_91"]).max())
    bound = float(np.abs(g25["scores_f32_91"] - g25["scores_f64_91"]).max()) / 100.0
    print("float64 restatement vs the reference's float64 scores: %.3e (bound %.3e)" % (d, bound))
    assert d <= bound, (d, bound)


def test_baselinepp_draws_finetune_linear_permutations():
    np.random.seed(4)
    lin, gnn = ft.draw_episode_perms("baseline++", 5, 5, 19, 5)
    after = np.random.permutation(11)
    assert gnn is None and len(lin) == 20 and all(sorted(p.tolist()) == list(range(25)) for p in lin)
    np.random.seed(4)
    lin_b, gnn_b = ft.draw_episode_perms("baseline", 5, 5, 19, 5)
    assert gnn_b is None and all((a == b).all() for a, b in zip(lin, lin_b))
    assert (np.random.permutation(11) == after).all()                     # the numpy stream is left where "baseline" leaves it


def test_baselinepp_checkpoint_lookup(tmp_path, monkeypatch):
    """finetune.baselinepp_checkpoint_file: the directory train.main --method baseline++ writes (no _<n>way_<k>shot suffix)."""
    from meta_fine_tuning_amd import configs
    monkeypatch.setattr(configs, "save_dir", str(tmp_path))
    base = str(tmp_path) + "/checkpoints/miniImageNet/"
    P = lambda *a: io_utils.parse_args('train', list(a))                    # noqa: E731
    assert ft.baselinepp_checkpoint_file(P("--method", "baseline++", "--save_iter", "0")) == base + "ResNet10_baseline++/0.tar"
    assert ft.baselinepp_checkpoint_file(P("--method", "baseline++", "--save_iter", "399", "--train_aug", "--n_shot", "20")) == \
        base + "ResNet10_baseline++_aug/399.tar"
    assert ft.baselinepp_checkpoint_file(P("--method", "baseline++")) is None                 # empty / absent directory
    d = tmp_path / "checkpoints" / "miniImageNet" / "ResNet10_baseline++"
    d.mkdir(parents=True)
    for name in ("3.tar", "12.tar", "best_model.tar"):
        (d / name).write_bytes(b"")
    assert ft.baselinepp_checkpoint_file(P("--method", "baseline++")) == str(d / "12.tar")    # the newest epoch, not best_model
    # the reference's own lookup for this method stays what it is: a directory train.main never writes
    assert ft.checkpoint_files(P("--method", "baseline++", "--save_iter", "5")) == (base + "ResNet10_baseline++_5way_5shot/5.tar", None)
    # a missing file is an error; the stand-in backbone is an explicit opt-in
    monkeypatch.delenv("MFT_STANDIN_WEIGHTS", raising=False)
    with pytest.raises(FileNotFoundError):
        ft._resolve_state("baseline++", base + "ResNet10_baseline++/77.tar", 5, True, False)
    monkeypatch.setenv("MFT_STANDIN_WEIGHTS", "1")
    sd, used = ft._resolve_state("baseline++", base + "ResNet10_baseline++/77.tar", 5, True, False)
    assert used is None and any(k.startswith("feature.trunk.7.") for k in sd)
