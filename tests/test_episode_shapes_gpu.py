"""Meta-training at episode shapes other than 5-way 5-shot on a real MI355X: the GnnNet head (fc + GNN_nl + score gather) forward
and hand-written backward against float64 autograd from 2- to 32-way and up to N = 260 graph nodes, two episodes in lockstep,
whole GnnNet.set_forward_loss(...).backward() steps at the shapes of golden G21 (the reference's own fp32 run), the hipGraph loop and
the lockstep step at 20-way, and the scratch-buffer free list across head configurations that share a buffer shape."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import meta_fine_tuning_amd  # noqa: F401
from meta_fine_tuning_amd import autograd_ops as AG
from meta_fine_tuning_amd import functional_bwd as FB
from meta_fine_tuning_amd import synthetic
from meta_fine_tuning_amd.io_utils import model_dict
from meta_fine_tuning_amd.methods.gnnnet import GnnNet
from oracle import mft_oracle as O

pytestmark = pytest.mark.gpu
torch.set_num_threads(8)

# (n_way, n_shot, n_query): N = n_way * (n_shot + 1) graph nodes
HEAD_SHAPES = [
    (2, 1, 16),      # N = 4: the smallest graph
    (2, 1, 1),       # fc BatchNorm1d over 4 rows
    (5, 1, 16),      # 1-shot
    (3, 4, 4),       # N = 15
    (5, 5, 16),      # the 5-way 5-shot control
    (10, 5, 8),      # N = 60
    (16, 5, 5),      # N = 96: the widest the column-sum of layer_last's bias gradient covered in one chunk
    (17, 1, 4),      # N = 34: the first width past 16 columns
    (20, 5, 4),      # N = 120
    (32, 1, 2),      # N = 64: the pair-softmax backward's form boundary; last Wcompute input K = Kpad = 256
    (13, 4, 6),      # N = 65: just past it
    (5, 20, 16),     # N = 105
    (10, 25, 2),     # N = 260 > 256
]
G21_SHAPES = [(20, 5, 4, 41, 51), (32, 1, 2, 42, 52), (3, 4, 4, 43, 53), (5, 20, 16, 44, 54)]     # = oracle/make_golden_g21.py SHAPES

# Bars of the head against float64, from a measurement over all HEAD_SHAPES rows and both lockstep rows on an MI355X (largest
# measured error in brackets).  The forward is fp32 rounding only.  Backward: a pair-MLP pre-activation within rounding of 0 can
# take the other leaky_relu slope (1 vs 0.01) in fp32, which moves the gradients behind the Wcomputes -- most of all the BatchNorm
# parameters of the pair MLP, summed over every pair position -- by up to a few 1e-2 of a tensor at the smallest graphs
# (2-way 1-shot: BatchNorm over 256 positions).  layer_last's fc.weight / fc.bias gradients depend on the forward and the scores'
# gradient only, so they are held far tighter: one column of the bias gradient left out at 17-way is 4.7e-2 of its norm, a
# wrong d(out) row stride is O(1) everywhere.
SCORE_BAR = 1e-5          # max |score - score64| / max(1, max |score64|)                        [1.5e-6]
LOSS_BAR = 1e-6           # |loss - loss64| / max(1, loss64)                                      [1.1e-7]
LAST_BAR = 1e-5           # ||g - g64|| / ||g64|| of gnn.layer_last.fc.weight / .bias          [1.1e-6]
REL_BAR = 3e-2            # every other gradient tensor and d(feats): ||g - g64|| / ||g64||       [1.5e-2]
MAX_BAR = 0.1             # ... and max |g - g64| / max |g64|                                      [3.5e-2]


def _head_model(n_way, n_support, seed):
    m = GnnNet(model_dict['ResNet10'], n_way=n_way, n_support=n_support)
    m.load_state_dict(synthetic.gnnnet_state_dict(seed=seed, n_way=n_way))
    m = m.cuda()
    m.train()
    return m


def _feats(n_way, ns, nq, seed, episodes=1):
    """Non-negative feature rows (pooled ReLU output), class after class, supports then queries, one episode after the other."""
    rs = np.random.RandomState(seed)
    return torch.from_numpy(np.abs(rs.standard_normal((episodes * n_way * (ns + nq), 512))).astype(np.float32))


def _head_params(model):
    return [("fc." + n, p) for n, p in model.fc.named_parameters()] + [("gnn." + n, p) for n, p in model.gnn.named_parameters()]


def _oracle_head(sd32, feats, n_way, ns, nq, episodes=1):
    """float64 fc + GNN_nl + cross entropy per episode (BatchNorm statistics per episode), mean over the episodes' losses."""
    sd = O.clone_state(sd32, torch.float64)
    keys = [k for k, v in sd.items() if (k.startswith("fc.") or k.startswith("gnn.")) and v.is_floating_point() and "running" not in k]
    for k in keys:
        sd[k].requires_grad_(True)
    f = feats.double().requires_grad_(True)
    per = n_way * (ns + nq)
    y = torch.from_numpy(np.repeat(np.arange(n_way), nq))
    scores, loss = [], 0.0
    for e in range(episodes):
        z = O.fc_project(sd, f[e * per:(e + 1) * per]).view(n_way, ns + nq, 128)
        sc = O.gnnnet_scores_from_z(sd, z, n_way, ns, nq)
        scores.append(sc)
        loss = loss + F.cross_entropy(sc, y) / episodes
    grads = torch.autograd.grad(loss, [f] + [sd[k] for k in keys])
    return torch.cat(scores).detach(), float(loss), grads[0], dict(zip(keys, grads[1:]))


def _head_errors(model, feats, n_way, ns, nq, episodes=1):
    """-> (forward scores error, taped scores error, loss error, dfeats (rel, max), {param: (rel, max)}) against float64."""
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    ref_sc, ref_loss, ref_df, ref_g = _oracle_head(sd, feats, n_way, ns, nq, episodes)
    fd = feats.cuda()
    with torch.no_grad():
        sc_fwd = AG.gnnnet_head(model, fd, ns, nq, episodes=episodes)
    fg = fd.clone().requires_grad_(True)
    for _, p in _head_params(model):
        p.grad = None
    sc = AG.gnnnet_head(model, fg, ns, nq, episodes=episodes)
    y = torch.from_numpy(np.tile(np.repeat(np.arange(n_way), nq), episodes)).cuda()
    loss = model.loss_fn(sc, y)
    loss.backward()
    torch.cuda.synchronize()
    scale = max(1.0, float(ref_sc.abs().max()))
    e_fwd = float((sc_fwd.cpu().double() - ref_sc).abs().max()) / scale
    e_tap = float((sc.detach().cpu().double() - ref_sc).abs().max()) / scale
    e_loss = abs(float(loss) - ref_loss) / max(1.0, ref_loss)

    def err(got, want):
        got = got.detach().cpu().double()
        return float((got - want).norm()) / float(want.norm()), float((got - want).abs().max()) / float(want.abs().max())

    errs = {}
    zeros = {}
    for name, p in _head_params(model):
        assert p.grad is not None and p.grad.shape == p.shape, name
        r = ref_g[name]
        if float(r.norm()) < 1e-9:                     # a bias in front of a BatchNorm: identically zero in float64
            zeros[name] = float(p.grad.abs().max())
            continue
        errs[name] = err(p.grad, r)
    return e_fwd, e_tap, e_loss, err(fg.grad, ref_df), errs, zeros


def _check_head(n_way, ns, nq, episodes, seed):
    model = _head_model(n_way, ns, seed)
    feats = _feats(n_way, ns, nq, seed + 100, episodes)
    e_fwd, e_tap, e_loss, e_df, errs, zeros = _head_errors(model, feats, n_way, ns, nq, episodes)
    last = ("gnn.layer_last.fc.weight", "gnn.layer_last.fc.bias")
    worst = max(((k, v) for k, v in errs.items() if k not in last), key=lambda kv: kv[1][0])
    print("head %2d-way %2d-shot %2d-query x%d: scores %.2e / %.2e, loss %.2e, layer_last.fc %.2e / %.2e, dfeats %.2e / %.2e, "
          "worst other %s %.2e / %.2e, zero-gradient biases %.1e" % (n_way, ns, nq, episodes, e_fwd, e_tap, e_loss, errs[last[0]][0],
                                                                    errs[last[1]][0], e_df[0], e_df[1], worst[0], worst[1][0],
                                                                    worst[1][1], max(zeros.values())))
    assert e_fwd < SCORE_BAR and e_tap < SCORE_BAR, (e_fwd, e_tap)
    assert e_loss < LOSS_BAR, e_loss
    assert e_df[0] < REL_BAR and e_df[1] < MAX_BAR, e_df
    for name, (rel, mx) in errs.items():
        assert rel < (LAST_BAR if name in last else REL_BAR) and mx < MAX_BAR, (name, rel, mx)
    # fc.0.bias and every Gconv's fc.bias but layer_last's sit in front of a BatchNorm; conv2d_*.bias of the Wcomputes too
    assert "fc.0.bias" in zeros and "gnn.layer_last.fc.bias" in errs
    for name, mx in zeros.items():
        assert mx < 1e-5, (name, mx)


@pytest.mark.parametrize("n_way,n_shot,n_query", HEAD_SHAPES)
def test_head_forward_backward_vs_float64(n_way, n_shot, n_query):
    """autograd_ops.gnnnet_head under no_grad (Fn.gnnnet_scores) and with autograd (head_forward_taped + head_backward) against
    O.fc_project + O.gnnnet_scores_from_z + cross entropy in float64: scores, loss, d(feats) and every fc.* / gnn.* gradient."""
    _check_head(n_way, n_shot, n_query, 1, seed=60 + n_way + n_shot)


@pytest.mark.parametrize("n_way,n_shot,n_query", [(3, 4, 4), (20, 5, 4)])
def test_head_lockstep_vs_two_float64_episodes(n_way, n_shot, n_query):
    """Two episodes in lockstep (separate BatchNorm statistics per episode) against two separate float64 episodes, losses and
    gradients averaged."""
    _check_head(n_way, n_shot, n_query, 2, seed=80 + n_way)


def _head_grads(model, feats, ns, nq):
    fg = feats.cuda().requires_grad_(True)
    for _, p in _head_params(model):
        p.grad = None
    sc = AG.gnnnet_head(model, fg, ns, nq)
    y = torch.from_numpy(np.repeat(np.arange(model.n_way), nq)).cuda()
    model.loss_fn(sc, y).backward()
    torch.cuda.synchronize()
    return [sc.detach().clone(), fg.grad.clone()] + [p.grad.clone() for _, p in _head_params(model)]


@pytest.mark.parametrize("first", ["3w4s4q", "5w5s16q"])
def test_scratch_free_list_across_head_shapes(first):
    """FB.ZeroLease hands out zero-padded scratch buffers keyed by shape: the Wcompute score gradient of a (3-way, 4-shot, 4-query)
    step is a (480, 32) buffer -- as is layer_last's raw output of a (5-way, 5-shot, 16-query) step, whose columns 0..4 hold
    values.  A step must give bit-identical results whether its buffers come fresh or from the other configuration's step."""
    small = _head_model(3, 4, seed=71)
    big = _head_model(5, 5, seed=72)
    f_small, f_big = _feats(3, 4, 4, 171), _feats(5, 5, 16, 172)
    runs = {"3w4s4q": (small, f_small, 4, 4), "5w5s16q": (big, f_big, 5, 16)}
    second = "5w5s16q" if first == "3w4s4q" else "3w4s4q"
    m, f, ns, nq = runs[second]
    FB.ZeroLease._free.clear()
    clean = _head_grads(m, f, ns, nq)
    FB.ZeroLease._free.clear()
    _head_grads(*runs[first])                        # its buffers go back to the free list when its tape dies
    assert any(k[0] == (480, 32) for k in FB.ZeroLease._free)
    after = _head_grads(m, f, ns, nq)
    for a, b in zip(clean, after):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------- whole meta-training steps (G21)
def _oracle_grads(sd32, x, n_way, n_support):
    sd = O.clone_state(sd32, torch.float64)
    pkeys = [k for k, v in sd.items() if v.is_floating_point() and "running" not in k]
    for k in pkeys:
        sd[k].requires_grad_(True)
    loss, scores = O.meta_train_loss(sd, x.double(), n_way, n_support)
    grads = torch.autograd.grad(loss, [sd[k] for k in pkeys])
    return float(loss.detach()), scores.detach(), dict(zip(pkeys, grads))


@pytest.mark.parametrize("n_way,n_shot,n_query,wseed,xseed", G21_SHAPES)
def test_set_forward_loss_backward_at_episode_shapes(golden_dir, n_way, n_shot, n_query, wseed, xseed):
    """GnnNet.set_forward_loss(x).backward() through ResNet10 and the head at the G21 shapes, against the float64 oracle (the bars
    and the ReLU sign-flip allowance of test_set_forward_loss_backward_all_parameters) and the reference's fp32 loss, scores,
    gradient norms and slices."""
    g = np.load(os.path.join(golden_dir, "g21_episode_shapes.npz"))
    t = "%dw%ds%dq" % (n_way, n_shot, n_query)
    sd = synthetic.gnnnet_state_dict(seed=wseed, n_way=n_way)
    model = GnnNet(model_dict['ResNet10'], n_way=n_way, n_support=n_shot)
    model.load_state_dict(sd)
    model = model.cuda()
    model.train()
    x = synthetic.train_episode(xseed, n_way, n_shot, n_query, 84)
    model.n_query = n_query
    loss = model.set_forward_loss(x)
    loss.backward()
    assert abs(float(loss.detach()) - float(g["loss_" + t])) < 2e-4
    ref_loss, ref_scores, ref = _oracle_grads(sd, x, n_way, n_shot)
    assert abs(float(loss.detach()) - ref_loss) < 2e-4
    named = dict(model.named_parameters())
    assert len(named) == 104
    rels = []
    for k, gr in ref.items():
        got = named[k].grad
        assert got is not None, k
        nrm = float(gr.norm())
        if nrm < 1e-9:
            assert float(got.norm()) < 1e-5, k
            continue
        rel = float((got.cpu().double() - gr).norm()) / nrm
        mx = float((got.cpu().double() - gr).abs().max()) / float(gr.abs().max())
        rels.append((rel, k))
        assert rel < 3e-2 and mx < 0.15, (k, rel, mx)
    print("step %s: loss %.2e from float64, worst relative gradient error %.2e (%s), median %.2e"
          % (t, abs(float(loss.detach()) - ref_loss), max(rels)[0], max(rels)[1], float(np.median([r for r, _ in rels]))))
    gn = {k: float(p.grad.norm()) for k, p in named.items()}
    for name, refn in zip(g["gradnames_" + t], g["gradnorms_" + t]):
        assert abs(gn[str(name)] - refn) <= 5e-3 * refn + 1e-6, name

    def near(got, want, floor):
        np.testing.assert_allclose(got.cpu().numpy(), want, atol=max(floor, 3e-3 * float(np.abs(want).max())))
    near(named["fc.0.weight"].grad[:4, :8], g["grad_fc0w_slice_" + t], 2e-5)
    near(named["gnn.layer_last.fc.weight"].grad[:, :8], g["grad_lastw_slice_" + t], 2e-5)
    near(named["gnn.layer_last.fc.bias"].grad, g["grad_lastb_" + t], 2e-5)


def test_lockstep_20way_matches_accumulated_single_episodes():
    """set_forward_loss_lockstep over 2 episodes of 20-way 5-shot 4-query against the 2 episodes one by one from the same
    parameters, losses and gradients averaged (test_lockstep_episodes_match_accumulated_single_episodes at 5-way)."""
    n_way, ns, nq, k = 20, 5, 4, 2
    sd = synthetic.gnnnet_state_dict(seed=31, n_way=n_way)
    xs = torch.stack([synthetic.train_episode(320 + i, n_way, ns, nq, 84) for i in range(k)]).cuda()

    def fresh():
        m = GnnNet(model_dict['ResNet10'], n_way=n_way, n_support=ns)
        m.load_state_dict(sd)
        m = m.cuda()
        m.train()
        m.n_query = nq
        return m

    ref_scores, ref_loss = [], 0.0
    acc = {n: torch.zeros_like(p, dtype=torch.float64) for n, p in fresh().named_parameters()}
    for i in range(k):
        m = fresh()
        sc = m.set_forward(xs[i])
        loss = m.loss_fn(sc, m._y_query())
        loss.backward()
        ref_scores.append(sc.detach())
        ref_loss += float(loss) / k
        for n, p in m.named_parameters():
            acc[n] += p.grad.double() / k
    model = fresh()
    loss = model.set_forward_loss_lockstep(xs)
    assert abs(float(loss) - ref_loss) < 1e-5
    loss.backward()
    scores = fresh().set_forward_lockstep(xs)
    assert scores.shape == (k * n_way * nq, n_way)
    got_sc = scores.detach().view(k, n_way * nq, n_way)
    for i in range(k):
        assert float((got_sc[i] - ref_scores[i]).abs().max()) < 2e-4, i
    rels = []
    for n, p in model.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape, n
        r = acc[n]
        nrm = float(r.norm())
        if nrm < 1e-9:
            assert float(p.grad.abs().max()) < 1e-6, n
            continue
        rel = float((p.grad.double() - r).norm()) / nrm
        rels.append(rel)
        assert rel < 1e-2, (n, rel)
    assert float(np.median(rels)) < 2e-3, float(np.median(rels))
