"""TPN on a real MI355X: the label-propagation head kernels (csrc/tpn.hip) against float64 with the float32 CPU chain as the
yardstick -- the discontinuous neighbour mask apart from the values --, the meta-training step against the float64 oracle and the
golden G30, lockstep episodes, the graphed episode loop, the `test` driver's lockstep scoring and train.main --method tpn."""
import functools
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import meta_fine_tuning_amd  # noqa: F401
from meta_fine_tuning_amd import _lib, feature_eval, ops, synthetic
from meta_fine_tuning_amd import autograd_ops as AG
from meta_fine_tuning_amd.io_utils import model_dict
from meta_fine_tuning_amd.methods.tpn import TPN
from oracle import mft_oracle as O

pytestmark = pytest.mark.gpu
torch.set_num_threads(8)

EPS = np.finfo(float).eps
K, ALPHA = 20, 0.99
HEAD = ["relation.fc3.weight", "relation.fc3.bias", "relation.fc4.weight", "relation.fc4.bias"]


def _g30(golden_dir):
    return np.load(os.path.join(golden_dir, "g30_tpn.npz"))


def tpn_chain(feats, head, n_way, n_support, n_query, episodes=1, k=K, alpha=ALPHA, mask=None, taps=None):
    """The seven steps of DESIGN.md section 18 on feature rows [episodes*n_way*(n_support+n_query), D] in the dtype of ``feats``
    (float64: the reference; float32: the yardstick); differentiable in feats and the head; ``mask`` [episodes, N, N] replaces the
    neighbour selection (it is symmetrised like the selection).  -> (scores [episodes*n_way*n_query, n_way], W before the mask
    [episodes, N, N], the symmetrised mask).  ``taps``: a list that receives (z, h, sigma) per episode, h and sigma keeping their
    gradients."""
    w3, b3, w4, b4 = head
    z_all = feats.view(episodes, n_way, n_support + n_query, -1)
    S, Q = n_way * n_support, n_way * n_query
    N = S + Q
    out, Ws, masks = [], [], []
    for e in range(episodes):
        z = torch.cat([z_all[e, :, :n_support].reshape(S, -1), z_all[e, :, n_support:].reshape(Q, -1)])
        h = z @ w3.t() + b3
        sigma = torch.relu(h) @ w4.t() + b4
        if taps is not None:
            h.retain_grad()
            sigma.retain_grad()
            taps.append((z, h, sigma))
        u = z / (sigma + EPS)
        W = torch.exp(-((u.unsqueeze(1) - u.unsqueeze(0)) ** 2).sum(2) / 2)
        if mask is None:
            idx = torch.sort(W.detach(), dim=1, descending=True, stable=True).indices[:, :min(k, N)]
            m = torch.zeros(N, N, dtype=W.dtype).scatter_(1, idx, 1.0)
        else:
            m = mask[e].to(W.dtype)
        m = ((m + m.t()) > 0).to(W.dtype)
        Ws.append(W.detach())
        masks.append(m)
        W = W * m
        r = torch.sqrt(1.0 / (W.sum(0) + EPS))
        Sn = r.unsqueeze(1) * W * r.unsqueeze(0)
        Y = torch.zeros(N, n_way, dtype=W.dtype)
        Y[torch.arange(S), torch.arange(S) // n_support] = 1.0
        out.append(torch.linalg.solve(torch.eye(N, dtype=W.dtype) - alpha * Sn, Y)[S:])
    return torch.cat(out), torch.stack(Ws), torch.stack(masks)


def _head(dtype=torch.float32, device="cpu"):
    hs = synthetic.tpn_head_state(30)
    return tuple(hs[k].to(device=device, dtype=dtype) for k in HEAD)


# ------------------------------------------------------------------------------------------------ kernels
# ((E, n_way, n_support, n_query), k): the training and the test shape, N < k, n_way = 1, the multi-episode stride, N = k, N = k + 1,
# the 64 boundary of the row selection, 20-shot, 50-shot with one query, the limits N = 256 and n_way = 32, and a small k
CASES = [((1, 5, 5, 16), K), ((1, 5, 5, 15), K), ((1, 2, 1, 1), K), ((2, 1, 1, 2), K), ((3, 3, 2, 3), K), ((1, 4, 2, 3), K),
         ((1, 3, 2, 5), K), ((1, 8, 7, 1), K), ((1, 5, 12, 1), K), ((1, 5, 20, 15), K), ((1, 5, 50, 1), K), ((1, 32, 7, 1), K),
         ((1, 3, 2, 3), 3)]
KINDS = ["randn", "relu"]
CASE_IDS = ["E%d_w%d_s%d_q%d_k%d" % (s + (k,)) for s, k in CASES]


def _nodes(shape):
    return shape[1] * (shape[2] + shape[3])


def _draws(shape):
    return 2 if _nodes(shape) >= 175 else 3


def _features(kind, shape, draw):
    # the recipe of tests/test_metaoptnet_gpu.py::_features
    E, n_way, ns, nq = shape
    g = torch.Generator().manual_seed(1000003 * draw + 7919 * E + 131 * n_way + 17 * ns + nq + (0 if kind == "randn" else 500000))
    f = torch.randn(E, n_way, ns + nq, 512, generator=g)
    if kind == "relu":          # non-negative and class-structured, as trunk outputs are
        mean = torch.randn(E, n_way, 1, 512, generator=g)
        f = torch.relu(0.5 * f + 0.5 * mean + 0.3)
    G = torch.randn(E * n_way * nq, n_way, generator=g)
    return f.reshape(-1, 512).contiguous(), G


def _kth(W, k):
    """[E, N, 1]: every row's min(k, N)-th largest entry."""
    return torch.sort(W, dim=2, descending=True).values[:, :, min(k, W.shape[2]) - 1:min(k, W.shape[2])]


@functools.lru_cache(maxsize=None)
def _references():
    """Every (case, kind, draw): inputs, the float64 affinities and mask, and the largest relative distance of the float32 CPU
    chain's W to the float64 W among the entries that can decide a selection (those not below their row's (k+1)-th largest: a
    smaller entry is not selected however it is rounded).  tau = 16 x the largest such distance over all inputs; the 16 allows for
    a device summation order that differs from torch's.  Computed once for the module and never modified."""
    refs, dist = {}, 0.0
    h64, h32 = _head(torch.float64), _head(torch.float32)
    for shape, k in CASES:
        E, n_way, ns, nq = shape
        for kind in KINDS:
            for draw in range(_draws(shape)):
                f, G = _features(kind, shape, draw)
                with torch.no_grad():
                    _, W64, m64 = tpn_chain(f.double(), h64, n_way, ns, nq, E, k=k)
                    _, W32, _ = tpn_chain(f, h32, n_way, ns, nq, E, k=k)
                if _nodes(shape) > k:
                    decisive = W64 >= _kth(W64, k + 1)
                    dist = max(dist, float(((W32.double() - W64).abs() / W64)[decisive].max()))
                refs[(shape, k, kind, draw)] = dict(f=f, G=G, W=W64, mask=m64)
    return refs, 16.0 * dist


def _ambiguous(W64, k, tau):
    """Entries (i, j) whose float64 affinity is within relative tau of the k-th largest of row i or of row j -- and, of those, only
    the ones a rounding can move across the selection's edge: a row's k-th largest entry is always within tau of itself, but it
    (like every other selected entry) can only drop out when it is also within tau of the (k+1)-th largest, the entry that would
    take its place.  With N <= k every entry is selected whatever its value: nothing is ambiguous."""
    N = W64.shape[2]
    if N <= k:
        return torch.zeros_like(W64, dtype=torch.bool)
    kth, nxt = _kth(W64, k), _kth(W64, k + 1)
    idx = torch.sort(W64, dim=2, descending=True, stable=True).indices[:, :, :k]
    selected = torch.zeros_like(W64, dtype=torch.bool).scatter_(2, idx, True)
    near = ((W64 - kth).abs() <= tau * kth) & (~selected | (W64 - nxt <= tau * kth))
    return near | near.transpose(1, 2)


def _assert_mask_rule(dev_mask, W64, m64, k, tau, what):
    amb = _ambiguous(W64, k, tau)
    differ = dev_mask.cpu().double() != m64
    E, N = W64.shape[0], W64.shape[1]
    print("tpn mask %s: tau %.3e, %d entries differ, %d ambiguous of E*N*k = %d" % (what, tau, int(differ.sum()), int(amb.sum()), E * N * k))
    assert int(amb.sum()) <= 0.10 * E * N * k, (what, int(amb.sum()))           # the rule cannot hide a failure
    assert not bool((differ & ~amb).any()), (what, int((differ & ~amb).sum()))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_unforced_mask_differs_from_float64_only_where_ambiguous(case, kind):
    refs, tau = _references()
    shape, k = case
    E, n_way, ns, nq = shape
    head = _head(device="cuda")
    for draw in range(_draws(shape)):
        r = refs[(shape, k, kind, draw)]
        _, tape = ops.tpn_forward(r["f"].cuda(), head, E, n_way, ns, nq, k=k, save=True)
        assert tape["mask"].shape == r["mask"].shape and tape["mask"].dtype == torch.uint8 and tape["W"].shape == r["W"].shape
        _assert_mask_rule(tape["mask"], r["W"], r["mask"], k, tau, "%s %s draw %d" % (case, kind, draw))
        if (shape == (1, 5, 5, 15) and kind == "relu") or _nodes(shape) <= k:
            # 20 class members per row with a gap of at least 0.12 behind them; or every entry is a neighbour
            assert torch.equal(tape["mask"].cpu().double(), r["mask"]), (case, kind, draw)
        dW = float(((tape["W"].cpu().double() - r["W"]).abs() / r["W"])[r["mask"] > 0].max())
        print("tpn W %s %s draw %d: largest relative distance of a kept device affinity to float64 %.3e" % (case, kind, draw, dW))


def test_the_wide_gap_input_has_its_gap():
    refs, tau = _references()
    for draw in range(3):
        W = refs[((1, 5, 5, 15), K, "relu", draw)]["W"]
        srt = torch.sort(W, dim=2, descending=True).values
        assert float(((srt[:, :, K - 1] - srt[:, :, K]) / srt[:, :, K - 1]).min()) >= 0.12
    assert 0.0 < tau < 1e-3, tau


def _rel_per_episode(got, want, E):
    got, want = got.reshape(E, -1), want.reshape(E, -1)
    return [float((got[e] - want[e]).norm() / want[e].norm()) for e in range(E)]


def _chain_step(f, G, shape, k, mask, dtype):
    """Forward + backward of the chain in ``dtype`` on the given mask -> scores, dfeats, the four parameter gradients (float64)
    and, per parameter, the sum over the nodes of the absolute values of the terms its gradient adds up."""
    E, n_way, ns, nq = shape
    x = f.to(dtype).requires_grad_(True)
    head = [p.clone().requires_grad_(True) for p in _head(dtype)]
    taps = []
    scores, _, _ = tpn_chain(x, head, n_way, ns, nq, E, k=k, mask=mask, taps=taps)
    (scores * G.to(dtype)).sum().backward()
    dh = torch.cat([h.grad for _, h, _ in taps]).double().abs()
    dsig = torch.cat([s.grad for _, _, s in taps]).double().abs()
    z = torch.cat([z for z, _, _ in taps]).detach().double().abs()
    a = torch.relu(torch.cat([h for _, h, _ in taps]).detach().double())
    denoms = [float((dh.t() @ z).norm()), float(dh.sum(0).norm()), float((dsig * a).sum(0).norm()), float(dsig.sum())]
    return scores.detach().double(), x.grad.double(), [p.grad.double() for p in head], denoms


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_kernels_match_float64_within_4x_the_float32_chain(case, kind):
    """Values on the device's own mask: scores, dfeats and the four parameter gradients within 4 x the distance of the float32 CPU
    chain to float64 on the same inputs and the same mask (the maximum over the draws of the shape and kind); a parameter
    gradient's distance is taken relative to the sum of the absolute values of its terms, which does not cancel."""
    refs, _ = _references()
    shape, k = case
    E, n_way, ns, nq = shape
    head = _head(device="cuda")
    runs = []
    for draw in range(_draws(shape)):
        r = refs[(shape, k, kind, draw)]
        scores, tape = ops.tpn_forward(r["f"].cuda(), head, E, n_way, ns, nq, k=k, save=True)
        grads = ops.tpn_backward(tape, r["G"].cuda())
        assert scores.shape == (E * n_way * nq, n_way) and grads[0].shape == r["f"].shape
        assert [tuple(g.shape) for g in grads[1:]] == [(8, 512), (8,), (1, 8), (1,)]
        mask = tape["mask"].cpu()
        s64, d64, p64, den = _chain_step(r["f"], r["G"], shape, k, mask, torch.float64)
        s32, d32, p32, _ = _chain_step(r["f"], r["G"], shape, k, mask, torch.float32)
        den = [max(d, 1e-300) for d in den]
        yard = [max(_rel_per_episode(s32, s64, E)), max(_rel_per_episode(d32, d64, E))]
        yard += [float((a - b).norm()) / d for a, b, d in zip(p32, p64, den)]
        err = [max(_rel_per_episode(scores.cpu().double(), s64, E)), max(_rel_per_episode(grads[0].cpu().double(), d64, E))]
        err += [float((g.cpu().double() - b).norm()) / d for g, b, d in zip(grads[1:], p64, den)]
        runs.append((err, yard))
    names = ["scores", "dfeats", "dW3", "db3", "dW4", "db4"]
    yard = [max(y[i] for _, y in runs) for i in range(6)]
    for draw, (err, _) in enumerate(runs):
        print("tpn %s %s draw %d: " % (case, kind, draw)
              + "  ".join("%s %.3e (yardstick %.3e, ratio %.2f)" % (n, e, y, e / max(y, 1e-300)) for n, e, y in zip(names, err, yard)))
    for draw, (err, _) in enumerate(runs):
        for n, e, y in zip(names, err, yard):
            assert e <= 4.0 * y, (draw, n, e, y)


def _run(f, G, shape, k=K, head=None):
    E, n_way, ns, nq = shape
    scores, tape = ops.tpn_forward(f, head or _head(device="cuda"), E, n_way, ns, nq, k=k, save=True)
    return (scores, tape["mask"], tape["W"]) + tuple(ops.tpn_backward(tape, G))


@pytest.mark.parametrize("shape", [(3, 3, 2, 3), (1, 5, 5, 16), (1, 32, 7, 1)], ids=lambda s: "E%d_w%d_s%d_q%d" % s)
def test_two_calls_are_bit_identical(shape):
    r = _references()[0][(shape, K, "relu", 0)]
    f, G = r["f"].cuda(), r["G"].cuda()
    for x, y in zip(_run(f, G, shape), _run(f, G, shape)):
        assert torch.equal(x, y)


def test_episodes_in_one_call_equal_single_calls():
    shape = (3, 3, 2, 3)
    r = _references()[0][(shape, K, "relu", 1)]
    f, G = r["f"].cuda(), r["G"].cuda()
    together = _run(f, G, shape)
    N, Q = 15, 9
    singles = [_run(f[e * N:(e + 1) * N], G[e * Q:(e + 1) * Q], (1, 3, 2, 3)) for e in range(3)]
    for i in range(4):                                   # scores, mask, W, dfeats: episode after episode
        assert torch.equal(together[i].reshape(3, -1), torch.stack([s[i].reshape(-1) for s in singles])), i
    # the parameter gradients add the episodes up in row order: the one-call sum is the float64 sum of the single calls, rounded
    for i in range(4, 8):
        want = sum(s[i].double() for s in singles)
        scale = sum(float(s[i].abs().max()) for s in singles)                  # (every single result carries its own rounding)
        assert float((together[i].double() - want).abs().max()) <= 2.0 ** -22 * scale, i


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_non_finite_features_give_non_finite_output_and_the_call_returns(bad):
    r = _references()[0][((1, 5, 5, 16), K, "relu", 0)]
    f = r["f"].clone()
    f[3, 7] = bad
    out = _run(f.cuda(), r["G"].cuda(), (1, 5, 5, 16))
    torch.cuda.synchronize()
    assert not bool(torch.isfinite(out[0]).all())
    f = torch.full_like(r["f"], bad)
    out = _run(f.cuda(), r["G"].cuda(), (1, 5, 5, 16))
    torch.cuda.synchronize()
    assert not bool(torch.isfinite(out[0]).any())


def test_out_of_range_arguments_are_refused():
    lib = _lib.lib()
    p = ops._p
    f = torch.zeros(300, 520, device="cuda")
    w3, b3, w4, b4 = _head(device="cuda")
    ws = torch.zeros(8, 1 << 18, device="cuda")
    dbl = torch.zeros(2, 4096, device="cuda", dtype=torch.float64)
    msk = torch.zeros(1 << 16, device="cuda", dtype=torch.uint8)
    st = ops._stream(f)

    def call_all(a):
        shp = (a["E"], a["n_way"], a["ns"], a["nq"], a["D"])
        u, hid, W, L, Fm, rinv, scores, dd = ws
        return [lib.mft_tpn_embed(p(f), a["ld"], *shp, p(w3), p(b3), p(w4), p(b4), p(u), p(hid), p(dbl[0]), st),
                lib.mft_tpn_affinity(*shp, p(u), p(W), st),
                lib.mft_tpn_propagate(*shp, p(W), a["k"], 0.99, None, p(L), p(Fm), p(msk), p(rinv), p(scores), st),
                lib.mft_tpn_propagate_backward(*shp, p(W), 0.99, p(L), p(Fm), p(msk), p(rinv), p(scores), max(a["n_way"], 1), p(dd), st),
                lib.mft_tpn_affinity_backward(*shp, p(u), p(hid), p(dbl[0]), p(dd), p(w3), p(w4), p(ws[6]), 512, p(dbl[1]), st),
                lib.mft_tpn_param_backward(p(f), a["ld"], *shp, p(hid), p(dbl[1]), p(ws[0]), p(ws[1]), p(ws[2]), p(ws[3]), st)]

    good = dict(ld=520, E=1, n_way=5, ns=5, nq=16, D=512, k=20)
    assert call_all(good) == [0] * 6
    for b in [dict(n_way=1, ns=256, nq=1), dict(n_way=33, ns=1, nq=1), dict(D=256), dict(n_way=0), dict(ns=0), dict(nq=0), dict(E=0),
              dict(n_way=5, ns=50, nq=15)]:
        a = dict(good)
        a.update(b)
        assert call_all(a) == [-22] * 6, b
    for k in (0, 257):
        assert call_all(dict(good, k=k))[2] == -22
    for ld in (500, 514):
        rc = call_all(dict(good, ld=ld))
        assert rc[0] == rc[5] == -22
    torch.cuda.synchronize()
    z = lambda *s: torch.zeros(*s, device="cuda")  # noqa: E731
    head = (w3, b3, w4, b4)
    for args, kw in [((z(257, 512), 1, 1, 256, 1), {}), ((z(66, 512), 1, 33, 1, 1), {}), ((z(105, 512), 1, 5, 5, 16), dict(k=0)),
                     ((z(105, 256), 1, 5, 5, 16), {}), ((z(325, 512), 1, 5, 50, 15), {}), ((z(100, 512), 1, 5, 5, 16), {}),
                     ((z(105, 514)[:, :512], 1, 5, 5, 16), {})]:
        with pytest.raises(ValueError):
            ops.tpn_forward(args[0], head, *args[1:], **kw)
    tape = ops.tpn_forward(z(105, 512), head, 1, 5, 5, 16, save=True)[1]
    with pytest.raises(ValueError):
        ops.tpn_backward(tape, z(80, 4))
    torch.cuda.synchronize()


def test_identity_mask_gives_y_over_one_minus_alpha():
    r = _references()[0][((1, 5, 5, 16), K, "randn", 0)]
    eye = torch.eye(105, dtype=torch.uint8, device="cuda")[None].contiguous()
    scores, tape = ops.tpn_forward(r["f"].cuda(), _head(device="cuda"), 1, 5, 5, 16, save=True, mask=eye)
    assert torch.equal(tape["mask"], eye)
    Fm = tape["F"][0].cpu().double()
    Y = torch.zeros(105, 5, dtype=torch.float64)
    Y[torch.arange(25), torch.arange(25) // 5] = 1.0
    # alpha travels as a float: its rounding (2^-24 relative) moves 1 / (1 - alpha) by at most 1e4 * 2^-24; the stored diagonal,
    # its root and the two divisions round F = 100 a few more times
    assert float((Fm[:25] - Y[:25] / (1.0 - ALPHA)).abs().max()) <= 1e4 * 2.0 ** -24 + 100.0 * 2.0 ** -20
    assert float(Fm[25:].abs().max()) == 0.0 and float(scores.abs().max()) == 0.0


def test_argmax_equals_float64_on_class_structured_features():
    refs, _ = _references()
    head64 = _head(torch.float64)
    for draw in range(3):
        r = refs[((1, 5, 5, 15), K, "relu", draw)]
        scores = ops.tpn_forward(r["f"].cuda(), _head(device="cuda"), 1, 5, 5, 15)[0]
        with torch.no_grad():
            want = tpn_chain(r["f"].double(), head64, 5, 5, 15)[0]
        assert torch.equal(scores.argmax(1).cpu(), want.argmax(1))
        assert torch.equal(want.argmax(1), torch.arange(5).repeat_interleave(15))             # and every query is classified right


# ------------------------------------------------------------------------------------------------ meta-training step
def _oracle(sd32, xs, masks=None):
    """float64 loss (mean over the episodes of xs [k, n_way, S+Q, 3, H, W]) and gradients of every parameter, on ``masks`` (a list
    of [1, N, N], or the float64 selection) -> (loss, gradients, the float64 affinities, the masks used)."""
    sd = O.clone_state(sd32, torch.float64)
    pkeys = [k for k, v in sd.items() if v.is_floating_point() and "running" not in k]
    for k in pkeys:
        sd[k].requires_grad_(True)
    n_way, per = xs.shape[1], xs.shape[2]
    losses, Ws, used = [], [], []
    for i, x in enumerate(xs):
        feats = O.resnet10_forward(sd, x.double().reshape(-1, *x.shape[2:]), prefix="feature.")
        sc, W, m = tpn_chain(feats, [sd[k] for k in HEAD], n_way, 5, per - 5, mask=None if masks is None else masks[i])
        losses.append(F.cross_entropy(sc, torch.from_numpy(np.repeat(np.arange(n_way), per - 5))))
        Ws.append(W)
        used.append(m)
    loss = torch.stack(losses).mean()
    grads = torch.autograd.grad(loss, [sd[k] for k in pkeys])
    return float(loss.detach()), dict(zip(pkeys, grads)), Ws, used


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
    sd.update(synthetic.tpn_head_state(30))
    return sd


def _model(sd, n_way=5):
    m = TPN(model_dict['ResNet10'], n_way=n_way, n_support=5)
    m.load_state_dict(sd)
    m = m.cuda()
    m.train()
    m.n_query = 16
    return m


def test_set_forward_loss_backward_vs_oracle_and_g30(golden_dir):
    g = _g30(golden_dir)
    sd = _state(30)
    model = _model(sd)
    x = synthetic.train_episode(30, 5, 5, 16, 84)
    gmask = torch.from_numpy(g["mask"])[None].contiguous()
    with AG.tpn_forced_graph(gmask.cuda()):
        with torch.no_grad():
            sc = model.set_forward(x)
        np.testing.assert_allclose(sc.cpu().numpy(), g["scores"], rtol=1e-3, atol=1e-3)
        loss = model.set_forward_loss(x)
        loss.backward()
        assert torch.equal(AG.tpn_last_graph()[0].cpu(), gmask)
    assert abs(float(loss.detach()) - float(g["loss"])) < 2e-4
    ref_loss, ref, Ws, used = _oracle(sd, x[None], [gmask])
    assert abs(ref_loss - float(g["loss"])) < 1e-9 and torch.equal(used[0][0], gmask[0].double())
    named = dict(model.named_parameters())
    assert set(ref) == set(named)
    _check_grads(named, ref)
    # the four head gradients: within 4x the distance of the float32 CPU step to float64 (G30 (d))
    for k in HEAD:
        want = torch.from_numpy(g["headgrad:" + k])
        assert float((ref[k] - want).norm()) <= 1e-8 * float(want.norm())
        err = float((named[k].grad.cpu().double() - want).norm() / want.norm())
        yard = float(g["f32err:headgrad:" + k])
        print("tpn step: %s rel err %.3e, G30 float32 distance %.3e, ratio %.2f" % (k, err, yard, err / yard))
        assert err <= 4.0 * yard, (k, err, yard)
    # G30 (b): BatchNorm gradients and every gradient's norm
    for name in g["bnnames"]:
        name = str(name)
        want = g["bngrad:" + name]
        got = named[name].grad.cpu().numpy()
        assert np.linalg.norm(got - want) <= 3e-2 * np.linalg.norm(want) + 1e-9, name
    gn = {k: float(p.grad.norm()) for k, p in named.items()}
    for name, refn in zip(g["gradnames"], g["gradnorms"]):
        assert abs(gn[str(name)] - refn) <= 1e-2 * refn + 1e-9, name
    # unforced: the device's own selection differs from G30's only where the float64 affinities are ambiguous
    model.set_forward_loss(x)
    _assert_mask_rule(AG.tpn_last_graph()[0], Ws[0], gmask.double(), K, _references()[1], "G30 episode")


def test_lockstep_two_episodes_equal_float64_mean():
    sd = _state(23)
    xs = torch.stack([synthetic.train_episode(400 + i, 5, 5, 16, 84) for i in range(2)])
    model = _model(sd)
    scores = model.set_forward_lockstep(xs.cuda())
    assert scores.shape == (2 * 80, 5)
    loss = model.set_forward_loss_lockstep(xs.cuda())
    loss.backward()
    masks = AG.tpn_last_graph()[0].cpu()
    assert masks.shape == (2, 105, 105)
    ref_loss, ref, Ws, _ = _oracle(sd, xs, [masks[0:1], masks[1:2]])            # the mean on the device's own neighbours ...
    assert abs(float(loss.detach()) - ref_loss) < 2e-4
    _check_grads(dict(model.named_parameters()), ref)
    _, _, _, used = _oracle_masks_only(sd, xs)                                 # ... which are float64's up to ambiguous entries
    for e in range(2):
        _assert_mask_rule(masks[e:e + 1], Ws[e], used[e], K, _references()[1], "lockstep episode %d" % e)


def _oracle_masks_only(sd32, xs):
    sd = O.clone_state(sd32, torch.float64)
    used = []
    with torch.no_grad():
        for x in xs:
            feats = O.resnet10_forward(sd, x.double().reshape(-1, *x.shape[2:]), prefix="feature.")
            used.append(tpn_chain(feats, [sd[k] for k in HEAD], xs.shape[1], 5, xs.shape[2] - 5)[2])
    return None, None, None, used


def test_graphed_episode_loop_is_bit_identical(capsys, monkeypatch):
    from meta_fine_tuning_amd import graph_step, optim
    eps = [synthetic.train_episode(800 + i, 5, 5, 16, 84) for i in range(6)]          # three eager warm-up steps, three replays

    class Loader:
        def __len__(self):
            return len(eps)

        def __iter__(self):
            for x in eps:
                yield x, None

    def run(graphed):
        monkeypatch.setattr(graph_step, "ENABLED", graphed)
        model = _model(_state(30))
        opt = optim.Adam(model.parameters())
        capsys.readouterr()
        model.train_loop(0, Loader(), opt)
        out = capsys.readouterr().out
        st = model.__dict__.get("_mft_graph_steps", {}).get("set_forward_loss")
        return out, {n: p.detach().clone() for n, p in model.named_parameters()}, [b.detach().clone() for b in model.buffers()], st

    out_e, par_e, buf_e, st_e = run(False)
    out_g, par_g, buf_g, st_g = run(True)
    assert st_e is None and st_g is not None and st_g.graph is not None and not st_g.failed
    assert out_g == out_e and out_e.count("Loss") == 1
    assert list(par_e) == list(par_g) and all(torch.equal(par_e[n], par_g[n]) for n in par_e)
    assert all(torch.equal(a, b) for a, b in zip(buf_e, buf_g))
    fresh = _state(30)
    for k in HEAD:                                                             # the head was trained
        assert not torch.equal(par_g[k].cpu(), fresh[k]), k


def test_tpn_step_issues_no_aten_device_kernels():
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tpn_step_worker.py")
    r = subprocess.run([sys.executable, worker], capture_output=True, text=True, timeout=900)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert lines, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    res = json.loads(lines[-1][len("RESULT "):])
    assert res["n_dev"] > 0 and not res["aten"] and not res["head_aten"] and not res["head_step_aten"], res
    # three launches forward (embed, affinity, propagate), three backward, whatever the shape
    assert res["head_n_dev"] == res["fwd_n_dev"] == res["fwd_n_dev_50shot"] == 3, res
    assert res["bwd_n_dev"] == res["bwd_n_dev_50shot"] == 3, res


# ------------------------------------------------------------------------------------------------ evaluation and CLI
def test_evaluate_in_lockstep_equals_a_loop_over_set_forward():
    g = torch.Generator().manual_seed(77)
    mean = torch.randn(8, 1, 512, generator=g)
    rows = torch.relu(0.5 * torch.randn(8, 25, 512, generator=g) + 0.5 * mean + 0.3).numpy()
    table = feature_eval.FeatureTable({c: list(rows[c]) for c in range(8)})
    model = feature_eval.build_model("tpn", model_dict["ResNet10"], 5, 5)
    model.load_state_dict(_state(30))
    model = model.cuda().eval()

    def seed():
        random.seed(10)
        np.random.seed(10)
        torch.manual_seed(10)

    seed()
    acc, s_lock = feature_eval.evaluate(model, "tpn", table, 5, 5, 15, 6, 4, return_scores=True)
    assert acc.shape == (6,) and float(acc.mean()) > 80.0                      # class-structured features: nearly all right
    seed()
    _, idx, _ = feature_eval.episode_tables(table.rows, 5, 5, 15, 6)
    feats = table.device_feats()
    for e in range(6):
        z = feats[torch.from_numpy(idx[e].reshape(-1)).to(feats.device)].view(5, 20, 512)
        with torch.no_grad():
            one = model.set_forward(z, is_feature=True)
        assert np.array_equal(one.cpu().numpy(), s_lock[e]), e


@pytest.mark.parametrize("extra", [[], ["--episodes_per_rank", "2"]], ids=["plain", "lockstep2"])
def test_train_main_tpn_writes_a_loadable_checkpoint(golden_dir, tmp_path, monkeypatch, extra):
    from meta_fine_tuning_amd import configs, train
    g = _g30(golden_dir)
    monkeypatch.setattr(configs, "save_dir", str(tmp_path))
    train.main(["--dataset", "miniImageNet", "--method", "tpn", "--model", "ResNet10", "--stop_epoch", "1"] + extra,
               n_episode=2, size=84)
    f = tmp_path / "checkpoints" / "miniImageNet" / "ResNet10_tpn_5way_5shot" / "0.tar"
    assert f.is_file()
    state = torch.load(str(f), map_location="cpu")["state"]
    assert list(state.keys()) == [str(k) for k in g["state_keys"]]
    fresh = TPN(model_dict['ResNet10'], n_way=5, n_support=5)
    fresh.load_state_dict(state)
    assert list(fresh.state_dict().keys()) == [str(k) for k in g["state_keys"]]


@pytest.mark.parametrize("adaptation", [False, True], ids=["head", "adaptation"])
def test_save_features_and_test_drivers_take_tpn(tmp_path, monkeypatch, capsys, adaptation):
    from meta_fine_tuning_amd import configs, save_features
    from meta_fine_tuning_amd import test as test_driver
    monkeypatch.setattr(configs, "save_dir", str(tmp_path))
    for k, v in (("MFT_POOL_PER_CLASS", "24"), ("MFT_IMAGE_SIZE", "64"), ("MFT_EPISODES", "6"), ("MFT_EPISODES_PER_BATCH", "4")):
        monkeypatch.setenv(k, v)
    monkeypatch.delenv("MFT_STANDIN_WEIGHTS", raising=False)
    argv = ["--dataset", "miniImageNet", "--method", "tpn", "--test_dataset", "ISIC"]
    with pytest.raises(FileNotFoundError):
        save_features.main(argv)
    monkeypatch.setenv("MFT_STANDIN_WEIGHTS", "1")                               # the stand-in backbone with synthetic.tpn_head_state behind it
    from meta_fine_tuning_amd.io_utils import parse_args
    state, loaded = save_features.resolve_state(parse_args('save_features', argv), verbose=False)
    assert loaded is None and [k for k in state if not k.startswith("feature.")] == HEAD
    assert all(torch.equal(state[k], v) for k, v in synthetic.tpn_head_state().items())
    featfile = save_features.main(argv)
    assert featfile.endswith("features/miniImageNet/ResNet10_tpn_5way_5shot/novel.npz")
    acc = test_driver.main(argv + (["--adaptation"] if adaptation else []))
    out = capsys.readouterr().out
    assert len(acc) == 6 and np.all((acc >= 0) & (acc <= 100)) and "6 Test Acc" in out
    with pytest.raises(NotImplementedError):
        test_driver.main(argv + ["--unsup"])
