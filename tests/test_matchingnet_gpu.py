"""MatchingNet on a real MI355X: the four kernel pairs of csrc/matchingnet.hip (LSTM step, attention read, read-out, NLL) and the
whole head against the float64 restatement of tests/test_matchingnet_cpu.py, the meta-training step against the golden G26,
lockstep episodes, the graphed episode loop, the test-time engine (FinetuneEngine(mode="matching")) and the train.main driver.

The yardstick of every float comparison is the same arithmetic in torch float32 on the CPU: per tensor, the HIP result's relative
L2 distance to float64 must stay within 4 x the largest float32-vs-float64 distance over the test's own draws (both sides are
float32 evaluations of one chain with different summation orders).  A draw whose float32 distance exceeds 1e-3 is ill-conditioned
and must not be used.
"""
import argparse
import copy
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import meta_fine_tuning_amd  # noqa: F401
from meta_fine_tuning_amd import _lib, ops, synthetic
from meta_fine_tuning_amd import autograd_ops as AG
from meta_fine_tuning_amd import finetune as ft
from meta_fine_tuning_amd.io_utils import model_dict
from meta_fine_tuning_amd.methods.matchingnet import MatchingNet
from oracle import mft_oracle as O
from test_matchingnet_cpu import fce, head_ref, lstm_cell, nll, readout  # noqa: F401

pytestmark = pytest.mark.gpu
torch.set_num_threads(8)
D = 512
FACTOR = 4.0


def _g26(golden_dir):
    return np.load(os.path.join(golden_dir, "g26_matchingnet.npz"))


def rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).norm() / b.norm())


def features(seed, E, n_way, ns, nq):
    """relu(1 + 0.1 class + 0.5 noise) rows [E * n_way * (ns + nq), 512] in float64: overlapping classes, so that the x100 softmax of
    the read-out is not saturated."""
    g = torch.Generator().manual_seed(seed)
    cls = torch.arange(n_way).repeat_interleave(ns + nq).repeat(E).double()
    noise = torch.randn(E * n_way * (ns + nq), D, generator=g, dtype=torch.float64)
    return torch.relu(1 + 0.1 * cls[:, None] + 0.5 * noise)


def head_state(dtype=torch.float64):
    return {k: v.to(dtype) for k, v in synthetic.matchingnet_head_state(26).items()}


class Yardstick:
    """Collects, per tensor name, the float32-CPU distances of every draw and the HIP distances; ``check`` asserts the bound."""

    def __init__(self):
        self.f32, self.hip = {}, {}

    def add(self, name, ref64, cpu32, hip):
        self.f32.setdefault(name, []).append(rel(cpu32, ref64))
        self.hip.setdefault(name, []).append(rel(hip, ref64))

    def check(self, what):
        for name in self.f32:
            f32, hip = max(self.f32[name]), max(self.hip[name])
            print("%s %-34s hip %.3e   float32 yardstick %.3e   ratio %.2f" % (what, name, hip, f32, hip / f32))
        for name in self.f32:
            f32, hip = max(self.f32[name]), max(self.hip[name])
            assert f32 <= 1e-3, (what, name, f32)
            assert hip <= FACTOR * f32, (what, name, hip, f32)


# (episodes, n_way, n_support, n_query) -> three seeds whose float64 restatement meets the conditions asserted in _head_reference
SHAPES = [(1, 5, 5, 16), (1, 2, 1, 1), (3, 3, 2, 3), (2, 5, 1, 15), (1, 5, 20, 3), (1, 32, 1, 1)]
SEEDS = {(1, 5, 5, 16): (1, 2, 3), (1, 2, 1, 1): (1, 2, 3), (3, 3, 2, 3): (1, 2, 3), (2, 5, 1, 15): (1, 2, 3),
         (1, 5, 20, 3): (1, 2, 3), (1, 32, 1, 1): (1, 2, 3)}


def _head_reference(shape, seed, dtype):
    """The whole head in ``dtype`` on the CPU: logp, loss, and the gradients of sum(logp * up) for a random upstream ``up``."""
    E, n_way, ns, nq = shape
    feats64 = features(seed, E, n_way, ns, nq)
    up64 = torch.randn(E * n_way * nq, n_way, generator=torch.Generator().manual_seed(seed + 1000), dtype=torch.float64)
    f = feats64.to(dtype).clone().requires_grad_(True)
    W = {k: v.requires_grad_(True) for k, v in head_state(dtype).items()}
    logp, parts = head_ref(W, f, n_way, ns, nq, E, parts=True)
    (logp * up64.to(dtype)).sum().backward()
    out = {"logp": logp.detach(), "loss": nll(logp.detach(), n_way, nq, E), "dfeats": f.grad}
    out.update({"d:" + k: W[k].grad for k in W})
    if dtype == torch.float64:       # the conditions every draw must meet (float64 side)
        assert 0.3 < float(out["loss"]) < 6, (shape, seed, float(out["loss"]))
        for k in W:
            assert float(W[k].grad.norm()) >= 1e-2, (shape, seed, k, float(W[k].grad.norm()))
        for _, _, cos in parts:
            assert float(cos.detach().abs().min()) >= 1e-3, (shape, seed, float(cos.detach().abs().min()))
    return out, feats64, up64


_REF_CACHE = {}


def _refs(shape):
    if shape not in _REF_CACHE:
        _REF_CACHE[shape] = [(_head_reference(shape, s, torch.float64), _head_reference(shape, s, torch.float32)[0])
                             for s in SEEDS[shape]]
    return _REF_CACHE[shape]


def _cuda_params():
    return [v.float().cuda().requires_grad_(True) for v in head_state().values()]


# ------------------------------------------------------------------------------------------------ whole head
@pytest.mark.parametrize("shape", SHAPES)
def test_head_forward_backward_match_float64(shape):
    E, n_way, ns, nq = shape
    y = Yardstick()
    for (r64, feats64, up64), r32 in _refs(shape):
        f = feats64.float().cuda().requires_grad_(True)
        plist = _cuda_params()
        logp = AG._MatchingHeadFn.apply(f, n_way, ns, nq, E, *plist)
        assert logp.shape == (E * n_way * nq, n_way)
        with torch.no_grad():          # the path that saves nothing gives the same bits
            W = {k: p.detach() for k, p in zip(ops.MN_KEYS, plist)}
            assert torch.equal(ops.matching_forward(W, f.detach(), E, n_way, ns, nq)[0], logp)
        logp.backward(up64.float().cuda())
        y.add("logp", r64["logp"], r32["logp"], logp)
        y.add("dfeats", r64["dfeats"], r32["dfeats"], f.grad)
        for k, p in zip(ops.MN_KEYS, plist):
            y.add("d:" + k, r64["d:" + k], r32["d:" + k], p.grad)
        # a second run: bit-identical
        f2 = feats64.float().cuda().requires_grad_(True)
        p2 = _cuda_params()
        lp2 = AG._MatchingHeadFn.apply(f2, n_way, ns, nq, E, *p2)
        lp2.backward(up64.float().cuda())
        assert torch.equal(lp2, logp) and torch.equal(f2.grad, f.grad)
        assert all(torch.equal(a.grad, b.grad) for a, b in zip(plist, p2))
    y.check("head %s" % (shape,))


# ------------------------------------------------------------------------------------------------ kernel pairs
def _draws(shape, n=3):
    return [1000 * sum(shape) + 17 * i for i in range(n)]


@pytest.mark.parametrize("shape", SHAPES)
def test_lstm_step_matches_float64(shape):
    """pre-activations + h W_hh^T -> gates -> c', h' (+ f), and back: d(pre-activations), dc, dh = d(gates) W_hh."""
    E, n_way, ns, nq = shape
    M = E * n_way * nq
    w64 = head_state()["FCE.lstmcell.weight_hh"]
    y = Yardstick()
    for seed in _draws(shape):
        g = torch.Generator().manual_seed(seed)
        pre, h, c, fa, dh, dc = (torch.randn(M, n, generator=g, dtype=torch.float64) * s
                                 for n, s in ((4 * D, 1.0), (D, 0.5), (D, 0.5), (D, 1.0), (D, 1.0), (D, 1.0)))
        res = {}
        for dt in (torch.float64, torch.float32):
            p_, h_, c_ = (t.to(dt).clone().requires_grad_(True) for t in (pre, h, c))
            h1, c1 = lstm_cell(p_, h_, c_, w64.to(dt))
            h1 = h1 + fa.to(dt)
            ((h1 * dh.to(dt)).sum() + (c1 * dc.to(dt)).sum()).backward()
            res[dt] = dict(h=h1.detach(), c=c1.detach(), dpre=p_.grad, dh=h_.grad, dc=c_.grad)
        gates, hd, cd = pre.float().cuda(), h.float().cuda(), c.float().cuda()
        w = w64.float().cuda()
        c1, h1 = torch.empty_like(cd), torch.empty_like(hd)
        ops.mn_gemm(M, 4 * D, hd, D, w, D, D, gates, 4 * D, c_in=gates, ldci=4 * D)
        ops.lstm_step_forward(gates, 4 * D, cd, D, fa.float().cuda(), c1, h1, D, M)
        dcd = dc.float().cuda()
        ops.lstm_step_backward(gates, 4 * D, cd, D, c1, D, dh.float().cuda(), D, None, 0, dcd, dcd, D, M)
        dhp = ops.mn_gemm(M, D, gates, 4 * D, w, D, 4 * D, torch.empty_like(hd), D, tb=False)
        r64, r32 = res[torch.float64], res[torch.float32]
        for name, got in (("h", h1), ("c", c1), ("dpre", gates), ("dh", dhp), ("dc", dcd)):
            y.add(name, r64[name], r32[name], got)
    y.check("lstm %s" % (shape,))


@pytest.mark.parametrize("shape", SHAPES)
def test_attention_read_matches_float64(shape):
    """a = softmax(h G^T), r = a G per episode, and back into h and G (the G part through the batched transposed GEMM)."""
    E, n_way, ns, nq = shape
    S, Q = n_way * ns, n_way * nq
    y = Yardstick()
    for seed in _draws(shape):
        g = torch.Generator().manual_seed(seed)
        h, G, dr = (torch.randn(*s, generator=g, dtype=torch.float64) * k for s, k in (((E, Q, D), 0.2), ((E, S, D), 0.2), ((E, Q, D), 1.0)))
        res = {}
        for dt in (torch.float64, torch.float32):
            h_, G_ = h.to(dt).clone().requires_grad_(True), G.to(dt).clone().requires_grad_(True)
            a = torch.softmax(h_ @ G_.transpose(1, 2), dim=2)
            r = a @ G_
            (r * dr.to(dt)).sum().backward()
            res[dt] = dict(a=a.detach(), r=r.detach(), dh=h_.grad, dG=G_.grad)
        hd, Gd, drd = h.float().cuda().view(E * Q, D), G.float().cuda(), dr.float().cuda().view(E * Q, D)
        a, r = torch.empty(E * Q, S, device="cuda"), torch.empty(E * Q, D, device="cuda")
        ops.mn_attention_forward(hd, Gd, E, Q, S, a, r)
        dlogit, dh = torch.empty_like(a), torch.empty_like(hd)
        ops.mn_attention_backward(drd, a, Gd, None, E, Q, S, dlogit, dh)
        dG = torch.empty_like(Gd)
        ops.mn_gemm(S, D, a, S, drd, D, Q, dG, D, ta=True, tb=False, batch=E, a1_bs=Q * S, b1_bs=Q * D, a2=dlogit, lda2=S, a2_bs=Q * S,
                    b2=hd, ldb2=D, b2_bs=Q * D, K2=Q, c_bs=S * D)
        r64, r32 = res[torch.float64], res[torch.float32]
        for name, got in (("a", a.view(E, Q, S)), ("r", r.view(E, Q, D)), ("dh", dh.view(E, Q, D)), ("dG", dG)):
            y.add(name, r64[name], r32[name], got)
    y.check("attention %s" % (shape,))


def _readout_case(y, F, G, up, E, n_way, ns, nq):
    S, Q = n_way * ns, n_way * nq
    res = {}
    for dt in (torch.float64, torch.float32):
        F_, G_ = F.to(dt).clone().requires_grad_(True), G.to(dt).clone().requires_grad_(True)
        outs = [readout(F_[e], G_[e], n_way, ns) for e in range(E)]
        logp = torch.stack([o[0] for o in outs])
        (logp * up.to(dt)).sum().backward()
        res[dt] = dict(logp=logp.detach(), dF=F_.grad, dG=G_.grad)
        if dt == torch.float64:
            cos = torch.stack([o[1] for o in outs]).detach()
            assert float(cos.abs().min()) >= 1e-3, float(cos.abs().min())
    Fd, Gd = F.float().cuda().view(E * Q, D), G.float().cuda()
    gnorm = torch.empty(E, S, device="cuda")
    zero, Gout = torch.zeros_like(Gd), torch.empty_like(Gd)          # G = G + 0 + 0: the launch that also writes the row norms
    _lib.check(_lib.lib().mft_mn_encode_combine(ops._p(Gd), ops._p(zero), ops._p(zero), E, S, D, ops._p(Gout), ops._p(gnorm),
                                                ops._stream()), "mft_mn_encode_combine")
    assert torch.equal(Gout, Gd)
    ro = ops.mn_readout_forward(Fd, Gd, gnorm, E, n_way, ns, nq)
    dF, dG = ops.mn_readout_backward(up.float().cuda().view(E * Q, n_way), Fd, Gd, gnorm, ro, E, n_way, ns, nq)
    r64, r32 = res[torch.float64], res[torch.float32]
    for name, got in (("logp", ro["logp"].view(E, Q, n_way)), ("dF", dF.view(E, Q, D)), ("dG", dG)):
        y.add(name, r64[name], r32[name], got)
    return cos


@pytest.mark.parametrize("shape", SHAPES)
def test_readout_matches_float64(shape):
    E, n_way, ns, nq = shape
    y = Yardstick()
    for seed in _draws(shape):
        f = features(seed, E, n_way, ns, nq).view(E, n_way, ns + nq, D)
        G = f[:, :, :ns].reshape(E, n_way * ns, D)
        F = f[:, :, ns:].reshape(E, n_way * nq, D)
        up = torch.randn(E, n_way * nq, n_way, generator=torch.Generator().manual_seed(seed + 1), dtype=torch.float64)
        _readout_case(y, F, G, up, E, n_way, ns, nq)
    y.check("readout %s" % (shape,))


SIGNED_SEEDS = (3, 5, 9)          # chosen on the CPU: no |cos| < 1e-3 in the float64 restatement


def test_readout_with_signed_rows_clamps_half_the_scores():
    """F and G with both signs: relu clamps about half of the cosines; shape (1, 3, 2, 3)."""
    E, n_way, ns, nq = 1, 3, 2, 3
    y = Yardstick()
    clamped = []
    for seed in SIGNED_SEEDS:
        g = torch.Generator().manual_seed(seed)
        F = torch.randn(E, n_way * nq, D, generator=g, dtype=torch.float64)
        G = torch.randn(E, n_way * ns, D, generator=g, dtype=torch.float64)
        up = torch.randn(E, n_way * nq, n_way, generator=g, dtype=torch.float64)
        cos = _readout_case(y, F, G, up, E, n_way, ns, nq)
        clamped.append(float((cos < 0).double().mean()))
    assert 0.3 < float(np.mean(clamped)) < 0.7, clamped
    y.check("readout signed")


@pytest.mark.parametrize("shape", SHAPES)
def test_nll_mean_matches_float64(shape):
    E, n_way, ns, nq = shape
    rows = E * n_way * nq
    yl = torch.from_numpy(np.tile(np.repeat(np.arange(n_way), nq), E))
    y = Yardstick()
    loss_fn = AG.NLLLoss()
    total = 0.0
    for seed in _draws(shape):
        g = torch.Generator().manual_seed(seed)
        logp = torch.log_softmax(torch.randn(rows, n_way, generator=g, dtype=torch.float64), dim=1) - 0.5
        up = torch.rand((), generator=g, dtype=torch.float64) + 0.5
        res = {}
        for dt in (torch.float64, torch.float32):
            lp = logp.to(dt).clone().requires_grad_(True)
            loss = torch.nn.functional.nll_loss(lp, yl)
            (loss * up.to(dt)).backward()
            res[dt] = dict(loss=loss.detach(), dlogp=lp.grad)
        lp = logp.float().cuda().requires_grad_(True)
        loss = loss_fn(lp, yl.cuda())
        (loss * up.float().cuda()).backward()
        total += float(loss.detach())
        y.add("loss", res[torch.float64]["loss"], res[torch.float32]["loss"], loss)
        y.add("dlogp", res[torch.float64]["dlogp"], res[torch.float32]["dlogp"], lp.grad)
        loss32 = loss_fn(logp.float().cuda(), yl.int().cuda())          # int32 labels: the same bits
        assert torch.equal(loss32, loss.detach())
        total += float(loss32)
    assert abs(float(loss_fn.loss_sum(lp.device)) - total) < 1e-6 * max(1.0, abs(total))        # the float64 running sum on the device
    y.check("nll %s" % (shape,))


def test_out_of_range_launcher_arguments_return_einval():
    lib = _lib.lib()
    f = torch.zeros(33 * 2 * 2, D, device="cuda")
    big = torch.zeros(1 << 20, device="cuda")
    st = ops._stream(f)

    def gather(**kw):
        a = dict(ld=D, E=1, n_way=5, ns=5, nq=2, D=D)
        a.update(kw)
        return lib.mft_mn_gather(ops._p(f), a["ld"], a["E"], a["n_way"], a["ns"], a["nq"], a["D"], ops._p(big), ops._p(big), None, st)

    def readout_fwd(**kw):
        a = dict(E=1, n_way=5, ns=5, nq=2, D=D)
        a.update(kw)
        return lib.mft_mn_readout_forward(ops._p(f), ops._p(f), ops._p(big), a["E"], a["n_way"], a["ns"], a["nq"], a["D"], ops._p(big),
                                          ops._p(big), ops._p(big), ops._p(big), ops._p(big), st)
    assert gather() == 0 and readout_fwd() == 0
    for bad in (dict(n_way=33), dict(n_way=0), dict(n_way=5, ns=52), dict(ns=0), dict(nq=0), dict(E=0), dict(D=256), dict(D=516)):
        assert gather(**bad) == -22, bad
        assert readout_fwd(**bad) == -22, bad
        a = dict(E=1, n_way=5, ns=5, nq=2, D=D)
        a.update(bad)
        rc = lib.mft_mn_readout_backward(ops._p(big), a["n_way"], ops._p(f), ops._p(f), ops._p(big), ops._p(big), ops._p(big), ops._p(big),
                                         ops._p(big), a["E"], a["n_way"], a["ns"], a["nq"], a["D"], ops._p(big), ops._p(big), ops._p(big), st)
        assert rc == -22, bad
    assert gather(ld=500) == -22 and gather(ld=514) == -22
    for S, Dd, Q, E in ((257, D, 4, 1), (0, D, 4, 1), (8, 256, 4, 1), (8, D, 0, 1), (8, D, 4, 0)):
        assert lib.mft_mn_attention_forward(ops._p(f), ops._p(f), E, Q, S, Dd, ops._p(big), ops._p(big), st) == -22
        assert lib.mft_mn_attention_backward(ops._p(f), ops._p(big), ops._p(f), None, E, Q, S, Dd, ops._p(big), ops._p(big), st) == -22
    assert lib.mft_lstm_step_forward(ops._p(big), 4 * D, 0, None, D, 0, None, D, ops._p(big), ops._p(big), D, 0, 4, 256, 1, st) == -22
    assert lib.mft_lstm_step_forward(ops._p(big), 4 * D - 4, 0, None, D, 0, None, D, ops._p(big), ops._p(big), D, 0, 4, D, 1, st) == -22
    assert lib.mft_lstm_step_backward(ops._p(big), 4 * D, 0, None, D, 0, ops._p(big), D, 0, ops._p(big), D, 0, None, D, 0, None,
                                      ops._p(big), D, 0, None, None, 0, 0, D, 1, st) == -22
    assert lib.mft_mn_gemm(0, 1, 0, 8, 1, ops._p(f), D, 0, ops._p(f), None, D, 0, D, None, 0, 0, None, 0, 0, 0, None, 0, 0, None, None,
                           ops._p(big), 8, 0, st) == -22
    assert lib.mft_mn_gemm(0, 1, 8, 8, 1, ops._p(f), D - 1, 0, ops._p(f), None, D, 0, D, None, 0, 0, None, 0, 0, 0, None, 0, 0, None, None,
                           ops._p(big), 8, 0, st) == -22
    assert lib.mft_nll_mean(ops._p(big), 4, ops._p(big), 0, 5, 8, ops._p(big), None, st) == -22
    assert lib.mft_nll_mean_backward(ops._p(big), 0, 5, 0, None, ops._p(big), 5, st) == -22
    with pytest.raises(ValueError):
        ops.matching_forward({}, torch.zeros(33 * 2, D, device="cuda"), 1, 33, 1, 1)
    with pytest.raises(ValueError):
        ops.matching_forward({}, torch.zeros(100, D, device="cuda"), 1, 5, 5, 16)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ meta-training step
def _state(seed):
    sd = synthetic.resnet10_state_dict(seed=seed, prefix="feature.")
    sd.update(synthetic.matchingnet_head_state(26))
    return sd


def _model(sd, n_way=5):
    m = MatchingNet(model_dict['ResNet10'], n_way=n_way, n_support=5)
    m.load_state_dict(sd)
    m = m.cuda()
    m.train()
    m.n_query = 16
    return m


def test_set_forward_loss_backward_match_g26(golden_dir):
    """G26 (a), (b) with G26 (e) x 4 as the bound: the float32 CPU run of the same step is the yardstick.  Every stored array is
    one quantity with one relative L2 distance; the gradient norms are two of them (the vector of the twelve head norms, the
    vector of the feature norms).  Scalar by scalar the float32 run's norm of a single parameter can land within 2.5e-7 of
    float64 by chance (trunk.5.C2.weight; the HIP step: 4.9e-6), which is no yardstick for another float32 evaluation."""
    g = _g26(golden_dir)
    model = _model(_state(26))
    x = synthetic.train_episode(26, 5, 5, 16, 84)
    with torch.no_grad():
        logp = model.set_forward(x)
    loss = model.set_forward_loss(x)
    loss.backward()
    named = dict(model.named_parameters())
    assert list(model.state_dict().keys()) == [str(k) for k in g["state_keys"]]
    rows = []

    def cmp(name, got, want, bound):
        got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
        err = float(np.linalg.norm((got - want).ravel()) / np.linalg.norm(want.ravel()))
        rows.append((name, err, float(bound)))

    cmp("logprobs", logp.cpu().numpy(), g["logprobs"], g["f32err:logprobs"])
    cmp("loss", float(loss.detach()), g["loss"], g["f32err:loss"])
    names = [str(n) for n in g["gradnames"]]
    gn = np.array([float(named[n].grad.double().norm()) for n in names])
    head = np.array([not n.startswith("feature.") for n in names])
    for i, n in enumerate(names):          # (per parameter, for the record; the stored quantities are the two vectors below)
        print("g26 gradnorm %-46s hip %.3e" % (n, abs(gn[i] - g["gradnorms"][i]) / g["gradnorms"][i]))
    cmp("gradnorms_head", gn[head], g["gradnorms"][head], g["f32err:gradnorms_head"])
    cmp("gradnorms_feature", gn[~head], g["gradnorms"][~head], g["f32err:gradnorms_feature"])
    for key in g.files:
        if key.startswith(("biasgrad:", "bngrad:")):
            cmp(key, named[key.split(":", 1)[1]].grad.cpu().numpy(), g[key], g["f32err:" + key])
    for name, err, bound in rows:
        print("g26 %-52s hip %.3e   float32 yardstick %.3e   ratio %.2f" % (name, err, bound, err / max(bound, 1e-300)))
    bad = [(n, e, b) for n, e, b in rows if not e <= FACTOR * b]
    assert not bad, bad


def _oracle(sd32, xs):
    """float64 loss (mean over the episodes of xs [k, n_way, S+Q, 3, H, W]) and gradients of every parameter."""
    sd = O.clone_state(sd32, torch.float64)
    pkeys = [k for k, v in sd.items() if v.is_floating_point() and "running" not in k]
    for k in pkeys:
        sd[k].requires_grad_(True)
    n_way, per = xs.shape[1], xs.shape[2]
    losses = []
    for x in xs:
        feats = O.resnet10_forward(sd, x.double().reshape(-1, *x.shape[2:]), prefix="feature.")
        losses.append(nll(head_ref(sd, feats, n_way, 5, per - 5), n_way, per - 5))
    loss = torch.stack(losses).mean()
    grads = torch.autograd.grad(loss, [sd[k] for k in pkeys])
    return float(loss.detach()), dict(zip(pkeys, grads))


def test_lockstep_two_episodes_equal_float64_mean():
    sd = _state(23)
    xs = torch.stack([synthetic.train_episode(400 + i, 5, 5, 16, 84) for i in range(2)])
    model = _model(sd)
    logp = model.set_forward_lockstep(xs.cuda())
    assert logp.shape == (2 * 80, 5)
    loss = model.set_forward_loss_lockstep(xs.cuda())
    loss.backward()
    ref_loss, ref = _oracle(sd, xs)
    assert abs(float(loss.detach()) - ref_loss) < 2e-4 * max(1.0, abs(ref_loss))
    named = dict(model.named_parameters())
    assert set(ref) == set(named)
    # bounds of tests/test_protonet_gpu.py::_check_grads (a ReLU whose pre-activation is ~1e-6 may flip in fp32)
    for k, gr in ref.items():
        got = named[k].grad
        assert got is not None, k
        nrm = float(gr.norm())
        relerr = float((got.cpu().double() - gr).norm()) / nrm
        mx = float((got.cpu().double() - gr).abs().max()) / float(gr.abs().max())
        assert relerr < 3e-2 and mx < 0.15, (k, relerr, mx)


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


def test_matchingnet_step_issues_no_aten_device_kernels():
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "method_step_worker.py")
    r = subprocess.run([sys.executable, worker, "matchingnet"], capture_output=True, text=True, timeout=900)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert lines, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    res = json.loads(lines[-1][len("RESULT "):])
    assert res["n_dev"] > 0 and res["head_n_dev"] > 0, res
    assert not res["aten"] and not res["head_aten"], res


# ------------------------------------------------------------------------------------------------ evaluation
def _eval_model(sd):
    m = MatchingNet(model_dict['ResNet10'], n_way=5, n_support=5)
    m.load_state_dict(sd)
    m.train()
    return m


def _feature_state(seed):
    return synthetic.resnet10_state_dict(seed=seed, prefix="feature.")


@pytest.mark.parametrize("E", [0, 1])
def test_finetune_with_matchingnet_matches_g26(golden_dir, E):
    g = _g26(golden_dir)
    sd = _feature_state(13)
    ft.params = argparse.Namespace(model="ResNet10", fine_tune_epoch=E)
    model = _eval_model(_state(13))
    liz = synthetic.test_episode(41, 5, 5, 15, 84, gen_examples=0)
    np.random.seed(10)
    sc = ft.finetune(liz, None, model, copy.deepcopy(sd), None, n_query=15, n_way=5, n_support=5)
    assert sc.shape == (75, 5) and model.n_query == 15
    ref = g["finetune_scores_E%d" % E]
    err = np.abs(sc.cpu().numpy() - ref)
    print("finetune E=%d max |score - G26| = %.3e" % (E, err.max()))
    if E == 0:
        assert err.max() < 1e-4                                                # forward only: G22's bar
    else:
        # 15 Adam steps on the last block: G22's bar after adaptation (tests/test_protonet_gpu.py)
        assert err.max() < 3e-2 and (sc.argmax(1).cpu().numpy() == ref.argmax(1)).mean() >= 0.96, err.max()


def test_finetune_batched_equals_single_episode_calls():
    sd = _feature_state(13)
    model = _eval_model(_state(13))
    eps = [synthetic.test_episode(60 + i, 5, 5, 15, 84, gen_examples=1) for i in range(4)]
    ft.params = argparse.Namespace(model="ResNet10", fine_tune_epoch=1)
    np.random.seed(3)
    single = [ft.finetune(ep, None, model, sd, None, n_way=5, n_support=5) for ep in eps]
    np.random.seed(3)
    batched = ft.finetune_batched(eps, model, sd, 1, 5, 5, episodes_per_batch=4)
    assert batched.shape == (4, 75, 5)
    for a, b in zip(single, batched):          # G22's bar after adaptation (tests/test_protonet_gpu.py, same reasoning)
        err = float((a - b).abs().max())
        assert err < 3e-2 and float((a.argmax(1) == b.argmax(1)).float().mean()) >= 0.96, err
    assert any(ent["cfg"][0] == "matching" for ent in ft._ENGINES.entries)


def test_frozen_backbone_branch_runs():
    sd = _feature_state(13)
    model = _eval_model(_state(13))
    ft.params = argparse.Namespace(model="ResNet10", fine_tune_epoch=1)
    liz = synthetic.test_episode(41, 5, 5, 15, 84, gen_examples=0)
    sc = ft.finetune(liz, None, model, sd, None, freeze_backbone=True, n_way=5, n_support=5)
    assert sc.shape == (75, 5)
    torch.testing.assert_close(sc.sum(1).cpu(), torch.ones(75), atol=1e-5, rtol=0)
    feat = ft._eval_backbone(sd, "ResNet10")
    with torch.no_grad():
        f = feat(liz[0].cuda().reshape(-1, 3, 84, 84))
    want = torch.softmax(head_ref(head_state(), f.cpu().double(), 5, 5, 15), dim=1)
    assert float((sc.cpu().double() - want).abs().max()) < 1e-4


def test_test_loop_runs_the_benchmarks_protocol(capsys):
    model = _model(_state(13))
    eps = [synthetic.train_episode(900 + i, 5, 5, 15, 84) for i in range(2)]
    with torch.no_grad():
        acc = model.test_loop([(x, None) for x in eps])
    assert 0 <= acc <= 100 and "Test Acc" in capsys.readouterr().out and model.n_query == 15


def test_evaluate_matchingnet_with_device_sampler():
    from meta_fine_tuning_amd import augment
    sd = _feature_state(13)
    model = _eval_model(_state(13)).cuda()
    pool = synthetic.class_pool_u8("EuroSAT", "cuda:0", seed=1, n_per_class=40)
    sampler = augment.EpisodeSampler(pool, 5, 20, seed=10)
    np.random.seed(10)
    accs = ft.evaluate(model, sd, 2, 5, 5, 15, 84, 2, 1, episodes_per_batch=2, verbose=False, method="matchingnet", sampler=sampler)
    assert accs.shape == (2,) and np.all((accs >= 0) & (accs <= 100))


# ------------------------------------------------------------------------------------------------ CLI
def test_train_main_matchingnet_writes_a_loadable_checkpoint(golden_dir, tmp_path, monkeypatch):
    from meta_fine_tuning_amd import configs, train
    g = _g26(golden_dir)
    monkeypatch.setattr(configs, "save_dir", str(tmp_path))
    model = train.main(["--dataset", "miniImageNet", "--method", "matchingnet", "--model", "ResNet10", "--stop_epoch", "1"], n_episode=2,
                       size=84)
    f = tmp_path / "checkpoints" / "miniImageNet" / "ResNet10_matchingnet_5way_5shot" / "0.tar"
    assert f.is_file()
    state = torch.load(str(f), map_location="cpu")["state"]
    assert list(state.keys()) == [str(k) for k in g["state_keys"]]
    fresh = MatchingNet(model_dict['ResNet10'], n_way=5, n_support=5)
    fresh.load_state_dict(state)
    fresh = fresh.cuda().train()
    model.train()
    x = synthetic.train_episode(31, 5, 5, 16, 84)
    with torch.no_grad():
        fresh.n_query = model.n_query = 16
        assert torch.equal(fresh.set_forward(x), model.set_forward(x))


def test_train_main_lockstep_runs(tmp_path, monkeypatch):
    from meta_fine_tuning_amd import configs, train
    monkeypatch.setattr(configs, "save_dir", str(tmp_path))
    train.main(["--dataset", "miniImageNet", "--method", "matchingnet", "--model", "ResNet10", "--stop_epoch", "1", "--train_aug",
                "--episodes_per_rank", "2"], n_episode=4, size=84)
    assert (tmp_path / "checkpoints" / "miniImageNet" / "ResNet10_matchingnet_aug_5way_5shot" / "0.tar").is_file()


def test_train_main_refuses_matchingnet_fine_tune():
    from meta_fine_tuning_amd import train
    with pytest.raises(NotImplementedError, match="matchingnet"):
        train.main(["--method", "matchingnet", "--fine_tune", "--stop_epoch", "1"])
