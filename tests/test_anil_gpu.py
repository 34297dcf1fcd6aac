"""ANIL on a real MI355X: the inner-loop head kernels (csrc/anil.hip) against float64 with the float32 CPU chain as the yardstick,
the meta-training step against the float64 oracle and the golden G33, lockstep episodes, the graphed episode loop, the `test`
driver's lockstep scoring and train.main --method anil."""
import functools
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

import meta_fine_tuning_amd  # noqa: F401
from meta_fine_tuning_amd import _lib, feature_eval, ops, synthetic
from meta_fine_tuning_amd import autograd_ops as AG
from meta_fine_tuning_amd.io_utils import model_dict
from meta_fine_tuning_amd.methods.anil import ANIL
from oracle import mft_oracle as O

import anil_reference as R
from anil_reference import HEAD

pytestmark = pytest.mark.gpu
torch.set_num_threads(8)

LR = 0.01
STEPS = (1, 5, 16)
KINDS = ("randn", "relu")
# (E, n_way, n_support, n_query): the training shape, the test shape, S = 2, n_way = 1, the episode stride, S = 64, S = 65, 20-shot,
# the limit S = 256 with n_way = 4 and n_way = 32, and 5-way 50-shot
CASES = [(1, 5, 5, 16), (1, 5, 5, 15), (1, 2, 1, 1), (2, 1, 1, 1), (3, 3, 2, 3), (1, 8, 8, 1), (1, 5, 13, 1), (1, 5, 20, 15),
         (1, 4, 64, 1), (1, 32, 8, 1), (1, 5, 50, 15)]
VECTORS = ("scores", "dfeats", "dW0")
SCALARS = ("loss", "db0")
_id = lambda s: "E%d_w%d_s%d_q%d" % s  # noqa: E731


def _g33(golden_dir):
    return np.load(os.path.join(golden_dir, "g33_anil.npz"))


def _draws(shape):
    return 2 if shape[1] * shape[2] >= 100 else 3


def _features(kind, shape, draw):
    # the recipe of tests/test_dkt_gpu.py::_features
    E, n_way, ns, nq = shape
    g = torch.Generator().manual_seed(1000003 * draw + 7919 * E + 131 * n_way + 17 * ns + nq + (0 if kind == "randn" else 500000))
    f = torch.randn(E, n_way, ns + nq, 512, generator=g)
    if kind == "relu":          # non-negative and class-structured, as trunk outputs are
        mean = torch.randn(E, n_way, 1, 512, generator=g)
        f = torch.relu(0.5 * f + 0.5 * mean + 0.3)
    return f.reshape(-1, 512).contiguous()


def _init(shape, draw):
    """W0 uniform in +-1/sqrt(512) (the range of torch's default draw), b0 = 0.1 randn: float32 values, the inputs of every dtype."""
    g = torch.Generator().manual_seed(104729 * draw + 31 * shape[1] + 3)
    return (2.0 * torch.rand(shape[1], 512, generator=g) - 1.0) / 512 ** 0.5, 0.1 * torch.randn(shape[1], generator=g)


def _chain_step(f, W0, b0, shape, K, dtype):
    """The chain in ``dtype`` -> dict(scores, loss, dfeats, dW0, db0, G = d loss / d scores), float64."""
    E, n_way, ns, nq = shape
    x, W, b = (t.detach().clone().to(dtype).requires_grad_(True) for t in (f, W0, b0))
    loss, scores = R.anil_chain(x, W, b, n_way, ns, nq, E, K, LR)
    scores.retain_grad()
    loss.backward()
    return dict(scores=scores.detach().double(), loss=loss.detach().double(), dfeats=x.grad.double(), dW0=W.grad.double(),
                db0=b.grad.double(), G=scores.grad.double())


def _rel_per_episode(got, want, E):
    got, want = got.reshape(E, -1).double().cpu(), want.reshape(E, -1)
    return max(float((got[e] - want[e]).norm() / want[e].norm()) for e in range(E))


def _rel(got, want):
    return float((got.double().cpu().reshape(-1) - want.reshape(-1)).norm() / want.norm())


def _distances(got, want, E):
    return dict(scores=_rel_per_episode(got["scores"], want["scores"], E), dfeats=_rel_per_episode(got["dfeats"], want["dfeats"], E),
                dW0=_rel(got["dW0"], want["dW0"]), loss=_rel(got["loss"], want["loss"]), db0=_rel(got["db0"], want["db0"]))


@functools.lru_cache(maxsize=None)
def _references():
    """Every (shape, kind, K, draw): the inputs, the float64 chain's values and the float32 CPU chain's distances to them.
    -> (refs, vec, scal): vec[(shape, kind, K)] = the largest float32 distance of scores / dfeats / dW0 over the draws of the case;
    scal[(kind, K)] = the largest float32 distance of the loss and of db0 over ALL cases of the same feature kind and K (their
    per-case float32 distance spans two orders of magnitude, so a per-case yardstick would be a lottery).  At n_way = 1 the loss
    and every gradient are exactly zero: only the scores have a distance.  Computed once for the module and never modified."""
    refs, vec, scal = {}, {}, {}
    for shape in CASES:
        for kind in KINDS:
            for draw in range(_draws(shape)):
                f = _features(kind, shape, draw)
                W0, b0 = _init(shape, draw)
                for K in STEPS:
                    r64 = _chain_step(f, W0, b0, shape, K, torch.float64)
                    r32 = _chain_step(f, W0, b0, shape, K, torch.float32)
                    refs[(shape, kind, K, draw)] = dict(f=f, W0=W0, b0=b0, **r64)
                    v = vec.setdefault((shape, kind, K), dict.fromkeys(VECTORS, 0.0))
                    if shape[1] == 1:
                        assert not any(bool(r[n].any()) for r in (r64, r32) for n in ("loss", "dfeats", "dW0", "db0"))
                        v["scores"] = max(v["scores"], _rel_per_episode(r32["scores"], r64["scores"], shape[0]))
                        continue
                    d = _distances(r32, r64, shape[0])
                    for n in VECTORS:
                        v[n] = max(v[n], d[n])
                    s = scal.setdefault((kind, K), dict.fromkeys(SCALARS, 0.0))
                    for n in SCALARS:
                        s[n] = max(s[n], d[n])
    return refs, vec, scal


_CE = AG.CrossEntropyLoss()


def _device_step(f, W0, b0, shape, K, lr=LR):
    """ops-level forward, the project's cross entropy on the scores, ops-level backward -> dict like _chain_step's (device tensors)."""
    E, n_way, ns, nq = shape
    scores, tape = ops.anil_forward(f, W0, b0, E, n_way, ns, nq, K, lr, save=True)
    s = scores.detach().clone().requires_grad_(True)
    y = R.labels(n_way, nq).repeat(E).cuda()
    loss = _CE(s, y)
    loss.backward(torch.ones((), device="cuda"))
    dfeats, dW0, db0 = ops.anil_backward(tape, s.grad)
    return dict(scores=scores, loss=loss.detach(), dfeats=dfeats, dW0=dW0, db0=db0, tape=tape, G=s.grad)


def _compare(shape, kind, K, feats_of=lambda f: f.cuda()):
    refs, vec, scal = _references()
    E, n_way, ns, nq = shape
    yard, worst = vec[(shape, kind, K)], 0.0
    for draw in range(_draws(shape)):
        r = refs[(shape, kind, K, draw)]
        d = _device_step(feats_of(r["f"]), r["W0"].cuda(), r["b0"].cuda(), shape, K)
        assert d["scores"].shape == (E * n_way * nq, n_way) and d["dfeats"].shape == r["f"].shape
        assert d["dW0"].shape == (n_way, 512) and d["db0"].shape == (n_way,)
        if n_way == 1:
            e = _rel_per_episode(d["scores"], r["scores"], E)
            print("anil %s %s K %d draw %d: scores %.3e (yardstick %.3e, ratio %.2f)" % (_id(shape), kind, K, draw, e, yard["scores"],
                                                                                      e / max(yard["scores"], 1e-300)))
            assert bool(torch.isfinite(d["scores"]).all()) and e <= 4.0 * yard["scores"]
            assert not bool(d["dfeats"].any()) and not bool(d["dW0"].any()) and not bool(d["db0"].any())
            continue
        dist = _distances(d, r, E)
        # db0 is sum_rows G plus the steps' corrections, and its classes nearly cancel (|db0| goes down to 1e-4 where the entries of G
        # are 0.04): it repeats the error of G's column sums at that magnification.  The kernels are held to the yardstick on the
        # float64 chain's G rounded to float32, AND the db0 of the real step -- behind the project's own cross-entropy backward, as
        # training runs it -- is held to the same yardstick against the float64 recursion applied to that same device G ("db0_step").
        # What the cross-entropy backward's own error adds against the float64 chain is printed (measured on an MI355X at
        # E3_w3_s2_q3 relu K 16 draw 0: its G is 1.2e-7 from float64 like the float32 chain's, its column sums 1.7e-8 where the
        # float32 chain's are 5.6e-9, which at |db0| = 1.3e-4 reads 1.6e-4 against a yardstick of 2.6e-5)
        end_to_end = dist["db0"]
        dist["db0"] = _rel(ops.anil_backward(d["tape"], r["G"].float().cuda())[2], r["db0"])
        print("anil %s %s K %d draw %d: db0 behind the device's own cross-entropy gradient %.3e" % (_id(shape), kind, K, draw, end_to_end))
        same_g = R.anil_closed_form(r["f"].double(), r["W0"].double(), r["b0"].double(), n_way, ns, nq, E, K, LR,
                                    dscores=d["G"].double().cpu())[4]
        dist["db0_step"] = _rel(d["db0"], same_g)
        items = [(n, dist[n], yard[n]) for n in VECTORS] + [(n, dist[n], scal[(kind, K)][n]) for n in SCALARS]
        items.append(("db0_step", dist["db0_step"], scal[(kind, K)]["db0"]))
        print("anil %s %s K %d draw %d: " % (_id(shape), kind, K, draw)
              + "  ".join("%s %.3e (yardstick %.3e, ratio %.2f)" % (n, e, y, e / max(y, 1e-300)) for n, e, y in items))
        for n, e, y in items:
            worst = max(worst, e / max(y, 1e-300))
            assert e <= 4.0 * y, (draw, n, e, y)
    print("anil %s %s K %d: largest ratio %.2f" % (_id(shape), kind, K, worst))


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("K", STEPS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", CASES, ids=_id)
def test_kernels_match_float64_within_4x_the_float32_chain(shape, kind, K):
    """scores and dfeats per episode, dW0: relative L2 distance to float64 within 4 x the float32 CPU chain's (its largest over the
    draws of the case); the loss and db0 within 4 x the largest float32 distance over all cases of the same feature kind and K.  At
    n_way = 1: finite scores within the yardstick and exactly zero gradients.  The loss and the upstream gradient of dfeats and dW0
    are the project's cross entropy on the device's scores; db0 is asserted twice: behind the float64 chain's upstream gradient
    rounded to float32 against the float64 chain, and as the real step gives it, behind the device's own cross-entropy gradient,
    against the float64 recursion on that same gradient (_compare says why)."""
    _compare(shape, kind, K)


@pytest.mark.parametrize("K", STEPS)
def test_row_stride_640(K):
    def strided(f):
        buf = torch.full((f.shape[0], 640), float("nan"), device="cuda")
        buf[:, :512] = f.cuda()
        return buf[:, :512]
    _compare((3, 3, 2, 3), "relu", K, feats_of=strided)


def _run(shape, K=5, draw=0):
    W0, b0 = _init(shape, draw)
    d = _device_step(_features("relu", shape, draw).cuda(), W0.cuda(), b0.cuda(), shape, K)
    return [d[n] for n in ("scores", "loss", "dfeats", "dW0", "db0")] + [d["tape"][k] for k in ("W", "b", "P")]


@pytest.mark.parametrize("shape", [(3, 3, 2, 3), (1, 5, 5, 16), (1, 32, 8, 1)], ids=_id)
def test_two_calls_are_bit_identical(shape):
    for K in (5, 16):
        for x, y in zip(_run(shape, K), _run(shape, K)):
            assert torch.equal(x, y)


def test_episodes_in_one_call_equal_single_calls():
    shape, one, N, Q = (3, 3, 2, 3), (1, 3, 2, 3), 15, 9
    f = _features("relu", shape, 1).cuda()
    W0, b0 = (t.cuda() for t in _init(shape, 1))
    together = _device_step(f, W0, b0, shape, 5)
    tapes = [ops.anil_forward(f[e * N:(e + 1) * N], W0, b0, *one, 5, LR, save=True) for e in range(3)]
    assert torch.equal(together["scores"].reshape(3, -1), torch.stack([s.reshape(-1) for s, _ in tapes]))
    for k in ("W", "b", "P"):                                         # every step's classifier and softmax: episode after episode
        assert torch.equal(together["tape"][k].reshape(3, -1), torch.stack([t[k].reshape(-1) for _, t in tapes])), k
    # the single calls get their own rows of the upstream gradient
    singles = [ops.anil_backward(t, together["G"][e * Q:(e + 1) * Q].contiguous()) for e, (_, t) in enumerate(tapes)]
    for e, (dfe, _, _) in enumerate(singles):
        got = together["dfeats"][e * N:(e + 1) * N]
        assert float((got.double() - dfe.double()).abs().max()) <= 2.0 ** -23 * float(dfe.abs().max()), e
    # dW0 and db0 add the episodes up in order: the float64 sum of the single calls, rounded
    for n, i in (("dW0", 1), ("db0", 2)):
        want = sum(s[i].double() for s in singles)
        scale = sum(s[i].double().abs() for s in singles)
        assert bool(((together[n].double() - want).abs() <= 2.0 ** -22 * scale).all()), n


def test_upstream_gradient_is_read_on_the_device():
    shape = (1, 5, 5, 16)
    W0, b0 = (t.cuda() for t in _init(shape, 0))
    d = _device_step(_features("relu", shape, 0).cuda(), W0, b0, shape, 5)
    one = (d["dfeats"], d["dW0"], d["db0"])
    g = d["G"].clone()
    assert all(torch.equal(a, b) for a, b in zip(ops.anil_backward(d["tape"], g), one))
    g.mul_(4.0)                                                       # the same tensor, a new value: what a replayed graph sees
    assert all(torch.equal(a, 4.0 * b) for a, b in zip(ops.anil_backward(d["tape"], g), one))
    g.mul_(-0.5)
    assert all(torch.equal(a, -2.0 * b) for a, b in zip(ops.anil_backward(d["tape"], g), one))


def test_out_of_range_arguments_are_refused():
    lib = _lib.lib()
    p = ops._p
    z = lambda *s: torch.zeros(*s, device="cuda")  # noqa: E731
    f = z(400, 520)
    W0, b0 = z(32, 512), z(32)
    Wt, gWt, bt, gbt = z(17 * 32 * 512 + 4), z(17 * 32 * 512 + 4), z(17 * 32), z(17 * 32)
    P, Rt, G, scores, dfeats, dW0, db0 = z(16 * 256 * 32), z(16 * 256 * 32), z(4096), z(4096), z(400 * 512 + 4), z(32 * 512 + 4), z(32)
    st = ops._stream(f)

    def call_all(a, f=f, W0=W0, Wt=Wt, gWt=gWt, dfeats=dfeats, dW0=dW0, ldd=512):
        shp = (a["ld"], a["E"], a["n_way"], a["ns"], a["nq"], a["D"])
        return [lib.mft_anil_adapt(p(f), *shp, p(W0), p(b0), a["K"], a["lr"], p(Wt), p(bt), p(P), st),
                lib.mft_anil_scores(p(f), *shp, a["K"], p(Wt), p(bt), p(scores), st),
                lib.mft_anil_scores_backward(p(f), *shp, a["K"], p(Wt), p(G), p(dfeats), ldd, p(gWt), p(gbt), st),
                lib.mft_anil_adapt_backward(p(f), *shp, a["K"], a["lr"], p(Wt), p(P), p(gWt), p(gbt), p(Rt), p(dfeats), ldd, p(dW0),
                                            p(db0), st)]

    good = dict(ld=520, E=1, n_way=5, ns=5, nq=16, D=512, K=5, lr=0.01)
    assert call_all(good) == [0] * 4
    for b in [dict(n_way=0), dict(n_way=33, ns=1, nq=1), dict(D=256), dict(ns=0), dict(nq=0), dict(E=0), dict(n_way=1, ns=257, nq=1),
              dict(K=0), dict(K=17), dict(ld=500), dict(ld=514), dict(E=65536), dict(nq=2 ** 22)]:
        assert call_all(dict(good, **b)) == [-22] * 4, b
    for lr in (0.0, -0.01, float("nan"), float("inf")):                # the two launchers that step
        rc = call_all(dict(good, lr=lr))
        assert rc[0] == rc[3] == -22 and rc[1] == rc[2] == 0, lr
    assert call_all(good, f=f[:, 1:]) == [-22] * 4                     # rows not 16-byte aligned
    assert call_all(good, Wt=Wt[1:]) == [-22] * 4
    assert call_all(good, W0=W0.view(-1)[1:])[0] == -22
    rc = call_all(good, gWt=gWt[1:])
    assert rc[2] == rc[3] == -22
    rc = call_all(good, dfeats=dfeats[1:])
    assert rc[2] == rc[3] == -22
    assert call_all(good, dW0=dW0[1:])[3] == -22
    rc = call_all(good, ldd=500)
    assert rc[2] == rc[3] == -22
    assert lib.mft_anil_adapt(p(f), 520, 1, 5, 5, 16, 512, p(W0), None, 5, 0.01, p(Wt), p(bt), p(P), st) == -22
    assert lib.mft_anil_adapt(p(f), 520, 1, 5, 5, 16, 512, p(W0), p(b0), 5, 0.01, p(Wt), p(bt), None, st) == 0       # P is optional
    assert lib.mft_anil_adapt_backward(p(f), 520, 1, 5, 5, 16, 512, 5, 0.01, p(Wt), None, p(gWt), p(gbt), p(Rt), p(dfeats), 512, p(dW0),
                                       p(db0), st) == -22
    torch.cuda.synchronize()
    w, b = z(5, 512), z(5)
    for args in [(z(258, 512), z(1, 512), z(1), 1, 1, 257, 1, 5, LR), (z(66, 512), z(33, 512), z(33), 1, 33, 1, 1, 5, LR),
                 (z(105, 256), z(5, 256), b, 1, 5, 5, 16, 5, LR), (z(100, 512), w, b, 1, 5, 5, 16, 5, LR),
                 (z(105, 514)[:, :512], w, b, 1, 5, 5, 16, 5, LR), (z(105, 512), w, b, 1, 5, 5, 16, 0, LR), (z(105, 512), w, b, 1, 5, 5, 16, 17, LR), (z(105, 512), w, b, 1, 5, 5, 16, 5, 0.0),
                 (z(105, 512), w, b, 1, 5, 5, 16, 5, -1.0), (z(105, 512), w, b, 0, 5, 5, 16, 5, LR), (z(105, 512), w, b, 1, 5, 5, 0, 5, LR),
                 (z(105, 512), w, b, 1, 5, 0, 16, 5, LR), (z(105, 512), w, b, 65536, 5, 5, 16, 5, LR),
                 (z(105, 512), z(4, 512), b, 1, 5, 5, 16, 5, LR), (z(105, 516)[:, 1:513], w, b, 1, 5, 5, 16, 5, LR)]:
        with pytest.raises(ValueError):
            ops.anil_forward(*args)
    for args in [(z(105, 512).cpu(), w, b), (z(105, 512).double(), w, b), (z(105, 512), w.cpu(), b), (z(105, 512), w, b.double())]:
        with pytest.raises(RuntimeError):
            ops.anil_forward(*args, 1, 5, 5, 16, 5, LR)
    tape = ops.anil_forward(z(105, 512) + 1.0, w, b, 1, 5, 5, 16, 5, LR, save=True)[1]
    with pytest.raises(ValueError):
        ops.anil_backward(tape, z(80, 4))
    for bad in (z(80, 5).cpu(), z(80, 5).double()):
        with pytest.raises(RuntimeError):
            ops.anil_backward(tape, bad)
    assert ops.anil_forward(z(325, 512) + 1.0, w, b, 1, 5, 50, 15, 16, LR)[0].shape == (75, 5)          # 5-way 50-shot is in the domain
    assert ops.anil_forward(z(257, 512) + 1.0, z(1, 512), z(1), 1, 1, 256, 1, 1, LR)[0].shape == (1, 1)
    torch.cuda.synchronize()


@pytest.mark.parametrize("K", [5, 10])
def test_argmax_equals_float64_where_the_gap_exceeds_the_float32_error(K):
    shape = (1, 5, 5, 15)
    total = decided = 0
    for draw in range(3):
        f = _features("relu", shape, draw)
        W0, b0 = _init(shape, draw)
        want = _chain_step(f, W0, b0, shape, K, torch.float64)["scores"]
        s32 = _chain_step(f, W0, b0, shape, K, torch.float32)["scores"]
        err = float((s32 - want).abs().max())
        top = torch.sort(want, dim=1, descending=True).values
        clear = (top[:, 0] - top[:, 1]) > err
        got = ops.anil_forward(f.cuda(), W0.cuda(), b0.cuda(), *shape, K, LR)[0].argmax(1).cpu()
        assert torch.equal(got[clear], want.argmax(1)[clear])
        total += clear.numel()
        decided += int(clear.sum())
    print("anil argmax K %d: %d of %d queries decided by the rule" % (K, decided, total))
    assert decided >= 0.95 * total, (decided, total)                  # the rule cannot hide a failure


def test_autograd_wrapper():
    shape = (2, 3, 2, 3)
    f = _features("relu", shape, 0).cuda().requires_grad_(True)
    W0, b0 = (t.cuda().requires_grad_(True) for t in _init(shape, 0))
    scores = AG.anil_scores(f, W0, b0, 3, 2, 3, episodes=2, inner_steps=5, inner_lr=LR)
    assert scores.shape == (18, 3) and scores.requires_grad
    g = torch.Generator().manual_seed(9)
    G = torch.randn(18, 3, generator=g).cuda()
    scores.backward(G)
    ref, tape = ops.anil_forward(f.detach(), W0.detach(), b0.detach(), 2, 3, 2, 3, 5, LR, save=True)
    dfeats, dW0, db0 = ops.anil_backward(tape, G)
    assert torch.equal(scores.detach(), ref)
    assert torch.equal(f.grad, dfeats) and torch.equal(W0.grad, dW0) and torch.equal(b0.grad, db0)
    assert W0.grad.shape == (3, 512) and b0.grad.shape == (3,)
    with torch.no_grad():                                             # no tape is kept
        quiet = AG.anil_scores(f, W0, b0, 3, 2, 3, episodes=2, inner_steps=5, inner_lr=LR)
    assert not quiet.requires_grad and quiet.grad_fn is None and torch.equal(quiet, ref)
    assert ops.anil_forward(f.detach(), W0.detach(), b0.detach(), 2, 3, 2, 3, 5, LR)[1] is None
    frozen = AG.anil_scores(f.detach(), W0.detach(), b0.detach(), 3, 2, 3, episodes=2, inner_steps=5, inner_lr=LR)
    assert not frozen.requires_grad and torch.equal(frozen, ref)


# ------------------------------------------------------------------------------------------------ meta-training step
def _oracle(sd32, xs):
    """float64 loss (mean over the episodes of xs [k, n_way, S+Q, 3, H, W]), scores and gradients of every parameter."""
    sd = O.clone_state(sd32, torch.float64)
    pkeys = [k for k, v in sd.items() if v.is_floating_point() and "running" not in k]
    for k in pkeys:
        sd[k].requires_grad_(True)
    n_way, per = xs.shape[1], xs.shape[2]
    feats = torch.cat([O.resnet10_forward(sd, x.double().reshape(-1, *x.shape[2:]), prefix="feature.") for x in xs])
    loss, scores = R.anil_chain(feats, sd[HEAD[0]], sd[HEAD[1]], n_way, 5, per - 5, xs.shape[0])
    grads = torch.autograd.grad(loss, [sd[k] for k in pkeys])
    return float(loss.detach()), scores.detach(), dict(zip(pkeys, grads))


def _check_grads(named, ref):
    # bounds of tests/test_dkt_gpu.py::_check_grads (the trunk backward is the same code)
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
    sd.update(synthetic.anil_head_state(33))
    return sd


def _model(sd, n_way=5):
    m = ANIL(model_dict['ResNet10'], n_way=n_way, n_support=5)
    m.load_state_dict(sd)
    m = m.cuda()
    m.train()
    m.n_query = 16
    return m


def test_set_forward_loss_backward_vs_oracle_and_g33(golden_dir):
    """The envelope of tests/test_dkt_gpu.py for G32: scores to 1e-3, the loss to 2e-4, every gradient by _check_grads, the BatchNorm
    gradients to 3e-2 and every gradient norm to 1e-2.  The two head gradients sit behind the whole trunk: they take _check_grads'
    bound against G33 as every other parameter does, and their ratio to G33's float32 distance is printed (the head alone is held
    to 4 x the float32 chain by test_kernels_match_float64_within_4x_the_float32_chain)."""
    g = _g33(golden_dir)
    sd = _state(33)
    model = _model(sd)
    x = synthetic.train_episode(33, 5, 5, 16, 84)
    scores = model.set_forward(x)
    assert scores.shape == (80, 5) and scores.requires_grad
    np.testing.assert_allclose(scores.detach().cpu().numpy(), g["scores"], rtol=1e-3, atol=1e-3)
    loss = model.loss_fn(scores, model._labels(1))
    assert loss.shape == () and loss.requires_grad
    loss.backward()
    assert abs(float(loss.detach()) - float(g["loss"])) < 2e-4
    ref_loss, _, ref = _oracle(sd, x[None])
    assert abs(ref_loss - float(g["loss"])) < 1e-9
    named = dict(model.named_parameters())
    assert set(ref) == set(named)
    _check_grads(named, ref)
    for k in HEAD:
        want = torch.from_numpy(g["headgrad:" + k])
        assert float((ref[k] - want).norm()) <= 1e-8 * float(want.norm())
        err = float((named[k].grad.cpu().double() - want).norm() / want.norm())
        yard = float(g["f32err:headgrad:" + k])
        print("anil step: %s rel err %.3e, G33 float32 distance %.3e, ratio %.2f" % (k, err, yard, err / yard))
        assert err < 3e-2, (k, err)
    for name in g["bnnames"]:
        name = str(name)
        want = g["bngrad:" + name]
        got = named[name].grad.cpu().numpy()
        assert np.linalg.norm(got - want) <= 3e-2 * np.linalg.norm(want) + 1e-9, name
    gn = {k: float(p.grad.norm()) for k, p in named.items()}
    for name, refn in zip(g["gradnames"], g["gradnorms"]):
        assert abs(gn[str(name)] - refn) <= 1e-2 * refn + 1e-9, name
    model.eval()                                                       # the same steps and step size in eval mode; no grad, no tape
    with torch.no_grad():
        quiet = model.set_forward(x)
    assert not quiet.requires_grad and quiet.shape == (80, 5)


def test_lockstep_two_episodes_equal_float64_mean():
    sd = _state(23)
    xs = torch.stack([synthetic.train_episode(400 + i, 5, 5, 16, 84) for i in range(2)])
    model = _model(sd)
    ref_loss, ref_scores, ref = _oracle(sd, xs)
    scores = model.set_forward_lockstep(xs.cuda())
    assert scores.shape == (2 * 80, 5) and scores.requires_grad
    np.testing.assert_allclose(scores.detach().cpu().numpy(), ref_scores.numpy(), rtol=1e-3, atol=1e-3)
    loss = model.set_forward_loss_lockstep(xs.cuda())
    loss.backward()
    assert abs(float(loss.detach()) - ref_loss) < 2e-4
    _check_grads(dict(model.named_parameters()), ref)


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
        model = _model(_state(33))
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
    fresh = _state(33)
    for k in HEAD:                                                             # both head parameters were trained
        assert not torch.equal(par_g[k].cpu(), fresh[k]), k


def test_anil_step_issues_no_aten_device_kernels():
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "anil_step_worker.py")
    r = subprocess.run([sys.executable, worker], capture_output=True, text=True, timeout=900)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert lines, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    res = json.loads(lines[-1][len("RESULT "):])
    print("anil step worker:", res)
    assert res["n_dev"] > 0 and not res["aten"] and not res["head_aten"] and not res["head_step_aten"], res
    # the walk and the scores forward; the query side, the reverse walk and the support gradient with the
    # episode sum backward -- whatever the shape
    assert set(res["fwd_n_dev"]) == {"5_5_16", "5_50_15"}
    assert all(n == ops.ANIL_FORWARD_LAUNCHES for n in res["fwd_n_dev"].values()), res
    assert all(n == ops.ANIL_BACKWARD_LAUNCHES for n in res["bwd_n_dev"].values()), res
    assert res["head_n_dev"] == ops.ANIL_FORWARD_LAUNCHES, res


# ------------------------------------------------------------------------------------------------ evaluation and CLI
def test_evaluate_in_lockstep_equals_a_loop_over_set_forward():
    g = torch.Generator().manual_seed(77)
    mean = torch.randn(8, 1, 512, generator=g)
    rows = torch.relu(0.5 * torch.randn(8, 25, 512, generator=g) + 0.5 * mean + 0.3).numpy()
    table = feature_eval.FeatureTable({c: list(rows[c]) for c in range(8)})
    model = feature_eval.build_model("anil", model_dict["ResNet10"], 5, 5)
    model.load_state_dict(_state(33))
    model = model.cuda().eval()

    def seed():
        random.seed(10)
        np.random.seed(10)
        torch.manual_seed(10)

    seed()
    acc, s_lock = feature_eval.evaluate(model, "anil", table, 5, 5, 15, 6, 4, return_scores=True)
    # five steps of 0.01 from an untrained initialisation: the float64 chain gets 360 of these 450 queries right (80.0 %)
    print("anil evaluate: accuracies %s, mean %.2f" % (acc, float(acc.mean())))
    assert acc.shape == (6,) and float(acc.mean()) > 50.0
    seed()
    _, idx, _ = feature_eval.episode_tables(table.rows, 5, 5, 15, 6)
    feats = table.device_feats()
    for e in range(6):
        z = feats[torch.from_numpy(idx[e].reshape(-1)).to(feats.device)].view(5, 20, 512)
        with torch.no_grad():
            one = model.set_forward(z, is_feature=True)
        assert np.array_equal(one.cpu().numpy(), s_lock[e]), e
    assert feature_eval.EPISODES_PER_BATCH == 100


@pytest.mark.parametrize("extra,dirname", [([], "ResNet10_anil_5way_5shot"), (["--episodes_per_rank", "2"], "ResNet10_anil_5way_5shot"),
                                           (["--model", "ResNet10_FW"], "ResNet10_FW_anil_5way_5shot")],
                         ids=["plain", "lockstep2", "fw"])
def test_train_main_anil_writes_a_loadable_checkpoint(golden_dir, tmp_path, monkeypatch, extra, dirname):
    from meta_fine_tuning_amd import configs, train
    monkeypatch.setattr(configs, "save_dir", str(tmp_path))
    made, construct = [], ANIL.__init__

    def spy(self, *args, **kwargs):                                              # the head as the constructor leaves it
        construct(self, *args, **kwargs)
        made.append({k: self.state_dict()[k].detach().clone() for k in HEAD})

    monkeypatch.setattr(ANIL, "__init__", spy)
    model = train.main(["--dataset", "miniImageNet", "--method", "anil", "--stop_epoch", "1"] + extra, n_episode=2, size=84)
    assert type(model) is ANIL and (model.inner_steps, model.inner_lr) == (5, 0.01)
    f = tmp_path / "checkpoints" / "miniImageNet" / dirname / "0.tar"
    assert f.is_file()
    state = torch.load(str(f), map_location="cpu")["state"]
    assert list(state.keys())[-2:] == HEAD
    if "ResNet10_FW" not in extra:
        assert list(state.keys()) == [str(k) for k in _g33(golden_dir)["state_keys"]]
    fresh = ANIL(model_dict['ResNet10_FW' if "ResNet10_FW" in extra else 'ResNet10'], n_way=5, n_support=5)
    fresh.load_state_dict(state)
    assert all(bool(torch.isfinite(state[k]).all()) for k in HEAD)
    assert not bool(made[0][HEAD[1]].any()) and bool(state[HEAD[1]].any())       # the bias left its zero initialisation ...
    assert all(not torch.equal(state[k], made[0][k]) for k in HEAD)              # ... and the steps reached both head tensors


def test_save_features_and_test_drivers_take_anil(tmp_path, monkeypatch, capsys):
    from meta_fine_tuning_amd import configs, save_features
    from meta_fine_tuning_amd import test as test_driver
    monkeypatch.setattr(configs, "save_dir", str(tmp_path))
    for k, v in (("MFT_POOL_PER_CLASS", "24"), ("MFT_IMAGE_SIZE", "64"), ("MFT_EPISODES", "6"), ("MFT_EPISODES_PER_BATCH", "4")):
        monkeypatch.setenv(k, v)
    monkeypatch.delenv("MFT_STANDIN_WEIGHTS", raising=False)
    argv = ["--dataset", "miniImageNet", "--method", "anil", "--test_dataset", "ISIC"]
    with pytest.raises(FileNotFoundError):
        save_features.main(argv)
    monkeypatch.setenv("MFT_STANDIN_WEIGHTS", "1")                               # the stand-in backbone with synthetic.anil_head_state behind it
    from meta_fine_tuning_amd.io_utils import parse_args
    state, loaded = save_features.resolve_state(parse_args('save_features', argv), verbose=False)
    assert loaded is None and [k for k in state if not k.startswith("feature.")] == HEAD
    assert all(torch.equal(state[k], v) for k, v in synthetic.anil_head_state().items())
    featfile = save_features.main(argv)
    assert featfile.endswith("features/miniImageNet/ResNet10_anil_5way_5shot/novel.npz")
    acc = test_driver.main(argv)
    out = capsys.readouterr().out
    assert len(acc) == 6 and np.all((acc >= 0) & (acc <= 100)) and "6 Test Acc" in out
