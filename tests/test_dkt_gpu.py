"""DKT on a real MI355X: the Gaussian-process head kernels (csrc/dkt.hip) against float64 with the float32 CPU chain as the
yardstick, the closed-form case, the meta-training step against the float64 oracle and the golden G32, lockstep episodes, the
graphed episode loop, the `test` driver's lockstep scoring and train.main --method dkt."""
import functools
import json
import math
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
from meta_fine_tuning_amd.methods.dkt import DKT
from oracle import mft_oracle as O

import dkt_reference as R
from dkt_reference import HEAD

pytestmark = pytest.mark.gpu
torch.set_num_threads(8)

MEAN, RAW_OS = 0.05, 0.2                    # a non-zero mean and an outputscale off its initial value
NOISES = (0.1, 0.01)                        # the initial noise and a tenth of it
KERNELS = ("cossim", "linear")
KINDS = ("randn", "relu")
# (E, n_way, n_support, n_query): the training shape, the test shape, N = 4, n_way = 1, the episode stride, N = 64, N = 65, 20-shot,
# and the limits N = 256 (four threads per factor row) with n_way = 4 and n_way = 32
CASES = [(1, 5, 5, 16), (1, 5, 5, 15), (1, 2, 1, 1), (2, 1, 1, 1), (3, 3, 2, 3), (1, 8, 7, 1), (1, 5, 12, 1), (1, 5, 20, 15),
         (1, 4, 49, 15), (1, 32, 7, 1)]
SCORE_CASES = [(1, 5, 50, 15), (1, 32, 8, 1)]           # S = 250 with N = 325, and S = 256: scored, not trained
SCALARS = ("loss", "dmean", "draw_outputscale", "draw_noise")
_id = lambda s: "E%d_w%d_s%d_q%d" % s  # noqa: E731


def _g32(golden_dir):
    return np.load(os.path.join(golden_dir, "g32_dkt.npz"))


def _draws(shape):
    return 2 if shape[1] * (shape[2] + shape[3]) >= 175 else 3


def _features(kind, shape, draw):
    # the recipe of tests/test_tpn_gpu.py::_features
    E, n_way, ns, nq = shape
    g = torch.Generator().manual_seed(1000003 * draw + 7919 * E + 131 * n_way + 17 * ns + nq + (0 if kind == "randn" else 500000))
    f = torch.randn(E, n_way, ns + nq, 512, generator=g)
    if kind == "relu":          # non-negative and class-structured, as trunk outputs are
        mean = torch.randn(E, n_way, 1, 512, generator=g)
        f = torch.relu(0.5 * f + 0.5 * mean + 0.3)
    return f.reshape(-1, 512).contiguous()


def _hyper(noise, dtype=torch.float32, device="cpu"):
    # the float32 values are the inputs; float64 takes the same numbers
    vals = [torch.tensor([v], dtype=torch.float32) for v in (MEAN, RAW_OS, R.raw_noise_for(noise))]
    return [v.to(device=device, dtype=dtype) for v in vals]


def _chain_step(f, shape, kernel, noise, dtype, loss):
    """The chain in ``dtype`` -> dict(scores, and with ``loss``: loss, dfeats, dmean, draw_outputscale, draw_noise), float64."""
    E, n_way, ns, nq = shape
    x = f.detach().clone().to(dtype).requires_grad_(True)
    hyper = [h.requires_grad_(True) for h in _hyper(noise, dtype)]
    val, scores, _ = R.dkt_chain(x, hyper, n_way, ns, nq, E, kernel, loss=loss)
    out = dict(scores=scores.detach().double())
    if loss:
        val.backward()
        out.update(loss=val.detach().double(), dfeats=x.grad.double(), dmean=hyper[0].grad.double(),
                   draw_outputscale=hyper[1].grad.double(), draw_noise=hyper[2].grad.double())
    return out


def _rel_per_episode(got, want, E):
    got, want = got.reshape(E, -1).double().cpu(), want.reshape(E, -1)
    return max(float((got[e] - want[e]).norm() / want[e].norm()) for e in range(E))


def _rel_scalar(got, want):
    return abs(float(got) - float(want)) / abs(float(want))


@functools.lru_cache(maxsize=None)
def _references():
    """Every (shape, kind, kernel, noise, draw): the input, the float64 chain's values and the float32 CPU chain's distances to
    them.  -> (refs, vec, scal): vec[(shape, kind, kernel, noise)] = the largest float32 distance of scores / dfeats over the draws of
    the case; scal[(kind, kernel)] = the largest float32 distance of the loss and of each scalar gradient over ALL cases of the same
    feature kind and kernel (one float32 scalar is often right by chance, so a per-case yardstick would be a lottery).  Computed
    once for the module and never modified."""
    refs, vec, scal = {}, {}, {}
    for shape in CASES + SCORE_CASES:
        loss = shape in CASES
        for kind in KINDS:
            for draw in range(_draws(shape)):
                f = _features(kind, shape, draw)
                for kernel in KERNELS:
                    for noise in NOISES:
                        r64 = _chain_step(f, shape, kernel, noise, torch.float64, loss)
                        r32 = _chain_step(f, shape, kernel, noise, torch.float32, loss)
                        refs[(shape, kind, kernel, noise, draw)] = dict(f=f, **r64)
                        v = vec.setdefault((shape, kind, kernel, noise), dict(scores=0.0, dfeats=0.0))
                        v["scores"] = max(v["scores"], _rel_per_episode(r32["scores"], r64["scores"], shape[0]))
                        if loss:
                            v["dfeats"] = max(v["dfeats"], _rel_per_episode(r32["dfeats"], r64["dfeats"], shape[0]))
                            s = scal.setdefault((kind, kernel), dict.fromkeys(SCALARS, 0.0))
                            for n in SCALARS:
                                s[n] = max(s[n], _rel_scalar(r32[n], r64[n]))
    return refs, vec, scal


def _device_step(f, shape, kernel, noise, loss=True):
    """ops-level loss forward + backward and scores on the device -> dict like _chain_step's (device tensors)."""
    E, n_way, ns, nq = shape
    hyper = _hyper(noise, device="cuda")
    out = dict(scores=ops.dkt_scores(f, hyper, E, n_way, ns, nq, kernel=kernel))
    if loss:
        val, tape = ops.dkt_loss_forward(f, hyper, E, n_way, ns, nq, kernel=kernel, save=True)
        dfeats, (dmean, dos, dnoise) = ops.dkt_loss_backward(tape)
        out.update(loss=val, dfeats=dfeats, dmean=dmean, draw_outputscale=dos, draw_noise=dnoise, tape=tape)
    return out


def _compare(shape, kind, kernel, loss, feats_of=lambda f: f.cuda()):
    refs, vec, scal = _references()
    E, n_way, ns, nq = shape
    worst = 0.0
    for noise in NOISES:
        yard = vec[(shape, kind, kernel, noise)]
        for draw in range(_draws(shape)):
            r = refs[(shape, kind, kernel, noise, draw)]
            d = _device_step(feats_of(r["f"]), shape, kernel, noise, loss)
            assert d["scores"].shape == (E * n_way * nq, n_way) and not d["scores"].requires_grad
            items = [("scores", _rel_per_episode(d["scores"], r["scores"], E), yard["scores"])]
            if loss:
                assert d["dfeats"].shape == r["f"].shape and d["loss"].shape == (1,)
                items.append(("dfeats", _rel_per_episode(d["dfeats"], r["dfeats"], E), yard["dfeats"]))
                items += [(n, _rel_scalar(d[n].cpu().double(), r[n]), scal[(kind, kernel)][n]) for n in SCALARS]
            print("dkt %s %s %s noise %.2f draw %d: " % (_id(shape), kind, kernel, noise, draw)
                  + "  ".join("%s %.3e (yardstick %.3e, ratio %.2f)" % (n, e, y, e / max(y, 1e-300)) for n, e, y in items))
            for n, e, y in items:
                worst = max(worst, e / max(y, 1e-300))
                assert e <= 4.0 * y, (noise, draw, n, e, y)
    print("dkt %s %s %s: largest ratio %.2f" % (_id(shape), kind, kernel, worst))


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", CASES, ids=_id)
def test_kernels_match_float64_within_4x_the_float32_chain(shape, kind, kernel):
    """scores and dfeats: relative L2 distance to float64 per episode within 4 x the float32 CPU chain's (its largest over the draws
    of the case); the loss and the three scalar gradients within 4 x the largest float32 distance over all cases of the same
    feature kind and kernel.  Both noise levels, mean 0.05."""
    _compare(shape, kind, kernel, True)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SCORE_CASES, ids=_id)
def test_scores_match_float64_beyond_the_loss_domain(shape, kind, kernel):
    _compare(shape, kind, kernel, False)
    E, n_way, ns, nq = shape
    if n_way * (ns + nq) > ops.DKT_MAX_M:                          # 5-way 50-shot with 15 queries: scored above, not trained
        with pytest.raises(ValueError, match="N = n_way"):
            ops.dkt_loss_forward(_features(kind, shape, 0).cuda(), _hyper(0.1, device="cuda"), E, n_way, ns, nq)


@pytest.mark.parametrize("kernel", KERNELS)
def test_row_stride_640(kernel):
    def strided(f):
        buf = torch.full((f.shape[0], 640), float("nan"), device="cuda")
        buf[:, :512] = f.cuda()
        return buf[:, :512]
    _compare((3, 3, 2, 3), "relu", kernel, True, feats_of=strided)


def test_one_hot_rows_have_closed_forms():
    """Distinct one-hot rows under cossim: K = (s + noise) I, so A = R / (s + noise) and
    loss = (sum R^2 / (2 (s + noise)) + C N log(s + noise) / 2 + C N log(2 pi) / 2) / N.  K's diagonal is stored once (2^-24
    relative), the pivot's root is rounded once (2 x 2^-24 on its square) and A is stored once: 4 x 2^-24 on A; the loss adds its
    own store.  The bound is the larger of that and 4 x the distance of the float32 CPU chain on the same input."""
    E, n_way, ns, nq = 2, 5, 5, 16
    N = n_way * (ns + nq)
    g = torch.Generator().manual_seed(5)
    cols = torch.stack([torch.randperm(512, generator=g)[:N] for _ in range(E)]).reshape(-1)
    f = torch.zeros(E * N, 512)
    f[torch.arange(E * N), cols] = 1.0 + torch.rand(E * N, generator=g)              # any positive length: cossim normalises it
    h64 = _hyper(0.1, torch.float64)
    mean, s, noise = (float(v) for v in R.hyper_values(h64))
    Rm = R.targets(n_way, ns + nq, torch.float64) - mean
    A = Rm / (s + noise)
    loss = (0.5 * float((Rm * Rm).sum()) / (s + noise) + 0.5 * n_way * N * math.log(s + noise)
            + 0.5 * n_way * N * math.log(2.0 * math.pi)) / N
    val32, _, _ = R.dkt_chain(f, _hyper(0.1), n_way, ns, nq, E, scores=False)
    val64, _, _ = R.dkt_chain(f.double(), h64, n_way, ns, nq, E, scores=False)
    assert abs(float(val64) - loss) < 1e-12 * abs(loss)
    val, tape = ops.dkt_loss_forward(f.cuda(), _hyper(0.1, device="cuda"), E, n_way, ns, nq, save=True)
    eps = 2.0 ** -24
    bound = max(5 * eps, 4.0 * abs(float(val32) - loss) / abs(loss))
    err = abs(float(val) - loss) / abs(loss)
    print("dkt one-hot: loss %.9f device rel err %.3e, float32 chain %.3e, bound %.3e" % (loss, err, abs(float(val32) - loss) / abs(loss), bound))
    assert err <= bound
    Ad = tape["A"].cpu().double()
    assert Ad.shape == (E, N, n_way)
    errA = float(((Ad - A[None]) / A[None]).abs().max())
    print("dkt one-hot: A largest relative error %.3e (bound %.3e)" % (errA, 4 * eps))
    assert errA <= 4 * eps
    # log det K = 2 sum log L_ii: each pivot's square is within 3 x 2^-24 of s + noise, which moves its logarithm by as much
    assert float((tape["stats"][:, 3].cpu() - N * math.log(s + noise)).abs().max()) <= 4 * eps * N


@pytest.mark.parametrize("kernel", KERNELS)
def test_an_all_zero_row_gives_finite_values(kernel):
    shape = (1, 5, 5, 16)
    f = _features("relu", shape, 0).clone()
    f[7] = 0.0
    d = _device_step(f.cuda(), shape, kernel, 0.1)
    torch.cuda.synchronize()
    for n in ("scores", "dfeats") + SCALARS:
        assert bool(torch.isfinite(d[n]).all()), n
    r64 = _chain_step(f, shape, kernel, 0.1, torch.float64, True)
    r32 = _chain_step(f, shape, kernel, 0.1, torch.float32, True)
    live = torch.arange(105) != 7                                    # the clamped row's own gradient is dU / 1e-12: compared apart
    for rows in (live, ~live):
        err = float((d["dfeats"].cpu().double()[rows] - r64["dfeats"][rows]).norm() / r64["dfeats"][rows].norm())
        yard = float((r32["dfeats"][rows] - r64["dfeats"][rows]).norm() / r64["dfeats"][rows].norm())
        print("dkt zero row %s (%d rows): dfeats rel err %.3e, float32 chain %.3e" % (kernel, int(rows.sum()), err, yard))
        assert err <= 4.0 * yard
    assert _rel_scalar(d["loss"].cpu().double(), r64["loss"]) <= 4.0 * _references()[2][("relu", kernel)]["loss"]


def _run(f, shape, kernel="cossim", noise=0.1):
    d = _device_step(f, shape, kernel, noise)
    return [d[n] for n in ("scores", "loss", "dfeats", "dmean", "draw_outputscale", "draw_noise")] + [d["tape"]["A"], d["tape"]["L"]]


@pytest.mark.parametrize("shape", [(3, 3, 2, 3), (1, 5, 5, 16), (1, 32, 7, 1)], ids=_id)
def test_two_calls_are_bit_identical(shape):
    f = _features("relu", shape, 0).cuda()
    for kernel in KERNELS:
        for x, y in zip(_run(f, shape, kernel), _run(f, shape, kernel)):
            assert torch.equal(x, y)


def test_episodes_in_one_call_equal_single_calls():
    shape = (3, 3, 2, 3)
    f = _features("relu", shape, 1).cuda()
    N = 15
    together = _device_step(f, shape, "cossim", 0.01)
    singles = [_device_step(f[e * N:(e + 1) * N], (1, 3, 2, 3), "cossim", 0.01) for e in range(3)]
    assert torch.equal(together["scores"].reshape(3, -1), torch.stack([s["scores"].reshape(-1) for s in singles]))
    for k in ("A", "L", "U", "stats"):                                # the factor, A and each episode's loss: episode after episode
        assert torch.equal(together["tape"][k].reshape(3, -1), torch.stack([s["tape"][k].reshape(-1) for s in singles])), k
    # one call averages: every episode's feature gradient is the single call's with a third of the upstream gradient, bit for bit
    third = torch.full((1,), 1.0 / 3.0, device="cuda")
    for e, s in enumerate(singles):
        dfe, _ = ops.dkt_loss_backward(s["tape"], third)
        got = together["dfeats"][e * N:(e + 1) * N]
        assert float((got.double() - dfe.double()).abs().max()) <= 2.0 ** -23 * float(dfe.abs().max()), e
    # the loss and the scalar gradients add the episodes up in order: the float64 mean of the single calls, rounded
    for n in SCALARS:
        want = sum(float(s[n].double()) for s in singles) / 3.0
        scale = sum(abs(float(s[n])) for s in singles) / 3.0
        assert abs(float(together[n].double()) - want) <= 2.0 ** -22 * scale, n


def test_upstream_gradient_is_read_on_the_device():
    shape = (1, 5, 5, 16)
    f = _features("relu", shape, 0).cuda()
    tape = ops.dkt_loss_forward(f, _hyper(0.1, device="cuda"), *shape, save=True)[1]
    one = ops.dkt_loss_backward(tape)
    g = torch.full((1,), 4.0, device="cuda")
    four = ops.dkt_loss_backward(tape, g)
    assert torch.equal(four[0], 4.0 * one[0]) and all(torch.equal(a, 4.0 * b) for a, b in zip(four[1], one[1]))
    g.fill_(-2.0)                                                     # the same tensor, a new value: what a replayed graph sees
    assert torch.equal(ops.dkt_loss_backward(tape, g)[0], -2.0 * one[0])


def test_out_of_range_arguments_are_refused():
    lib = _lib.lib()
    p = ops._p
    f = torch.zeros(400, 520, device="cuda")
    mean, ros, rno = _hyper(0.1, device="cuda")
    ws = torch.zeros(8, 1 << 18, device="cuda")
    dbl = torch.zeros(3, 4096, device="cuda", dtype=torch.float64)
    st = ops._stream(f)

    def call_all(a, so=0):
        shp = (a["E"], a["n_way"], a["ns"], a["nq"], a["D"])
        U, K, L, A, V, B, W, out = ws
        loss_args = (p(dbl[1]), p(out), None, None) if so == 0 else (None, None, None, p(W))
        return [lib.mft_dkt_normalise(p(f), a["ld"], *shp, 0, p(U), p(dbl[0]), st),
                lib.mft_dkt_gram(*shp, so, p(U), p(ros), p(rno), p(K), st),
                lib.mft_dkt_factor(*shp, so, p(U), p(K), p(mean), p(ros), p(L), p(A), *loss_args, st),
                lib.mft_dkt_solve(*shp, p(U), p(L), p(A), p(V), p(B), p(dbl[0][2048:]), st),
                lib.mft_dkt_backward(*shp, 0, p(U), p(dbl[0]), p(A), p(V), p(B), p(ros), None, p(ws[7]), 512, p(dbl[2]), st),
                lib.mft_dkt_hyper_backward(*shp, p(dbl[2]), p(dbl[0][2048:]), p(dbl[1]), p(ros), p(rno), None, p(out[0:]), p(out[4:]), p(out[8:]), st),
                lib.mft_dkt_scores(*shp, p(U), p(W), p(mean), p(out), st)]

    good = dict(ld=520, E=1, n_way=5, ns=5, nq=16, D=512)
    assert call_all(good) == [0] * 7 and call_all(good, so=1)[:3] == [0] * 3
    for b in [dict(n_way=33, ns=1, nq=1), dict(D=256), dict(n_way=0), dict(ns=0), dict(nq=0), dict(E=0), dict(n_way=1, ns=257, nq=1)]:
        a = dict(good)
        a.update(b)
        assert call_all(a) == [-22] * 7, b
        assert call_all(a, so=1)[:3] == [-22] * 3, b
    big = dict(good, ns=50, nq=15)                                     # N = 325, S = 250: the loss launches refuse, the scores launches run
    assert call_all(big)[1:6] == [-22] * 5
    rc = call_all(big, so=1)
    assert rc[:3] == [0] * 3 and rc[6] == 0
    for ld in (500, 514):
        assert call_all(dict(good, ld=ld))[0] == -22
    shp = (1, 5, 5, 16, 512)
    U, K, L, A, V, B, W, out = ws
    assert lib.mft_dkt_normalise(p(f[:, 1:]), 520, *shp, 0, p(U), p(dbl[0]), st) == -22          # rows not 16-byte aligned
    assert lib.mft_dkt_gram(*shp, 0, p(U[1:]), p(ros), p(rno), p(K), st) == -22
    assert lib.mft_dkt_scores(*shp, p(U), p(W[1:]), p(mean), p(out), st) == -22
    assert lib.mft_dkt_backward(*shp, 0, p(U), p(dbl[0]), p(A), p(V), p(B), p(ros), None, p(ws[7]), 500, p(dbl[2]), st) == -22
    # a factor call whose outputs do not match its mode
    assert lib.mft_dkt_factor(*shp, 0, p(U), p(K), p(mean), p(ros), p(L), p(A), p(dbl[1]), p(out), None, p(W), st) == -22
    assert lib.mft_dkt_factor(*shp, 1, p(U), p(K), p(mean), p(ros), p(L), p(A), p(dbl[1]), p(out), None, p(W), st) == -22
    assert lib.mft_dkt_factor(*shp, 0, p(U), p(K), p(mean), p(ros), p(L), p(A), None, None, None, None, st) == -22
    torch.cuda.synchronize()
    z = lambda *s: torch.zeros(*s, device="cuda")  # noqa: E731
    hyper = (mean, ros, rno)
    for args in [(z(258, 512), 1, 1, 257, 1), (z(66, 512), 1, 33, 1, 1), (z(105, 256), 1, 5, 5, 16), (z(100, 512), 1, 5, 5, 16),
                 (z(105, 514)[:, :512], 1, 5, 5, 16)]:
        with pytest.raises(ValueError):
            ops.dkt_loss_forward(args[0], hyper, *args[1:])
        with pytest.raises(ValueError):
            ops.dkt_scores(args[0], hyper, *args[1:])
    with pytest.raises(ValueError):
        ops.dkt_loss_forward(z(325, 512), hyper, 1, 5, 50, 15)
    with pytest.raises(ValueError):
        ops.dkt_loss_forward(z(257, 512), hyper, 1, 1, 256, 1)          # N = 257; S = 256 is scored
    assert ops.dkt_scores(z(257, 512) + 1.0, hyper, 1, 1, 256, 1).shape == (1, 1)
    assert ops.dkt_scores(z(325, 512) + 1.0, hyper, 1, 5, 50, 15).shape == (75, 5)
    with pytest.raises(ValueError, match="kernel"):
        ops.dkt_scores(z(105, 512), hyper, 1, 5, 5, 16, kernel="rbf")
    with pytest.raises(RuntimeError):
        ops.dkt_scores(z(105, 512), (mean, ros, rno.double()), 1, 5, 5, 16)
    torch.cuda.synchronize()


def test_argmax_equals_float64_where_the_gap_exceeds_the_float32_error():
    refs, _, _ = _references()
    shape = (1, 5, 5, 15)
    total = decided = 0
    for kernel in KERNELS:
        for noise in NOISES:
            for draw in range(3):
                r = refs[(shape, "relu", kernel, noise, draw)]
                want = r["scores"]
                s32 = _chain_step(r["f"], shape, kernel, noise, torch.float32, False)["scores"]
                err = float((s32 - want).abs().max())
                top = torch.sort(want, dim=1, descending=True).values
                clear = (top[:, 0] - top[:, 1]) > err
                got = ops.dkt_scores(r["f"].cuda(), _hyper(noise, device="cuda"), *shape, kernel=kernel).argmax(1).cpu()
                assert torch.equal(got[clear], want.argmax(1)[clear])
                total += clear.numel()
                decided += int(clear.sum())
                assert torch.equal(want.argmax(1), torch.arange(5).repeat_interleave(15))         # and every query is classified right
    assert decided >= 0.95 * total, (decided, total)                  # the rule cannot hide a failure


def test_autograd_wrappers():
    shape = (2, 3, 2, 3)
    f = _features("relu", shape, 0).cuda().requires_grad_(True)
    hyper = [h.requires_grad_(True) for h in _hyper(0.1, device="cuda")]
    loss = AG.dkt_loss(f, *hyper, 3, 2, 3, episodes=2, kernel="linear")
    assert loss.shape == () and loss.requires_grad
    (2.0 * loss).backward()
    d = _device_step(f.detach(), shape, "linear", 0.1)
    assert torch.equal(loss.detach().reshape(1), d["loss"])
    two = torch.full((1,), 2.0, device="cuda")
    dfeats, dh = ops.dkt_loss_backward(d["tape"], two)
    assert torch.equal(f.grad, dfeats) and all(torch.equal(h.grad, g) and h.grad.shape == (1,) for h, g in zip(hyper, dh))
    scores = AG.dkt_scores(f, *hyper, 3, 2, 3, episodes=2, kernel="linear")
    assert not scores.requires_grad and torch.equal(scores, d["scores"])     # a prediction: never differentiated through
    with torch.no_grad():
        assert torch.equal(AG.dkt_loss(f, *hyper, 3, 2, 3, episodes=2, kernel="linear").reshape(1), d["loss"])
    acc = torch.zeros((), device="cuda", dtype=torch.float64)
    for _ in range(2):
        AG.dkt_loss(f, *hyper, 3, 2, 3, episodes=2, kernel="linear", loss_sum=acc)
    assert abs(float(acc) - 2.0 * float(d["loss"])) <= 1e-6 * abs(float(d["loss"]))


# ------------------------------------------------------------------------------------------------ meta-training step
def _oracle(sd32, xs, kernel="cossim"):
    """float64 loss (mean over the episodes of xs [k, n_way, S+Q, 3, H, W]) and gradients of every parameter."""
    sd = O.clone_state(sd32, torch.float64)
    pkeys = [k for k, v in sd.items() if v.is_floating_point() and "running" not in k]
    for k in pkeys:
        sd[k].requires_grad_(True)
    n_way, per = xs.shape[1], xs.shape[2]
    feats = torch.cat([O.resnet10_forward(sd, x.double().reshape(-1, *x.shape[2:]), prefix="feature.") for x in xs])
    loss, _, _ = R.dkt_chain(feats, [sd[k] for k in HEAD], n_way, 5, per - 5, xs.shape[0], kernel, scores=False)
    grads = torch.autograd.grad(loss, [sd[k] for k in pkeys])
    return float(loss.detach()), dict(zip(pkeys, grads))


def _check_grads(named, ref):
    # bounds of tests/test_tpn_gpu.py::_check_grads (the trunk backward is the same code)
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
    sd.update(synthetic.dkt_head_state(32))
    return sd


def _model(sd, n_way=5, kernel="cossim"):
    m = DKT(model_dict['ResNet10'], n_way=n_way, n_support=5, kernel=kernel)
    m.load_state_dict(sd)
    m = m.cuda()
    m.train()
    m.n_query = 16
    return m


def test_set_forward_loss_backward_vs_oracle_and_g32(golden_dir):
    """The envelope of tests/test_tpn_gpu.py for G30: scores to 1e-3, the loss to 2e-4, every gradient by _check_grads, the
    BatchNorm gradients to 3e-2 and every gradient norm to 1e-2.  The three head gradients are scalars behind the whole trunk: they
    take _check_grads' bound against G32 as every other parameter does, and their ratio to G32's float32 distance is printed (the
    head alone is held to 4 x the float32 chain by test_kernels_match_float64_within_4x_the_float32_chain)."""
    g = _g32(golden_dir)
    sd = _state(32)
    model = _model(sd)
    x = synthetic.train_episode(32, 5, 5, 16, 84)
    with torch.no_grad():
        sc = model.set_forward(x)
    assert not sc.requires_grad
    np.testing.assert_allclose(sc.cpu().numpy(), g["scores"], rtol=1e-3, atol=1e-3)
    assert not model.set_forward(x).requires_grad                      # with autograd on too: a prediction
    loss = model.set_forward_loss(x)
    assert loss.shape == () and loss.requires_grad
    loss.backward()
    assert abs(float(loss.detach()) - float(g["loss"])) < 2e-4
    ref_loss, ref = _oracle(sd, x[None])
    assert abs(ref_loss - float(g["loss"])) < 1e-9
    named = dict(model.named_parameters())
    assert set(ref) == set(named)
    _check_grads(named, ref)
    for k in HEAD:
        want = torch.from_numpy(g["headgrad:" + k])
        assert float((ref[k] - want).norm()) <= 1e-8 * float(want.norm())
        err = float((named[k].grad.cpu().double() - want).norm() / want.norm())
        yard = float(g["f32err:headgrad:" + k])
        print("dkt step: %s rel err %.3e, G32 float32 distance %.3e, ratio %.2f" % (k, err, yard, err / yard))
        assert err < 3e-2, (k, err)
    for name in g["bnnames"]:
        name = str(name)
        want = g["bngrad:" + name]
        got = named[name].grad.cpu().numpy()
        assert np.linalg.norm(got - want) <= 3e-2 * np.linalg.norm(want) + 1e-9, name
    gn = {k: float(p.grad.norm()) for k, p in named.items()}
    for name, refn in zip(g["gradnames"], g["gradnorms"]):
        assert abs(gn[str(name)] - refn) <= 1e-2 * refn + 1e-9, name
    big = DKT(model_dict['ResNet10'], n_way=5, n_support=50).cuda()
    with pytest.raises(ValueError, match="N = n_way"):                 # refused before the trunk pass: x is never a valid image batch
        big.set_forward_loss(torch.zeros(5, 65, 1))


@pytest.mark.parametrize("kernel", KERNELS)
def test_lockstep_two_episodes_equal_float64_mean(kernel):
    sd = _state(23)
    xs = torch.stack([synthetic.train_episode(400 + i, 5, 5, 16, 84) for i in range(2)])
    model = _model(sd, kernel=kernel)
    scores = model.set_forward_lockstep(xs.cuda())
    assert scores.shape == (2 * 80, 5) and not scores.requires_grad
    loss = model.set_forward_loss_lockstep(xs.cuda())
    loss.backward()
    ref_loss, ref = _oracle(sd, xs, kernel)
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
        model = _model(_state(32))
        opt = optim.Adam(model.parameters())
        capsys.readouterr()
        model.train_loop(0, Loader(), opt)
        out = capsys.readouterr().out
        st = model.__dict__.get("_mft_graph_steps", {}).get("set_forward_loss")
        return out, {n: p.detach().clone() for n, p in model.named_parameters()}, [b.detach().clone() for b in model.buffers()], st, model

    out_e, par_e, buf_e, st_e, model_e = run(False)
    out_g, par_g, buf_g, st_g, model_g = run(True)
    assert st_e is None and st_g is not None and st_g.graph is not None and not st_g.failed
    assert out_g == out_e and out_e.count("Loss") == 1
    assert list(par_e) == list(par_g) and all(torch.equal(par_e[n], par_g[n]) for n in par_e)
    assert all(torch.equal(a, b) for a, b in zip(buf_e, buf_g))
    fresh = _state(32)
    for k in HEAD:                                                             # the three hyperparameters were trained
        assert not torch.equal(par_g[k].cpu(), fresh[k]), k
    # the replayed loss follows its input: two episodes give two losses, each the eager model's bit for bit
    replayed = [st_g(x.cuda()).detach().clone() for x in eps[:2]]
    eager = [model_e.set_forward_loss(x).detach() for x in eps[:2]]
    assert not torch.equal(replayed[0], replayed[1])
    assert all(torch.equal(a, b) for a, b in zip(replayed, eager))


def test_dkt_step_issues_no_aten_device_kernels():
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dkt_step_worker.py")
    r = subprocess.run([sys.executable, worker], capture_output=True, text=True, timeout=900)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert lines, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    res = json.loads(lines[-1][len("RESULT "):])
    print("dkt step worker:", res)
    assert res["n_dev"] > 0 and not res["aten"] and not res["head_aten"] and not res["head_step_aten"], res
    # the loss is normalise, Gram, factor and the one-thread mean behind it; three launches backward; the
    # scores are normalise, Gram, factor and scores -- whatever the shape
    assert res["fwd_n_dev"] == 4 and res["bwd_n_dev"] == 3, res
    assert res["head_n_dev"] == res["scores_n_dev_50shot"] == 4, res


# ------------------------------------------------------------------------------------------------ evaluation and CLI
def test_evaluate_in_lockstep_equals_a_loop_over_set_forward():
    g = torch.Generator().manual_seed(77)
    mean = torch.randn(8, 1, 512, generator=g)
    rows = torch.relu(0.5 * torch.randn(8, 25, 512, generator=g) + 0.5 * mean + 0.3).numpy()
    table = feature_eval.FeatureTable({c: list(rows[c]) for c in range(8)})
    model = feature_eval.build_model("dkt", model_dict["ResNet10"], 5, 5)
    model.load_state_dict(_state(32))
    model = model.cuda().eval()

    def seed():
        random.seed(10)
        np.random.seed(10)
        torch.manual_seed(10)

    seed()
    acc, s_lock = feature_eval.evaluate(model, "dkt", table, 5, 5, 15, 6, 4, return_scores=True)
    assert acc.shape == (6,) and float(acc.mean()) > 80.0                      # class-structured features: nearly all right
    seed()
    _, idx, _ = feature_eval.episode_tables(table.rows, 5, 5, 15, 6)
    feats = table.device_feats()
    for e in range(6):
        z = feats[torch.from_numpy(idx[e].reshape(-1)).to(feats.device)].view(5, 20, 512)
        with torch.no_grad():
            one = model.set_forward(z, is_feature=True)
        assert np.array_equal(one.cpu().numpy(), s_lock[e]), e
    assert feature_eval.EPISODES_PER_BATCH == 100


@pytest.mark.parametrize("extra,dirname", [([], "ResNet10_dkt_5way_5shot"), (["--kernel", "linear"], "ResNet10_dkt_linear_5way_5shot"),
                                           (["--episodes_per_rank", "2"], "ResNet10_dkt_5way_5shot"),
                                           (["--model", "ResNet10_FW"], "ResNet10_FW_dkt_5way_5shot")],
                         ids=["plain", "linear", "lockstep2", "fw"])
def test_train_main_dkt_writes_a_loadable_checkpoint(golden_dir, tmp_path, monkeypatch, extra, dirname):
    from meta_fine_tuning_amd import configs, train
    monkeypatch.setattr(configs, "save_dir", str(tmp_path))
    model = train.main(["--dataset", "miniImageNet", "--method", "dkt", "--stop_epoch", "1"] + extra, n_episode=2, size=84)
    assert type(model) is DKT and model.kernel == ("linear" if "linear" in extra else "cossim")
    f = tmp_path / "checkpoints" / "miniImageNet" / dirname / "0.tar"
    assert f.is_file()
    state = torch.load(str(f), map_location="cpu")["state"]
    assert list(state.keys())[-3:] == HEAD
    if "ResNet10_FW" not in extra:
        assert list(state.keys()) == [str(k) for k in _g32(golden_dir)["state_keys"]]
    fresh = DKT(model_dict['ResNet10_FW' if "ResNet10_FW" in extra else 'ResNet10'], n_way=5, n_support=5)
    fresh.load_state_dict(state)
    init = DKT(model_dict['ResNet10'], n_way=5, n_support=5).gp
    assert all(bool(torch.isfinite(state[k]).all()) for k in HEAD)
    assert any(not torch.equal(state[k], getattr(init, k[3:]).detach()) for k in HEAD)           # the step reached the head


def test_save_features_and_test_drivers_take_dkt(tmp_path, monkeypatch, capsys):
    from meta_fine_tuning_amd import configs, save_features
    from meta_fine_tuning_amd import test as test_driver
    monkeypatch.setattr(configs, "save_dir", str(tmp_path))
    for k, v in (("MFT_POOL_PER_CLASS", "24"), ("MFT_IMAGE_SIZE", "64"), ("MFT_EPISODES", "6"), ("MFT_EPISODES_PER_BATCH", "4")):
        monkeypatch.setenv(k, v)
    monkeypatch.delenv("MFT_STANDIN_WEIGHTS", raising=False)
    argv = ["--dataset", "miniImageNet", "--method", "dkt", "--test_dataset", "ISIC"]
    with pytest.raises(FileNotFoundError):
        save_features.main(argv)
    monkeypatch.setenv("MFT_STANDIN_WEIGHTS", "1")                               # the stand-in backbone with synthetic.dkt_head_state behind it
    from meta_fine_tuning_amd.io_utils import parse_args
    state, loaded = save_features.resolve_state(parse_args('save_features', argv), verbose=False)
    assert loaded is None and [k for k in state if not k.startswith("feature.")] == HEAD
    assert all(torch.equal(state[k], v) for k, v in synthetic.dkt_head_state().items())
    featfile = save_features.main(argv)
    assert featfile.endswith("features/miniImageNet/ResNet10_dkt_5way_5shot/novel.npz")
    acc = test_driver.main(argv)
    out = capsys.readouterr().out
    assert len(acc) == 6 and np.all((acc >= 0) & (acc <= 100)) and "6 Test Acc" in out
    with pytest.raises(FileNotFoundError):                                       # another kernel is another directory
        test_driver.main(argv + ["--kernel", "linear"])
