"""FEAT on a real MI355X: the set-to-set head kernels (csrc/feat.hip) against float64 with the float32 CPU chain as the yardstick,
the exact cases, determinism, the refusals, the dropout draw against its host restatement, the meta-training step against the
float64 oracle and the golden G31, lockstep episodes, the graphed episode loop, the `test` driver's lockstep scoring and
train.main --method feat."""
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
from meta_fine_tuning_amd.methods.feat import FEAT
from oracle import mft_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import feat_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu
torch.set_num_threads(8)

HEAD = R.HEAD


def _g31(golden_dir):
    return np.load(os.path.join(golden_dir, "g31_feat.npz"))


def _head(dtype=torch.float32, device="cpu"):
    hs = synthetic.feat_head_state(31)
    head = [hs[k].to(device=device, dtype=dtype) for k in HEAD]
    # (the constructor's LayerNorm is the identity affine: move it off ones and zeros so that dln_w and ln_b are exercised)
    g = torch.Generator().manual_seed(4242)
    head[3] = (head[3].cpu().double() + 0.1 * torch.randn(512, generator=g, dtype=torch.float64)).to(device=device, dtype=dtype)
    head[4] = (0.1 * torch.randn(512, generator=g, dtype=torch.float64)).to(device=device, dtype=dtype)
    return tuple(h.contiguous() for h in head)


# ------------------------------------------------------------------------------------------------ kernels
# (E, n_way, n_support, n_query): the training and the test shape, T = 1, two episodes of one class, T = 2, the multi-episode
# stride, 20-shot, T = 64 / 65 / 66 (the second softmax entry of a lane) and the n_way limit
CASES = [(1, 5, 5, 16), (1, 5, 5, 15), (1, 1, 1, 1), (2, 1, 1, 2), (1, 2, 1, 1), (3, 3, 2, 3), (1, 5, 20, 15), (1, 4, 48, 16),
         (1, 3, 63, 2), (1, 5, 50, 16), (1, 32, 1, 1)]
MODES = ["eval", "train_ones", "train_masks"]
KINDS = ["randn", "relu"]
CASE_IDS = ["E%d_w%d_s%d_q%d" % s for s in CASES]


def _draws(shape):
    return 1 if shape[1] * (shape[2] + shape[3]) >= 175 else 2


def _features(kind, shape, draw):
    # the recipe of tests/test_tpn_gpu.py::_features, with the second upstream gradient the train mode needs
    E, n_way, ns, nq = shape
    g = torch.Generator().manual_seed(1000003 * draw + 7919 * E + 131 * n_way + 17 * ns + nq + (0 if kind == "randn" else 500000))
    f = torch.randn(E, n_way, ns + nq, 512, generator=g)
    if kind == "relu":          # non-negative and class-structured, as trunk outputs are
        mean = torch.randn(E, n_way, 1, 512, generator=g)
        f = torch.relu(0.5 * f + 0.5 * mean + 0.3)
    G = torch.randn(E * n_way * nq, n_way, generator=g)
    Greg = torch.randn(E * n_way * (ns + nq), n_way, generator=g)
    return f.reshape(-1, 512).contiguous(), G, Greg


def _masks(mode, shape, draw):
    if mode != "train_masks":
        return None
    return synthetic.feat_masks(900 + draw, *shape)


def _chain_step(f, G, Greg, shape, mode, masks, dtype):
    """Forward + backward of the chain in ``dtype`` -> dict(scores, reg, dfeats, the seven parameter gradients) in float64 and
    the per-parameter sums of the absolute values of the terms."""
    E, n_way, ns, nq = shape
    x = f.to(dtype).requires_grad_(True)
    head = [p.clone().requires_grad_(True) for p in _head(dtype)]
    taps = []
    scores, reg = R.feat_chain(x, head, n_way, ns, nq, E, train=mode != "eval", masks=masks, taps=taps)
    obj = (scores * G.to(dtype)).sum()
    if reg is not None:
        obj = obj + (reg * Greg.to(dtype)).sum()
    obj.backward()
    out = dict(scores=scores.detach().double(), reg=None if reg is None else reg.detach().double(), dfeats=x.grad.double(),
               params=[p.grad.double() for p in head])
    return out, R.term_sums(taps)


@functools.lru_cache(maxsize=None)
def _reference(shape, kind, mode, draw):
    """Inputs, the float64 step and the float32 CPU chain's distances to it.  Computed once per (case, kind, mode, draw)."""
    f, G, Greg = _features(kind, shape, draw)
    masks = _masks(mode, shape, draw)
    r64, den = _chain_step(f, G, Greg, shape, mode, masks, torch.float64)
    r32, _ = _chain_step(f, G, Greg, shape, mode, masks, torch.float32)
    return dict(f=f, G=G, Greg=Greg, masks=masks, r64=r64, den=[max(d, 1e-300) for d in den], yard=_distances(r32, r64, den, shape[0]))


def _rel_per_episode(got, want, E):
    got, want = got.reshape(E, -1), want.reshape(E, -1)
    return max(float((got[e] - want[e]).norm() / want[e].norm()) for e in range(E))


def _distances(r, r64, den, E):
    d = [_rel_per_episode(r["scores"], r64["scores"], E)]
    d.append(0.0 if r64["reg"] is None else _rel_per_episode(r["reg"], r64["reg"], E))
    d.append(_rel_per_episode(r["dfeats"], r64["dfeats"], E))
    return d + [float((a - b).norm()) / max(dn, 1e-300) for a, b, dn in zip(r["params"], r64["params"], den)]


def _device_step(f, G, Greg, shape, mode, masks, head=None, ld=512):
    E, n_way, ns, nq = shape
    head = head or _head(device="cuda")
    x = f.cuda()
    if ld != 512:
        wide = torch.zeros(x.shape[0], ld, device="cuda")
        wide[:, :512] = x
        x = wide[:, :512]
    m = None if masks is None else tuple(t.cuda() for t in masks)
    scores, reg, tape = ops.feat_forward(x, head, E, n_way, ns, nq, mode != "eval", masks=m, save=True)
    grads = ops.feat_backward(tape, G.cuda(), None if mode == "eval" else Greg.cuda())
    return scores, reg, tape, grads


NAMES = ["scores", "reg", "dfeats", "dWq", "dWk", "dWv", "dln_w", "dln_b", "dWfc", "dbfc"]


def _check_case(shape, kind, mode, ld=512):
    runs = []
    for draw in range(_draws(shape)):
        r = _reference(shape, kind, mode, draw)
        scores, reg, _, grads = _device_step(r["f"], r["G"], r["Greg"], shape, mode, r["masks"], ld=ld)
        E, n_way, ns, nq = shape
        assert scores.shape == (E * n_way * nq, n_way) and grads[0].shape == r["f"].shape
        assert (reg is None) == (mode == "eval") and (reg is None or reg.shape == (E * n_way * (ns + nq), n_way))
        assert [tuple(g.shape) for g in grads[1:]] == [tuple(s) for s in ops.FEAT_HEAD_SHAPES]
        dev = dict(scores=scores.cpu().double(), reg=None if reg is None else reg.cpu().double(), dfeats=grads[0].cpu().double(),
                   params=[g.cpu().double() for g in grads[1:]])
        runs.append((_distances(dev, r["r64"], r["den"], E), r["yard"]))
    yard = [max(y[i] for _, y in runs) for i in range(len(NAMES))]
    worst = 0.0
    for draw, (err, _) in enumerate(runs):
        print("feat %s %s %s ld %d draw %d: " % (shape, kind, mode, ld, draw)
              + "  ".join("%s %.3e (yardstick %.3e, ratio %.2f)" % (n, e, y, e / max(y, 1e-300)) for n, e, y in zip(NAMES, err, yard)))
        worst = max([worst] + [e / y for e, y in zip(err, yard) if y > 0.0])
    print("feat %s %s %s: largest ratio %.2f" % (shape, kind, mode, worst))
    for draw, (err, _) in enumerate(runs):
        for n, e, y in zip(NAMES, err, yard):
            assert e <= 4.0 * y, (draw, n, e, y)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_kernels_match_float64_within_4x_the_float32_chain(case, kind, mode):
    """Scores, reg, dfeats and the seven parameter gradients within 4 x the distance of the float32 CPU chain to float64 on the
    same inputs and multipliers (the maximum over the draws of the shape, kind and mode); a parameter gradient's distance is taken
    relative to the sum of the absolute values of its terms, which does not cancel."""
    _check_case(case, kind, mode)


@pytest.mark.parametrize("mode", MODES)
def test_row_stride_520(mode):
    _check_case((3, 3, 2, 3), "relu", mode, ld=520)


# ------------------------------------------------------------------------------------------------ exact cases
def test_one_token_attention_output_equals_v_bit_for_bit():
    for shape in ((1, 1, 1, 1), (2, 1, 1, 2)):
        r = _reference(shape, "randn", "eval", 0)
        _, _, tape, _ = _device_step(r["f"], r["G"], r["Greg"], shape, "eval", None)
        assert torch.equal(tape["o"], tape["qkv"][2]) and bool((tape["P"] == 1.0).all())


def test_all_zero_output_multiplier_gives_layernorm_of_x():
    shape = (1, 3, 2, 3)
    f, G, Greg = _features("relu", shape, 0)
    m_att, m_out = synthetic.feat_masks(5, *shape)
    head = _head(device="cuda")
    _, _, tape, _ = _device_step(f, G, Greg, shape, "train_masks", (m_att, torch.zeros_like(m_out)), head=head)
    X = tape["X"].cpu().double()
    want = F.layer_norm(X, (512,), head[3].cpu().double(), head[4].cpu().double(), 1e-5)
    # h = 0 * y + X = X exactly; the device rounds LayerNorm(X), evaluated in double, once
    assert float((tape["A"].cpu().double() - want).abs().max()) <= 2.0 ** -23 * float(want.abs().max())
    assert torch.equal(tape["X"][3:].cpu(), f)                                  # the class sets are the rows themselves


# ------------------------------------------------------------------------------------------------ determinism and refusals
def _flat(out):
    scores, reg, tape, grads = out
    return [scores] + ([] if reg is None else [reg]) + list(grads)


@pytest.mark.parametrize("shape", [(3, 3, 2, 3), (1, 5, 5, 16)], ids=lambda s: "E%d_w%d_s%d_q%d" % s)
def test_two_calls_are_bit_identical(shape):
    r = _reference(shape, "relu", "train_masks", 0)
    a = _flat(_device_step(r["f"], r["G"], r["Greg"], shape, "train_masks", r["masks"]))
    b = _flat(_device_step(r["f"], r["G"], r["Greg"], shape, "train_masks", r["masks"]))
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_episodes_in_one_call_equal_single_calls():
    shape = (3, 3, 2, 3)
    r = _reference(shape, "relu", "train_masks", 1)
    f, G, Greg, (m_att, m_out) = r["f"], r["G"], r["Greg"], r["masks"]
    together = _flat(_device_step(f, G, Greg, shape, "train_masks", (m_att, m_out)))
    N, Q, T, n = 15, 9, 5, 3
    singles = []
    for e in range(3):
        ma = torch.cat([m_att[e * n * n:(e + 1) * n * n], m_att[3 * n * n + e * n * T * T:3 * n * n + (e + 1) * n * T * T]])
        mo = torch.cat([m_out[e * n:(e + 1) * n], m_out[3 * n + e * N:3 * n + (e + 1) * N]])
        singles.append(_flat(_device_step(f[e * N:(e + 1) * N], G[e * Q:(e + 1) * Q], Greg[e * N:(e + 1) * N], (1, 3, 2, 3), "train_masks",
                                          (ma.contiguous(), mo.contiguous()))))
    for i in range(3):                                   # scores, reg, dfeats: episode after episode
        assert torch.equal(together[i].reshape(3, -1), torch.stack([s[i].reshape(-1) for s in singles])), i
    # the parameter gradients add the episodes up in row order: the one-call sum is the float64 sum of the single calls, rounded
    for i in range(3, 10):
        want = sum(s[i].double() for s in singles)
        scale = sum(float(s[i].abs().max()) for s in singles)
        assert float((together[i].double() - want).abs().max()) <= 2.0 ** -22 * scale, i


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_non_finite_features_give_non_finite_output_and_the_call_returns(bad):
    shape = (1, 5, 5, 16)
    r = _reference(shape, "relu", "train_ones", 0)
    f = r["f"].clone()
    f[3, 7] = bad
    out = _device_step(f, r["G"], r["Greg"], shape, "train_ones", None)
    torch.cuda.synchronize()
    assert not bool(torch.isfinite(out[0]).all()) and not bool(torch.isfinite(out[1]).all())
    f = torch.full_like(r["f"], bad)
    out = _device_step(f, r["G"], r["Greg"], shape, "train_ones", None)
    torch.cuda.synchronize()
    assert not bool(torch.isfinite(out[0]).any()) and not bool(torch.isfinite(out[1]).any())


def test_out_of_range_arguments_are_refused():
    lib = _lib.lib()
    p = ops._p
    f = torch.zeros(700, 520, device="cuda")
    head = _head(device="cuda")
    wq, wk, wv, ln_w, ln_b, wfc, bfc = head
    big = [torch.zeros(3 * 701 * 512, device="cuda") for _ in range(8)]
    idx = torch.zeros(1, device="cuda", dtype=torch.int64)
    st = ops._stream(f)

    def call_all(a):
        shp = (a["E"], a["n_way"], a["ns"], a["nq"], a["D"], 1)
        b = big
        return [lib.mft_feat_tokens(p(f), a["ld"], *shp, p(b[0]), st),
                lib.mft_feat_project(p(b[0]), *shp, p(wq), p(wk), p(wv), p(b[1]), st),
                lib.mft_feat_attention(p(b[1]), *shp, None, p(b[2]), p(b[3]), st),
                lib.mft_feat_fc(p(b[3]), *shp, p(wfc), p(bfc), p(b[4]), st),
                lib.mft_feat_norm(p(b[4]), p(b[0]), *shp, None, p(ln_w), p(ln_b), p(b[5]), p(b[6]), p(b[7]), st),
                lib.mft_feat_scores(p(f), a["ld"], *shp, p(b[5]), 64.0, 32.0, p(b[2]), p(b[3]), p(b[4]), st),
                lib.mft_feat_scores_backward(p(f), a["ld"], *shp, p(b[5]), p(b[3]), p(b[2]), p(b[4]), 64.0, 32.0, p(b[6]), p(b[7]), st),
                lib.mft_feat_norm_backward(p(b[7]), p(b[4]), p(b[0]), *shp, None, p(ln_w), p(b[6]), p(b[6]), p(b[2]), p(b[3]), p(b[5]),
                                           p(b[5][512:]), p(b[5][1024:]), st),
                lib.mft_feat_fc_backward(p(b[2]), p(b[3]), *shp, p(wfc), p(b[4]), p(b[5]), st),
                lib.mft_feat_attention_backward(p(b[4]), p(b[1]), p(b[2]), None, *shp, p(b[3]), p(b[5]), st),
                lib.mft_feat_project_backward(p(b[5]), p(b[0]), p(b[3]), *shp, p(wq), p(wk), p(wv), p(b[4]), p(b[6]), st),
                lib.mft_feat_dfeats(p(b[6]), p(b[4]), *shp, p(b[7]), a["ld"], st),
                lib.mft_feat_draw(*shp[:5], 0.1, 0.5, 0, p(idx), None, None, p(b[2]), p(b[3]), st),
                lib.mft_feat_loss(p(b[2]), p(b[4]), *shp[:4], 0.01, p(b[5]), None, st),
                lib.mft_feat_loss_backward(p(b[2]), p(b[4]), *shp[:4], 0.01, None, p(b[6]), p(b[7]), st)]

    good = dict(ld=520, E=1, n_way=5, ns=5, nq=16, D=512)
    assert call_all(good) == [0] * 15
    assert call_all(dict(good, ns=50)) == [0] * 15                              # 5-way 50-shot, 16 queries: T = 66
    for b in [dict(n_way=33, ns=1, nq=1), dict(n_way=0), dict(ns=0), dict(nq=0), dict(E=0), dict(ns=113), dict(n_way=1, ns=128, nq=1)]:
        assert call_all(dict(good, **b)) == [-22] * 15, b
    assert call_all(dict(good, D=256))[:13] == [-22] * 13                       # (the two loss launchers take no D)
    for ld in (500, 514):
        rc = call_all(dict(good, ld=ld))
        assert rc[0] == rc[5] == rc[6] == rc[11] == -22
    assert lib.mft_feat_draw(1, 5, 5, 16, 512, 1.0, 0.5, 0, p(idx), None, None, p(big[2]), p(big[3]), st) == -22
    assert lib.mft_feat_draw(1, 5, 5, 16, 512, 0.1, 0.5, 0, p(idx), p(big[4]), None, p(big[2]), p(big[3]), st) == -22
    torch.cuda.synchronize()
    z = lambda *s: torch.zeros(*s, device="cuda")  # noqa: E731
    for args in [(z(130, 512), 1, 1, 129, 1), (z(66, 512), 1, 33, 1, 1), (z(105, 256), 1, 5, 5, 16), (z(100, 512), 1, 5, 5, 16),
                 (z(105, 514)[:, :512], 1, 5, 5, 16), (z(105, 512), 1, 5, 0, 21)]:
        with pytest.raises(ValueError):
            ops.feat_forward(args[0], head, *args[1:], False)
    with pytest.raises(ValueError):                                            # multipliers belong to train mode
        ops.feat_forward(z(105, 512), head, 1, 5, 5, 16, False, masks=(z(10), z(10)))
    with pytest.raises(RuntimeError):
        ops.feat_forward(torch.zeros(105, 512), head, 1, 5, 5, 16, False)


# ------------------------------------------------------------------------------------------------ dropout draw
def test_dropout_draw_equals_the_host_philox_restatement():
    shape, seed = (1, 3, 2, 3), 0x1234567887654321
    index = torch.tensor([5], device="cuda", dtype=torch.int64)
    m_att, m_out = ops.feat_draw(*shape, seed, index)
    assert int(index.item()) == 6                                               # the launch stores index + 1
    ha, ho = R.draw_masks(seed, 5, *shape)
    assert m_att.shape == ha.shape == (3 * 3 + 3 * 25,) and m_out.shape == ho.shape == (3 + 15, 512)
    assert np.array_equal(m_att.cpu().numpy(), ha) and np.array_equal(m_out.cpu().numpy(), ho)
    assert set(np.unique(ho)) == {np.float32(0.0), np.float32(2.0)}
    assert set(np.unique(m_att.cpu().numpy())) <= {np.float32(0.0), np.float32(1.0 / (1.0 - float(np.float32(0.1))))}
    assert 0.35 < float((m_out == 0).float().mean()) < 0.65
    index.fill_(5)
    again = ops.feat_draw(*shape, seed, index)
    assert torch.equal(again[0], m_att) and torch.equal(again[1], m_out)        # the same index twice: the same masks
    nxt = ops.feat_draw(*shape, seed, index)                                    # the next index (6): others
    assert int(index.item()) == 7 and not torch.equal(nxt[1], m_out)
    assert np.array_equal(nxt[1].cpu().numpy(), R.draw_masks(seed, 6, *shape)[1])
    other = ops.feat_draw(*shape, seed + 1, torch.tensor([5], device="cuda", dtype=torch.int64))
    assert not torch.equal(other[1], m_out)
    forced = ops.feat_draw(*shape, seed, index, masks_in=(nxt[0], nxt[1]))      # the test hook copies, and still advances
    assert torch.equal(forced[0], nxt[0]) and torch.equal(forced[1], nxt[1]) and int(index.item()) == 8


# ------------------------------------------------------------------------------------------------ meta-training step
def _oracle(sd32, xs, masks=None, train=True):
    """float64 loss (mean over the episodes of xs [k, n_way, S+Q, 3, H, W]) and gradients of every parameter on the forced
    multipliers ``masks`` (the k-episode layout) -> (total, main, gradients)."""
    sd = O.clone_state(sd32, torch.float64)
    pkeys = [k for k, v in sd.items() if v.is_floating_point() and "running" not in k]
    for k in pkeys:
        sd[k].requires_grad_(True)
    k_ep, n_way, per = xs.shape[0], xs.shape[1], xs.shape[2]
    feats = torch.cat([O.resnet10_forward(sd, x.double().reshape(-1, *x.shape[2:]), prefix="feature.") for x in xs])
    scores, reg = R.feat_chain(feats, [sd[k] for k in HEAD], n_way, 5, per - 5, k_ep, train=train, masks=masks)
    total, main, _ = R.feat_loss(scores, reg, n_way, 5, per - 5, k_ep)
    grads = torch.autograd.grad(total, [sd[k] for k in pkeys])
    return float(total.detach()), float(main.detach()), dict(zip(pkeys, grads))


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
    sd.update(synthetic.feat_head_state(31))
    return sd


def _model(sd, n_way=5):
    m = FEAT(model_dict['ResNet10'], n_way=n_way, n_support=5)
    m.load_state_dict(sd)
    m = m.cuda()
    m.train()
    m.n_query = 16
    return m


def test_set_forward_loss_backward_vs_oracle_and_g31(golden_dir):
    g = _g31(golden_dir)
    sd = _state(31)
    model = _model(sd)
    x = synthetic.train_episode(31, 5, 5, 16, 84)
    masks = synthetic.feat_masks(31, 1, 5, 5, 16)
    model.eval()
    with torch.no_grad():
        sc = model.set_forward(x)
    np.testing.assert_allclose(sc.cpu().numpy(), g["eval_scores"], rtol=1e-3, atol=1e-3)
    model.train()
    before = int(model.feat_draw_index.item())
    with AG.feat_forced_masks(tuple(m.cuda() for m in masks)):
        loss = model.set_forward_loss(x)
        loss.backward()
    assert int(model.feat_draw_index.item()) == before + 1
    main, aux = (float(t) for t in model.last_terms)
    assert abs(float(loss.detach()) - float(g["loss"])) < 2e-4 and abs(main - float(g["loss_main"])) < 2e-4
    assert abs(aux - float(g["loss_aux"])) < 2e-4
    ref_loss, ref_main, ref = _oracle(sd, x[None], masks)
    assert abs(ref_loss - float(g["loss"])) < 1e-9 and abs(ref_main - float(g["loss_main"])) < 1e-9
    named = dict(model.named_parameters())
    assert set(ref) == set(named)
    _check_grads(named, ref)
    # the seven head gradients: within 4x the distance of the float32 CPU step to float64 (G31 (d))
    for k in HEAD:
        full = ref[k]
        key, want, got = "headgrad:" + k, full, named[k].grad.cpu().double()
        if full.dim() == 2:
            key, want, got = "headgrad_rows:" + k, full[::32], got[::32]
        stored = torch.from_numpy(g[key])
        assert float((want - stored).norm()) <= 1e-8 * float(stored.norm()), k
        err = float((got - stored).norm() / stored.norm())
        yard = float(g["f32err:" + key])
        print("feat step: %s rel err %.3e, G31 float32 distance %.3e, ratio %.2f" % (k, err, yard, err / yard))
        assert err <= 4.0 * yard, (k, err, yard)
    for name in g["bnnames"]:
        name = str(name)
        want = g["bngrad:" + name]
        got = named[name].grad.cpu().numpy()
        assert np.linalg.norm(got - want) <= 3e-2 * np.linalg.norm(want) + 1e-9, name
    gn = {k: float(p.grad.norm()) for k, p in named.items()}
    for name, refn in zip(g["gradnames"], g["gradnorms"]):
        assert abs(gn[str(name)] - refn) <= 1e-2 * refn + 1e-9, name
    # unforced: the generator's masks differ from the forced ones, and the main term is what the running sum receives
    base = float(model.loss_fn.loss_sum(loss.device).item())
    other = model.set_forward_loss(x)
    assert float(other.detach()) != float(loss.detach())
    assert abs(float(model.loss_fn.loss_sum(loss.device).item()) - base - float(model.last_terms[0])) < 1e-6


def test_lockstep_two_episodes_equal_float64_mean():
    sd = _state(23)
    xs = torch.stack([synthetic.train_episode(400 + i, 5, 5, 16, 84) for i in range(2)])
    model = _model(sd)
    masks = synthetic.feat_masks(77, 2, 5, 5, 16)
    with AG.feat_forced_masks(tuple(m.cuda() for m in masks)):
        loss = model.set_forward_loss_lockstep(xs.cuda())
        loss.backward()
    ref_loss, _, ref = _oracle(sd, xs, masks)
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
        model = _model(_state(31))
        model.feat_draw_index.fill_(11)                                        # the same starting draw index
        opt = optim.Adam(model.parameters())
        capsys.readouterr()
        model.train_loop(0, Loader(), opt)
        out = capsys.readouterr().out
        st = model.__dict__.get("_mft_graph_steps", {}).get("set_forward_loss")
        return out, {n: p.detach().clone() for n, p in model.named_parameters()}, [b.detach().clone() for b in model.buffers()], st, model

    out_e, par_e, buf_e, st_e, m_e = run(False)
    out_g, par_g, buf_g, st_g, m_g = run(True)
    assert st_e is None and st_g is not None and st_g.graph is not None and not st_g.failed
    assert out_g == out_e and out_e.count("Loss") == 1
    assert list(par_e) == list(par_g) and all(torch.equal(par_e[n], par_g[n]) for n in par_e)
    assert all(torch.equal(a, b) for a, b in zip(buf_e, buf_g))
    assert int(m_e.feat_draw_index.item()) == int(m_g.feat_draw_index.item()) == 11 + 6    # every replay drew fresh masks
    fresh = _state(31)
    for k in HEAD:                                                             # the head was trained
        assert not torch.equal(par_g[k].cpu(), fresh[k]), k


def test_feat_step_issues_no_aten_device_kernels():
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "feat_step_worker.py")
    r = subprocess.run([sys.executable, worker], capture_output=True, text=True, timeout=900)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert lines, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    res = json.loads(lines[-1][len("RESULT "):])
    assert res["n_dev"] > 0 and not res["aten"] and not res["head_aten"] and not res["head_step_aten"], res
    # the launch count is a function of the shape arguments alone
    assert res["fwd_n_dev"] == res["fwd_n_dev_50shot"] and res["bwd_n_dev"] == res["bwd_n_dev_50shot"], res
    assert res["head_n_dev"] == 6 and res["fwd_n_dev"] == 8 and res["bwd_n_dev"] == 11, res


# ------------------------------------------------------------------------------------------------ evaluation and CLI
def test_evaluate_in_lockstep_equals_a_loop_over_set_forward():
    g = torch.Generator().manual_seed(77)
    mean = torch.randn(8, 1, 512, generator=g)
    rows = torch.relu(0.5 * torch.randn(8, 25, 512, generator=g) + 0.5 * mean + 0.3).numpy()
    table = feature_eval.FeatureTable({c: list(rows[c]) for c in range(8)})
    model = feature_eval.build_model("feat", model_dict["ResNet10"], 5, 5)
    model.load_state_dict(_state(31))
    model = model.cuda().eval()

    def seed():
        random.seed(10)
        np.random.seed(10)
        torch.manual_seed(10)

    seed()
    acc, s_lock = feature_eval.evaluate(model, "feat", table, 5, 5, 15, 6, 4, return_scores=True)
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
def test_train_main_feat_writes_a_loadable_checkpoint(golden_dir, tmp_path, monkeypatch, extra):
    from meta_fine_tuning_amd import configs, train
    g = _g31(golden_dir)
    monkeypatch.setattr(configs, "save_dir", str(tmp_path))
    train.main(["--dataset", "miniImageNet", "--method", "feat", "--model", "ResNet10", "--stop_epoch", "1"] + extra,
               n_episode=2, size=84)
    f = tmp_path / "checkpoints" / "miniImageNet" / "ResNet10_feat_5way_5shot" / "0.tar"
    assert f.is_file()
    state = torch.load(str(f), map_location="cpu")["state"]
    assert list(state.keys()) == [str(k) for k in g["state_keys"]]
    fresh = FEAT(model_dict['ResNet10'], n_way=5, n_support=5)
    fresh.load_state_dict(state)
    assert list(fresh.state_dict().keys()) == [str(k) for k in g["state_keys"]]


def test_save_features_and_test_drivers_take_feat(tmp_path, monkeypatch, capsys):
    from meta_fine_tuning_amd import configs, save_features
    from meta_fine_tuning_amd import test as test_driver
    monkeypatch.setattr(configs, "save_dir", str(tmp_path))
    for k, v in (("MFT_POOL_PER_CLASS", "24"), ("MFT_IMAGE_SIZE", "64"), ("MFT_EPISODES", "6"), ("MFT_EPISODES_PER_BATCH", "4")):
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("MFT_STANDIN_WEIGHTS", "1")                               # the stand-in backbone with synthetic.feat_head_state behind it
    argv = ["--dataset", "miniImageNet", "--method", "feat", "--test_dataset", "ISIC"]
    from meta_fine_tuning_amd.io_utils import parse_args
    state, loaded = save_features.resolve_state(parse_args('save_features', argv), verbose=False)
    assert loaded is None and [k for k in state if not k.startswith("feature.")] == HEAD
    assert all(torch.equal(state[k], v) for k, v in synthetic.feat_head_state().items())
    featfile = save_features.main(argv)
    assert featfile.endswith("features/miniImageNet/ResNet10_feat_5way_5shot/novel.npz")
    acc = test_driver.main(argv)
    out = capsys.readouterr().out
    assert len(acc) == 6 and np.all((acc >= 0) & (acc <= 100)) and "6 Test Acc" in out
