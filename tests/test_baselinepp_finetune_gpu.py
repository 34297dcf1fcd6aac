"""Baseline++ at test time on a real MI355X: the fused head step (mft_dist_head_step) against the float64 restatement of
tests/test_baselinepp_finetune_cpu.py, FinetuneEngine(mode="dist") against the reference's golden G25, lockstep against single
episodes, the frozen route of evaluate() and the train.main -> finetune.main round trip for --method baseline++."""
import argparse
import os

import numpy as np
import pytest
import torch

import meta_fine_tuning_amd  # noqa: F401
from meta_fine_tuning_amd import _lib, ops, synthetic
from meta_fine_tuning_amd import engine as eng
from meta_fine_tuning_amd import finetune as ft
from test_baselinepp_finetune_cpu import head_step64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HYPER = dict(lr=0.01, b1=0.9, b2=0.999, eps=1e-8, wd=0.001)
MOMENTS = ("mV", "vV", "mg", "vg")


def _rel(got, want):
    return float((got.cpu().double() - want).norm() / want.norm())


# ------------------------------------------------------------------------------------------------ the kernel
#         k, n_way, D, groups, ldf, (group, row) of an all-zero feature row
SHAPES = [(5, 5, 512, 3, 512, (1, 2)), (1, 2, 512, 1, 520, None), (16, 16, 512, 2, 512, None), (4, 5, 64, 2, 64, None)]


def head_inputs(k, n_way, D, groups, zero, step):
    """Per group, from RandomState(100 k + n_way + group): feat = |N(0,1)|, V = U(-1,1) / sqrt(D), g = ||v_c||, random labels,
    and for step > 1 random first moments with positive second moments of the size the gradients have (0.05 and 0.05^2)."""
    t = {n: [] for n in ("feat", "V", "g", "y") + MOMENTS}
    for grp in range(groups):
        rs = np.random.RandomState(100 * k + n_way + grp)
        feat = np.abs(rs.standard_normal((k, D)))
        if zero is not None and zero[0] == grp:
            feat[zero[1]] = 0.0
        V = rs.uniform(-1, 1, (n_way, D)) / np.sqrt(D)
        V = V.astype(np.float32).astype(np.float64)
        t["feat"].append(feat.astype(np.float32).astype(np.float64))
        t["V"].append(V)
        t["g"].append(np.linalg.norm(V, axis=1).astype(np.float32).astype(np.float64))
        t["y"].append(rs.randint(0, n_way, k))
        for n, shape in (("mV", (n_way, D)), ("vV", (n_way, D)), ("mg", (n_way,)), ("vg", (n_way,))):
            if step == 1:
                a = np.zeros(shape)
            elif n[0] == "m":
                a = 0.05 * rs.standard_normal(shape)
            else:
                a = 0.05 ** 2 * rs.uniform(0.5, 1.0, shape)
            t[n].append(a.astype(np.float32).astype(np.float64))
    return {n: torch.from_numpy(np.stack(v)) for n, v in t.items()}


def launch(inp, k, n_way, D, groups, ldf, step):
    """One mft_dist_head_step launch on device copies of ``inp``; feat and dfeat are [groups * k, ldf] buffers whose padding columns
    hold NaN.  -> dict of everything the launch writes (device tensors)."""
    fbuf = torch.full((groups * k, ldf), float("nan"), device=DEV)
    fbuf[:, :D] = inp["feat"].reshape(groups * k, D).float().to(DEV)
    dbuf = torch.full((groups * k, ldf), float("nan"), device=DEV)
    d = {n: inp[n].float().to(DEV).contiguous() for n in ("V", "g") + MOMENTS}
    y = inp["y"].reshape(-1).to(torch.int32).to(DEV)
    loss = torch.full((groups,), float("nan"), device=DEV)
    dfeat, loss = ops.dist_head_step(fbuf[:, :D], y, d["V"], d["g"], d["mV"], d["vV"], d["mg"], d["vg"], 2.0, step,
                                     dfeat=dbuf[:, :D], loss=loss, lr=HYPER["lr"], weight_decay=HYPER["wd"])
    torch.cuda.synchronize()
    d.update(dfeat=dfeat, loss=loss, dbuf=dbuf)
    return d


@pytest.mark.parametrize("step", [7, 1])
@pytest.mark.parametrize("k,n_way,D,groups,ldf,zero", SHAPES)
def test_head_step_matches_float64(k, n_way, D, groups, ldf, zero, step):
    inp = head_inputs(k, n_way, D, groups, zero, step)
    got = launch(inp, k, n_way, D, groups, ldf, step)
    n_el = n_skip = 0
    for grp in range(groups):
        V, g = inp["V"][grp].clone(), inp["g"][grp].clone()
        mom = {n: inp[n][grp].clone() for n in MOMENTS}
        loss, dx, dV, dg = head_step64(inp["feat"][grp], inp["y"][grp], V, g, mom, step, 2.0, **HYPER)
        e_loss = abs(float(got["loss"][grp]) - float(loss)) / abs(float(loss))
        rows = [r for r in range(k) if zero is None or (grp, r) != zero]
        dgot = got["dfeat"][grp * k:(grp + 1) * k]
        e_dx = _rel(dgot[rows], dx[rows])
        e_m = max(_rel(got[n][grp], mom[n]) for n in MOMENTS)
        print("k %d n_way %d D %d group %d step %d: rel loss %.2e dfeat %.2e moments %.2e" % (k, n_way, D, grp, step, e_loss, e_dx, e_m))
        assert e_loss < 1e-5 and e_dx < 1e-5 and e_m < 1e-5, (e_loss, e_dx, e_m)
        if zero is not None and zero[0] == grp:                          # dxh / eps_n: finite, and compared apart (it dominates the norm)
            assert _rel(dgot[zero[1]], dx[zero[1]]) < 1e-5
        # the updated head: one fp32 rounding of the weight plus 1e-5 of the update
        for name, w_new, w_old, grad in (("V", V, inp["V"][grp], dV), ("g", g, inp["g"][grp], dg)):
            err = (got[name][grp].cpu().double() - w_new).abs()
            bound = 2.0 ** -24 * w_new.abs() + 1e-5 * (w_new - w_old).abs()
            keep = torch.ones_like(err, dtype=torch.bool)
            if step == 1:                                                # the first Adam step is sign-like where the gradient is ~ eps
                keep = (grad + HYPER["wd"] * w_old).abs() >= 1e-6
            n_el += keep.numel()
            n_skip += int((~keep).sum())
            worst = float((err - bound)[keep].max())
            assert worst <= 0.0, (name, grp, worst, float(err[keep].max()))
    assert n_skip <= 1e-3 * n_el, (n_skip, n_el)
    for t in (got["dfeat"], got["loss"], got["V"], got["g"]) + tuple(got[n] for n in MOMENTS):
        assert bool(torch.isfinite(t).all())
    if ldf > D:
        assert bool(torch.isnan(got["dbuf"][:, D:]).all())                # the padding columns of dfeat are nobody's to write
    # a second launch on the same inputs: bit-identical
    again = launch(inp, k, n_way, D, groups, ldf, step)
    for n in ("dfeat", "loss", "V", "g") + MOMENTS:
        assert torch.equal(got[n], again[n]), n


def test_head_step_refuses_shapes_outside_its_domain():
    lib = _lib.lib()
    feat = torch.ones(2 * 17, 520, device=DEV)
    dfeat = torch.zeros(2 * 17, 520, device=DEV)
    y = torch.zeros(2 * 17, dtype=torch.int32, device=DEV)
    V, mV, vV = (torch.ones(2, 17, 520, device=DEV) for _ in range(3))
    g, mg, vg = (torch.ones(2, 17, device=DEV) for _ in range(3))
    loss = torch.zeros(2, device=DEV)

    def run(k=5, n_way=5, D=512, groups=2, ldf=512, lddf=512, step=1, off=0):
        return lib.mft_dist_head_step(feat.data_ptr() + off, ldf, ops._p(y), k, groups, n_way, D, 2.0, ops._p(V), ops._p(g), ops._p(mV),
                                      ops._p(vV), ops._p(mg), ops._p(vg), ops._p(dfeat), lddf, ops._p(loss), step, 0.01, 0.9, 0.999,
                                      1e-8, 0.001, ops._stream(feat))

    assert run() == 0
    for kw in [dict(k=17), dict(n_way=17), dict(D=514, ldf=520, lddf=520), dict(ldf=510), dict(k=0), dict(n_way=0), dict(D=516, ldf=520, lddf=520),
               dict(lddf=508), dict(ldf=514), dict(groups=0), dict(step=0), dict(off=4)]:
        assert run(**kw) == -22, kw
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        ops.dist_head_step(feat[:10, :512], y[:10], V[:, :5, :512].contiguous(), g[:, :4].contiguous(), mV[:, :5, :512].contiguous(),
                           vV[:, :5, :512].contiguous(), mg[:, :5].contiguous(), vg[:, :5].contiguous(), 2.0, 1)


# ------------------------------------------------------------------------------------------------ the engine
@pytest.fixture(scope="module")
def g25(golden_dir):
    return np.load(os.path.join(golden_dir, "g25_baselinepp_finetune.npz"))


@pytest.mark.parametrize("ep", [91, 92])
def test_finetune_dist_vs_reference_golden(g25, ep):
    """finetune_dist (cosine head + last block, 100 Adam steps) against the reference's finetune_linear with a distLinear head
    (G25): the argmax of its float64 scores on every query (its own three runs agree on every one, margin >= 0.67), and within 4 x
    its own fp32-vs-fp64 distance of those scores -- the project's convention for a second fp32 implementation."""
    sd = synthetic.gnnnet_state_dict(seed=37)
    liz = synthetic.test_episode(ep, 5, 5, 15, 84, gen_examples=1)
    np.random.seed(10)
    sc = ft.finetune_dist([v.to(DEV) for v in liz], None, sd, None, linear=True, head=(g25["v0_%d" % ep], g25["g0_%d" % ep]))
    assert (np.random.permutation(7) == g25["next_perm_%d" % ep]).all()
    sc = sc.cpu().numpy()
    f64 = g25["scores_f64_%d" % ep]
    d_ref = float(np.abs(g25["scores_f32_%d" % ep] - f64).max())
    d = float(np.abs(sc - f64).max())
    print("episode %d: max|scores - scores_f64| = %.3e (the reference's fp32 vs fp64: %.3e)" % (ep, d, d_ref))
    assert sc.shape == (75, 5)
    assert (sc.argmax(1) == f64.argmax(1)).all()
    assert d <= 4.0 * d_ref, (d, d_ref)
    ft._DIST_ENGINES.clear()


def test_dist_engine_batched_equals_single():
    """Two episodes in lockstep (dist mode) give each episode the scores it gets alone."""
    sd = synthetic.gnnnet_state_dict(seed=39)
    eps = [synthetic.test_episode(700 + i, 5, 5, 15, 84, gen_examples=0) for i in range(2)]
    rs = np.random.RandomState(9)
    perms = [[rs.permutation(25) for _ in range(20)] for _ in range(2)]
    torch.manual_seed(21)
    v0, g0 = ft.dist_head_init(5, n=2)
    e2 = eng.FinetuneEngine(sd, n_views=2, fine_tune_epoch=20, episodes_per_batch=2, device=DEV, mode="dist")
    both = e2.run_batch(eps, perms=perms, classifier_init=(v0, g0)).clone()
    assert both.shape == (2, 75, 5)
    torch.testing.assert_close(both.sum(2).cpu(), torch.ones(2, 75), atol=1e-5, rtol=0)
    e1 = eng.FinetuneEngine(sd, n_views=2, fine_tune_epoch=20, episodes_per_batch=1, device=DEV, mode="dist")
    for i in range(2):
        one = e1.run_batch([eps[i]], perms=[perms[i]], classifier_init=(v0[i:i + 1], g0[i:i + 1]))[0]
        # the BatchNorm reduction is chunked by launch size, so E=1 and E=2 round differently; 100 Adam steps amplify that
        assert float((one - both[i]).abs().max()) < 2e-2
        assert float((one.argmax(1) == both[i].argmax(1)).float().mean()) >= 0.96
    with pytest.raises(RuntimeError):
        e1.run_batch([eps[0]], perms=[perms[0]])                          # the mode needs its heads
    e1.close(); e2.close()


# ------------------------------------------------------------------------------------------------ evaluate and the command line
def test_evaluate_frozen_route_is_baselinepp_batched():
    """evaluate(method="baseline++", freeze_backbone=True) = Baseline++'s own protocol: one baselinepp_batched call per batch."""
    sd = synthetic.resnet10_state_dict(seed=13, prefix="feature.")
    ft.params = argparse.Namespace(model="ResNet10", fine_tune_epoch=1)
    np.random.seed(6)
    torch.manual_seed(12)
    accs = ft.evaluate(None, None, 3, 5, 5, 15, 84, 0, 1, seed0=60, episodes_per_batch=2, verbose=False, method="baseline++", state_b=sd,
                       freeze_backbone=True)
    eps = [synthetic.test_episode(60 + i, 5, 5, 15, 84, gen_examples=0) for i in range(3)]
    np.random.seed(6)
    torch.manual_seed(12)
    want = torch.cat([ft.baselinepp_batched(eps[:2], sd, 5, 5, episodes_per_batch=2), ft.baselinepp_batched(eps[2:], sd, 5, 5, episodes_per_batch=2)])
    y = np.repeat(range(5), 15)
    pred = want.view(3, 75, 5).argmax(2).cpu().numpy()
    assert np.array_equal(accs, np.asarray([float(np.mean(p == y)) * 100 for p in pred]))
    # and the scores themselves, through the per-episode entry point with a pinned head: torch.equal
    rs = np.random.RandomState(2)
    perms = [[rs.permutation(25) for _ in range(100)]]
    heads = ft.dist_head_init(5, n=1)
    a = ft.baselinepp_batched(eps[:1], sd, 5, 5, episodes_per_batch=1, perms=perms, heads=heads)
    np.random.seed(2)
    b = ft.finetune_dist([v.to(DEV) for v in eps[0]], None, sd, None, freeze_backbone=True, head=(heads[0][0], heads[1][0]))
    assert torch.equal(a, b)


def test_train_main_then_finetune_main_baselinepp_round_trip(tmp_path, monkeypatch, capsys):
    """What train.main --method baseline++ writes is what finetune.main --method baseline++ evaluates."""
    from meta_fine_tuning_amd import configs, train
    monkeypatch.setattr(configs, "save_dir", str(tmp_path))
    torch.manual_seed(0)
    train.main(["--dataset", "miniImageNet", "--method", "baseline++", "--model", "ResNet10", "--num_classes", "10", "--stop_epoch", "1"],
               n_episode=2, size=84)
    f = tmp_path / "checkpoints" / "miniImageNet" / "ResNet10_baseline++" / "0.tar"
    assert f.is_file()
    capsys.readouterr()
    monkeypatch.setenv("MFT_EPISODES", "2")
    monkeypatch.setenv("MFT_EPISODES_PER_BATCH", "2")
    monkeypatch.delenv("MFT_STANDIN_WEIGHTS", raising=False)
    argv = ["--method", "baseline++", "--save_iter", "0", "--fine_tune_epoch", "1", "--gen_examples", "1", "--model", "ResNet10"]
    torch.manual_seed(31)
    accs = ft.main(argv)
    cap = capsys.readouterr()
    assert ft.main.loaded["baseline++"] == str(f) and ("loading baseline++ checkpoint %s" % f) in cap.err
    assert cap.out.splitlines()[0] == "False" and "2 Test Acc = " in cap.out
    assert "SYNTHETIC" not in cap.out                                     # an untagged accuracy line: real weights were read
    assert len(accs) == 2 and np.all((accs >= 0) & (accs <= 100))
    state = ft.load_checkpoint_state(str(f))
    assert "classifier.L.weight_v" in state
    np.random.seed(10)
    torch.manual_seed(31)
    ref = ft.evaluate(None, None, 2, 5, 5, 15, 84, 1, 1, episodes_per_batch=2, verbose=False, method="baseline++", state_b=state,
                      device_episodes=True, balance=True)
    assert np.array_equal(accs, ref)
    # --save_iter -1: the newest epoch of that directory
    torch.manual_seed(31)
    accs_newest = ft.main(["--method", "baseline++", "--fine_tune_epoch", "1", "--gen_examples", "1", "--model", "ResNet10"])
    assert ft.main.loaded["baseline++"] == str(f) and np.array_equal(accs_newest, accs)
    # a mis-pointed save_dir is an error, never a plausible number
    monkeypatch.setattr(configs, "save_dir", str(tmp_path / "empty"))
    with pytest.raises(FileNotFoundError):
        ft.main(argv)
    # the stand-in backbone is an explicit opt-in and tags its line
    monkeypatch.setenv("MFT_STANDIN_WEIGHTS", "1")
    capsys.readouterr()
    ft.main(argv)
    out = capsys.readouterr().out
    assert ft.main.loaded["baseline++"] is None
    assert "SYNTHETIC stand-in weights" in [ln for ln in out.splitlines() if "Test Acc" in ln][0]
    with pytest.raises(NotImplementedError):
        ft.main(["--method", "protonet"])
    ft._DIST_ENGINES.clear()


def test_lookahead_loader_parks_dist_scores():
    """The reference-shaped loop with LookaheadLoader: finetune_dist() per episode returns the lockstep batch's scores."""
    sd = synthetic.gnnnet_state_dict(seed=41)
    ft.params = argparse.Namespace(model="ResNet10", fine_tune_epoch=1)
    loader = ft.SyntheticNovelLoader(range(2), 5, 5, 15, 84, 0, seed0=720)
    torch.manual_seed(5)
    heads = ft.dist_head_init(5, n=2)
    np.random.seed(3)
    got = []
    for elem in ft.LookaheadLoader(loader, "baseline++", None, state_b=sd, fine_tune_epoch=1, episodes_per_batch=2, classifiers=heads):
        liz_x = [x for (x, _y) in elem]
        got.append(ft.finetune_dist(liz_x, None, state_in=sd, linear=True, save_it=-1))
    assert not ft._READY
    np.random.seed(3)
    eps = [[v.to(DEV) for v in synthetic.test_episode(720 + i, 5, 5, 15, 84, 0)] for i in range(2)]
    want = ft.scores_batched("baseline++", eps, None, None, sd, 1, episodes_per_batch=2, classifiers=heads)
    assert torch.equal(torch.stack(got), want)
    ft._DIST_ENGINES.clear()
