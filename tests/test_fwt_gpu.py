"""ResNet10_FW on a real MI355X: the two kernels of csrc/fwt.hip against the numpy generator and float64, the
whole meta-training step against the reference's golden G28 with forced noise, lockstep episodes on both BatchNorm paths, identity
in eval mode, purity of the ResNet10 step, the graphed episode loop, and the train.main driver."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import meta_fine_tuning_amd  # noqa: F401
from meta_fine_tuning_amd import _lib, backbone, ops, synthetic
from meta_fine_tuning_amd import autograd_ops as AG
from meta_fine_tuning_amd import functional_bwd as FB
from meta_fine_tuning_amd.backbone import FWT_COLS, FWT_LAYERS
from meta_fine_tuning_amd.io_utils import model_dict
from meta_fine_tuning_amd.methods.gnnnet import GnnNet
from meta_fine_tuning_amd.methods.protonet import ProtoNet
from oracle import mft_oracle as O
from test_fwt_cpu import fw_forward, fwt_normals, fwt_words, g28, g28_state

pytestmark = pytest.mark.gpu
torch.set_num_threads(8)
DEV = "cuda"


# ------------------------------------------------------------------------------------------------ kernels alone
def _layers(C, rs):
    """Seven layers of C channels each, one after the other in a 7 C wide noise layout; gamma / beta on both sides of the softplus
    threshold (100 x = 20)."""
    out = []
    for l in range(7):
        w = torch.from_numpy(rs.uniform(0.5, 1.5, C).astype(np.float32)).to(DEV)
        b = torch.from_numpy((rs.standard_normal(C) * 0.1).astype(np.float32)).to(DEV)
        gamma = torch.from_numpy(rs.uniform(0.01, 0.5, C).astype(np.float32)).to(DEV)
        beta = torch.from_numpy(rs.uniform(0.01, 0.9, C).astype(np.float32)).to(DEV)
        out.append(("L%d" % l, C, l * C, w, b, gamma, beta))
    return out


def _softplus64(x):
    x = x.astype(np.float64)
    return np.where(100.0 * x > 20.0, x, np.log1p(np.exp(np.minimum(100.0 * x, 20.0))) / 100.0)


def _close(got, want, scale, what):
    """|got - want| <= 1e-6 x the magnitude of the terms that were summed (a few fp32 ulp of each O(1) term)."""
    err = np.abs(got.astype(np.float64) - want)
    assert (err <= 1e-6 * scale).all(), (what, float((err / scale).max()))


@pytest.mark.parametrize("groups", [1, 3])
@pytest.mark.parametrize("C", [64, 512])
def test_kernels_against_numpy_and_float64(C, groups):
    rs = np.random.RandomState(C + groups)
    layers = _layers(C, rs)
    ld = 7 * C
    seed, idx0 = 0x123456789ABCDEF0, (1 << 32) + 5
    index = torch.tensor([idx0], dtype=torch.int64, device=DEV)
    names = [l[0] for l in layers]
    st = FB.FwtState(layers, groups, ld, seed, index, need_gamma_beta=names, want_words=True)
    assert int(index.item()) == idx0 + 1
    # generator: words bit for bit, normals within one fp32 ulp of the float64 Box-Muller
    w0, w1 = fwt_words(seed, idx0, groups, ld)
    words = st.words.cpu().numpy().view(np.uint32)
    assert np.array_equal(words[:, 0], w0) and np.array_equal(words[:, 1], w1)
    noise = st.noise.cpu().numpy()
    ref = fwt_normals(seed, idx0, groups, ld).astype(np.float32)
    assert (np.abs(noise - ref) <= np.spacing(np.abs(ref))).all()
    # fold, against float64 on the device's own normals
    for name, _, col, w, b, gamma, beta in layers:
        ng, nb = noise[:, 0, col:col + C].astype(np.float64), noise[:, 1, col:col + C].astype(np.float64)
        w64, b64 = w.cpu().numpy().astype(np.float64), b.cpu().numpy().astype(np.float64)
        sg, sb = _softplus64(gamma.cpu().numpy()), _softplus64(beta.cpu().numpy())
        gm, bt = 1.0 + ng * sg, nb * sb
        wf, bf = (t.cpu().numpy() for t in st.affine[name])
        assert wf.shape == (groups, C)
        mag = 1.0 + np.abs(ng * sg)
        _close(wf, gm * w64, mag * np.abs(w64), name + " w'")
        _close(bf, gm * b64 + bt, mag * np.abs(b64) + np.abs(bt), name + " b'")
    # unfold, against float64
    want = {}
    for name, _, col, w, b, gamma, beta in layers:
        dwf, dbf = st.grad_slots(name)
        dwf.copy_(torch.from_numpy(rs.standard_normal((groups, C)).astype(np.float32)))
        dbf.copy_(torch.from_numpy(rs.standard_normal((groups, C)).astype(np.float32)))
        ng, nb = noise[:, 0, col:col + C].astype(np.float64), noise[:, 1, col:col + C].astype(np.float64)
        gm = st._gm[name].cpu().numpy().astype(np.float64)
        w64, b64 = w.cpu().numpy().astype(np.float64), b.cpu().numpy().astype(np.float64)
        dw, db = dwf.cpu().numpy().astype(np.float64), dbf.cpu().numpy().astype(np.float64)
        sig_g = 1.0 / (1.0 + np.exp(-100.0 * gamma.cpu().numpy().astype(np.float64)))
        sig_b = 1.0 / (1.0 + np.exp(-100.0 * beta.cpu().numpy().astype(np.float64)))
        want[name] = ((gm * dw).sum(0), np.abs(gm * dw).sum(0), (gm * db).sum(0), np.abs(gm * db).sum(0),
                      sig_g * (ng * (w64 * dw + b64 * db)).sum(0), (np.abs(ng) * (np.abs(w64 * dw) + np.abs(b64 * db))).sum(0),
                      sig_b * (nb * db).sum(0), np.abs(nb * db).sum(0))
    grads = {}
    st.unfold(grads)
    for name in names:
        a = want[name]
        _close(grads[name + ".weight"].cpu().numpy(), a[0], a[1], name + " dw")
        _close(grads[name + ".bias"].cpu().numpy(), a[2], a[3], name + " db")
        _close(grads[name + ".gamma"].cpu().numpy().reshape(-1), a[4], a[5], name + " dgamma")
        _close(grads[name + ".beta"].cpu().numpy().reshape(-1), a[6], a[7], name + " dbeta")
    again = {}
    st.unfold(again)
    assert all(torch.equal(grads[k], again[k]) for k in grads)                  # fixed summation order: reruns are bit-identical
    # two more launches advance the index by two; the same (seed, index) gives the same bits, another seed does not
    st2 = FB.FwtState(layers, groups, ld, seed, index)
    st3 = FB.FwtState(layers, groups, ld, seed, index)
    assert int(index.item()) == idx0 + 3 and not torch.equal(st2.noise, st3.noise) and not torch.equal(st2.noise, st.noise)
    index.fill_(idx0)
    rep = FB.FwtState(layers, groups, ld, seed, index)
    assert torch.equal(rep.noise, st.noise) and torch.equal(rep.fold, st.fold)
    index.fill_(idx0)
    assert not torch.equal(FB.FwtState(layers, groups, ld, seed + 1, index).noise, st.noise)
    # noise_in replaces the generator; the index still advances
    forced = torch.from_numpy(rs.standard_normal((groups, 2, ld)).astype(np.float32)).to(DEV)
    fs = FB.FwtState(layers, groups, ld, seed, index, noise_in=forced)
    assert int(index.item()) == idx0 + 2
    for _, _, col, *_ in layers:
        assert torch.equal(fs.noise[:, :, col:col + C], forced[:, :, col:col + C])
    name, _, col, w, b, gamma, beta = layers[3]
    gm = 1.0 + forced[:, 0, col:col + C].double().cpu().numpy() * _softplus64(gamma.cpu().numpy())
    _close(fs.affine[name][0].cpu().numpy(), gm * w.cpu().numpy().astype(np.float64), (1 + np.abs(gm - 1)) * np.abs(w.cpu().numpy()), "forced w'")


def test_launchers_refuse_shapes_outside_their_domain():
    lib = _lib.lib()
    rs = np.random.RandomState(0)
    lay = _layers(64, rs)
    index = torch.zeros(1, dtype=torch.int64, device=DEV)
    noise = torch.zeros(2, 2, 8 * 520, device=DEV)
    buf = torch.zeros(3, 2 * 520, device=DEV)
    p520 = torch.ones(520, device=DEV)

    def jobs(n, C=64, col_step=64, cls=FB._FwtJob):
        arr = (cls * n)()
        for i, a in enumerate(arr):
            for f, _ in cls._fields_[:-2]:
                setattr(a, f, (p520 if f in ("w", "b", "gamma", "beta") else buf).data_ptr())
            a.C, a.col = C, (i % 8) * col_step
        return arr

    def fold(n, groups=1, C=64, ld=8 * 520):
        return lib.mft_fwt_draw_fold(jobs(n, C, C), n, groups, ld, 0, ops._p(index), None, ops._p(noise), None, ops._stream(noise))

    def unfold(n, groups=1, C=64, ld=8 * 520):
        return lib.mft_fwt_unfold(jobs(n, C, C, FB._FwtGradJob), n, groups, ld, ops._p(noise), ops._stream(noise))

    for fn in (fold, unfold):
        assert fn(1) == 0 and fn(8, 2, 512) == 0
        assert fn(0) == -22 and fn(9) == -22 and fn(1, groups=0) == -22 and fn(1, C=516) == -22 and fn(1, C=0) == -22
        assert fn(2, C=64, ld=100) == -22                       # a layer's columns must lie inside the noise rows
    torch.cuda.synchronize()
    assert int(index.item()) == 2                                # refused launches drew nothing
    with pytest.raises(ValueError):
        FB.FwtState(lay + lay[:2], 1, 7 * 64, 0, index)
    with pytest.raises(ValueError):
        FB.FwtState(lay, 2, 7 * 64, 0, index, noise_in=torch.zeros(1, 2, 7 * 64, device=DEV))


# ------------------------------------------------------------------------------------------------ the whole step against G28
def _gnn_model():
    m = GnnNet(model_dict['ResNet10_FW'], n_way=5, n_support=5)
    m.load_state_dict(g28_state())
    m = m.cuda()
    m.train()
    m.n_query = 16
    return m


_ORACLE = {}


def _g28_oracle(noise):
    """float64 gradients of EVERY parameter (gamma / beta included) of the G28 step, by autograd on the torch restatement: computed
    once, shared, never modified."""
    if "g28" not in _ORACLE:
        sd = O.clone_state(g28_state(), torch.float64)
        pkeys = [k for k, v in sd.items() if v.is_floating_point() and "running" not in k]
        for k in pkeys:
            sd[k].requires_grad_(True)
        x = synthetic.train_episode(28, 5, 5, 16, 84).double()
        feats = fw_forward(sd, x.reshape(-1, 3, 84, 84), noise[0], "feature.")
        sc = O.gnnnet_scores_from_z(sd, O.fc_project(sd, feats).view(5, 21, -1), 5, 5, 16)
        loss = F.cross_entropy(sc, torch.from_numpy(np.repeat(np.arange(5), 16)))
        _ORACLE["g28"] = (float(loss.detach()), dict(zip(pkeys, torch.autograd.grad(loss, [sd[k] for k in pkeys]))))
    return _ORACLE["g28"]


def _check_grads(named, ref):
    # bounds of tests/test_protonet_gpu.py::_check_grads (a ReLU whose pre-activation is ~1e-6 may flip in fp32 and perturb a
    # handful of entries)
    for k, gr in ref.items():
        got = named[k].grad
        assert got is not None, k
        nrm = float(gr.norm())
        if nrm < 1e-9:
            assert float(got.norm()) < 1e-5, k
            continue
        rel = float((got.cpu().double() - gr).norm()) / nrm
        mx = float((got.cpu().double() - gr).abs().max()) / float(gr.abs().max())
        print("grad %-48s rel %.3e max %.3e" % (k, rel, mx))
        assert rel < 3e-2 and mx < 0.15, (k, rel, mx)


def test_step_with_forced_noise_matches_g28(golden_dir):
    g = g28(golden_dir)
    model = _gnn_model()
    x = synthetic.train_episode(28, 5, 5, 16, 84)
    noise = torch.from_numpy(g["noise"])
    fw_names = [str(n) for n in g["fwtnames"]]
    with AG.fwt_forced_noise(model.feature, noise.cuda()):
        with torch.no_grad():
            sc = model.set_forward(x)
        loss = model.set_forward_loss(x)
        loss.backward()
        named = dict(model.named_parameters())
        print("scores max err %.3e  loss err %.3e" % (float(np.abs(sc.cpu().numpy() - g["scores"]).max()), abs(float(loss) - float(g["loss"]))))
        np.testing.assert_allclose(sc.cpu().numpy(), g["scores"], rtol=1e-3, atol=1e-3)
        assert abs(float(loss.detach()) - float(g["loss"])) < 2e-4
        assert all(named[n].grad is None for n in fw_names)                  # frozen by default, as in the reference
        ref_loss, ref = _g28_oracle(noise)
        assert abs(ref_loss - float(g["loss"])) < 1e-9
        _check_grads(named, {k: v for k, v in ref.items() if k not in fw_names})
        for name in g["bnnames"]:
            name = str(name)
            want = g["bngrad:" + name]
            got = named[name].grad.cpu().numpy()
            assert np.linalg.norm(got - want) <= 3e-2 * np.linalg.norm(want) + 1e-9, name
        gn = {k: float(p.grad.norm()) for k, p in named.items() if p.grad is not None}
        for name, refn in zip(g["gradnames"], g["gradnorms"]):
            assert abs(gn[str(name)] - refn) <= 1e-2 * refn + 1e-9, name
        # the learned variant: gamma / beta trainable -- the same bounds, against the reference's second backward and the oracle
        for p in named.values():
            p.grad = None
        for n in fw_names:
            named[n].requires_grad = True
        model.set_forward_loss(x).backward()
        _check_grads(named, {k: ref[k] for k in fw_names})
        for n in fw_names:
            want = g["fwtgrad:" + n]
            got = named[n].grad.cpu().numpy()
            assert got.shape == want.shape
            assert np.linalg.norm(got - want) <= 3e-2 * np.linalg.norm(want) + 1e-9, n
    assert int(model.feature.fwt_draw_index.item()) == 3 and "_fwt_forced" not in model.feature.__dict__


# ------------------------------------------------------------------------------------------------ lockstep
def _proto_oracle(sd32, xs, noise, ns):
    sd = O.clone_state(sd32, torch.float64)
    pkeys = [k for k, v in sd.items() if v.is_floating_point() and "running" not in k and not k.endswith((".gamma", ".beta"))]
    for k in pkeys:
        sd[k].requires_grad_(True)
    n_way, per = xs.shape[1], xs.shape[2]
    losses = []
    for e, x in enumerate(xs):
        z = fw_forward(sd, x.double().reshape(-1, *x.shape[2:]), noise[e], "feature.").view(n_way, per, -1)
        proto, q = z[:, :ns].mean(1), z[:, ns:].reshape(n_way * (per - ns), -1)
        sc = -((q[:, None, :] - proto[None, :, :]) ** 2).sum(2)
        losses.append(F.cross_entropy(sc, torch.from_numpy(np.repeat(np.arange(n_way), per - ns))))
    loss = torch.stack(losses).mean()
    return float(loss.detach()), dict(zip(pkeys, torch.autograd.grad(loss, [sd[k] for k in pkeys])))


@pytest.mark.parametrize("size", [64, 84])       # 64: trunk.6 / trunk.7 have at most 512 rows per group (the one-launch BatchNorm path)
def test_lockstep_two_episodes_equal_float64_mean(size):
    sd = synthetic.resnet10_fw_state_dict(31, prefix="feature.")
    xs = torch.stack([synthetic.train_episode(500 + i, 3, 2, 3, size) for i in range(2)])
    noise = torch.from_numpy(np.random.RandomState(size).standard_normal((2, 2, FWT_COLS)).astype(np.float32))
    model = ProtoNet(model_dict['ResNet10_FW'], n_way=3, n_support=2)
    model.load_state_dict(sd)
    model = model.cuda()
    model.train()
    model.n_query = 3
    h6 = -(-size // 16)                      # trunk.6's map side: 4 at 64 x 64 (240 rows per episode), 6 at 84 x 84 (540 rows)
    assert ops.bn_forward_small_ok(256, 15 * h6 * h6) == (size == 64)
    with AG.fwt_forced_noise(model.feature, noise.cuda()):
        loss = model.set_forward_loss_lockstep(xs.cuda())
        loss.backward()
    ref_loss, ref = _proto_oracle(sd, xs, noise, 2)
    print("lockstep %d: loss %.6f ref %.6f" % (size, float(loss), ref_loss))
    assert abs(float(loss.detach()) - ref_loss) < 2e-4
    _check_grads(dict(model.named_parameters()), ref)
    # without forced noise the two episodes of one call draw different noise
    st = AG.fwt_draw(model.feature, 2)
    assert not torch.equal(st.noise[0], st.noise[1])


# ------------------------------------------------------------------------------------------------ identity and purity
def test_eval_mode_is_resnet10_bit_for_bit(golden_dir):
    g = g28(golden_dir)
    sd = synthetic.resnet10_fw_state_dict(28)
    fw = backbone.ResNet10_FW()
    fw.load_state_dict(sd)
    plain = backbone.ResNet10()
    plain.load_state_dict(backbone.plain_state_dict(sd))
    fw, plain = fw.cuda().eval(), plain.cuda().eval()
    x = synthetic.train_episode(28, 5, 5, 16, 84).reshape(-1, 3, 84, 84)[:10].cuda()
    with torch.no_grad():
        a, b = fw(x), plain(x)
    assert torch.equal(a, b)
    assert int(fw.fwt_draw_index.item()) == 0                                # eval mode draws nothing
    np.testing.assert_allclose(a.cpu().numpy(), g["eval_feats"], rtol=1e-4, atol=1e-4)
    # train mode without autograd: the noise is on (taped launches, tape dropped) and the index advances
    fw.train()
    with torch.no_grad():
        c = fw(x)
    assert int(fw.fwt_draw_index.item()) == 1 and not torch.equal(c, a)
    # the last-block-only backward is not built for this backbone
    for p in AG._base_params(fw)[:-9]:
        p.requires_grad = False
    with pytest.raises(NotImplementedError, match="last-block-only"):
        fw(x)


def _proto_model(name, seed=27):
    sd = (synthetic.resnet10_fw_state_dict if name == 'ResNet10_FW' else synthetic.resnet10_state_dict)(seed, prefix="feature.")
    m = ProtoNet(model_dict[name], n_way=5, n_support=5)
    m.load_state_dict(sd)
    m = m.cuda()
    m.train()
    m.n_query = 16
    return m


def test_resnet10_step_issues_no_fwt_launch(monkeypatch):
    seen = []
    real = FB.resnet10_forward_taped

    def spy(*a, **kw):
        seen.append(kw.get("fwt", a[4] if len(a) > 4 else None))
        return real(*a, **kw)
    monkeypatch.setattr(FB, "resnet10_forward_taped", spy)
    x = synthetic.train_episode(800, 5, 5, 16, 84)
    for name, n_fwt in (("ResNet10", 0), ("ResNet10_FW", 1)):
        model = _proto_model(name)
        with _lib.LaunchTimer() as t:
            model.set_forward_loss(x).backward()
        calls = t.collect()
        t.close()
        assert len(calls.get("mft_fwt_draw_fold", [])) == n_fwt and len(calls.get("mft_fwt_unfold", [])) == n_fwt, name
        assert len(seen) == 1 and (seen.pop() is None) == (n_fwt == 0)
        assert all(p.grad is not None for n, p in model.named_parameters() if not n.endswith((".gamma", ".beta")))


# ------------------------------------------------------------------------------------------------ graph
def test_graphed_episode_loop_is_bit_identical_and_draws_fresh_noise(capsys, monkeypatch):
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
        model = _proto_model('ResNet10_FW')
        opt = optim.Adam(model.parameters())
        capsys.readouterr()
        model.train_loop(0, Loader(), opt)
        out = capsys.readouterr().out
        st = model.__dict__.get("_mft_graph_steps", {}).get("set_forward_loss")
        return out, [p.detach().clone() for p in model.parameters()], [b.detach().clone() for b in model.buffers()], st, model

    out_e, par_e, buf_e, st_e, _ = run(False)
    out_g, par_g, buf_g, st_g, model = run(True)
    assert st_e is None and st_g is not None and st_g.graph is not None and not st_g.failed
    assert out_g == out_e and out_e.count("Loss") == 1
    assert all(torch.equal(a, b) for a, b in zip(par_e, par_g))
    assert all(torch.equal(a, b) for a, b in zip(buf_e, buf_g))              # (the draw index among them: six draws each)
    assert int(model.feature.fwt_draw_index.item()) == 6
    # two consecutive replays on the same episode and the same parameters: the index advances inside the graph
    l1 = float(st_g(eps[0].cuda()).item())
    l2 = float(st_g(eps[0].cuda()).item())
    assert st_g.graph is not None and l1 != l2 and int(model.feature.fwt_draw_index.item()) == 8


# ------------------------------------------------------------------------------------------------ CLI
def test_train_main_protonet_writes_an_86_key_checkpoint(tmp_path, monkeypatch):
    from meta_fine_tuning_amd import configs, train
    monkeypatch.setattr(configs, "save_dir", str(tmp_path))
    train.main(["--dataset", "miniImageNet", "--method", "protonet", "--model", "ResNet10_FW", "--stop_epoch", "1"], n_episode=2, size=84,
               pool_images_per_class=24)
    f = tmp_path / "checkpoints" / "miniImageNet" / "ResNet10_FW_protonet_5way_5shot" / "0.tar"
    assert f.is_file()
    state = torch.load(str(f), map_location="cpu")["state"]
    assert list(state.keys()) == list(synthetic.resnet10_fw_state_dict(0, prefix="feature.").keys()) and len(state) == 86
    assert not any("fwt" in k for k in state)
    fresh = ProtoNet(model_dict['ResNet10'], n_way=5, n_support=5)
    fresh.load_state_dict(backbone.plain_state_dict(state))


@pytest.mark.parametrize("args", [["--method", "gnnnet"], ["--method", "gnnnet", "--episodes_per_rank", "2"], ["--method", "matchingnet"],
                                  ["--method", "metaoptnet"], ["--method", "protonet", "--episodes_per_rank", "2"],
                                  ["--method", "baseline", "--num_classes", "10"], ["--method", "baseline++", "--num_classes", "10"]],
                         ids=lambda a: "_".join(a[1::2]))
def test_train_main_runs_every_method(args, tmp_path, monkeypatch, capsys):
    from meta_fine_tuning_amd import configs, train
    monkeypatch.setattr(configs, "save_dir", str(tmp_path))
    model = train.main(["--dataset", "miniImageNet", "--model", "ResNet10_FW", "--stop_epoch", "1"] + args, n_episode=4, size=84,
                       pool_images_per_class=24)
    out = capsys.readouterr().out
    assert "Loss" in out and "nan" not in out.lower()
    steps = 4 // int(args[3]) if "--episodes_per_rank" in args else 4
    assert int(model.feature.fwt_draw_index.item()) == steps
    assert sum(k.endswith((".gamma", ".beta")) for k in model.state_dict()) == 14
