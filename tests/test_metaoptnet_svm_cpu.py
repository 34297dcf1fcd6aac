"""MetaOptNet-SVM on the CPU: a float64 oracle of the Crammer-Singer dual and of its adjoint that shares
nothing with the package (numpy; a torch.autograd.Function around it for whole-model steps), its KKT residuals at the ten head
shapes, a second route to the same optimum, central differences of its gradient, the golden G29, and the Python surface of the
head: MetaOptNet(head="svm"), --head, directory names."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

C_REG = 0.1

# (E, n_way, n_support, n_query): the shapes of tests/test_metaoptnet_gpu.py
SHAPES = [(1, 5, 5, 16), (1, 2, 1, 1), (2, 1, 1, 2), (3, 3, 2, 3), (2, 5, 1, 15), (1, 5, 13, 2), (1, 5, 20, 3), (1, 5, 50, 2),
          (1, 32, 8, 1), (1, 32, 1, 1)]
KINDS = ["randn", "relu"]


# ------------------------------------------------------------------------------------------------ the oracle
def one_hot(n_way, n_support):
    S = n_way * n_support
    Y = np.zeros((S, n_way))
    Y[np.arange(S), np.arange(S) // n_support] = 1.0
    return Y


def project_rows(V, total):
    """Every row of V onto {b >= 0, sum b = total} by sorting."""
    n = V.shape[1]
    u = -np.sort(-V, axis=1)
    css = np.cumsum(u, axis=1) - total
    rho = (u - css / np.arange(1, n + 1) > 0).sum(1)
    tau = css[np.arange(V.shape[0]), rho - 1] / rho
    return np.maximum(V - tau[:, None], 0.0)


def face_project(X, free):
    """Onto the face's subspace: zero off the free set, every row sums to zero."""
    X = np.where(free, X, 0.0)
    return np.where(free, X - X.sum(1, keepdims=True) / np.maximum(free.sum(1, keepdims=True), 1), 0.0)


def face_solve(M, B, free, rtol=1e-14, max_it=100000):
    """x in the face's subspace with P M P x = P B, by conjugate gradients; the stop is relative to |B_F|."""
    r = face_project(B, free)
    x = np.zeros_like(r)
    rr = float((r * r).sum())
    bb = float((np.where(free, B, 0.0) ** 2).sum())
    p = r.copy()
    for _ in range(max_it):
        if not rr > rtol * rtol * bb:
            break
        q = face_project(M @ p, free)
        pq = float((p * q).sum())
        if not pq > 0.0:
            break
        a = rr / pq
        x += a * p
        r -= a * q
        rn = float((r * r).sum())
        p = face_project(r + (rn / rr) * p, free)
        rr = rn
    return x


def svm_dual(K, n_way, n_support, rounds=100000):
    """argmin 1/2 tr(a^T (K + I) a) - tr(Y^T a)  s.t.  a <= C Y, a 1 = 0  ->  (alpha, free).  Rounds of 50 accelerated
    projected-gradient steps and one conjugate-gradient solve on the face of the free set; ends when a full face step leaves
    every multiplier of a bound entry non-negative."""
    S = n_way * n_support
    Y, M = one_hot(n_way, n_support), K + np.eye(S)
    CY = C_REG * Y
    lip = float(np.linalg.eigvalsh(M)[-1]) * (1.0 + 1e-9)
    a = np.zeros((S, n_way))
    for _ in range(rounds):
        a_prev, t = a.copy(), 1.0
        for _ in range(50):
            tn = 0.5 * (1.0 + np.sqrt(1.0 + 4.0 * t * t))
            y = a + ((t - 1.0) / tn) * (a - a_prev)
            an = CY - project_rows(CY - (y - (M @ y - Y) / lip), C_REG)
            if float(((y - an) * (an - a)).sum()) > 0.0:
                tn = 1.0
            a_prev, a, t = a, an, tn
        free = a < CY
        d = face_solve(M, Y - M @ a, free)
        pos = free & (d > 0)
        ratio = np.where(pos, (CY - a) / np.where(pos, d, 1.0), np.inf)
        step = min(1.0, float(ratio.min()))
        a = np.minimum(a + step * d, CY)
        if step < 1.0:
            a[pos & (ratio <= step)] = CY[pos & (ratio <= step)]
            continue
        k = kkt(M, a, n_way, n_support)
        if k["min_multiplier"] >= 0.0:
            return a, a < CY
    raise RuntimeError("svm_dual: no optimum after %d rounds" % rounds)


def kkt(M, a, n_way, n_support, free=None):
    """The KKT quantities of ``a`` in float64: feasibility, the residual of stationarity on the free set (with the row multiplier
    w_i = -mean over the free set of the gradient), the smallest multiplier on the bound set, the smallest slack on the free set,
    and |M| |a| for relative bounds."""
    Y = one_hot(n_way, n_support)
    CY = C_REG * Y
    if free is None:
        free = a < CY
    g = M @ a - Y
    w = -np.where(free, g, 0.0).sum(1, keepdims=True) / np.maximum(free.sum(1, keepdims=True), 1)
    res = g + w
    return dict(over=float(np.maximum(a - CY, 0.0).max()), rowsum=float(np.abs(a.sum(1)).max()), res=res, free=free,
                stationarity=float(np.abs(res[free]).max()) if free.any() else 0.0,
                min_multiplier=float((-res[~free]).min()) if (~free).any() else np.inf,
                min_slack=float((CY - a)[free].min()) if free.any() else np.inf,
                gmax=float(np.abs(g).max()), scale=np.abs(M) @ np.abs(a))


def split(feats, n_way, n_support):
    """feats [n_way, n_support + n_query, D] -> (Z_S [S, D], Z_Q [Q, D]) class-major."""
    D = feats.shape[-1]
    return feats[:, :n_support].reshape(-1, D), feats[:, n_support:].reshape(-1, D)


def head_step(feats, G, scale, n_way, n_support):
    """One episode in float64: feats [n_way, n_support + n_query, D], G = d(loss)/d(scores) [Q, n_way] (None: forward only) ->
    dict(scores, alpha, free, dfeats, dscale)."""
    feats = np.asarray(feats, dtype=np.float64)
    zs, zq = split(feats, n_way, n_support)
    M = zs @ zs.T + np.eye(len(zs))
    alpha, free = svm_dual(zs @ zs.T, n_way, n_support)
    W = zs.T @ alpha
    out = dict(scores=scale * (zq @ W), alpha=alpha, free=free, M=M)
    if G is None:
        return out
    G = np.asarray(G, dtype=np.float64)
    dW = scale * (zq.T @ G)
    U = face_solve(M, zs @ dW, free)
    dzs = alpha @ dW.T - U @ W.T - alpha @ (zs.T @ U).T
    dzq = scale * (G @ W.T)
    nq = feats.shape[1] - n_support
    df = np.concatenate([dzs.reshape(n_way, n_support, -1), dzq.reshape(n_way, nq, -1)], axis=1)
    out.update(dfeats=df, dscale=float((G * (zq @ W)).sum()), U=U)
    return out


def episodes_step(f, G, scale, shape):
    """f [E * n_way * (ns + nq), D], G [E * n_way * nq, n_way] -> scores, dfeats, dscale and the per-episode results."""
    E, n_way, ns, nq = shape
    f = np.asarray(f, dtype=np.float64).reshape(E, n_way, ns + nq, -1)
    G = np.asarray(G, dtype=np.float64).reshape(E, n_way * nq, n_way)
    eps = [head_step(f[e], G[e], scale, n_way, ns) for e in range(E)]
    return (np.concatenate([r["scores"] for r in eps]), np.concatenate([r["dfeats"].reshape(-1, f.shape[-1]) for r in eps]),
            sum(r["dscale"] for r in eps), eps)


class SvmHead64(torch.autograd.Function):
    """The oracle as a differentiable torch op on float64 feature rows [n_way * (ns + nq), D] of ONE episode."""

    @staticmethod
    def forward(ctx, feats, scale, n_way, n_support):
        f = feats.detach().numpy().reshape(n_way, -1, feats.shape[-1])
        ctx.f, ctx.scale, ctx.shape = f, float(scale.detach()), (n_way, n_support)
        return torch.from_numpy(head_step(f, None, ctx.scale, n_way, n_support)["scores"])

    @staticmethod
    def backward(ctx, G):
        r = head_step(ctx.f, G.numpy(), ctx.scale, *ctx.shape)
        return torch.from_numpy(r["dfeats"].reshape(-1, ctx.f.shape[-1])), torch.tensor([r["dscale"]], dtype=torch.float64), None, None


def features(kind, shape, draw):
    """The inputs of tests/test_metaoptnet_gpu.py::_features: float32 rows and a random d(scores)."""
    E, n_way, ns, nq = shape
    g = torch.Generator().manual_seed(1000003 * draw + 7919 * E + 131 * n_way + 17 * ns + nq + (0 if kind == "randn" else 500000))
    f = torch.randn(E, n_way, ns + nq, 512, generator=g)
    if kind == "relu":          # non-negative and class-structured, as trunk outputs are
        mean = torch.randn(E, n_way, 1, 512, generator=g)
        f = torch.relu(0.5 * f + 0.5 * mean + 0.3)
    G = torch.randn(E * n_way * nq, n_way, generator=g)
    return f.reshape(-1, 512).contiguous(), G


@functools.lru_cache(maxsize=None)
def solved(shape, kind, draw):
    """The oracle's forward at one input (episode 0), shared by the tests below and never modified."""
    E, n_way, ns, nq = shape
    f, _ = features(kind, shape, draw)
    f = f.double().numpy().reshape(E, n_way, ns + nq, -1)
    return f[0], head_step(f[0], None, 0.8125, n_way, ns)


# ------------------------------------------------------------------------------------------------ the oracle, tested
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "E%d_w%d_s%d_q%d" % s)
def test_oracle_satisfies_kkt(shape, kind):
    _, n_way, ns, _ = shape
    _, r = solved(shape, kind, 0)
    k = kkt(r["M"], r["alpha"], n_way, ns)
    print("svm oracle %s %s: over %.1e rowsum %.1e stationarity %.1e min multiplier %.2e min slack %.2e"
          % (shape, kind, k["over"], k["rowsum"], k["stationarity"], k["min_multiplier"], k["min_slack"]))
    assert k["over"] == 0.0 and k["rowsum"] <= 1e-10 and k["stationarity"] <= 1e-10
    assert k["min_multiplier"] >= -1e-10
    assert (r["free"].sum(1) >= 1).all()
    if n_way == 1:
        assert not r["alpha"].any() and r["free"].all()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", [(1, 2, 1, 1), (3, 3, 2, 3), (2, 5, 1, 15)], ids=lambda s: "E%d_w%d_s%d_q%d" % s)
def test_oracle_equals_plain_projected_gradient_from_another_start(shape, kind):
    _, n_way, ns, _ = shape
    _, r = solved(shape, kind, 0)
    M, Y = r["M"], one_hot(n_way, ns)
    CY = C_REG * Y
    step = 1.0 / float(np.linalg.eigvalsh(M)[-1])
    a = CY - C_REG / n_way                      # the centre of every row's simplex
    for _ in range(200000):
        an = CY - project_rows(CY - (a - step * (M @ a - Y)), C_REG)
        moved = np.abs(an - a).max()
        a = an
        if moved <= 1e-17:                      # below the spacing of doubles at the size of alpha: it no longer moves
            break
    assert np.abs(a - r["alpha"]).max() <= 1e-9


@pytest.mark.parametrize("shape,kind", [((3, 3, 2, 3), "randn"), ((1, 5, 5, 16), "relu")], ids=["w3_s2", "w5_s5"])
def test_oracle_gradient_matches_central_differences(shape, kind):
    E, n_way, ns, nq = shape
    f, G = features(kind, shape, 0)
    f = f.double().numpy().reshape(E, n_way, ns + nq, -1)[0]
    G = G.double().numpy()[:n_way * nq]
    r = head_step(f, G, 0.8125, n_way, ns)
    rs = np.random.RandomState(7)
    h = 1e-5
    for _ in range(6):
        c, i, j = rs.randint(n_way), rs.randint(ns), rs.randint(512)
        fp, fm = f.copy(), f.copy()
        fp[c, i, j] += h
        fm[c, i, j] -= h
        fd = ((G * head_step(fp, None, 0.8125, n_way, ns)["scores"]).sum()
              - (G * head_step(fm, None, 0.8125, n_way, ns)["scores"]).sum()) / (2 * h)
        assert abs(fd - r["dfeats"][c, i, j]) <= 1e-5 * max(abs(fd), np.abs(r["dfeats"]).max()), (c, i, j, fd, r["dfeats"][c, i, j])
    fd = ((G * head_step(f, None, 0.8125 + h, n_way, ns)["scores"]).sum()
          - (G * head_step(f, None, 0.8125 - h, n_way, ns)["scores"]).sum()) / (2 * h)
    assert abs(fd - r["dscale"]) <= 1e-5 * abs(fd)


# ------------------------------------------------------------------------------------------------ the golden G29
def g29(golden_dir):
    return np.load(os.path.join(golden_dir, "g29_metaoptnet_svm.npz"))


def test_oracle_reproduces_g29(golden_dir):
    from meta_fine_tuning_amd import synthetic
    from oracle import mft_oracle as O
    g = g29(golden_dir)
    torch.set_num_threads(8)
    sd = O.clone_state(synthetic.resnet10_state_dict(seed=27, prefix="feature."), torch.float64)
    scale = float(synthetic.metaoptnet_head_state(27)["scale"])
    x = synthetic.train_episode(27, 5, 5, 16, 84).double()
    with torch.no_grad():
        feats = O.resnet10_forward(sd, x.reshape(-1, *x.shape[2:]), prefix="feature.").view(5, 21, -1).numpy()
    r = head_step(feats, None, scale, 5, 5)
    assert r["scores"].shape == g["scores"].shape == (80, 5)
    assert np.linalg.norm(r["scores"] - g["scores"]) <= 1e-9 * np.linalg.norm(g["scores"])
    assert np.abs(r["alpha"] - g["alpha"]).max() <= 1e-9
    assert (r["free"] == g["free"]).all() and 0 < int(g["free"].sum()) < g["free"].size        # some entries sit on their bound
    loss = float(F.cross_entropy(torch.from_numpy(r["scores"]), torch.from_numpy(np.repeat(np.arange(5), 16))))
    assert abs(loss - float(g["loss"])) < 1e-9


# ------------------------------------------------------------------------------------------------ the Python surface
def test_model_with_svm_head_keeps_keys_and_names_its_engine_mode(golden_dir):
    from meta_fine_tuning_amd.io_utils import model_dict
    from meta_fine_tuning_amd.methods.metaoptnet import MetaOptNet
    keys = [str(k) for k in g29(golden_dir)["state_keys"]]
    svm = MetaOptNet(model_dict['ResNet10'], n_way=5, n_support=5, head="svm")
    ridge = MetaOptNet(model_dict['ResNet10'], n_way=5, n_support=5)
    assert list(svm.state_dict().keys()) == keys == list(ridge.state_dict().keys())
    assert svm.ENGINE_MODE == "svm" and "ENGINE_MODE" in vars(svm) and svm.head == "svm"
    assert ridge.ENGINE_MODE == "ridge" and "ENGINE_MODE" not in vars(ridge) and ridge.head == "ridge"
    assert (MetaOptNet.METHOD, MetaOptNet.ENGINE_MODE) == ("metaoptnet", "ridge")
    assert svm.head_state()["head"] == "svm" and ridge.head_state()["head"] == "ridge"
    assert svm.head_state()["scale"].shape == (1,) and svm.head_params()[0] is svm.scale
    with pytest.raises(ValueError):
        MetaOptNet(model_dict['ResNet10'], n_way=5, n_support=5, head="qp")
    with pytest.raises(ValueError):
        MetaOptNet(model_dict['ResNet10'], n_way=33, n_support=1, head="svm")


@pytest.mark.parametrize("script", ["train", "save_features", "test"])
def test_head_flag_parses_and_names_the_directories(script, monkeypatch, tmp_path):
    from meta_fine_tuning_amd import configs, save_features
    from meta_fine_tuning_amd.io_utils import method_dir_name, parse_args
    monkeypatch.setattr(configs, "save_dir", str(tmp_path))
    base = ["--dataset", "miniImageNet", "--method", "metaoptnet", "--train_aug"]
    p0, p1 = parse_args(script, base), parse_args(script, base + ["--head", "svm"])
    assert p0.head == "ridge" and p1.head == "svm"
    assert save_features.checkpoint_dir(p0) == "%s/checkpoints/miniImageNet/ResNet10_metaoptnet_aug_5way_5shot" % tmp_path
    assert save_features.checkpoint_dir(p1) == "%s/checkpoints/miniImageNet/ResNet10_metaoptnet_svm_aug_5way_5shot" % tmp_path
    if script != "train":
        assert save_features.features_file(p1) == "%s/features/miniImageNet/ResNet10_metaoptnet_svm_aug_5way_5shot/novel.npz" % tmp_path
        assert save_features.features_file(p0) == "%s/features/miniImageNet/ResNet10_metaoptnet_aug_5way_5shot/novel.npz" % tmp_path
    assert method_dir_name("protonet") == "protonet" and method_dir_name("metaoptnet", "svm") == "metaoptnet_svm"
    with pytest.raises(ValueError):
        save_features.checkpoint_dir(parse_args(script, base + ["--head", "qp"]))
    with pytest.raises(ValueError):
        save_features.checkpoint_dir(parse_args(script, ["--method", "protonet", "--head", "svm"]))


def test_bad_head_is_refused_by_the_drivers():
    from meta_fine_tuning_amd import feature_eval, train
    from meta_fine_tuning_amd.io_utils import model_dict
    with pytest.raises(ValueError):
        train.main(["--method", "metaoptnet", "--head", "qp", "--stop_epoch", "1"])
    with pytest.raises(ValueError):
        feature_eval.build_model("metaoptnet", model_dict['ResNet10'], 5, 5, head="qp")
    with pytest.raises(ValueError):
        feature_eval.build_model("protonet", model_dict['ResNet10'], 5, 5, head="svm")
    with pytest.raises(NotImplementedError, match="metaoptnet"):
        train.main(["--method", "metaoptnet", "--head", "svm", "--fine_tune", "--stop_epoch", "1"])
    assert feature_eval.build_model("metaoptnet", model_dict['ResNet10'], 5, 5, head="svm").ENGINE_MODE == "svm"


def test_cpu_tensor_into_the_svm_head_raises_runtime_error():
    from meta_fine_tuning_amd import autograd_ops as AG
    from meta_fine_tuning_amd import ops
    feats = torch.zeros(5 * 21, 512)
    with pytest.raises(RuntimeError):
        AG.metaoptnet_svm_head(feats, torch.ones(1), 5, 5, 16)
    with pytest.raises(RuntimeError):
        ops.svm_forward(feats, torch.ones(1), 1, 5, 5, 16)
    with pytest.raises(RuntimeError):
        ops.svm_backward(dict(feats=feats, scale=torch.ones(1), shape=(1, 5, 5, 16)), torch.zeros(80, 5))
    with pytest.raises(ValueError):
        ops.svm_check(1, 33, 1, 1)
    assert ops.svm_check(1, 5, 50, 2) is None


def test_dropin_aliases_export_the_head():
    import importlib.util
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for rel, names in ((("methods", "metaoptnet.py"), ("MetaOptNet", "HEADS")), (("io_utils.py",), ("method_dir_name", "HEADS"))):
        spec = importlib.util.spec_from_file_location("_dropin_svm_" + rel[-1][:-3], os.path.join(here, "meta-fine-tuning_amd", "dropin", *rel))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        assert all(hasattr(mod, n) for n in names)
