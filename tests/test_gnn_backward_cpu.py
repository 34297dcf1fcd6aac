"""The float64 references of the GNN head's backward (tests/gnn_backward_refs.py) against torch.autograd through the CPU oracle:
each function gets a float64 forward's own exact tape and slope decisions and must reproduce autograd's gradients to 1e-10 -- two
groups with different statistics, node features whose last columns are tied (the one-hot label columns).  No package code runs."""
import numpy as np
import pytest
import torch

import gnn_backward_refs as R
from oracle import mft_oracle as O

TOL = 1e-10
CH = R.WC_CH


def _close(a, b, what=""):
    den = float(b.abs().max())
    err = float((a - b).abs().max())
    assert err <= TOL * max(den, 1e-300), (what, err, den)


def _wc_state(rs, name, F):
    sd = {}
    dims = [(F, 192), (192, 192), (192, 96), (96, 96)]
    for li, (a, b) in enumerate(dims, start=1):
        sd["%s.conv2d_%d.weight" % (name, li)] = torch.from_numpy(rs.uniform(-1, 1, (b, a, 1, 1)) / np.sqrt(a))
        sd["%s.conv2d_%d.bias" % (name, li)] = torch.from_numpy(rs.uniform(-1, 1, (b,)) / np.sqrt(a))
        sd["%s.bn_%d.weight" % (name, li)] = torch.from_numpy(rs.uniform(0.5, 1.5, (b,)))
        sd["%s.bn_%d.bias" % (name, li)] = torch.from_numpy(rs.uniform(-0.3, 0.3, (b,)))
    sd[name + ".conv2d_last.weight"] = torch.from_numpy(rs.uniform(-1, 1, (1, 96, 1, 1)) / np.sqrt(96))
    sd[name + ".conv2d_last.bias"] = torch.from_numpy(rs.uniform(-1, 1, (1,)))
    return sd


def _nodes(rs, B, N, F, n_way):
    """Node features whose last n_way columns are one-hot labels (zero for every n_way-th node): tied columns."""
    x = rs.standard_normal((B, N, F))
    x[:, :, F - n_way:] = 0.0
    for n in range(N):
        if n % (n_way + 1) != n_way:
            x[:, n, F - n_way + n % n_way] = 1.0
    return x


@pytest.fixture(scope="module")
def wc_run():
    """One float64 Wcompute forward + autograd backward per group through oracle.mft_oracle.wcompute (two groups of four graphs,
    N = 16, F = 21: 2,048 positions), with every intermediate the references are given or
    must reproduce: the raw layer outputs z_l and their gradients (captured at the oracle's BatchNorm), the per-position score
    gradient (conv2d_last.bias passed as a per-position tensor), x's and the parameters' gradients."""
    rs = np.random.RandomState(7)
    groups, gpg, N, F, n_way = 2, 4, 16, 21, 5
    name = "gnn.layer_w0"
    sd = _wc_state(rs, name, F)
    x = torch.from_numpy(_nodes(rs, groups * gpg, N, F, n_way))
    x[gpg:, :, :F - n_way] *= 1.7                                       # the second group: other statistics
    dA = torch.from_numpy(rs.standard_normal((groups * gpg, N, N)))
    x.requires_grad_(True)
    params = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    taped = []                                                           # per BatchNorm call: its input

    real_bn = O.batchnorm_train

    def bn_tap(h, gamma, beta, *a, **k):
        h.retain_grad()
        taped.append(h)
        return real_bn(h, gamma, beta, *a, **k)

    O.batchnorm_train = bn_tap
    try:
        probes, As = [], []
        for g in range(groups):
            p = dict(params)
            probe = torch.zeros(gpg * N * N, 1, dtype=torch.float64, requires_grad=True)
            p[name + ".conv2d_last.bias"] = params[name + ".conv2d_last.bias"] + probe
            probes.append(probe)
            As.append(O.wcompute(p, name, x[g * gpg:(g + 1) * gpg]))
    finally:
        O.batchnorm_train = real_bn
    A = torch.cat(As)
    (A * dA).sum().backward()
    P = N * (N + 1) // 2
    i, j = R.pair_rows(N)
    run = {"groups": groups, "gpg": gpg, "N": N, "F": F, "P": P, "name": name, "sd": sd, "x": x.detach(), "dx": x.grad, "A": A.detach(),
           "dA": dA, "grads": {k[len(name) + 1:]: v.grad for k, v in params.items()},
           "ds_full": torch.stack([p.grad.view(gpg, N, N) for p in probes]).view(groups * gpg, N, N),
           "z_ut": [], "dz_full": [], "bn": [], "masks": []}
    for li in range(4):
        zs = [taped[g * 4 + li] for g in range(groups)]                 # [gpg * N * N, C] each
        C = CH[li]
        gam, beta = sd["%s.bn_%d.weight" % (name, li + 1)], sd["%s.bn_%d.bias" % (name, li + 1)]
        tabs = [R.bn_tables(zg.detach(), gam, beta) for zg in zs]
        run["bn"].append(tuple(torch.stack([t[k] for t in tabs]) for k in range(4)))
        zf = torch.stack([zg.detach().view(gpg, N, N, C) for zg in zs])                # [groups, gpg, N, N, C]
        assert float((zf - zf.transpose(2, 3)).abs().max()) <= 1e-13 * float(zf.abs().max())      # the same at (i, j) and (j, i)
        z_ut = zf[:, :, i, j]
        run["z_ut"].append(z_ut)
        run["dz_full"].append(torch.stack([zg.grad.view(gpg, N, N, C) for zg in zs]))
        run["masks"].append(R.slope_mask(z_ut, run["bn"][li][0], run["bn"][li][1]))
    return run


def _w(run, li):
    w = run["sd"]["%s.conv2d_%d.weight" % (run["name"], li + 1)]
    return w.view(w.shape[0], -1)


def _g_full(run, li):
    """dL/d(activation of layer li) per position: the next linear layer's data gradient of autograd's own dz (the score's for
    the last layer)."""
    if li == 3:
        w5 = run["sd"][run["name"] + ".conv2d_last.weight"].view(1, 96)
        return run["ds_full"].view(run["groups"], run["gpg"], run["N"], run["N"], 1) * w5
    return run["dz_full"][li + 1] @ _w(run, li + 1)


@pytest.mark.parametrize("li", [0, 1, 2, 3])
def test_pair_bn_act_backward_full_and_merged_equal_autograd(wc_run, li):
    r = wc_run
    N = r["N"]
    gam = r["sd"]["%s.bn_%d.weight" % (r["name"], li + 1)]
    sc, sh, m, s = r["bn"][li]
    g_full = _g_full(r, li)
    assert float((g_full - g_full.transpose(2, 3)).abs().max()) > 0.1 * float(g_full.abs().max())      # independent at (i, j), (j, i)
    dz, su, sux = R.pair_bn_act_backward_full(g_full, r["z_ut"][li], sc, sh, m, s, gam, N, mask_ut=r["masks"][li])
    _close(dz, r["dz_full"][li], "dz_full")
    _close(su.sum(0), r["grads"]["bn_%d.bias" % (li + 1)], "dbeta")
    _close(sux.sum(0), r["grads"]["bn_%d.weight" % (li + 1)], "dgamma")
    assert float((su[0] - su[1]).abs().max()) > 0                       # the groups' sums differ
    # without a mask argument the decisions are z * scale + shift > 0
    dz0, _, _ = R.pair_bn_act_backward_full(g_full, r["z_ut"][li], sc, sh, m, s, gam, N)
    assert torch.equal(dz0, dz)
    # form (2) on merged rows == form (1) merged
    dzm, sum_, suxm = R.pair_bn_act_backward_merged(R.merge_full(g_full, N), r["z_ut"][li], sc, sh, m, s, gam, N, mask_ut=r["masks"][li])
    _close(dzm, R.merge_full(dz, N), "dz_ut")
    _close(sum_, su, "sum u")
    _close(suxm, sux, "sum u xhat")
    # the zero gradient of the convolution's bias in front of the BatchNorm
    assert float(r["grads"]["conv2d_%d.bias" % (li + 1)].abs().max()) <= 1e-10 * float(dz.abs().sum())


def test_softmax_backward_full_equals_autograd(wc_run):
    r = wc_run
    assert float(r["A"].diagonal(dim1=1, dim2=2).abs().max()) == 0.0
    ds = R.softmax_backward_full(r["A"], r["dA"])
    _close(ds, r["ds_full"], "ds")
    i, j = R.pair_rows(r["N"])
    ut = R.softmax_backward_merged(r["A"], r["dA"])
    want = ds[:, i, j] + torch.where(i != j, ds[:, j, i], torch.zeros((), dtype=ds.dtype))
    assert torch.equal(ut, want)


def test_absdiff_backward_full_equals_autograd(wc_run):
    r = wc_run
    dd = r["dz_full"][0] @ _w(r, 0)                                      # [groups, gpg, N, N, F]: dL/d|x_i - x_j| per position
    dd = dd.view(-1, r["N"], r["N"], r["F"])
    x = r["x"]
    assert int((x.unsqueeze(2) == x.unsqueeze(1)).sum()) > x.shape[0] * r["N"] * r["F"]       # ties beyond i == j: sign 0
    _close(R.absdiff_backward_full(x, dd), r["dx"], "dx")
    _close(R.absdiff_backward_merged(x, R.merge_full(dd, r["N"])), r["dx"], "dx from merged rows")


def test_wcompute_backward_from_tape_equals_autograd(wc_run):
    r = wc_run
    B, P = r["groups"] * r["gpg"], r["P"]
    z = [t.reshape(B * P, -1) for t in r["z_ut"]]
    masks = [t.reshape(B * P, -1) for t in r["masks"]]
    gammas = [r["sd"]["%s.bn_%d.weight" % (r["name"], li + 1)] for li in range(4)]
    dx, grads = R.wcompute_backward_from_tape(r["x"], z, r["bn"], r["A"], r["dA"], [_w(r, li) for li in range(4)], gammas,
                                              r["sd"][r["name"] + ".conv2d_last.weight"].view(96), masks, r["groups"])
    _close(dx, r["dx"], "dx")
    assert sorted(grads) == sorted(r["grads"])
    for k, v in grads.items():
        if k.endswith(".bias") and k.startswith("conv2d"):
            assert float(v.abs().max()) == 0.0
            assert float(r["grads"][k].abs().max()) <= 1e-10 * float(r["dx"].abs().sum()), k
        else:
            assert v.shape == r["grads"][k].shape, k
            _close(v, r["grads"][k], k)
    # a flipped slope decision is a different function: the mask argument is what decides
    flipped = [m.clone() for m in masks]
    flipped[1][::3] = ~flipped[1][::3]
    dx2, _ = R.wcompute_backward_from_tape(r["x"], z, r["bn"], r["A"], r["dA"], [_w(r, li) for li in range(4)], gammas,
                                           r["sd"][r["name"] + ".conv2d_last.weight"].view(96), flipped, r["groups"])
    assert float((dx2 - dx).abs().max()) > 1e-3 * float(dx.abs().max())


def test_wcompute_backward_from_tape_runs_in_float32(wc_run):
    """The yardstick of the device tests: the same function in float32 stays within float32 rounding of float64."""
    r = wc_run
    B, P = r["groups"] * r["gpg"], r["P"]

    def f(t):
        return t.float()

    dx, grads = R.wcompute_backward_from_tape(f(r["x"]), [f(t.reshape(B * P, -1)) for t in r["z_ut"]], [tuple(f(t) for t in b) for b in r["bn"]],
                                              f(r["A"]), f(r["dA"]), [f(_w(r, li)) for li in range(4)],
                                              [f(r["sd"]["%s.bn_%d.weight" % (r["name"], li + 1)]) for li in range(4)],
                                              f(r["sd"][r["name"] + ".conv2d_last.weight"].view(96)),
                                              [t.reshape(B * P, -1) for t in r["masks"]], r["groups"])
    assert dx.dtype == torch.float32 and all(v.dtype == torch.float32 for v in grads.values())
    assert R.distance(dx, r["dx"]) < 1e-4
    assert R.distance(grads["conv2d_1.weight"], r["grads"]["conv2d_1.weight"]) < 1e-4


def test_graph_aggregate_backward_equals_autograd():
    """Through oracle.mft_oracle.gconv without BatchNorm: the gradient of cat(x, A x) is the linear layer's data gradient."""
    rs = np.random.RandomState(11)
    groups, gpg, N, F, cout = 2, 3, 7, 21, 48
    B = groups * gpg
    sd = {"g.fc.weight": torch.from_numpy(rs.uniform(-1, 1, (cout, 2 * F)) / np.sqrt(2 * F)), "g.fc.bias": torch.from_numpy(rs.uniform(-1, 1, (cout,)))}
    x = torch.from_numpy(_nodes(rs, B, N, F, 5))
    x[gpg:] *= 1.7
    A = torch.softmax(torch.from_numpy(rs.standard_normal((B, N, N))) - 1e8 * torch.eye(N), dim=2)
    G = torch.from_numpy(rs.standard_normal((B, N, cout)))
    x.requires_grad_(True)
    A.requires_grad_(True)
    (O.gconv(sd, "g", A, x, False) * G).sum().backward()
    dy = G @ sd["g.fc.weight"]                                           # gradient of cat(x, A x), [B, N, 2F]
    dy = torch.cat([dy, torch.full((B, N, 3), 1e30, dtype=dy.dtype)], dim=2)              # padding columns are not read
    dx, dA = R.graph_aggregate_backward(A.detach(), x.detach(), dy, F)
    _close(dx, x.grad, "dx")
    _close(dA, A.grad, "dA")


def nodes_by_indexing(z, episodes, n_way, ns, nq, fold):
    """The node assembly one element at a time (gnnnet.py:34-38,82-83,212; gnnnet_copy.py:67-72)."""
    zf = z.shape[1]
    S = 2 * ns if fold else ns
    rows = []
    for e in range(episodes):
        for q in range(nq):
            for c in range(n_way):
                base = (e * n_way + c) * (S + nq)
                for s in range(ns + 1):
                    lab = torch.zeros(n_way, dtype=z.dtype)
                    if s < ns:
                        v = 0.5 * (z[base + s] + z[base + s + ns]) if fold else z[base + s]
                        lab[c] = 1.0
                    else:
                        v = z[base + S + q]
                    rows.append(torch.cat([v, lab]))
    return torch.stack(rows).view(-1, zf + n_way)


@pytest.mark.parametrize("n_way,ns,nq,episodes,fold", [(2, 1, 1, 1, 0), (5, 5, 4, 1, 0), (3, 2, 3, 2, 0), (5, 3, 4, 1, 1), (3, 2, 3, 2, 1)])
def test_build_graph_nodes_and_backward_equal_plain_indexing(n_way, ns, nq, episodes, fold):
    rs = np.random.RandomState(n_way * 100 + ns * 10 + nq + fold)
    zf = 12
    S = 2 * ns if fold else ns
    z = torch.from_numpy(rs.standard_normal((episodes * n_way * (S + nq), zf))).requires_grad_(True)
    want = nodes_by_indexing(z, episodes, n_way, ns, nq, fold)
    got = R.build_graph_nodes(z.detach(), episodes, n_way, ns, nq, fold)
    assert torch.equal(got, want.detach())
    g = torch.from_numpy(rs.standard_normal(tuple(want.shape)))
    (want * g).sum().backward()
    gp = torch.cat([g[:, :zf], torch.full((g.shape[0], 5), 1e30, dtype=g.dtype)], dim=1)       # label / padding gradients are not read
    _close(R.build_graph_nodes_backward(gp, zf, episodes, n_way, ns, nq, fold), z.grad, "dz")


def test_bn_backward_equals_autograd():
    rs = np.random.RandomState(3)
    groups, rows, C = 2, 34, 12
    x = torch.from_numpy(rs.standard_normal((groups, rows, C)))
    x[1] = x[1] * 1.7 + 0.4
    x.requires_grad_(True)
    gamma = torch.from_numpy(rs.uniform(0.5, 1.5, (C,))).requires_grad_(True)
    beta = torch.from_numpy(rs.uniform(-0.3, 0.3, (C,))).requires_grad_(True)
    dy = torch.from_numpy(rs.standard_normal((groups, rows, C)))
    sum((O.batchnorm_train(x[g], gamma, beta) * dy[g]).sum() for g in range(groups)).backward()
    tabs = [R.bn_tables(x[g].detach(), gamma.detach(), beta.detach()) for g in range(groups)]
    mean, rstd = torch.stack([t[2] for t in tabs]), torch.stack([t[3] for t in tabs])
    dx, dg, db = R.bn_backward(x.detach(), dy, mean, rstd, gamma.detach())
    _close(dx, x.grad, "dx")
    _close(dg, gamma.grad, "dgamma")
    _close(db, beta.grad, "dbeta")
