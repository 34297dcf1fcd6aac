"""Plain-torch statements of the GNN head's backward operators (gnn.py:16-28,65-132; gnnnet.py:34-38,82-83,212; gnnnet_copy.py:
67-72), written as functions of ``dtype``: float64 is the reference the HIP launchers are held to, float32 the yardstick (the same
arithmetic at the device's precision).  tests/test_gnn_backward_cpu.py proves every function against torch.autograd through the
CPU oracle; tests/test_gnn_backward_gpu.py compares the launchers with them.  Nothing here touches the package.

Layouts.  A graph has N nodes and P = N(N+1)/2 upper-triangle pair rows p(i, j) = i*N - i(i-1)/2 + (j - i), i <= j.  "Full" tensors
carry every (i, j) position of the reference's N x N formulation, "merged" (``_ut``) tensors one row per unordered pair: an
activation is the same at (i, j) and (j, i), a merged gradient is the sum of the gradients at the two positions (the diagonal
has one).  BatchNorm statistics belong to a group (the graphs of one episode), the affine parameters are shared by the groups."""
import numpy as np
import torch

SLOPE = 0.01         # F.leaky_relu's default (gnn.py:86)
BN_EPS = 1e-5


def pair_rows(N):
    """(i, j) of the P upper-triangle rows in row order, as int64 tensors."""
    i, j = np.triu_indices(N)
    return torch.from_numpy(i.astype(np.int64)), torch.from_numpy(j.astype(np.int64))


def pair_position(N):
    """[N, N] int64: the upper-triangle row that position (i, j) reads, p(min(i, j), max(i, j))."""
    i = torch.arange(N).view(N, 1).expand(N, N)
    j = torch.arange(N).view(1, N).expand(N, N)
    a, c = torch.minimum(i, j), torch.maximum(i, j)
    return a * N - (a * (a - 1)) // 2 + (c - a)


def expand_ut(v_ut, N):
    """[..., P, C] values on upper-triangle rows -> [..., N, N, C] (the same value at (i, j) and (j, i))."""
    return v_ut[..., pair_position(N), :]


def merge_full(d_full, N):
    """[..., N, N, C] per-position gradients -> [..., P, C]: d[i, j] + d[j, i] for i < j, d[i, i] on the diagonal."""
    i, j = pair_rows(N)
    off = (i != j).to(d_full.dtype).view(-1, 1)
    return d_full[..., i, j, :] + off * d_full[..., j, i, :]


def pair_count(N, dtype):
    """[P, 1]: how many positions of the N x N formulation a merged row stands for (1 on the diagonal, 2 off it)."""
    i, j = pair_rows(N)
    return (1 + (i != j).to(dtype)).view(-1, 1)


def bn_tables(z_full_rows, gamma, beta, eps=BN_EPS):
    """(scale, shift, mean, rstd) [C] of a train-mode BatchNorm over the rows of z_full_rows [positions, C] (biased variance)."""
    mean = z_full_rows.mean(0)
    rstd = 1.0 / torch.sqrt(z_full_rows.var(0, unbiased=False) + eps)
    scale = gamma * rstd
    return scale, beta - mean * scale, mean, rstd


def slope_mask(z, scale, shift):
    """The positive-side decision of leaky_relu(z * scale + shift) per element; z [groups, ..., C], scale / shift [groups, C]."""
    g, C = scale.shape
    sh = (g,) + (1,) * (z.dim() - 2) + (C,)
    return z * scale.view(sh) + shift.view(sh) > 0


def pair_bn_act_backward_full(g_full, z_ut, scale, shift, mean, rstd, gamma, N, mask_ut=None, slope=SLOPE):
    """BatchNorm2d(train) + leaky_relu backward of one Wcompute layer in the N x N formulation (gnn.py:65-102 under autograd).
    g_full [groups, gpg, N, N, C]: dL/d(activation) per position; z_ut [groups, gpg, P, C]: the layer's raw output on upper-triangle
    rows; scale / shift / mean / rstd [groups, C]; gamma [C]; mask_ut (bool, like z_ut): where the activation takes slope 1
    (default: z * scale + shift > 0).  -> (dz_full like g_full, sum u [groups, C], sum u * xhat [groups, C])."""
    groups, gpg = g_full.shape[:2]
    C = g_full.shape[-1]
    if mask_ut is None:
        mask_ut = slope_mask(z_ut, scale, shift)
    b = (groups, 1, 1, 1, C)
    one = torch.ones((), dtype=g_full.dtype)
    u = g_full * torch.where(expand_ut(mask_ut, N), one, one * slope)
    xhat = (expand_ut(z_ut, N) - mean.view(b)) * rstd.view(b)
    su, sux = u.sum((1, 2, 3)), (u * xhat).sum((1, 2, 3))
    n_tot = gpg * N * N
    dz = (gamma.view(1, 1, 1, 1, C) * rstd.view(b)) * (u - su.view(b) / n_tot - xhat * (sux.view(b) / n_tot))
    return dz, su, sux


def pair_bn_act_backward_merged(g_ut, z_ut, scale, shift, mean, rstd, gamma, N, mask_ut=None, slope=SLOPE):
    """The same on merged rows: g_ut [groups, gpg, P, C] carries the sum of the two positions' gradients, the mean-subtraction
    terms count a row ``cnt`` times (1 on the diagonal, 2 off it).  -> (dz_ut, sum u, sum u * xhat)."""
    groups, gpg = g_ut.shape[:2]
    C = g_ut.shape[-1]
    if mask_ut is None:
        mask_ut = slope_mask(z_ut, scale, shift)
    b = (groups, 1, 1, C)
    one = torch.ones((), dtype=g_ut.dtype)
    u = g_ut * torch.where(mask_ut, one, one * slope)
    xhat = (z_ut - mean.view(b)) * rstd.view(b)
    su, sux = u.sum((1, 2)), (u * xhat).sum((1, 2))
    n_tot = gpg * N * N
    cnt = pair_count(N, g_ut.dtype)
    dz = (gamma.view(1, 1, 1, C) * rstd.view(b)) * (u - cnt * (su.view(b) / n_tot) - cnt * xhat * (sux.view(b) / n_tot))
    return dz, su, sux


def softmax_backward_full(A, dA):
    """Row softmax backward: ds = A * (dA - <A, dA>_row); A, dA [B, N, N]."""
    return A * (dA - (A * dA).sum(-1, keepdim=True))


def softmax_backward_merged(A, dA):
    """-> ds_ut [B, P]: ds[i, j] + ds[j, i] for i < j, ds[i, i] on the diagonal."""
    return merge_full(softmax_backward_full(A, dA).unsqueeze(-1), A.shape[-1]).squeeze(-1)


def absdiff_backward_full(x, dd):
    """d = |x_i - x_j| backward: dx[b, i, f] = sum_j sign(x_i - x_j) * (dd[b, i, j, f] + dd[b, j, i, f]), sign(0) = 0 as torch.abs
    differentiates.  x [B, N, F], dd [B, N, N, F]."""
    sg = torch.sign(x.unsqueeze(2) - x.unsqueeze(1))
    return (sg * (dd + dd.transpose(1, 2))).sum(2)


def absdiff_backward_merged(x, dd_ut):
    """The same from merged rows dd_ut [B, P, F] (a row carries both positions' gradients; diagonal rows never count)."""
    N = x.shape[1]
    i = torch.arange(N)
    upper = (i.view(N, 1) < i.view(1, N)).to(x.dtype).view(1, N, N, 1)
    return absdiff_backward_full(x, expand_ut(dd_ut, N) * upper)


def absdiff_ut(x):
    """|x_i - x_j| on the upper-triangle rows: [B, N, F] -> [B, P, F]."""
    i, j = pair_rows(x.shape[1])
    return (x[:, i] - x[:, j]).abs()


def graph_aggregate_backward(A, x, dy, F):
    """y = cat(x, A x) backward (gmul, gnn.py:16-28, J = 2): dx = dy[:, :F] + A^T dy[:, F:2F], dA = dy[:, F:2F] x^T.
    A [B, N, N], x [B, N, F], dy [B, N, >= 2F] -> (dx [B, N, F], dA [B, N, N])."""
    d2 = dy[..., F:2 * F]
    return dy[..., :F] + A.transpose(1, 2) @ d2, d2 @ x.transpose(1, 2)


def build_graph_nodes(z, episodes, n_way, n_support, n_query, fold):
    """z_stack + cat(z, support_label) (gnnnet.py:34-38,82-83,212): z [episodes * n_way * (S + n_query), zf], S = n_support or, with
    ``fold``, 2 * n_support (supports k and k + n_support averaged, gnnnet_copy.py:67-72) -> nodes [episodes * n_query * n_way *
    (n_support + 1), zf + n_way]: graph (e, q) holds every class's supports and its q-th query, one-hot label behind a support."""
    zf = z.shape[1]
    S = 2 * n_support if fold else n_support
    z4 = z.view(episodes, n_way, S + n_query, zf)
    sup = z4[:, :, :S]
    if fold:
        sup = 0.5 * (sup[:, :, :n_support] + sup[:, :, n_support:])
    qry = z4[:, :, S:]                                                              # [E, n_way, nq, zf]
    sup = sup.unsqueeze(1).expand(episodes, n_query, n_way, n_support, zf)
    feat = torch.cat([sup, qry.permute(0, 2, 1, 3).unsqueeze(3)], dim=3)             # [E, nq, n_way, ns + 1, zf]
    lab = torch.zeros(n_way, n_support + 1, n_way, dtype=z.dtype)
    for c in range(n_way):
        lab[c, :n_support, c] = 1.0
    lab = lab.view(1, 1, n_way, n_support + 1, n_way).expand(episodes, n_query, n_way, n_support + 1, n_way)
    return torch.cat([feat, lab], dim=4).reshape(-1, zf + n_way)


def build_graph_nodes_backward(dnodes, zf, episodes, n_way, n_support, n_query, fold):
    """dnodes [rows, >= zf] -> dz [episodes * n_way * (S + n_query), zf]: a support gathers from all n_query graphs of its episode
    (half of it to each of the two folded supports), a query from its own graph."""
    d = dnodes[:, :zf].reshape(episodes, n_query, n_way, n_support + 1, zf)
    dsup = d[:, :, :, :n_support].sum(1)                                             # [E, n_way, ns, zf]
    if fold:
        dsup = torch.cat([0.5 * dsup, 0.5 * dsup], dim=2)
    dq = d[:, :, :, n_support].permute(0, 2, 1, 3)                                   # [E, n_way, nq, zf]
    return torch.cat([dsup, dq], dim=2).reshape(-1, zf)


def bn_backward(x, dy, mean, rstd, gamma):
    """Train-mode BatchNorm1d backward with per-group statistics and shared affine parameters: x, dy [groups, rows, C];
    mean / rstd [groups, C]; gamma [C] -> (dx like x, dgamma [C], dbeta [C]: summed over the groups)."""
    rows = x.shape[1]
    xhat = (x - mean.unsqueeze(1)) * rstd.unsqueeze(1)
    db, dg = dy.sum(1), (dy * xhat).sum(1)
    dx = (gamma * rstd).unsqueeze(1) * (dy - db.unsqueeze(1) / rows - xhat * (dg.unsqueeze(1) / rows))
    return dx, dg.sum(0), db.sum(0)


WC_CH = (192, 192, 96, 96)


def wcompute_backward_from_tape(x, z, bn, A, dA, weights, gammas, w_last, masks, groups, slope=SLOPE):
    """The whole gnn.Wcompute backward (gnn.py:78-132 under autograd) from a forward's tape.
    x [B, N, F] node features; z: the four raw layer outputs on upper-triangle rows [B * P, C_l], graphs of a group consecutive;
    bn: per layer (scale, shift, mean, rstd) [groups, C_l]; A, dA [B, N, N]; weights: conv2d_1..4 as [C_l, C_(l-1)] matrices;
    gammas: bn_1..4.weight; w_last [96]; masks: per layer bool [B * P, C_l], True where the activation takes slope 1.
    -> (dx [B, N, F], grads) with grads keyed like the state dict below the Wcompute's prefix ('conv2d_1.weight', 'bn_1.weight',
    ...; the bias of a convolution in front of a BatchNorm, and conv2d_last's under the row softmax, have zero gradient).
    A merged off-diagonal row enters a weight gradient once: its gradient already carries both positions."""
    B, N, F = x.shape
    P = N * (N + 1) // 2
    gpg = B // groups
    dt = x.dtype
    one = torch.ones((), dtype=dt)

    def act(li):
        sc, sh = bn[li][0], bn[li][1]
        C = sc.shape[1]
        y = z[li].view(groups, gpg * P, C) * sc.view(groups, 1, C) + sh.view(groups, 1, C)
        return (y * torch.where(masks[li].view(groups, gpg * P, C), one, one * slope)).view(B * P, C)

    grads = {}
    ds = softmax_backward_merged(A, dA).reshape(B * P, 1)
    grads["conv2d_last.weight"] = (ds.t() @ act(3)).view(1, -1, 1, 1)
    grads["conv2d_last.bias"] = torch.zeros(1, dtype=dt)
    dh = ds * w_last.view(1, -1)
    dx = None
    for li in (3, 2, 1, 0):
        sc, sh, m, s = bn[li]
        C = sc.shape[1]
        dz, su, sux = pair_bn_act_backward_merged(dh.view(groups, gpg, P, C), z[li].view(groups, gpg, P, C), sc, sh, m, s, gammas[li], N,
                                                  mask_ut=masks[li].view(groups, gpg, P, C), slope=slope)
        dz = dz.reshape(B * P, C)
        grads["bn_%d.weight" % (li + 1)], grads["bn_%d.bias" % (li + 1)] = sux.sum(0), su.sum(0)
        grads["conv2d_%d.bias" % (li + 1)] = torch.zeros(C, dtype=dt)
        w = weights[li]
        if li > 0:
            grads["conv2d_%d.weight" % (li + 1)] = (dz.t() @ act(li - 1)).view(C, -1, 1, 1)
            dh = dz @ w
        else:
            grads["conv2d_1.weight"] = (dz.t() @ absdiff_ut(x).reshape(B * P, F)).view(C, F, 1, 1)
            dx = absdiff_backward_merged(x, (dz @ w).view(B, P, F))
    return dx, grads


# ---------------------------------------------------------------------------------------------- the bar of the device comparisons

FLOOR = 8.0 * 2.0 ** -24        # eight float32 roundings of the tensor's largest value


def distance(v, ref64):
    """max|v - ref| / max|ref| (0 for an all-zero reference that is met exactly)."""
    v, ref64 = torch.as_tensor(v).double(), torch.as_tensor(ref64).double()
    den = float(ref64.abs().max())
    err = float((v - ref64).abs().max())
    return err / den if den > 0 else (0.0 if err == 0 else float("inf"))


def ratio_to_float32_chain(dev, ref64, ref32):
    """-> (device distance, bar, distance / yardstick): the bar is 4 x the distance of the float32 CPU run of the same reference to
    its float64 run, and never below FLOOR -- where the CPU chain happens to be exact (a copy, a sum of two terms) the device may
    still round each of a handful of operations once."""
    err, yard = distance(dev, ref64), distance(ref32, ref64)
    return err, max(4.0 * yard, FLOOR), err / max(yard, FLOOR / 4.0)
