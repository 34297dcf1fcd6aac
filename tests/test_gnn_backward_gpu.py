"""Every backward launcher of the GNN head on its own, and the chain wcompute_taped -> wcompute_backward, against the float64
references of tests/gnn_backward_refs.py (proved against autograd by tests/test_gnn_backward_cpu.py) on a real MI355X.

The bar (as in tests/test_metaoptnet_gpu.py and tests/test_tpn_gpu.py): for every output tensor max|device - float64| / max|float64|
is at most 4 x the same distance of the same reference run in float32 on the CPU, and never below eight float32 roundings of the
tensor's largest value (gnn_backward_refs.FLOOR: where the CPU chain is exact -- a copy, a sum of two terms -- the device may still
round a handful of operations once).  What is pure selection is array-equal.  Slope decisions: where a test controls z, scale and
shift it moves every |z * scale + shift| < 1e-3 away from zero before the launch; the chain differentiates the DEVICE's own tape
with the decisions z * scale + shift > 0 taken in float64 from the tape's float32 values, and asserts that no tape element lies
where a float32 evaluation could decide otherwise.

Largest measured ratio per launcher on an MI355X (device distance / float32-CPU distance, the latter taken as at least a quarter of
the floor; the bar is 4; every test prints its own and the module prints the maxima at its end):
    mft_pair_softmax_ut_backward    1.34        mft_pair_bn_act_backward        1.58
    mft_pair_dx_gather              1.85        mft_graph_aggregate_backward    1.00  (7.95 at N = 130 before the node's own
    mft_build_graph_nodes_backward  1.00                                              gradient was added last: csrc/backward.hip)
    mft_act_backward (accumulating) 0.44        mft_bn_backward_act (FB.bn_bwd) 1.86
    mft_masked_softmax_backward     1.00        mft_pair_absdiff_backward       2.12
    chain, register-K layers        2.10        chain, tile layers              1.62
"""
import numpy as np
import pytest
import torch

import meta_fine_tuning_amd  # noqa: F401
from meta_fine_tuning_amd import _lib, ops, synthetic
from meta_fine_tuning_amd import functional as Fn
from meta_fine_tuning_amd import functional_bwd as FB

import gnn_backward_refs as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
torch.set_num_threads(8)
F64, F32 = torch.float64, torch.float32
SLOPE32 = np.float32(ops.LRELU_SLOPE)
RATIOS = {}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def t(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def both(fn):
    """fn(dtype) -> a tensor or a tuple of tensors: (its float64 run, its float32 run)."""
    return fn(F64), fn(F32)


def held(launcher, what, got, ref64, ref32):
    """Asserts the bar for one output tensor and records the ratio under the launcher's name."""
    err, bar, ratio = R.ratio_to_float32_chain(got.detach().cpu(), ref64, ref32)
    RATIOS[launcher] = max(RATIOS.get(launcher, 0.0), ratio)
    print("%s %s: distance %.3e, bar %.3e, ratio to the float32 chain %.2f" % (launcher, what, err, bar, ratio))
    assert err <= bar, (launcher, what, err, bar, ratio)


def agree(launcher, what, a, b, ref64, ref32):
    """Two routes on the device: max|a - b| / max|float64| within the same bar."""
    den = float(ref64.abs().max())
    err = float((a.detach().cpu().double() - b.detach().cpu().double()).abs().max()) / den
    yard = R.distance(ref32, ref64)
    ratio = err / max(yard, R.FLOOR / 4.0)
    RATIOS[launcher] = max(RATIOS.get(launcher, 0.0), ratio)
    print("%s %s: distance %.3e, float32 chain %.3e, ratio %.2f" % (launcher, what, err, yard, ratio))
    assert err <= max(4.0 * yard, R.FLOOR), (launcher, what, err, yard)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(RATIOS):
        print("\nlargest ratio %-40s %.2f" % (k, RATIOS[k]), end="")
    print()


def softmax_A(rs, B, N):
    """A real masked row softmax in float32: the diagonal is exactly 0."""
    s = torch.from_numpy(rs.standard_normal((B, N, N)).astype(np.float32)) - 1e8 * torch.eye(N)
    A = torch.softmax(s, dim=2)
    assert float(A.diagonal(dim1=1, dim2=2).abs().max()) == 0.0
    return A.numpy()


def tied_nodes(rs, B, N, F, ld=256, n_way=5, pad=1e30):
    """[B * N, ld] node features: the last n_way of the F columns are one-hot labels (tied between nodes), columns from F on
    hold ``pad`` (never read)."""
    x = np.full((B * N, ld), pad, dtype=np.float32)
    v = rs.standard_normal((B, N, F)).astype(np.float32)
    v[:, :, F - n_way:] = 0.0
    for n in range(N):
        if n % (n_way + 1) != n_way:
            v[:, n, F - n_way + n % n_way] = 1.0
    x[:, :F] = v.reshape(B * N, F)
    return x


# ================================================================================================ mft_pair_softmax_ut_backward

def run_softmax_ut(A, dA, ldds):
    B, N = A.shape[:2]
    P = N * (N + 1) // 2
    ij = Fn.pair_index_table(N, DEV)
    ds = torch.full((B * P, ldds), -7.0, device=DEV)
    rd = torch.empty((B * N,), device=DEV)
    db5 = torch.full((1,), 5.0, device=DEV)
    Ad, dAd = dev(A), dev(dA)                      # (named: a temporary would be freed, and its memory reused, before the launch)
    _lib.call("mft_pair_softmax_ut_backward", ops._p(Ad), ops._p(dAd), ops._p(ij), ops._p(rd), ops._p(ds), ldds, B, N, ops._p(db5),
              ops._stream())
    return ds, db5


@pytest.mark.parametrize("ldds", [1, 32])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("N", [4, 7, 30, 64, 65, 130])
def test_pair_softmax_ut_backward(N, B, ldds):
    """N <= 64: the inline row-dot form; above: the row-dot launch.  Asymmetric dA with a non-zero diagonal."""
    rs = np.random.RandomState(1000 * N + 10 * B + ldds)
    A = softmax_A(rs, B, N)
    dA = rs.standard_normal((B, N, N)).astype(np.float32)
    assert np.abs(np.diagonal(dA, axis1=1, axis2=2)).min() > 0
    ds, db5 = run_softmax_ut(A, dA, ldds)
    r64, r32 = both(lambda d: R.softmax_backward_merged(t(A, d), t(dA, d)).reshape(-1))
    held("mft_pair_softmax_ut_backward", "ds", ds[:, 0], r64, r32)
    assert float(db5[0]) == 0.0
    assert bool((ds[:, 1:] == -7.0).all())


def test_pair_softmax_ut_backward_past_the_grid_cap():
    """N = 130, 250 graphs: 2,128,750 rows, more than 8,192 blocks of 256: the grid-stride loop takes the rest."""
    rs = np.random.RandomState(77)
    B, N = 250, 130
    assert B * (N * (N + 1) // 2) > 8192 * 256
    A = softmax_A(rs, B, N)
    dA = rs.standard_normal((B, N, N)).astype(np.float32)
    ds, db5 = run_softmax_ut(A, dA, 1)
    r64, r32 = both(lambda d: R.softmax_backward_merged(t(A, d), t(dA, d)).reshape(-1))
    held("mft_pair_softmax_ut_backward", "ds", ds[:, 0], r64, r32)
    assert float(db5[0]) == 0.0


# ================================================================================================ mft_pair_bn_act_backward

def bn_act_inputs(rs, C, N, groups, gpg, full=True):
    """z [groups, gpg, P, C] (every group its own level and spread), the groups' BatchNorm tables over the N x N positions, gamma,
    and merged gradients g_ut split into independent per-position values: a at (i, j), g_ut - a at (j, i) with a = g_ut * r rounded
    to float32, r in [1/2, 1) -- the difference is then exact in float32 (Sterbenz), so the merged row IS the sum of the two."""
    P = N * (N + 1) // 2
    z = rs.standard_normal((groups, gpg, P, C))
    z = (z * (1.0 + 0.6 * np.arange(groups)).reshape(-1, 1, 1, 1) + 0.4 * np.arange(groups).reshape(-1, 1, 1, 1)).astype(np.float32)
    gamma = rs.uniform(0.5, 1.5, (C,)).astype(np.float32)
    beta = rs.uniform(-0.3, 0.3, (C,)).astype(np.float32)
    cnt = R.pair_count(N, F64).numpy().reshape(1, P, 1)
    n_tot = gpg * N * N
    z64 = z.astype(np.float64)
    mean = (z64 * cnt).sum((1, 2)) / n_tot
    var = (((z64 - mean[:, None, None]) ** 2) * cnt).sum((1, 2)) / n_tot
    rstd = 1.0 / np.sqrt(var + 1e-5)
    scale = (gamma * rstd).astype(np.float32)
    shift = (beta - mean * gamma * rstd).astype(np.float32)
    mean, rstd = mean.astype(np.float32), rstd.astype(np.float32)
    # slope decisions: every |z * scale + shift| < 1e-3 is moved to +-2e-3 (the tables are inputs of the launcher: they stay)
    sc64, sh64 = scale.astype(np.float64)[:, None, None], shift.astype(np.float64)[:, None, None]
    y = z.astype(np.float64) * sc64 + sh64
    near = np.abs(y) < 1e-3
    z = np.where(near, (np.where(y >= 0, 2e-3, -2e-3) - sh64) / sc64, z).astype(np.float32)
    assert np.abs(z.astype(np.float64) * sc64 + sh64).min() >= 1e-3
    g_ut = rs.standard_normal((groups, gpg, P, C)).astype(np.float32)
    a = (g_ut * rs.uniform(0.5, 1.0, g_ut.shape).astype(np.float32)).astype(np.float32)
    b = (g_ut - a).astype(np.float32)
    assert np.array_equal((a.astype(np.float64) + b.astype(np.float64)), g_ut.astype(np.float64))
    if not full:
        return z, (scale, shift, mean, rstd), gamma, g_ut, None
    i, j = np.triu_indices(N)
    off = i != j
    g_full = np.zeros((groups, gpg, N, N, C), dtype=np.float32)
    g_full[:, :, i, j] = np.where(off[None, None, :, None], a, g_ut)
    g_full[:, :, j[off], i[off]] = b[:, :, off]
    return z, (scale, shift, mean, rstd), gamma, g_ut, g_full


def run_bn_act(z, tabs, gamma, g_ut, N, ldg):
    groups, gpg, P, C = z.shape
    rows = groups * gpg * P
    g = np.full((rows, ldg), 1e30, dtype=np.float32)
    g[:, :C] = g_ut.reshape(rows, C)
    sums, dpar, dbz = torch.full((groups, 2 * C), 3.0, device=DEV), torch.full((2 * C,), 3.0, device=DEV), torch.full((C,), 3.0, device=DEV)
    ws = torch.empty((groups * int(_lib.lib().mft_pair_bwd_stats_ws_floats(gpg * P, C)),), device=DEV)
    dz = torch.full((rows + 1, C), -7.0, device=DEV)
    sc, sh, m, s = (dev(a) for a in tabs)
    gd, zd, gam = dev(g), dev(z.reshape(rows, C)), dev(gamma)
    _lib.call("mft_pair_bn_act_backward", ops._p(gd), ldg, ops._p(zd), C, ops._p(sc), ops._p(sh), ops._p(m), ops._p(s),
              ops._p(gam), ops._p(Fn.pair_index_table(N, DEV)), N, gpg * P, groups, gpg * N * N, ops.LRELU_SLOPE, ops._p(ws),
              ops._p(sums), ops._p(dpar), ops._p(dbz), ops._p(dz), ops._stream())
    assert bool((dz[rows] == -7.0).all())
    return dz[:rows], sums, dpar, dbz


def check_bn_act(out, ref64, ref32, groups, C):
    dz, sums, dpar, dbz = out
    (dz64, su64, sux64), (dz32, su32, sux32) = ref64, ref32
    held("mft_pair_bn_act_backward", "dz", dz, dz64.reshape(-1, C), dz32.reshape(-1, C))
    for g in range(groups):
        held("mft_pair_bn_act_backward", "sum u [%d]" % g, sums[g, :C], su64[g], su32[g])
        held("mft_pair_bn_act_backward", "sum u xhat [%d]" % g, sums[g, C:], sux64[g], sux32[g])
    held("mft_pair_bn_act_backward", "dbeta", dpar[:C], su64.sum(0), su32.sum(0))
    held("mft_pair_bn_act_backward", "dgamma", dpar[C:], sux64.sum(0), sux32.sum(0))
    acc = sums[0].clone()
    for g in range(1, groups):
        acc = acc + sums[g]
    assert torch.equal(dpar, acc)                  # the group sums added up, in group order
    assert bool((dbz == 0).all())


@pytest.mark.parametrize("groups,gpg", [(1, 1), (1, 3), (3, 2)])
@pytest.mark.parametrize("N", [4, 7, 30, 65])
@pytest.mark.parametrize("C", [96, 192])
def test_pair_bn_act_backward_vs_full_reference(C, N, groups, gpg):
    """Against the N x N formulation, merged; ldg = C and ldg > C (N = 4, 7 with one group: fewer rows than one statistics block)."""
    rs = np.random.RandomState(C + 10 * N + 1000 * groups + gpg)
    z, tabs, gamma, g_ut, g_full = bn_act_inputs(rs, C, N, groups, gpg)

    def ref(d):
        dz, su, sux = R.pair_bn_act_backward_full(t(g_full, d), t(z, d), *(t(a, d) for a in tabs), t(gamma, d), N)
        return R.merge_full(dz, N), su, sux

    r64, r32 = both(ref)
    for ldg in (C, C + 32):
        check_bn_act(run_bn_act(z, tabs, gamma, g_ut, N, ldg), r64, r32, groups, C)


def test_pair_bn_act_backward_past_both_grid_caps():
    """C = 192, N = 130, one group of 11 graphs: 93,665 rows -- more than 1,024 statistics blocks of 64 rows and more than 16,384
    dz blocks; against the merged-row reference (the full expansion would take 11 x 130 x 130 x 192 doubles several times over)."""
    rs = np.random.RandomState(130)
    C, N, groups, gpg = 192, 130, 1, 11
    P = N * (N + 1) // 2
    assert gpg * P == 93665 and gpg * P > 1024 * 64 and gpg * P * (C // 4) > 16384 * 256
    z, tabs, gamma, g_ut, _ = bn_act_inputs(rs, C, N, groups, gpg, full=False)
    r64, r32 = both(lambda d: R.pair_bn_act_backward_merged(t(g_ut, d), t(z, d), *(t(a, d) for a in tabs), t(gamma, d), N))
    check_bn_act(run_bn_act(z, tabs, gamma, g_ut, N, C), r64, r32, groups, C)


@pytest.mark.parametrize("why,C,ldg,rpg,n_tot", [("C = 128", 128, 128, 28, 49), ("ldg < C", 96, 92, 28, 49), ("rows_per_group % P", 96, 96, 30, 49),
                                                ("n_tot < rows_per_group", 96, 96, 28, 27)])
def test_pair_bn_act_backward_refuses_out_of_domain_arguments(why, C, ldg, rpg, n_tot):
    """MFT_EINVAL before any launch: the outputs keep their fill."""
    N = 7
    buf = torch.zeros((64, 256), device=DEV)
    tab = torch.ones((256,), device=DEV)
    out = torch.full((64 * 256,), -7.0, device=DEV)
    rc = _lib.lib().mft_pair_bn_act_backward(ops._p(buf), ldg, ops._p(buf), C, ops._p(tab), ops._p(tab), ops._p(tab), ops._p(tab), ops._p(tab),
                                            ops._p(Fn.pair_index_table(N, DEV)), N, rpg, 1, n_tot, ops.LRELU_SLOPE, ops._p(out), ops._p(out),
                                            ops._p(out), ops._p(out), ops._p(out), ops._stream())
    torch.cuda.synchronize()
    assert rc == _lib.MFT_EINVAL, why
    assert bool((out == -7.0).all())


# ================================================================================================ mft_pair_absdiff_ut

def absdiff_rows(x, B, N, F, row0, nrows):
    i, j = np.triu_indices(N)
    P = i.size
    r = np.arange(row0, row0 + nrows)
    b, p = r // P, r % P
    return np.abs(x[b * N + i[p], :F] - x[b * N + j[p], :F])


@pytest.mark.parametrize("F", [130, 133, 229, 256])
def test_pair_absdiff_ut_windows(F):
    """Array-equal to numpy for windows that start inside a graph, straddle a graph boundary, are one row long or the whole
    range; zero in columns F .. Kp - 1 although x holds 1e30 there; the row behind the window keeps its fill."""
    rs = np.random.RandomState(F)
    B, N = 3, 7
    P = N * (N + 1) // 2
    Kp = ops.round_up(F, 32)
    x = tied_nodes(rs, B, N, F)
    xd, ij = dev(x), Fn.pair_index_table(N, DEV)
    for row0, nrows in [(5, 10), (20, 20), (P + 2, 1), (0, B * P), (B * P - 1, 1)]:
        d = torch.full((nrows + 1, Kp), -7.0, device=DEV)
        _lib.call("mft_pair_absdiff_ut", ops._p(xd), x.shape[1], ops._p(ij), ops._p(d), Kp, F, N, row0, nrows, ops._stream())
        got = d.cpu().numpy()
        assert np.array_equal(got[:nrows, :F], absdiff_rows(x, B, N, F, row0, nrows)), (row0, nrows)
        assert np.all(got[:nrows, F:] == 0) and np.all(got[nrows] == -7.0), (row0, nrows)


@pytest.mark.parametrize("F", [229, 256])
def test_pair_absdiff_ut_full_chunk(F):
    """The product's full chunk: PAIR_CHUNK_ROWS = 16,384 rows at Kp = 256, starting inside a graph (N = 30, 36 graphs)."""
    rs = np.random.RandomState(F + 1)
    B, N, nrows, row0 = 36, 30, 16384, 100
    assert FB.PAIR_CHUNK_ROWS == nrows and B * (N * (N + 1) // 2) >= row0 + nrows
    x = tied_nodes(rs, B, N, F)
    d = torch.full((nrows + 1, 256), -7.0, device=DEV)
    xd = dev(x)
    _lib.call("mft_pair_absdiff_ut", ops._p(xd), 256, ops._p(Fn.pair_index_table(N, DEV)), ops._p(d), 256, F, N, row0, nrows, ops._stream())
    got = d.cpu().numpy()
    assert np.array_equal(got[:nrows, :F], absdiff_rows(x, B, N, F, row0, nrows))
    assert np.all(got[:nrows, F:] == 0) and np.all(got[nrows] == -7.0)


# ================================================================================================ mft_pair_dx_gather

def run_dx_gather(xd, dd, dX0, B, N, F, windows):
    Kp = dd.shape[1]
    dX = dev(dX0)
    ddd = dev(dd)
    for r0, nr in windows:
        chunk = ddd[r0:r0 + nr].clone()                # as the backward has it: the chunk's own buffer
        _lib.call("mft_pair_dx_gather", ops._p(xd), xd.shape[1], ops._p(chunk), Kp, ops._p(dX), dX.shape[1], B, N, F, r0, nr, ops._stream())
    return dX


@pytest.mark.parametrize("F", [130, 133, 229])
@pytest.mark.parametrize("N", [4, 5, 6, 7, 13, 30])
def test_pair_dx_gather(N, F):
    """The six-at-a-time j loop with every tail length; dX accumulates; tied columns give sign 0; the diagonal rows of dd hold large
    finite values that must not arrive; two and three windows that split a graph add up to the one-window result."""
    rs = np.random.RandomState(100 * N + F)
    B = 3
    P = N * (N + 1) // 2
    Kp = ops.round_up(F, 32)
    x = tied_nodes(rs, B, N, F)
    i, j = np.triu_indices(N)
    dd = rs.standard_normal((B * P, Kp)).astype(np.float32)
    dd.reshape(B, P, Kp)[:, i == j] = 3e30
    dX0 = rs.standard_normal((B * N, 256)).astype(np.float32)

    def ref(d):
        x3 = t(x[:, :F], d).view(B, N, F)
        ddu = t(dd[:, :F], d).view(B, P, F) * t((i != j).astype(np.float64), d).view(1, P, 1)
        return t(dX0[:, :F], d) + R.absdiff_backward_merged(x3, ddu).reshape(B * N, F)

    r64, r32 = both(ref)
    xd = dev(x)
    one = run_dx_gather(xd, dd, dX0, B, N, F, [(0, B * P)])
    held("mft_pair_dx_gather", "dX", one[:, :F], r64, r32)
    assert np.array_equal(one[:, F:].cpu().numpy(), dX0[:, F:])
    # the diagonal rows are left out, not multiplied by sign(x_i - x_i) = 0: infinities there change nothing
    dd_inf = dd.copy()
    dd_inf.reshape(B, P, Kp)[:, i == j] = np.inf
    assert torch.equal(run_dx_gather(xd, dd_inf, dX0, B, N, F, [(0, B * P)]), one)
    c1, c2 = P + P // 2, 2 * P + 1
    for windows in ([(0, c1), (c1, B * P - c1)], [(0, c1), (c1, c2 - c1), (c2, B * P - c2)]):
        split = run_dx_gather(xd, dd, dX0, B, N, F, windows)
        held("mft_pair_dx_gather", "dX over %d windows" % len(windows), split[:, :F], r64, r32)
        agree("mft_pair_dx_gather", "windows against one window", split[:, :F], one[:, :F], r64, r32)
        assert np.array_equal(split[:, F:].cpu().numpy(), dX0[:, F:])


# ================================================================================================ mft_graph_aggregate_backward

@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("F", [130, 133, 229, 256, 260])
@pytest.mark.parametrize("N", [4, 7, 30, 65, 130])
def test_graph_aggregate_backward(N, F, B):
    """F <= 256: the register form of dA; F = 260: the loop form (accepted by the launcher, reached by no head)."""
    rs = np.random.RandomState(1000 * N + F + B)
    ldx = max(256, ops.round_up(F, 32))
    lddy, lddx = ops.round_up(2 * F, 32), ldx + 32
    A = softmax_A(rs, B, N)
    x = tied_nodes(rs, B, N, F, ld=ldx)
    dy = rs.standard_normal((B * N, lddy)).astype(np.float32)
    dX0 = rs.standard_normal((B * N, lddx)).astype(np.float32)

    def ref(d):
        dx, dA = R.graph_aggregate_backward(t(A, d), t(x[:, :F], d).view(B, N, F), t(dy, d).view(B, N, lddy), F)
        return dx.reshape(B * N, F), dA, t(dX0[:, :F], d) + dx.reshape(B * N, F)

    (dx64, dA64, acc64), (dx32, dA32, acc32) = both(ref)
    Ad, xd, dyd = dev(A), dev(x), dev(dy)
    for accumulate in (0, 1):
        dX = torch.full((B * N, lddx), -7.0, device=DEV) if accumulate == 0 else dev(dX0)
        keep = dX[:, F:].clone()
        dA = torch.full((B, N, N), -7.0, device=DEV)
        _lib.call("mft_graph_aggregate_backward", ops._p(Ad), ops._p(xd), ldx, ops._p(dyd), lddy, ops._p(dX), lddx, ops._p(dA), B, N, F,
                  accumulate, ops._stream())
        held("mft_graph_aggregate_backward", "dA", dA, dA64, dA32)
        if accumulate:
            held("mft_graph_aggregate_backward", "dX (accumulated)", dX[:, :F], acc64, acc32)
        else:
            held("mft_graph_aggregate_backward", "dX (overwritten)", dX[:, :F], dx64, dx32)
        assert torch.equal(dX[:, F:], keep)


# ================================================================================================ mft_build_graph_nodes(_backward)

@pytest.mark.parametrize("n_way,ns,nq,episodes,fold", [(2, 1, 1, 1, 0), (5, 5, 16, 1, 0), (17, 1, 4, 2, 0), (32, 1, 2, 1, 0), (5, 25, 16, 1, 1),
                                                       (3, 2, 3, 2, 1)])
def test_build_graph_nodes_forward_backward_and_adjoint(n_way, ns, nq, episodes, fold):
    rs = np.random.RandomState(100 * n_way + 10 * ns + nq + fold)
    zf, ld = 128, 256
    S = 2 * ns if fold else ns
    z = rs.standard_normal((episodes * n_way * (S + nq), zf)).astype(np.float32)
    nodes = ops.build_graph_nodes(dev(z), episodes, n_way, ns, nq, ld=ld, fold=bool(fold))
    want = R.build_graph_nodes(t(z, F32), episodes, n_way, ns, nq, fold)        # (0.5 * (a + b) in float32: the kernel's own two operations)
    assert torch.equal(nodes[:, :zf + n_way].cpu(), want)
    assert bool((nodes[:, zf + n_way:] == 0).all())
    rows = nodes.shape[0]
    g = rs.standard_normal((rows, ld)).astype(np.float32)
    dz = torch.full((z.shape[0] + 1, zf), -7.0, device=DEV)
    gd = dev(g)
    _lib.call("mft_build_graph_nodes_backward", ops._p(gd), ld, ops._p(dz), zf, episodes, n_way, ns, nq, fold, ops._stream())
    assert bool((dz[-1] == -7.0).all())
    dz = dz[:-1]
    r64, r32 = both(lambda d: R.build_graph_nodes_backward(t(g, d), zf, episodes, n_way, ns, nq, fold))
    held("mft_build_graph_nodes_backward", "dz", dz, r64, r32)
    # <build(z), g> = <z, build_backward(g)> over the feature columns (the label columns do not depend on z), in float64
    lhs = nodes[:, :zf].cpu().double() * t(g[:, :zf], F64)
    rhs = t(z, F64) * dz.cpu().double()
    lhs32 = want[:, :zf].double() * t(g[:, :zf], F64)
    rhs32 = t(z, F64) * r32.double()
    den = float(lhs.abs().sum())
    err, yard = abs(float(lhs.sum() - rhs.sum())) / den, abs(float(lhs32.sum() - rhs32.sum())) / den
    print("build_graph_nodes adjoint: %.3e (float32 chain %.3e)" % (err, yard))
    assert err <= max(4.0 * yard, R.FLOOR), (err, yard)


# ================================================================================================ mft_act_backward

@pytest.mark.parametrize("C", [48, 50])
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("act", [ops.ACT_NONE, ops.ACT_RELU, ops.ACT_LRELU])
def test_act_backward_through_the_wrapper(act, accumulate, C):
    """Offsets into 256-wide buffers; y exactly 0 takes the negative-side slope; without accumulation the result is a selection
    (one float32 product at most): array-equal."""
    rs = np.random.RandomState(10 * act + accumulate + C)
    rows, dy_off, y_off, dx_off = 333, 133, 7, 65
    dy, y, dx0 = (rs.standard_normal((rows, 256)).astype(np.float32) for _ in range(3))
    y[rs.uniform(size=y.shape) < 0.2] = 0.0
    assert (y[:, y_off:y_off + C] == 0).sum() > 100
    neg = {ops.ACT_NONE: np.float32(1), ops.ACT_RELU: np.float32(0), ops.ACT_LRELU: SLOPE32}[act]
    fac = np.where(y[:, y_off:y_off + C] > 0, np.float32(1), neg).astype(np.float32)
    dx = dev(dx0)
    FB.act_backward(dev(dy), dev(y), dx, C, act, bool(accumulate), dy_off=dy_off, y_off=y_off, dx_off=dx_off)
    got = dx.cpu().numpy()
    sel = dy[:, dy_off:dy_off + C] * fac
    if accumulate:
        r64, r32 = both(lambda d: t(dx0[:, dx_off:dx_off + C], d) + t(dy[:, dy_off:dy_off + C], d) * t(fac, d))
        held("mft_act_backward", "dx (accumulated)", dx[:, dx_off:dx_off + C], r64, r32)
    else:
        assert np.array_equal(got[:, dx_off:dx_off + C], sel)
    keep = np.ones(256, dtype=bool)
    keep[dx_off:dx_off + C] = False
    assert np.array_equal(got[:, keep], dx0[:, keep])


# ================================================================================================ mft_bn_backward_act through FB.bn_bwd

@pytest.mark.parametrize("hook", [None, 11000])
@pytest.mark.parametrize("rpg", [4, 34, 480, 600])
@pytest.mark.parametrize("groups", [1, 2, 4])
@pytest.mark.parametrize("C", [48, 128])
def test_bn_bwd_as_the_head_calls_it(C, groups, rpg, hook):
    """No activation, lease=None, dbias_zero: C = 48 in a 64-wide buffer (Gconv's BatchNorm1d: padding columns of dx exactly 0) and
    C = 128 (fc.1); the one-launch route (up to 512 rows per group and 1,024 in all), the three-launch route above, and the
    three-launch route everywhere (test hook 11000)."""
    rs = np.random.RandomState(C + 1000 * groups + rpg)
    ld = ops.round_up(C, 64)
    rows = groups * rpg
    x = np.zeros((rows, ld), dtype=np.float32)
    xv = rs.standard_normal((groups, rpg, C)) * (1.0 + 0.6 * np.arange(groups)).reshape(-1, 1, 1) + 0.4 * np.arange(groups).reshape(-1, 1, 1)
    x[:, :C] = xv.reshape(rows, C).astype(np.float32)
    dy = np.zeros((rows, ld), dtype=np.float32)
    dy[:, :C] = rs.standard_normal((rows, C)).astype(np.float32)
    gamma = rs.uniform(0.5, 1.5, (C,)).astype(np.float32)
    x64 = x[:, :C].astype(np.float64).reshape(groups, rpg, C)
    mean = x64.mean(1).astype(np.float32)
    rstd = (1.0 / np.sqrt(x64.var(1) + 1e-5)).astype(np.float32)
    if hook is not None:
        assert _lib.lib().mft_debug_set_conv_tile(hook) == 0
    dbz = torch.full((C,), 5.0, device=DEV)
    dx, dg, db = FB.bn_bwd(dev(x), dev(dy), C, rows, dev(mean), dev(rstd), dev(gamma), lease=None, groups=groups, dbias_zero=dbz)
    _lib.lib().mft_debug_reset()

    def ref(d):
        return R.bn_backward(t(x[:, :C], d).view(groups, rpg, C), t(dy[:, :C], d).view(groups, rpg, C), t(mean, d), t(rstd, d), t(gamma, d))

    (dx64, dg64, db64), (dx32, dg32, db32) = both(ref)
    assert tuple(dx.shape) == (rows, ld)
    held("mft_bn_backward_act", "dx", dx[:, :C], dx64.reshape(rows, C), dx32.reshape(rows, C))
    held("mft_bn_backward_act", "dgamma", dg, dg64, dg32)
    held("mft_bn_backward_act", "dbeta", db, db64, db32)
    assert bool((dx[:, C:] == 0).all())
    assert bool((dbz == 0).all())


# ================================================================================================ the exported launchers without a caller

@pytest.mark.parametrize("N", [7, 65])
def test_masked_softmax_backward_and_second_route(N):
    """mft_masked_softmax_backward against the full reference; merged, it is a second route to mft_pair_softmax_ut_backward."""
    rs = np.random.RandomState(N)
    B = 2
    A = softmax_A(rs, B, N)
    dA = rs.standard_normal((B, N, N)).astype(np.float32)
    ds = torch.full((B * N * N + 1,), -7.0, device=DEV)
    Ad, dAd = dev(A), dev(dA)
    _lib.call("mft_masked_softmax_backward", ops._p(Ad), ops._p(dAd), ops._p(ds), 1, B, N, ops._stream())
    assert float(ds[-1]) == -7.0
    ds = ds[:-1].view(B, N, N)
    r64, r32 = both(lambda d: R.softmax_backward_full(t(A, d), t(dA, d)))
    held("mft_masked_softmax_backward", "ds", ds, r64, r32)
    ut, _ = run_softmax_ut(A, dA, 1)
    m64, m32 = both(lambda d: R.softmax_backward_merged(t(A, d), t(dA, d)).reshape(-1))
    merged = R.merge_full(ds.cpu().double().unsqueeze(-1), N).reshape(-1)
    held("mft_masked_softmax_backward", "merged against the float64 merged form", merged, m64, m32)
    agree("mft_masked_softmax_backward", "merged against the upper-triangle launcher", merged, ut[:, 0], m64, m32)


@pytest.mark.parametrize("N", [7, 65])
def test_pair_absdiff_backward_and_second_route(N):
    """mft_pair_absdiff_backward (per-position dd) against the full reference; mft_pair_dx_gather on the rows merged in float32 --
    the same two-term sum the kernel forms -- is the second route."""
    rs = np.random.RandomState(N + 1)
    B, F = 2, 133
    P = N * (N + 1) // 2
    Kp = ops.round_up(F, 32)
    x = tied_nodes(rs, B, N, F)
    dd = rs.standard_normal((B, N, N, Kp)).astype(np.float32)
    dX0 = rs.standard_normal((B * N, 256)).astype(np.float32)
    dX = dev(dX0)
    xd, ddd = dev(x), dev(dd)
    _lib.call("mft_pair_absdiff_backward", ops._p(xd), 256, ops._p(ddd), Kp, ops._p(dX), 256, B, N, F, ops._stream())
    r64, r32 = both(lambda d: t(dX0[:, :F], d) + R.absdiff_backward_full(t(x[:, :F], d).view(B, N, F), t(dd[..., :F], d)).reshape(B * N, F))
    held("mft_pair_absdiff_backward", "dX", dX[:, :F], r64, r32)
    assert np.array_equal(dX[:, F:].cpu().numpy(), dX0[:, F:])
    i, j = np.triu_indices(N)
    dd_ut = (dd[:, i, j] + dd[:, j, i]).astype(np.float32).reshape(B * P, Kp)
    ut = run_dx_gather(dev(x), dd_ut, dX0, B, N, F, [(0, B * P)])
    agree("mft_pair_absdiff_backward", "against mft_pair_dx_gather on merged rows", ut[:, :F], dX[:, :F], r64, r32)


# ================================================================================================ wcompute_taped -> wcompute_backward

CHAIN_SHAPES = [(7, 133, 6, 2), (30, 181, 4, 2), (13, 229, 3, 1), (33, 160, 2, 1), (64, 256, 2, 1)]
# per shape the first input seed at which no element of the device's tape, in either form of the layers, lies in the band where
# a float32 evaluation of z * scale + shift could take the other sign (found on the device by scanning seeds 0, 1, ...)
CHAIN_SEEDS = {(7, 133, 6, 2): 0, (30, 181, 4, 2): 0, (13, 229, 3, 1): 0, (33, 160, 2, 1): 0, (64, 256, 2, 1): 4}
WAYS = [(1 << 30, None, False), (0, 100, False), (1 << 30, 100, True), (0, None, True)]      # (PAIR_RK_ROWS, PAIR_CHUNK_ROWS, WgradBatch)
_heads = {}


def chain_head(F):
    n_way, name = {133: (5, "layer_w0"), 181: (5, "layer_w1"), 229: (5, "w_comp_last"), 160: (32, "layer_w0"), 256: (32, "w_comp_last")}[F]
    if n_way not in _heads:
        sd = synthetic.gnn_head_state_dict(seed=5, n_way=n_way)
        _heads[n_way] = (sd, Fn.GnnHeadWeights(sd, DEV, n_way))
    return _heads[n_way] + (name, n_way)


def chain_inputs(shape, seed):
    N, F, B, groups = shape
    rs = np.random.RandomState(1000 * seed + N + F)
    n_way = chain_head(F)[3]
    x = tied_nodes(rs, B, N, F, n_way=n_way)
    x.reshape(B, N, 256)[B // groups:, :, :F - n_way] *= 1.7               # later episodes: other statistics
    dA = rs.standard_normal((B, N, N)).astype(np.float32)
    return x, dA, rs


def tape_band_count(tape):
    """Elements of the tape with |z * scale + shift| <= 2^-21 (|z * scale| + |shift|), evaluated in float64."""
    n = 0
    groups = tape["groups"]
    for z, (sc, sh, _, _) in zip(tape["z"], tape["bn"]):
        C = z.shape[1]
        zs = z.double().view(groups, -1, C) * sc.double().view(groups, 1, C)
        sh = sh.double().view(groups, 1, C)
        n += int(((zs + sh).abs() <= 2.0 ** -21 * (zs.abs() + sh.abs())).sum())
    return n


@pytest.mark.parametrize("way", range(4))
@pytest.mark.parametrize("shape", CHAIN_SHAPES, ids=lambda s: "N%d-F%d-B%d-g%d" % s)
def test_wcompute_chain_against_float64_on_the_device_tape(shape, way, monkeypatch):
    N, F, B, groups = shape
    rk_rows, chunk, batched = WAYS[way]
    sd, G, name, n_way = chain_head(F)
    x, dA, rs = chain_inputs(shape, CHAIN_SEEDS[shape])
    monkeypatch.setattr(FB, "PAIR_RK_ROWS", rk_rows)
    if chunk is not None:
        monkeypatch.setattr(FB, "PAIR_CHUNK_ROWS", chunk)
    P = N * (N + 1) // 2
    xd, dAd = dev(x), dev(dA)
    A, tape = FB.wcompute_taped(G, name, xd, F, B, N, groups)
    tape["lease"] = FB.ZeroLease()
    assert tape_band_count(tape) == 0                 # inside the band an fp32 evaluation could decide either way: asserted, not skipped
    pre = "gnn." + name

    def ref(d):
        z = [v.cpu().to(d) for v in tape["z"]]
        bn = [tuple(v.cpu().to(d) for v in b) for b in tape["bn"]]
        masks = []
        for v, b in zip(tape["z"], tape["bn"]):
            C = v.shape[1]
            y = v.cpu().double().view(groups, -1, C) * b[0].cpu().double().view(groups, 1, C) + b[1].cpu().double().view(groups, 1, C)
            masks.append((y > 0).view(-1, C))
        ws = [sd["%s.conv2d_%d.weight" % (pre, li)].to(d).view(R.WC_CH[li - 1], -1) for li in range(1, 5)]
        gam = [sd["%s.bn_%d.weight" % (pre, li)].to(d) for li in range(1, 5)]
        dx, grads = R.wcompute_backward_from_tape(t(x[:, :F], d).view(B, N, F), z, bn, tape["A"].cpu().to(d), t(dA, d), ws, gam,
                                                  sd[pre + ".conv2d_last.weight"].to(d).view(96), masks, groups)
        return dx.reshape(B * N, F), grads

    (dx64, g64), (dx32, g32) = both(ref)
    dX0 = (rs.standard_normal((B * N, 256)) * float(dx64.abs().max())).astype(np.float32)      # dX accumulates: values of dx's own size
    outs = []
    for _ in range(2):
        dX, grads = dev(dX0), {}
        wb = ops.WgradBatch(True) if batched else None
        FB.wcompute_backward(G, tape, dAd, xd, dX, B, N, grads, pre, wb=wb)
        if wb is not None:
            wb.flush()
        torch.cuda.synchronize()
        outs.append((dX, grads))
    dX, grads = outs[0]
    tag = "chain (rk)" if rk_rows else "chain (tile)"
    held(tag, "dX", dX[:, :F], t(dX0[:, :F], F64) + dx64, t(dX0[:, :F], F32) + dx32)
    assert np.array_equal(dX[:, F:].cpu().numpy(), dX0[:, F:])
    assert sorted(grads) == sorted(pre + "." + k for k in g64)
    for k in sorted(g64):
        got = grads[pre + "." + k]
        assert tuple(got.shape) == tuple(g64[k].shape), k
        if k.startswith("conv2d") and k.endswith(".bias"):
            assert bool((got == 0).all()), k
        else:
            held(tag, k, got, g64[k], g32[k])
    assert torch.equal(outs[1][0], dX)                 # a second run is bit-identical
    for k, v in grads.items():
        assert torch.equal(outs[1][1][k], v), k
