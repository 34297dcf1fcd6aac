"""Why the tolerance of tests/test_loss_optim_gpu.py can tell the two ways of writing a float32 log-sum-exp apart -- no GPU.

A softmax probability is exp(x - lse).  Forming lse = mx + log(se) first rounds it to ulp(|mx|), so the probabilities (and the
loss lse - x[y]) lose accuracy in proportion to the size of the logits; (x - mx) - log(se) keeps both terms small and does
not.  A float32 numpy emulation of each form (exact exp / log, rounded to float32 after every operation) is measured against
float64 over the range cases the GPU file uses, next to float32 torch (`e32`), and the GPU file's bound max(4 * e32, 3e-7)
must admit the shifted form everywhere and reject the mx + log(se) form wherever the logits are large.

This module also holds the inputs, labels and float64 / float32 references the GPU file shares."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

# (offset, scale) of scale * N(0, 1) + offset; "shift" = logits quantised to multiples of 2^-10 in [-8, 8] plus 1024 (exact in
# float32), compared against the float64 result of the UNSHIFTED logits (softmax and cross entropy are shift invariant)
RANGES = [(0, 3), (0, 30), (1000, 3), (-1000, 3), (-3000, 300), "shift"]
LARGE = [(1000, 3), (-1000, 3), (-3000, 300)]           # where the mx + log(se) form must exceed the bound
SHIFT = 1024.0


def range_id(rng):
    return rng if isinstance(rng, str) else "off%g_scale%g" % rng


def tol(e32):
    """The bound on an unscaled probability / gradient error: 4 x what float32 torch does on the same input, never below 3e-7."""
    return max(4.0 * e32, 3e-7)


def make_logits(rng, rows, C, seed):
    """-> (float32 logits as the kernel gets them, float64 logits the reference uses)."""
    n = np.random.RandomState(seed).standard_normal((rows, C))
    if rng == "shift":
        q = np.clip(np.round(n * 3 * 1024) / 1024, -8, 8)
        x = torch.from_numpy((q + SHIFT).astype(np.float32))
        assert torch.equal(x.double(), torch.from_numpy(q) + SHIFT)       # the shift is exact
        return x, torch.from_numpy(q)
    off, scale = rng
    x = torch.from_numpy((n * scale + off).astype(np.float32))
    return x, x.double()


def make_labels(rows, C, seed):
    """Label vectors (int64) that name both class 0 and class C-1: one vector, or -- a single row cannot hold both -- two."""
    y = np.random.RandomState(seed).randint(0, C, size=rows)
    if rows == 1:
        return [torch.tensor([c]) for c in sorted({0, C - 1})]
    y[np.random.RandomState(seed + 1).permutation(rows)[:2]] = [0, C - 1]
    return [torch.from_numpy(y)]


def ce_ref(x, y):
    """Per-row cross entropy and its unscaled gradient softmax - onehot, in x's dtype on the CPU."""
    xa = x.clone().requires_grad_(True)
    rl = F.cross_entropy(xa, y, reduction="none")
    d, = torch.autograd.grad(rl.sum(), xa)
    return rl.detach(), d


def ce_refs(x, x64, y):
    """-> (float64 per-row loss, float64 unscaled gradient, e32 = float32 torch's max gradient error against it)."""
    rl, d = ce_ref(x64, y)
    _, d32 = ce_ref(x, y)
    return rl, d, float((d32.double() - d).abs().max())


# ------------------------------------------------------------------------------------- the two forms, emulated in float32

def _f32(a):
    return np.asarray(a, dtype=np.float32)


def emulate(x, y, shifted):
    """One kernel row pass in float32: every + - and every exp / log result is rounded to float32; exp and log themselves are
    exact (float64), so what is measured is the form, not an approximation of the transcendental functions."""
    x = _f32(x.numpy())
    rows, C = x.shape
    mx = x.max(1, keepdims=True)
    sh = _f32(x - mx)
    e = _f32(np.exp(sh.astype(np.float64)))
    part = np.zeros((rows, 64), np.float32)       # the kernels' order: lane l sums classes l, l + 64, ...; then a tree over the wave
    for c in range(C):
        part[:, c % 64] = _f32(part[:, c % 64] + e[:, c])
    w = 64
    while w > 1:
        w //= 2
        part = _f32(part[:, :w] + part[:, w:2 * w])
    se = part
    lg = _f32(np.log(se.astype(np.float64)))
    xy = x[np.arange(rows), y.numpy()][:, None]
    if shifted:
        p = _f32(np.exp(_f32(sh - lg).astype(np.float64)))
        loss = _f32(lg - _f32(xy - mx))
    else:
        lse = _f32(mx + lg)
        p = _f32(np.exp(_f32(x - lse).astype(np.float64)))
        loss = _f32(lse - xy)
    onehot = np.zeros_like(x)
    onehot[np.arange(rows), y.numpy()] = 1.0
    return torch.from_numpy(loss[:, 0]), torch.from_numpy(_f32(p - onehot))


@pytest.mark.parametrize("C", [5, 64, 200])
@pytest.mark.parametrize("rng", RANGES, ids=range_id)
def test_bound_admits_shifted_form_and_rejects_max_plus_log_form(rng, C):
    rows = 64
    x, x64 = make_logits(rng, rows, C, 100 + C)
    y = make_labels(rows, C, 200 + C)[0]
    rl, d, e32 = ce_refs(x, x64, y)
    err = {}
    for shifted in (True, False):
        l, g = emulate(x, y, shifted)
        err[shifted] = float((g.double() - d).abs().max())
        if shifted:
            assert float(((l.double() - rl).abs() / rl.abs().clamp(min=1.0)).max()) <= 2e-6
    print("%s C=%d: shifted %.2e, mx+log(se) %.2e, e32 %.2e, bound %.2e" % (range_id(rng), C, err[True], err[False], e32, tol(e32)))
    assert e32 < 1e-6                       # a cap on the yardstick: the bound can never grow to where it admits the old form
    assert err[True] <= tol(e32)
    if rng in LARGE:
        assert err[False] > tol(e32)
