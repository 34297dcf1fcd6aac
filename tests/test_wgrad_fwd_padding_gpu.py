"""csrc/wgrad_fwd.hip at the edges of its addressing: taps that leave the image, rows beyond the episode, the last K tile.

The walker requests every operand with a range-checked buffer load: a padding tap, a row beyond the episode's pixels and a
request for a tile after the last one are all "addresses past the end of the buffer" that come back as zeros.  These tests run
the smallest shapes the launcher accepts (Cin a multiple of 128, Cout a multiple of 32, <= 48 rows, <= 8 images per episode)
with every operand placed inside a larger allocation filled with NaN: a request that reaches a neighbour instead of the zeros
shows up as a NaN or as a bit that differs from the plain launcher, a store that strays shows up in the guard bands.  `-m gpu`
only."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import meta_fine_tuning_amd  # noqa: F401
from meta_fine_tuning_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 8192                      # floats of NaN on either side of every operand (a multiple of 4: the operand stays 16-byte aligned)
NAN_BITS = 0x7FC00000

# name, Cin, k, stride, pad, H   (all: 3 x 3 output pixels per image)
LAYERS = [
    ("3x3s1p1_H3_c128", 128, 3, 1, 1, 3),        # every tap but the centre leaves the image somewhere; 9 K tiles (odd)
    ("3x3s1p1_H3_c256", 256, 3, 1, 1, 3),        # two input-channel tiles per tap; 18 K tiles
    ("3x3s2p1_H6_c128", 128, 3, 2, 1, 6),
    ("1x1s2p0_H6_c128", 128, 1, 2, 0, 6),        # a single K tile: no next tile at all
]
MODES = [ops.WF_RAW, ops.WF_ENTRY, ops.WF_EXIT]


def rnd(shape, seed, scale=1.0):
    return torch.from_numpy((np.random.RandomState(seed).standard_normal(shape) * scale).astype(np.float32))


def guarded(t):
    """A contiguous device copy of ``t`` in the middle of an allocation whose remainder is NaN: (view, whole allocation)."""
    buf = torch.full((t.numel() + 2 * GUARD,), float("nan"), device=DEV)
    view = buf[GUARD:GUARD + t.numel()].view(t.shape)
    view.copy_(t)
    return view, buf


def guards_intact(buf):
    bits = buf.view(torch.int32)
    return bool((bits[:GUARD] == NAN_BITS).all()) and bool((bits[-GUARD:] == NAN_BITS).all())


class Case:
    """One layer x episode shape: host operands (generated once) and the plain launcher's result per epilogue form."""

    def __init__(self, Cin, Cout, k, stride, pad, H, G, ipg, seed):
        self.Cin, self.Cout, self.k, self.stride, self.pad, self.H, self.G, self.ipg = Cin, Cout, k, stride, pad, H, G, ipg
        self.OH = (H + 2 * pad - k) // stride + 1
        self.rows = ipg * self.OH * self.OH
        n, K = G * ipg, k * k * Cin
        self.n, self.K = n, K
        self.x = rnd((n, H, H, Cin), seed + 1)                            # NHWC
        self.xn = rnd((n, H, H, Cin), seed + 2)
        self.dy = rnd((n, self.OH, self.OH, Cout), seed + 3) * 1e-2
        self.w = rnd((G, Cout, K), seed + 4, scale=0.02)                  # packed [Cout][kh][kw][ci]
        self.m = rnd((G, Cout, K), seed + 5) * 1e-3
        self.v = rnd((G, Cout, K), seed + 6).abs() * 1e-6
        self.gam, self.bet = 1.0 + 0.1 * rnd((G, Cout), seed + 7), 0.1 * rnd((G, Cout), seed + 8)
        self.gas, self.bes = 1.0 + 0.1 * rnd((G, Cout), seed + 9), 0.1 * rnd((G, Cout), seed + 10)
        self.sc = rnd((G * self.rows, Cout), seed + 11)                   # the shortcut branch's raw output (EXIT reads it)
        self._plain = {}

    def plain(self, lib, exact):
        """(w, m, v, dw) of ops.conv2d_wgrad_adam on identical copies.  That launcher takes output channels in multiples of 64
        and works on them in independent tiles of 32 (as the walker does), so 32 channels run as the first of two identical tiles."""
        if exact not in self._plain:
            rep = 1 if self.Cout % 64 == 0 else 2
            C = self.Cout * rep
            w, m, v = (t.repeat(1, rep, 1).to(DEV) for t in (self.w, self.m, self.v))
            dy = self.dy.repeat(1, 1, 1, rep).to(DEV)
            dw = torch.zeros_like(w)
            lib.mft_debug_reset()
            if exact:
                lib.mft_debug_set_conv_tile(9003)
            ops.conv2d_wgrad_adam(self.x.to(DEV), dy, w, m, v, C, self.k, self.k, self.stride, self.pad, 7, imgs_per_group=self.ipg, dw=dw)
            lib.mft_debug_reset()
            self._plain[exact] = tuple(t[:, :self.Cout].contiguous() for t in (w, m, v, dw))
        return self._plain[exact]

    def launch(self, lib, mode, exact, fwd=True, with_dw=True):
        """The fused launch on fresh guarded copies; returns every tensor it could have touched."""
        lib.mft_wgrad_fwd_set_exact(exact)
        o = {}
        for name in ("x", "xn", "dy", "w", "m", "v"):
            o[name], o[name + "_buf"] = guarded(getattr(self, name))
        if with_dw:
            o["dw"], o["dw_buf"] = guarded(torch.zeros_like(self.w))
        kw = {}
        if fwd:
            nan = lambda *s: torch.full(s, float("nan"), device=DEV)      # noqa: E731
            o["raw"] = nan(self.n * self.OH * self.OH, self.Cout)
            kw.update(x_next=o["xn"], mode=mode, raw=o["raw"])
            if mode != ops.WF_RAW:
                o["act"], o["mean"], o["rstd"] = nan(*o["raw"].shape), nan(self.G, self.Cout), nan(self.G, self.Cout)
                kw.update(act=o["act"], gamma=self.gam.to(DEV), beta=self.bet.to(DEV), gbs=self.Cout, mean=o["mean"], rstd=o["rstd"])
            if mode == ops.WF_EXIT:
                o["means"], o["rstds"], o["pooled"] = nan(self.G, self.Cout), nan(self.G, self.Cout), nan(self.n, self.Cout)
                kw.update(sc_raw=self.sc.to(DEV), gamma_s=self.gas.to(DEV), beta_s=self.bes.to(DEV), mean_s=o["means"], rstd_s=o["rstds"],
                          pooled=o["pooled"])
        assert ops.wgrad_adam_next_forward(o["x"], o["dy"], o["w"], o["m"], o["v"], self.k, self.k, self.stride, self.pad, 7, self.ipg,
                                           dw=o.get("dw"), **kw)
        torch.cuda.synchronize()
        lib.mft_wgrad_fwd_set_exact(0)
        return o

    def check_update(self, o, ref, tag):
        wr, mr, vr, dwr = ref
        assert torch.equal(o["w"], wr) and torch.equal(o["m"], mr) and torch.equal(o["v"], vr), tag
        if "dw" in o:
            assert torch.equal(o["dw"], dwr), tag
        for name in ("x", "xn", "dy", "w", "m", "v", "dw"):
            if name + "_buf" in o:
                assert guards_intact(o[name + "_buf"]), (tag, name)
        assert torch.equal(o["x"].cpu(), self.x) and torch.equal(o["xn"].cpu(), self.xn) and torch.equal(o["dy"].cpu(), self.dy), tag
        for name in ("w", "m", "v", "dw", "raw", "act", "mean", "rstd", "means", "rstds", "pooled"):
            if name in o:
                assert bool(torch.isfinite(o[name]).all()), (tag, name)

    def check_forward(self, o, mode, tag):
        """The next step against float64 on the weights the launch itself produced (tolerances: tests/test_kernels_gpu.py,
        test_wgrad_adam_next_forward_kernel)."""
        G, rows, Cout, Cin, k, ipg = self.G, self.rows, self.Cout, self.Cin, self.k, self.ipg
        eps = ops.BN_EPS
        wg = o["w"].cpu().double().view(G, Cout, k, k, Cin).permute(0, 1, 4, 2, 3)          # OIHW per episode
        xn = self.xn.double().permute(0, 3, 1, 2)
        raw_r = torch.empty((G, rows, Cout), dtype=torch.float64)
        for g in range(G):
            out = F.conv2d(xn[g * ipg:(g + 1) * ipg], wg[g], None, self.stride, self.pad)
            raw_r[g] = out.permute(0, 2, 3, 1).reshape(rows, Cout)
        got = o["raw"].view(G, rows, Cout).cpu().double()
        scale = float(raw_r.abs().max())
        assert float((got - raw_r).abs().max()) <= 3e-6 * scale, (tag, float((got - raw_r).abs().max()), scale)
        if mode == ops.WF_RAW:
            return
        mu = raw_r.mean(1, keepdim=True)
        rs = 1.0 / (raw_r.var(1, unbiased=False, keepdim=True) + eps).sqrt()
        assert float((o["mean"].cpu().double() - mu[:, 0]).abs().max()) <= 3e-6 * scale, tag
        assert float((o["rstd"].cpu().double() / rs[:, 0] - 1).abs().max()) <= 2e-5, tag
        y = (raw_r - mu) * rs * self.gam.double()[:, None] + self.bet.double()[:, None]
        if mode == ops.WF_EXIT:
            sc = self.sc.double().view(G, rows, Cout)
            mus = sc.mean(1, keepdim=True)
            rss = 1.0 / (sc.var(1, unbiased=False, keepdim=True) + eps).sqrt()
            assert float((o["means"].cpu().double() - mus[:, 0]).abs().max()) <= 3e-6 * float(sc.abs().max()), tag
            assert float((o["rstds"].cpu().double() / rss[:, 0] - 1).abs().max()) <= 2e-5, tag
            y = y + (sc - mus) * rss * self.gas.double()[:, None] + self.bes.double()[:, None]
        y = y.clamp_min(0)
        assert float((o["act"].view(G, rows, Cout).cpu().double() - y).abs().max()) <= 2e-5 * max(float(y.abs().max()), 1.0), tag
        if mode == ops.WF_EXIT:
            pr = y.view(G, ipg, self.OH * self.OH, Cout).mean(2).reshape(self.n, Cout)
            assert float((o["pooled"].cpu().double() - pr).abs().max()) <= 2e-5 * max(float(pr.abs().max()), 1.0), tag


@pytest.mark.parametrize("ipg", [1, 3, 5])                 # 9 rows (most of the 48-row tile is beyond the episode), 27 (NT = 16), 45 (NT = 24)
@pytest.mark.parametrize("name,Cin,k,stride,pad,H", LAYERS)
def test_walker_padding_rows_and_guard_bands(name, Cin, k, stride, pad, H, ipg):
    """All three modes x Cout 32 / 64 x 1, 3 (natural workgroup order) and 8 (XCD-remapped) episodes x fast / exact epilogue:
    w, m, v, dw bit-identical to the plain launcher, all outputs finite, NaN guard bands and inputs untouched, the next step's
    forward against float64; and the launch without a next step gives the same update."""
    from meta_fine_tuning_amd import _lib
    lib = _lib.lib()
    for Cout in (32, 64):
        for G in (1, 3, 8):
            case = Case(Cin, Cout, k, stride, pad, H, G, ipg, seed=1000 + 10 * G + Cout)
            for exact in (0, 1):
                ref = case.plain(lib, exact)
                assert not torch.equal(ref[0].cpu(), case.w)
                for mode in MODES:
                    tag = (name, ipg, Cout, G, exact, mode)
                    o = case.launch(lib, mode, exact)
                    case.check_update(o, ref, tag)
                    case.check_forward(o, mode, tag)
                # the last inner step: no next step, no gradient output -- the same update and nothing else written
                o = case.launch(lib, ops.WF_RAW, exact, fwd=False, with_dw=False)
                case.check_update(o, ref, (name, ipg, Cout, G, exact, "no next step"))


@pytest.mark.parametrize("name,Cin,k,stride,pad,H", [LAYERS[0], LAYERS[2]])
def test_walker_repeat_launch_gives_identical_bits(name, Cin, k, stride, pad, H):
    """The same launch twice in a row on fresh copies, and once more after an unrelated launch of another mode and shape: identical
    bits in every output.  Whatever supplies the zeros of the padding taps is never written."""
    from meta_fine_tuning_amd import _lib
    lib = _lib.lib()
    case = Case(Cin, 64, k, stride, pad, H, 3, 3, seed=2000)
    other = Case(128, 32, 1, 2, 0, 6, 8, 5, seed=2100)
    keys = ("w", "m", "v", "dw", "raw", "act", "mean", "rstd", "means", "rstds", "pooled")
    a = case.launch(lib, ops.WF_EXIT, 0)
    b = case.launch(lib, ops.WF_EXIT, 0)
    other.launch(lib, ops.WF_ENTRY, 0)
    c = case.launch(lib, ops.WF_EXIT, 0)
    for key in keys:
        assert torch.equal(a[key], b[key]) and torch.equal(a[key], c[key]), key
        assert bool(torch.isfinite(a[key]).all()), key
    case.check_update(c, case.plain(lib, 0), name)
