"""Tensor-level wrappers over the C-ABI kernels (include/mft_hip.h).

PyTorch is plumbing here: it owns device memory (caching allocator) and the
current HIP stream; every arithmetic op is a launch into libmft_hip.so.  All
activations are NHWC fp32 CUDA tensors.  Nothing in this module falls back to
torch math: a CPU tensor or a missing library raises.
"""
import ctypes
import os

import torch

from . import _lib
from . import settings

ACT_NONE, ACT_RELU, ACT_LRELU = 0, 1, 2
BN_EPS = 1e-5
LRELU_SLOPE = 0.01


import threading

_tls = threading.local()      # per host thread: the device of the pointer arguments marshalled for the launch being assembled


def _stream(t=None):
    """The current HIP stream of the device THIS launch's tensors live on.  ``t``: a tensor / torch.device / index names the
    device explicitly; without it the device is the one the ``_p()`` calls of the same argument list saw (Python evaluates
    arguments left to right and every launcher takes the stream last).  The record is per host thread and is consumed here, so
    it can neither leak into a later launch nor be overwritten by another thread's engine on another device; a launch whose
    pointer arguments sit on two devices raises."""
    dev = getattr(_tls, "dev", None)
    _tls.dev = None
    if t is not None:
        dev = t.device.index if torch.is_tensor(t) else (t.index if isinstance(t, torch.device) else int(t))
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _p(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("meta_fine_tuning_amd ops need CUDA (HIP) tensors; got a CPU tensor (no CPU fallback)")
    prev = getattr(_tls, "dev", None)
    if prev is not None and prev != t.device.index and getattr(_tls, "strict", True):
        _tls.dev = None
        raise RuntimeError("one launch got pointers on cuda:%d and cuda:%d" % (prev, t.device.index))
    _tls.dev = t.device.index
    return ctypes.c_void_p(t.data_ptr())


def _f32c(t):
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise RuntimeError("expected a contiguous float32 tensor, got %s contiguous=%s" % (t.dtype, t.is_contiguous()))
    return t


def round_up(a, b):
    return (a + b - 1) // b * b


# ------------------------------------------------------------------------------------ layout

def nchw_to_nhwc(x):
    """[n,C,H,W] -> [n,H,W,C] (boundary ingest)."""
    _f32c(x)
    n, C, H, W = x.shape
    y = torch.empty((n, H, W, C), device=x.device, dtype=torch.float32)
    _lib.call("mft_nchw_to_nhwc", _p(x), _p(y), n, C, H, W, _stream())
    return y


def pack_conv_weight(w, rows32=False):
    """OIHW (or [out,in] Linear) -> packed [Cout, roundup(KH*KW*Cin,32)].  ``rows32``: the pack lives in a buffer whose row count is
    rounded up to 32 with zero rows (``pk.rows32``: that buffer) -- the operand the data-gradient launch wants when Cout % 32 != 0
    (the reduction runs over Cout); a refresh through PackPlan rewrites the Cout real rows only, the padding stays zero."""
    if w.dim() == 2:
        w = w.view(w.shape[0], w.shape[1], 1, 1)
    w = _f32c(w.detach())
    Cout, Cin, KH, KW = w.shape
    kpad = round_up(KH * KW * Cin, 32)
    if rows32 and Cout % 32 != 0:
        buf = torch.zeros((round_up(Cout, 32), kpad), device=w.device, dtype=torch.float32)
        pk = buf[:Cout]
        pk.rows32 = buf
    else:
        pk = torch.empty((Cout, kpad), device=w.device, dtype=torch.float32)
    _lib.call("mft_pack_oihw", _p(w), _p(pk), Cout, Cin, KH, KW, kpad, _stream())
    return pk


class PackPlan:
    """The OIHW -> packed copies of a set of live parameters as ONE launch (mft_pack_oihw_multi): ``add`` registers
    (source parameter, packed destination) pairs -- both must stay where they are --, ``run`` refreshes every destination."""

    def __init__(self):
        self.jobs, self.total, self.table, self.keep = [], 0, None, []

    def add(self, w, pk):
        w4 = w if w.dim() == 4 else w.view(w.shape[0], w.shape[1], 1, 1)
        Cout, Cin, KH, KW = w4.shape
        assert w.is_cuda and w.dtype == torch.float32 and w.is_contiguous() and pk.is_contiguous() and pk.shape == (Cout, round_up(KH * KW * Cin, 32))
        self.jobs.append((w.data_ptr(), pk.data_ptr(), Cout, Cin, KH * KW, pk.shape[1], self.total))
        self.total += pk.numel()
        self.keep.append((w, pk))
        self.table = None

    def add_transposed(self, w, pkT):
        """``w`` [Cout, Cin] (or [Cout, Cin, 1, 1]) -> ``pkT`` [rows >= Cin, roundup(Cout, 32)] = W^T zero-padded: the operand with which
        the FORWARD GEMM kernel computes a linear layer's data gradient dx = dy @ W (10-27 % faster per launch than the BT form reading
        the forward pack, bit-identical: tools/gemm_vs_dgrad_1x1.py), refreshed by the same launch as the forward packs."""
        Cout, Cin = w.shape[0], w.shape[1]
        assert w.is_cuda and w.dtype == torch.float32 and w.is_contiguous() and w.numel() == Cout * Cin
        assert pkT.is_contiguous() and pkT.shape[0] >= Cin and pkT.shape[1] == round_up(Cout, 32)
        self.jobs.append((w.data_ptr(), pkT.data_ptr(), Cout, Cin, -1, pkT.shape[1], self.total))
        self.total += pkT.numel()
        self.keep.append((w, pkT))
        self.table = None

    def sources(self):
        return [w for w, _ in self.keep]

    def run(self):
        if not self.jobs:
            return
        if self.table is None:
            import numpy as np
            self.table = torch.from_numpy(np.asarray(self.jobs, dtype=np.int64)).to(self.keep[0][1].device)
        _lib.call("mft_pack_oihw_multi", _p(self.table), len(self.jobs), self.total, _stream())


class SplitPlan:
    """bf16x3 planes of several packed weight matrices refreshed by ONE launch (mft_split_bf16x3_multi): the per-step companion of
    PackPlan for the meta-training layers that run on the split-precision kernels.  ``add(pk, Cout, Cin, taps, transposed)``
    allocates the planes [3, rows, K] (rows, K = Cout, taps*Cin -- or Cin, taps*Cout for the transposed data-gradient operand),
    fills them once and registers the job; ``run()`` refreshes every registered set from its (in-place updated) source."""

    def __init__(self):
        self.jobs, self.total, self.table, self.keep = [], 0, None, []
        self.retired = []          # job tables an earlier recording may still read: kept alive for good

    def add(self, pk, Cout, Cin, taps, transposed=False):
        assert pk.is_cuda and pk.dtype == torch.float32 and pk.is_contiguous() and pk.shape == (Cout, taps * Cin) and (taps * Cin) % 32 == 0
        if torch.cuda.is_current_stream_capturing():
            # a new job uploads a table (a synchronous host-to-device copy) and fills planes outside any recording: the episode
            # loops run three eager steps before they record, so every layer's job exists by then
            raise RuntimeError("SplitPlan.add() under stream capture: run one eager step first (the planes of every layer are "
                               "registered by the first forward)")
        n = pk.numel()
        planes = torch.empty((3, Cin, taps * Cout) if transposed else (3, Cout, taps * Cin), device=pk.device, dtype=torch.int16)
        self.jobs.append((pk.data_ptr(), planes.data_ptr(), n, Cout, Cin, taps, 1 if transposed else 0, self.total))
        self.total += n
        self.keep.append((pk, planes))
        if self.table is not None:
            self.retired.append(self.table)      # a hipGraph recorded before this job existed replays run() with the OLD table: it must
        self.table = None                        # stay valid (it refreshes the jobs that recording uses; the next run() builds the new one)
        self._launch(len(self.jobs) - 1)
        return planes

    def _launch(self, only=None):
        import numpy as np
        if only is not None:                       # a job that has just been added: fill its planes now, alone
            j = list(self.jobs[only])
            j[7] = 0
            tab = torch.from_numpy(np.asarray([j], dtype=np.int64)).to(self.keep[only][0].device)
            _lib.call("mft_split_bf16x3_multi", _p(tab), 1, j[2], _stream())
            return
        if self.table is None:
            self.table = torch.from_numpy(np.asarray(self.jobs, dtype=np.int64)).to(self.keep[0][0].device)
        _lib.call("mft_split_bf16x3_multi", _p(self.table), len(self.jobs), self.total, _stream())

    def run(self):
        if self.jobs:
            self._launch()


def unpack_conv_weight(pk, shape):
    Cout, Cin, KH, KW = shape
    w = torch.empty(shape, device=pk.device, dtype=torch.float32)
    _lib.call("mft_unpack_oihw", _p(pk), _p(w), Cout, Cin, KH, KW, pk.shape[-1], _stream())
    return w


def pack_dgrad_weight(w_pk, Cout, Cin, KH, KW, groups=1):
    """packed fwd weights [groups, Cout, KH*KW*Cin] -> dgrad weights [groups, Cin, KH*KW*Cout]."""
    w_pk = _f32c(w_pk)
    K = KH * KW * Cin
    wt = torch.empty((groups, Cin, KH * KW * Cout), device=w_pk.device, dtype=torch.float32)
    _lib.call("mft_pack_dgrad", _p(w_pk), _p(wt), Cout, Cin, KH, KW, groups, Cout * K, Cin * KH * KW * Cout, _stream())
    return wt


# ------------------------------------------------------------------------------------ conv / gemm

def conv2d(x, w_pk, Cout, KH, KW, stride, pad, imgs_per_group=0, bias=None, out=None):
    """x [n,H,W,Cin] NHWC, w_pk [Cout,Kpad] or [groups,Cout,Kpad] -> [n,OH,OW,Cout]."""
    _f32c(x)
    n, H, W, Cin = x.shape
    OH = (H + 2 * pad - KH) // stride + 1
    OW = (W + 2 * pad - KW) // stride + 1
    if out is None:
        out = torch.empty((n, OH, OW, Cout), device=x.device, dtype=torch.float32)
    wgs = 0
    if w_pk.dim() == 3:
        wgs = w_pk.shape[1] * w_pk.shape[2]
        if imgs_per_group <= 0 or n // imgs_per_group != w_pk.shape[0]:
            raise RuntimeError("per-group weights need imgs_per_group with n/imgs_per_group == groups")
    if ((wgs == 0 and imgs_per_group <= 0) or (w_pk.dim() == 3 and w_pk.shape[0] == 1)) and Cin != 3:        # (one group = one weight set)
        # one weight set, few output tiles, long reduction (one 105-image meta-training episode): K sliced across workgroups
        nws = _ksplit_ws(n * OH * OW, Cout, w_pk.shape[-1])
        if nws:
            ws = torch.empty((nws,), device=x.device, dtype=torch.float32)
            _lib.call("mft_conv2d_nhwc_ksplit", _p(x), Cin, _p(w_pk), _p(bias), _p(out), Cout, n, H, W, Cin, Cout, KH, KW, stride, pad,
                      _p(ws), _stream())
            return out
    if w_pk.dim() == 3 and 1 < w_pk.shape[0] <= SMALL_GROUPS and bias is None and Cin != 3:
        # a few episodes in lockstep: grid.y = episode on the K-sliced implicit GEMM (the weight-streaming kernels need >= 16
        # episodes to fill the GPU)
        G = w_pk.shape[0]
        nws = _ksplit_ws(imgs_per_group * OH * OW, Cout, w_pk.shape[-1], G)
        if nws:
            ws = torch.empty((nws,), device=x.device, dtype=torch.float32)
            _lib.call("mft_conv2d_nhwc_ksplit_grouped", _p(x), Cin, _p(w_pk), _p(out), Cout, n, H, W, Cin, Cout, KH, KW, stride, pad,
                      imgs_per_group, wgs, _p(ws), _stream())
            return out
    _lib.call("mft_conv2d_nhwc", _p(x), Cin, _p(w_pk), _p(bias), _p(out), Cout, n, H, W, Cin, Cout, KH, KW, stride, pad, imgs_per_group,
              wgs, _stream())
    return out


SMALL_GROUPS = settings.current().small_groups     # up to this many per-episode weight sets take the K-sliced GEMM route
_KSPLIT_WS = {}


def _ksplit_ws(rows, cols, K, groups=1):
    """floats of workspace for the K-sliced convolution / data-gradient launch of this shape (0: not sliced); memoised."""
    key = (rows, cols, K, groups)
    v = _KSPLIT_WS.get(key)
    if v is None:
        v = _KSPLIT_WS[key] = int(_lib.lib().mft_conv_ksplit_ws_floats(rows, cols, K) if groups == 1 else
                                  _lib.lib().mft_conv_ksplit_grouped_ws_floats(rows, cols, K, groups))
    return v


def split_weight_x3(w_pk):
    """packed fp32 weights [Cout, Kpad] -> three bf16 planes [3, Cout, Kpad] (int16 storage) for conv2d_x3."""
    _f32c(w_pk)
    planes = torch.empty((3,) + tuple(w_pk.shape), device=w_pk.device, dtype=torch.int16)
    _lib.call("mft_split_bf16x3", _p(w_pk), _p(planes), w_pk.numel(), _stream())
    return planes


def split_weight_h2(w_pk):
    """packed fp32 weights [Cout, Kpad] -> two fp16 planes [2, Cout, Kpad] (int16 storage): hi = fp16(w), lo = fp16((w - hi) * 2^11)
    (csrc/conv_x3.hip, "f16x2").  The conv2d_x3* wrappers below take either kind of planes and launch the matching kernels."""
    _f32c(w_pk)
    planes = torch.empty((2,) + tuple(w_pk.shape), device=w_pk.device, dtype=torch.int16)
    _lib.call("mft_split_f16x2", _p(w_pk), _p(planes), w_pk.numel(), _stream())
    return planes


def _x3_fn(w3, stem):
    """The C entry point for these weight planes: three bf16 planes -> mft_conv2d_nhwc_x3*, two fp16 planes -> mft_conv2d_nhwc_h2*."""
    return "mft_conv2d_nhwc_%s%s" % ({3: "x3", 2: "h2"}[int(w3.shape[0])], stem)


def conv2d_x3(x, w3, Cout, KH, KW, stride, pad, out=None):
    """conv2d for frozen shared weights on the bf16 / fp16 matrix cores with fp32 accuracy (6-term bf16x3 or 3-term f16x2 products,
    by the kind of ``w3``).  x [n,H,W,Cin] fp32, w3 = split_weight_x3 / split_weight_h2(pack_conv_weight(w)) -> [n,OH,OW,Cout] fp32."""
    _f32c(x)
    n, H, W, Cin = x.shape
    OH = (H + 2 * pad - KH) // stride + 1
    OW = (W + 2 * pad - KW) // stride + 1
    if out is None:
        out = torch.empty((n, OH, OW, Cout), device=x.device, dtype=torch.float32)
    _lib.call(_x3_fn(w3, ""), _p(x), Cin, _p(w3), w3.shape[1] * w3.shape[2], _p(out), Cout, n, H, W, Cin, Cout, KH, KW, stride, pad,
              _stream())
    return out


def conv2d_x3_bnstats(x, w3, Cout, KH, KW, stride, pad, imgs_per_group, out, ws, mean, rstd, eps=BN_EPS):
    """conv2d_x3 that also returns the following train-mode BatchNorm's statistics per group of ``imgs_per_group`` images
    (computed from the output tiles while they are still in registers).  ``ws``: >= mft_conv2d_x3_stats_ws_floats floats."""
    _f32c(x)
    n, H, W, Cin = x.shape
    if not _lib.try_call(_x3_fn(w3, "_bnstats"), _p(x), Cin, _p(w3), w3.shape[1] * w3.shape[2], _p(out), Cout, n, H, W, Cin, Cout, KH, KW,
                         stride, pad, imgs_per_group, eps, _p(ws), _p(mean), _p(rstd), _stream()):
        return None                       # outside the fused form's domain (e.g. an input of 2 GiB or more): caller uses conv + bn_stats
    return out, mean, rstd


def conv2d_x3_bnin_bnstats(c_raw, in_ws, in_gamma, in_beta, w3, Cout, imgs_per_group, out, ws, mean=None, rstd=None, eps=BN_EPS):
    """3x3 / stride 1 / pad 1 conv2d_x3 of relu(BatchNorm(c_raw)): ``c_raw`` [n,H,W,Cin] is the raw output of the previous
    bf16x3 convolution, ``in_ws`` its statistics partials (SimpleBlock's C1 -> BN1 -> ReLU -> C2, backbone.py:251-256, as one
    launch).  This convolution's own partials go to ``ws``; ``mean`` / ``rstd`` None = leave them as partials for the consumer.
    Returns None outside the kernel's domain."""
    _f32c(c_raw)
    n, H, W, Cin = c_raw.shape
    if not _lib.try_call(_x3_fn(w3, "_bnin_bnstats"), _p(c_raw), Cin, _p(in_ws), _p(in_gamma), _p(in_beta), _p(w3),
                         w3.shape[1] * w3.shape[2], _p(out), Cout, n, H, W, Cin, Cout, imgs_per_group, eps, _p(ws), _p(mean), _p(rstd),
                         _stream()):
        return None
    return out


def bn_apply_x3ws(x2d, C, rows_per_group, n_groups, ws, gamma, beta, out, act=ACT_NONE, res=None, res_ws=None, res_gamma=None,
                  res_beta=None, slope=LRELU_SLOPE, eps=BN_EPS, stats=None, res_stats=None):
    """bn_apply for the output of a bf16x3 convolution whose statistics are still per-tile partials ``ws`` (and ``res_ws`` for a
    BatchNorm'd residual branch): the merge happens in the prologue of the apply launch.  ``stats`` / ``res_stats`` = optional
    (mean, rstd) [n_groups, C] buffers that receive the merged statistics."""
    _f32c(x2d)
    m, r = stats if stats is not None else (None, None)
    rm, rr = res_stats if res_stats is not None else (None, None)
    _lib.call("mft_bn_apply_x3ws", _p(x2d), x2d.shape[-1], _p(out), out.shape[-1], C, rows_per_group, n_groups, _p(ws), _p(gamma),
              _p(beta), _p(res), 0 if res is None else res.shape[-1], _p(res_ws), _p(res_gamma), _p(res_beta), act, slope, eps, _p(m),
              _p(r), _p(rm), _p(rr), _stream())
    return out


def gemm(a, K, w_pk, N, bias=None, out=None, ldo=None, rows_per_group=0):
    """out[m, :N] = a[m, :K] @ w_pk[:N, :K].T + bias.  `a` is [M, lda] with lda >= K, K % 32 == 0."""
    _f32c(a)
    M, lda = a.shape
    if out is None:
        ldo = N if ldo is None else ldo
        out = torch.empty((M, ldo), device=a.device, dtype=torch.float32)
    else:
        ldo = out.shape[1]
    wgs = 0
    if w_pk.dim() == 3:
        wgs = w_pk.shape[1] * w_pk.shape[2]
    _lib.call("mft_conv2d_nhwc", _p(a), lda, _p(w_pk), _p(bias), _p(out), ldo, M, 1, 1, K, N, 1, 1, 1, 0, rows_per_group, wgs, _stream())
    return out


def gemm_rk(a, K, w_pk, N, bias=None, out=None, ldo=None):
    """``gemm`` for the skinny linear layers of a meta-training step (a few hundred rows, K <= 512): the register-K kernel
    (mft_gemm_rk, csrc/gnn.hip) -- 16-row tiles, no LDS staging.  Same contract as ``gemm`` for a 2-D pack; columns N.. of ``out``
    are left alone."""
    _f32c(a)
    M, lda = a.shape
    assert w_pk.dim() == 2 and w_pk.shape[1] == K and w_pk.shape[0] >= N and K % 16 == 0 and K <= 512, (tuple(w_pk.shape), K, N)
    if out is None:
        ldo = N if ldo is None else ldo
        out = torch.empty((M, ldo), device=a.device, dtype=torch.float32)
    else:
        ldo = out.shape[1]
    _lib.call("mft_gemm_rk", _p(a), lda, _p(w_pk), w_pk.shape[0], K, _p(bias), _p(out), ldo, M, N, _stream())
    return out


def conv2d_dgrad(dy, w_pk, Cin, KH, KW, pad, imgs_per_group=0, out=None, stride=1, in_hw=None):
    """dy [n,OH,OW,Cout], forward weight pack [Cout,KH*KW*Cin] or [groups,...] -> dx [n,H,W,Cin].
    ``in_hw`` = (H, W) of the forward input (needed when stride > 1; defaults to dy's size for stride 1)."""
    _f32c(dy)
    n, OH, OW, Cout = dy.shape
    H, W = (OH, OW) if in_hw is None else in_hw
    if out is None:
        out = torch.empty((n, H, W, Cin), device=dy.device, dtype=torch.float32)
    wgs = w_pk.shape[1] * w_pk.shape[2] if w_pk.dim() == 3 else 0
    if ((wgs == 0 and imgs_per_group <= 0) or (w_pk.dim() == 3 and w_pk.shape[0] == 1)) and Cin % 64 == 0:
        nws = _ksplit_ws(n * H * W, Cin, KH * KW * Cout)
        if nws:
            ws = torch.empty((nws,), device=dy.device, dtype=torch.float32)
            _lib.call("mft_conv2d_dgrad_nhwc_ksplit", _p(dy), Cout, _p(w_pk), _p(out), Cin, n, H, W, Cin, Cout, KH, KW, stride, pad,
                      _p(ws), _stream())
            return out
    if w_pk.dim() == 3 and 1 < w_pk.shape[0] <= SMALL_GROUPS and Cin % 64 == 0 and stride == 1 and imgs_per_group > 0:
        nws = _ksplit_ws(imgs_per_group * H * W, Cin, KH * KW * Cout, w_pk.shape[0])
        if nws:
            ws = torch.empty((nws,), device=dy.device, dtype=torch.float32)
            _lib.call("mft_conv2d_dgrad_nhwc_ksplit_grouped", _p(dy), Cout, _p(w_pk), _p(out), Cin, n, H, W, Cin, Cout, KH, KW, stride,
                      pad, imgs_per_group, wgs, _p(ws), _stream())
            return out
    _lib.call("mft_conv2d_dgrad_nhwc", _p(dy), Cout, _p(w_pk), _p(out), Cin, n, H, W, Cin, Cout, KH, KW, stride, pad, imgs_per_group, wgs,
              _stream())
    return out


def conv2d_wgrad(x, dy, Cout, KH, KW, stride, pad, imgs_per_group=0, out=None, ldy=None):
    """x [n,H,W,Cin], dy [n,OH,OW,Cout] (row stride ldy) -> dw [groups, Cout, roundup(KH*KW*Cin,32)] (packed layout)."""
    _f32c(x)
    _f32c(dy)
    n, H, W, Cin = x.shape
    groups = 1 if imgs_per_group <= 0 else n // imgs_per_group
    K = round_up(KH * KW * Cin, 32)
    if out is None:
        out = torch.empty((groups, Cout, K), device=x.device, dtype=torch.float32)
    nws = int(_lib.lib().mft_conv2d_wgrad_ws_floats(n, H, W, Cin, Cout, KH, KW, stride, pad, imgs_per_group))
    ws = torch.empty((nws,), device=x.device, dtype=torch.float32) if nws > 0 else None
    _lib.call("mft_conv2d_wgrad_nhwc", _p(x), Cin, _p(dy), dy.shape[-1] if ldy is None else ldy, _p(out), n, H, W, Cin, Cout, KH, KW,
              stride, pad, imgs_per_group, Cout * K, _p(ws), _stream())
    return out


def conv2d_wgrad_oihw(x, dy, Cout, KH, KW, stride, pad, cin_valid=0, cout_valid=0, out=None):
    """Weight gradient of a shared-weight convolution as torch lays Conv2d.weight.grad out: [Cout, Cin, KH, KW].
    ``cin_valid`` / ``cout_valid``: the operands carry zero-padded channels; only that corner is written (contiguously)."""
    _f32c(x)
    _f32c(dy)
    n, H, W, Cin = x.shape
    if out is None:
        out = torch.empty((cout_valid or Cout, cin_valid or Cin, KH, KW), device=x.device, dtype=torch.float32)
    ws = torch.empty((int(_lib.lib().mft_conv2d_wgrad_oihw_ws_floats(n, H, W, Cin, Cout, KH, KW, stride, pad)),), device=x.device,
                     dtype=torch.float32)
    _lib.call("mft_conv2d_wgrad_oihw", _p(x), Cin, _p(dy), dy.shape[-1], _p(out), n, H, W, Cin, Cout, KH, KW, stride, pad, cin_valid,
              cout_valid, _p(ws), _stream())
    return out


class WgradBatch:
    """Weight gradients of one backward pass, DEFERRED: ``add`` takes the same arguments as ``conv2d_wgrad_oihw`` and returns the
    output tensor at once -- its contents exist after ``flush()``, which runs all registered problems in ONE pair of launches per
    16 jobs (mft_conv2d_wgrad_oihw_multi).  Nothing downstream of a layer reads its weight gradient, so the meta-training backward
    registers every layer's as it goes and flushes at the end: 31 + 31 launches per step become 2 + 2 (+ the stem's own), each job
    bit-identical to its own launch.  The operands are kept alive (and must not be overwritten) until the flush.
    ``MFT_WGRAD_BATCH=0``: every ``add`` launches immediately (A/B and bit-identity reference)."""

    def __init__(self, enabled=True):
        self.enabled = enabled
        self.jobs, self.keep, self.after = [], [], []

    def add(self, x, dy, Cout, KH, KW, stride, pad, cin_valid=0, cout_valid=0):
        if not self.enabled:
            return conv2d_wgrad_oihw(x, dy, Cout, KH, KW, stride, pad, cin_valid, cout_valid)
        _f32c(x)
        _f32c(dy)
        n, H, W, Cin = x.shape
        out = torch.empty((cout_valid or Cout, cin_valid or Cin, KH, KW), device=x.device, dtype=torch.float32)
        ws = torch.empty((int(_lib.lib().mft_conv2d_wgrad_oihw_ws_floats(n, H, W, Cin, Cout, KH, KW, stride, pad)),), device=x.device,
                         dtype=torch.float32)
        self.jobs.append((x.data_ptr(), dy.data_ptr(), out.data_ptr(), ws.data_ptr(), Cin, dy.shape[-1], n, H, W, Cin, Cout, KH, KW, stride,
                          pad, cin_valid, cout_valid, 0))
        self.keep.append((x, dy, out, ws))
        return out

    def then(self, fn):
        """Run ``fn()`` right after the flush (work that reads a deferred gradient, e.g. the sum over row chunks)."""
        if not self.enabled:
            fn()
        else:
            self.after.append(fn)

    def flush(self):
        if self.jobs:
            job = _lib.struct("MftWgradJob")
            arr = (job * len(self.jobs))(*[job(*j) for j in self.jobs])
            dev = self.keep[0][0].device
            _lib.call("mft_conv2d_wgrad_oihw_multi", arr, len(self.jobs), _stream(dev))
        for fn in self.after:
            fn()
        self.jobs, self.keep, self.after = [], [], []


def conv2d_wgrad_adam(x, dy, w, m, v, Cout, KH, KW, stride, pad, step, imgs_per_group=0, lr=0.01, beta1=0.9,
                      beta2=0.999, eps=1e-8, dw=None, hyper=None):
    """Weight gradient of a conv with the Adam update of (w, m, v) [groups, Cout, KH*KW*Cin] fused in the epilogue.
    ``hyper``: device tensor {lr/(1-b1^t), 1/sqrt(1-b2^t)} maintained by adam_hyper_advance (hipGraph replay); replaces step/lr."""
    _f32c(x)
    _f32c(dy)
    n, H, W, Cin = x.shape
    K = KH * KW * Cin
    if hyper is not None:
        _lib.call("mft_conv2d_wgrad_adam_nhwc_dev", _p(x), Cin, _p(dy), Cout, _p(w), _p(m), _p(v), _p(dw), n, H, W, Cin, Cout, KH, KW,
                  stride, pad, imgs_per_group, Cout * K, _p(hyper), beta1, beta2, eps, _stream())
        return
    _lib.call("mft_conv2d_wgrad_adam_nhwc", _p(x), Cin, _p(dy), Cout, _p(w), _p(m), _p(v), _p(dw), n, H, W, Cin, Cout, KH, KW, stride, pad,
              imgs_per_group, Cout * K, step, lr, beta1, beta2, eps, _stream())


WF_RAW, WF_ENTRY, WF_EXIT = 0, 1, 2


def wgrad_adam_next_forward(x, dy, w, m, v, KH, KW, stride, pad, step, imgs_per_group, x_next=None, mode=WF_RAW, raw=None, act=None,
                            gamma=None, beta=None, gbs=0, mean=None, rstd=None, sc_raw=None, gamma_s=None, beta_s=None, mean_s=None,
                            rstd_s=None, pooled=None, lr=0.01, beta1=0.9, beta2=0.999, eps=1e-8, dw=None, hyper=None):
    """Weight gradient + Adam of (w, m, v) [groups, Cout, KH*KW*Cin] for inner step t and -- with ``x_next`` -- the same layer's
    convolution of step t+1 from the weight tiles just updated (csrc/wgrad_fwd.hip).  Returns False outside the kernel's domain."""
    _f32c(x)
    _f32c(dy)
    n, H, W, Cin = x.shape
    Cout = dy.shape[-1]
    return _lib.try_call(
        "mft_wgrad_adam_next_forward",
        _p(x), Cin, _p(dy), Cout, _p(w), _p(m), _p(v), _p(dw), n, H, W, Cin, Cout, KH, KW, stride, pad, imgs_per_group,
        Cout * KH * KW * Cin, 1 if hyper is not None else step, _p(hyper), lr, beta1, beta2, eps, _p(x_next), mode, _p(raw), _p(act),
        _p(gamma), _p(beta), gbs, _p(mean), _p(rstd), _p(sc_raw), _p(gamma_s), _p(beta_s), _p(mean_s), _p(rstd_s), _p(pooled),
        BN_EPS, _stream())


def conv2d_wgrad_adam_dgrad(x, dy, w, m, v, dxp, step, imgs_per_group, lr=0.01, beta1=0.9, beta2=0.999, eps=1e-8, hyper=None):
    """Weight gradient + Adam of a per-episode 3x3/s1/p1 convolution that also leaves the data gradient as 9 per-tap partials
    in ``dxp`` [groups, 9, rows, Cin] (csrc/wgrad_dgrad.hip).  Returns False when the shape is outside the kernel's domain."""
    n, H, W, Cin = x.shape
    Cout = dy.shape[-1]
    gs = w.shape[1] * w.shape[2]
    if hyper is not None:
        return _lib.try_call("mft_conv2d_wgrad_adam_dgrad_nhwc_dev", _p(x), Cin, _p(dy), Cout, _p(w), _p(m), _p(v), _p(dxp), n, H, W, Cin,
                             Cout, imgs_per_group, gs, _p(hyper), beta1, beta2, eps, _stream())
    return _lib.try_call("mft_conv2d_wgrad_adam_dgrad_nhwc", _p(x), Cin, _p(dy), Cout, _p(w), _p(m), _p(v), _p(dxp), n, H, W, Cin, Cout,
                         imgs_per_group, gs, step, lr, beta1, beta2, eps, _stream())


# ------------------------------------------------------------------------------------ batch norm

def bn_stats(x2d, C, rows_per_group, n_groups, running_mean=None, running_var=None, momentum=0.1, eps=BN_EPS,
             num_batches_tracked=None):
    """x2d [rows, ld] -> mean, rstd [n_groups, C].  ``num_batches_tracked`` (int64 scalar tensor, with running statistics only):
    incremented by the same launch."""
    _f32c(x2d)
    ld = x2d.shape[-1]
    mean = torch.empty((n_groups, C), device=x2d.device, dtype=torch.float32)
    rstd = torch.empty_like(mean)
    nws = _lib.lib().mft_bn_stats_ws_floats(C, rows_per_group, n_groups)
    ws = torch.empty((max(int(nws), 1),), device=x2d.device, dtype=torch.float32)
    _lib.call("mft_bn_stats", _p(x2d), ld, C, rows_per_group, n_groups, eps, _p(mean), _p(rstd), _p(ws), _p(running_mean), _p(running_var),
              momentum, _p(num_batches_tracked), _stream())
    return mean, rstd


BN_AFFINE_FMA = 0x100


def bn_apply(x2d, C, rows_per_group, n_groups, mean, rstd, gamma, beta, act=ACT_NONE, res=None, res_bn=None,
             out=None, gb_group_stride=0, slope=LRELU_SLOPE, fma_affine=False):
    """y = act(bn(x) [+ res | + bn(res)]).  res_bn = (mean, rstd, gamma, beta) of the residual branch.
    ``fma_affine``: y = fma(x, rstd*gamma, beta - mean*rstd*gamma), the arithmetic of the frozen trunk's folded BatchNorm kernels
    (bit-identical to them)."""
    _f32c(x2d)
    if fma_affine:
        act = act | BN_AFFINE_FMA
    if out is None:
        out = torch.empty_like(x2d)
    rm = rr = rg = rb = None
    if res_bn is not None:
        rm, rr, rg, rb = res_bn
    _lib.call("mft_bn_apply", _p(x2d), x2d.shape[-1], _p(out), out.shape[-1], C, rows_per_group, n_groups, _p(mean), _p(rstd), _p(gamma),
              _p(beta), gb_group_stride, _p(res), 0 if res is None else res.shape[-1], _p(rm), _p(rr), _p(rg), _p(rb), act, slope,
              _stream())
    return out


def bn_stats_multi(jobs, momentum=0.1, eps=BN_EPS):
    """``jobs``: list of (x2d, C, rows_per_group, n_groups, running_mean | None, running_var | None, num_batches_tracked | None) --
    bn_stats of each in ONE launch pair (mft_bn_stats_multi, up to 8 jobs); returns [(mean, rstd), ...]."""
    arr = (_lib.struct("MftBnStatsJob") * len(jobs))()
    out, keep = [], []
    for a, (x, C, rpg, ng, rm, rv, nbt) in zip(arr, jobs):
        _f32c(x)
        mean = torch.empty((ng, C), device=x.device, dtype=torch.float32)
        rstd = torch.empty_like(mean)
        ws = torch.empty((max(int(_lib.lib().mft_bn_stats_ws_floats(C, rpg, ng)), 1),), device=x.device, dtype=torch.float32)
        a.x, a.mean, a.rstd, a.ws = x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), ws.data_ptr()
        a.running_mean = None if rm is None else rm.data_ptr()
        a.running_var = None if rv is None else rv.data_ptr()
        a.num_batches_tracked = None if nbt is None else nbt.data_ptr()
        a.ldx, a.C, a.rows_per_group, a.n_groups, a.eps, a.momentum = x.shape[-1], C, rpg, ng, eps, momentum
        out.append((mean, rstd))
        keep.append(ws)
    _lib.call("mft_bn_stats_multi", arr, len(jobs), _stream(jobs[0][0].device))
    return out


def bn_forward_small_ok(C, rows_per_group):
    """The one-launch train-mode BatchNorm (mft_bn_forward_small) takes this problem: four-channel column groups, at most
    mft_bn_forward_small_max_rows() rows per group (512: the head's BatchNorm1d layers; a test hook can move it)."""
    return C % 4 == 0 and 0 < rows_per_group <= int(_lib.lib().mft_bn_forward_small_max_rows())


def bn_forward_small(x2d, C, rows_per_group, n_groups, gamma, beta, act=ACT_NONE, running=None, res=None, res_bn=None, out=None,
                     momentum=0.1, eps=BN_EPS, slope=LRELU_SLOPE, out_col=0):
    """bn_stats + bn_apply of a small tensor in ONE launch: -> (y, mean, rstd) -- or (y, mean, rstd, res_mean, res_rstd) when the
    residual goes through its own BatchNorm: ``res_bn`` = (gamma, beta, running | None).  ``running`` = (running_mean, running_var,
    num_batches_tracked) or None; group 0 advances them, as bn_stats does.  ``out_col``: write into columns out_col .. out_col + C of
    the (wider) matrix ``out``."""
    _f32c(x2d)
    dev = x2d.device
    if out is None:
        out = torch.empty_like(x2d)
    assert out_col >= 0 and out_col + C <= out.shape[-1]
    mean = torch.empty((n_groups, C), device=dev, dtype=torch.float32)
    rstd = torch.empty_like(mean)
    j = _lib.struct("MftBnFwdJob")()
    j.x, j.y, j.gamma, j.beta, j.mean, j.rstd = (t.data_ptr() for t in (x2d, out, gamma, beta, mean, rstd))
    j.y = out.data_ptr() + 4 * out_col
    rm, rv, nbt = running if running is not None else (None, None, None)
    j.running_mean, j.running_var, j.num_batches_tracked = (None if t is None else t.data_ptr() for t in (rm, rv, nbt))
    rmean = rrstd = None
    if res is not None:
        _f32c(res)
        j.res, j.ldr = res.data_ptr(), res.shape[-1]
        if res_bn is not None:
            rg, rb, rrun = res_bn
            rmean = torch.empty((n_groups, C), device=dev, dtype=torch.float32)
            rrstd = torch.empty_like(rmean)
            j.res_gamma, j.res_beta, j.res_mean, j.res_rstd = rg.data_ptr(), rb.data_ptr(), rmean.data_ptr(), rrstd.data_ptr()
            rrm, rrv, rnbt = rrun if rrun is not None else (None, None, None)
            j.res_running_mean, j.res_running_var, j.res_num_batches_tracked = (None if t is None else t.data_ptr() for t in (rrm, rrv, rnbt))
    j.ldx, j.ldy, j.C, j.rows_per_group, j.n_groups, j.act = x2d.shape[-1], out.shape[-1], C, rows_per_group, n_groups, act
    j.eps, j.momentum, j.slope = eps, momentum, slope
    _lib.call("mft_bn_forward_small", ctypes.byref(j), _stream(dev))
    if rmean is not None:
        return out, mean, rstd, rmean, rrstd
    return out, mean, rstd


def bn_backward_multi(jobs):
    """``jobs``: list of (x2d, dy2d, y_act | None, C, rows, groups, mean, rstd, gamma, act) -- BatchNorm backward (+ activation
    derivative) of each in ONE launch triple (mft_bn_backward_act_multi); returns [(dx, dgamma [C], dbeta [C]), ...] with the
    parameter gradients summed over the groups."""
    arr = (_lib.struct("MftBnBwdJob") * len(jobs))()
    out, keep = [], []
    for a, (x, dy, ya, C, rows, groups, mean, rstd, gamma, act) in zip(arr, jobs):
        _f32c(x)
        _f32c(dy)
        dev = x.device
        rpg = rows // groups
        dx = torch.empty_like(x)
        dg, db = torch.empty((C,), device=dev, dtype=torch.float32), torch.empty((C,), device=dev, dtype=torch.float32)
        ws = torch.empty((int(_lib.lib().mft_bn_backward_ws_floats(C, rpg, groups)),), device=dev, dtype=torch.float32)
        a.x, a.dy, a.dx, a.mean, a.rstd, a.gamma, a.ws = (t.data_ptr() for t in (x, dy, dx, mean, rstd, gamma, ws))
        a.y_act = None if ya is None else ya.data_ptr()
        one = groups == 1
        a.dgamma, a.dbeta = (dg.data_ptr(), db.data_ptr()) if one else (None, None)
        a.dgamma_sum, a.dbeta_sum = (None, None) if one else (dg.data_ptr(), db.data_ptr())
        a.dbias_zero = None
        a.ldx, a.lddy, a.ldya, a.lddx = x.shape[-1], dy.shape[-1], 0 if ya is None else ya.shape[-1], dx.shape[-1]
        a.C, a.rows_per_group, a.n_groups, a.act, a.slope = C, rpg, groups, act, LRELU_SLOPE
        out.append((dx, dg, db))
        keep.append(ws)
    _lib.call("mft_bn_backward_act_multi", arr, len(jobs), _stream(jobs[0][0].device))
    return out


def bn_apply_multi(jobs):
    """``jobs``: list of (x2d, C, rows_per_group, n_groups, mean, rstd, gamma, beta, act, out) -- bn_apply of each (no residual) in ONE
    launch per 16 jobs (mft_bn_apply_multi); returns the list of outputs."""
    if not jobs:
        return []
    arr = (_lib.struct("MftBnApplyJob") * len(jobs))()
    for a, (x, C, rpg, ng, mean, rstd, gamma, beta, act, out) in zip(arr, jobs):
        _f32c(x)
        a.x, a.y, a.mean, a.rstd, a.gamma, a.beta = (t.data_ptr() for t in (x, out, mean, rstd, gamma, beta))
        a.ldx, a.ldy, a.C, a.rows_per_group, a.n_groups, a.act, a.slope = x.shape[-1], out.shape[-1], C, rpg, ng, act, LRELU_SLOPE
    _lib.call("mft_bn_apply_multi", arr, len(jobs), _stream(jobs[0][0].device))
    return [j[-1] for j in jobs]


def bn_relu_maxpool(x, mean, rstd, gamma, beta, imgs_per_group=0):
    _f32c(x)
    n, H, W, C = x.shape
    OH, OW = (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1
    y = torch.empty((n, OH, OW, C), device=x.device, dtype=torch.float32)
    _lib.call("mft_bn_relu_maxpool", _p(x), _p(y), n, H, W, C, imgs_per_group, _p(mean), _p(rstd), _p(gamma), _p(beta), _stream())
    return y


def bn_relu_maxpool_gather(cache, src_idx, n_img, mean, rstd, gamma, beta, imgs_per_group, out=None):
    """bn_relu_maxpool over images cache[src_idx[n]] (cache [slots,H,W,C]); n_img = src_idx.numel()."""
    _f32c(cache)
    _, H, W, C = cache.shape
    OH, OW = (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1
    if out is None:
        out = torch.empty((n_img, OH, OW, C), device=cache.device, dtype=torch.float32)
    _lib.call("mft_bn_relu_maxpool_gather", _p(cache), _p(src_idx), _p(out), n_img, H, W, C, imgs_per_group, _p(mean), _p(rstd), _p(gamma),
              _p(beta), _stream())
    return out


def bn_image_moments(x):
    """x [n_img,H,W,C] -> per-image (mean [n_img,C], M2 [n_img,C]) over the H*W pixels."""
    _f32c(x)
    n, H, W, C = x.shape
    mean = torch.empty((n, C), device=x.device, dtype=torch.float32)
    m2 = torch.empty_like(mean)
    _lib.call("mft_bn_image_moments", _p(x), C, C, H * W, n, _p(mean), _p(m2), _stream())
    return mean, m2


def bn_combine_moments(mean_img, m2_img, idx_i32, rows_per_img, imgs_per_group, n_groups, mean=None, rstd=None, eps=BN_EPS):
    """Mini-batch BatchNorm statistics of the groups of images idx[g*k:(g+1)*k] from cached per-image moments."""
    C = mean_img.shape[1]
    if mean is None:
        mean = torch.empty((n_groups, C), device=mean_img.device, dtype=torch.float32)
        rstd = torch.empty_like(mean)
    _lib.call("mft_bn_combine_moments", _p(mean_img), _p(m2_img), _p(idx_i32), C, rows_per_img, imgs_per_group, n_groups, eps, _p(mean),
              _p(rstd), _stream())
    return mean, rstd


def global_avgpool(x):
    _f32c(x)
    n, H, W, C = x.shape
    y = torch.empty((n, C), device=x.device, dtype=torch.float32)
    _lib.call("mft_global_avgpool", _p(x), _p(y), n, H * W, C, _stream())
    return y


def avgpool_relu_backward(dfeat, out):
    _f32c(dfeat)
    _f32c(out)
    n, H, W, C = out.shape
    d = torch.empty_like(out)
    _lib.call("mft_avgpool_relu_backward", _p(dfeat), _p(out), _p(d), n, H * W, C, _stream())
    return d


def bn_backward(x2d, dy2d, C, rows_per_group, n_groups, mean, rstd, gamma, relu_out=None, need_dx=True,
                gb_group_stride=0):
    """-> dx [rows,C] (or None), dgamma [n_groups,C], dbeta [n_groups,C]."""
    _f32c(x2d)
    _f32c(dy2d)
    dx = torch.empty_like(x2d) if need_dx else None
    dg = torch.empty((n_groups, C), device=x2d.device, dtype=torch.float32)
    db = torch.empty_like(dg)
    _lib.call("mft_bn_backward", _p(x2d), x2d.shape[-1], _p(dy2d), dy2d.shape[-1], _p(relu_out),
              0 if relu_out is None else relu_out.shape[-1], _p(dx), 0 if dx is None else dx.shape[-1], C, rows_per_group, n_groups,
              _p(mean), _p(rstd), _p(gamma), gb_group_stride, _p(dg), _p(db), _stream())
    return dx, dg, db


# ------------------------------------------------------------------------------------ loss / optim

def cross_entropy(logits, labels_i32, rows_per_group, n_groups, need_grad=True):
    """-> loss [n_groups], dlogits (or None)."""
    _f32c(logits)
    rows, C = logits.shape
    buf = torch.empty((n_groups + rows,), device=logits.device, dtype=torch.float32)
    d = torch.empty_like(logits) if need_grad else None
    _lib.call("mft_cross_entropy", _p(logits), C, _p(labels_i32), C, rows_per_group, n_groups, _p(buf), _p(d), _stream())
    return buf[:n_groups], d


def softmax_rows(x):
    _f32c(x)
    rows, C = x.shape
    y = torch.empty_like(x)
    _lib.call("mft_softmax_rows", _p(x), C, _p(y), C, C, rows, _stream())
    return y


def _proto_check(feats, episodes, n_way, n_support, n_query):
    _f32c(feats)
    if feats.dim() != 2 or feats.shape[0] != episodes * n_way * (n_support + n_query):
        raise ValueError("ProtoNet head: feats %s is not [episodes*n_way*(n_support+n_query) = %d, D]"
                         % (tuple(feats.shape), episodes * n_way * (n_support + n_query)))


def proto_scores(feats, episodes, n_way, n_support, n_query, softmax=False, out=None):
    """ProtoNet scores (methods/protonet.py set_forward): feats [episodes*n_way*(n_support+n_query), D] (class-major rows, one
    episode after the other) -> [episodes*n_way*n_query, n_way] = -||q - p_c||^2; ``softmax``: their row softmax instead."""
    _proto_check(feats, episodes, n_way, n_support, n_query)
    D = feats.shape[1]
    rows = episodes * n_way * n_query
    if out is not None and (tuple(out.shape) != (rows, n_way) or not out.is_contiguous()):
        raise ValueError("proto_scores: out must be a contiguous [%d, %d] tensor" % (rows, n_way))
    y = out if out is not None else torch.empty((rows, n_way), device=feats.device, dtype=torch.float32)
    _lib.call("mft_proto_scores", _p(feats), feats.stride(0), episodes, n_way, n_support, n_query, D, _p(y), 1 if softmax else 0,
              _stream())
    return y


def proto_backward(feats, dscores, episodes, n_way, n_support, n_query, out=None):
    """d(scores) -> d(feats) for every row of every episode (one launch, no zero fill)."""
    _proto_check(feats, episodes, n_way, n_support, n_query)
    _f32c(dscores)
    if tuple(dscores.shape) != (episodes * n_way * n_query, n_way):
        raise ValueError("proto_backward: dscores is %s, expected [%d, %d]" % (tuple(dscores.shape), episodes * n_way * n_query, n_way))
    if out is not None and (out.shape != feats.shape or not out.is_contiguous()):
        raise ValueError("proto_backward: out must be a contiguous tensor shaped like feats")
    D = feats.shape[1]
    dx = out if out is not None else torch.empty((feats.shape[0], D), device=feats.device, dtype=torch.float32)
    _lib.call("mft_proto_backward", _p(feats), feats.stride(0), episodes, n_way, n_support, n_query, D, _p(dscores), dscores.stride(0),
              _p(dx), dx.stride(0), _stream())
    return dx


def dist_scale(n_classes):
    """distLinear's scale factor: 2 up to 200 classes, 10 above."""
    return 2.0 if n_classes <= 200 else 10.0


def _dist_rows(x, what):
    if x.dim() != 2 or x.dtype != torch.float32 or x.stride(1) != 1:
        raise RuntimeError("%s: expected float32 rows [R, D] with unit column stride, got %s %s" % (what, x.dtype, tuple(x.shape)))
    return x


def dist_linear_forward(x, g, v, scale, softmax=False):
    """Baseline++ scores (backbone.distLinear), one launch: x [n_groups * rows, D] (row stride free), v [C, D] or
    [n_groups, C, D], g [C, 1] / [C] or [n_groups, C] -> scale * g_c (x_r . v_c) / ((||x_r|| + 1e-5) ||v_c||) as
    [n_groups * rows, C]; ``softmax``: the row softmax of that instead."""
    _dist_rows(x, "dist_linear_forward")
    _f32c(v)
    _f32c(g)
    n_groups = v.shape[0] if v.dim() == 3 else 1
    C, D = v.shape[-2], v.shape[-1]
    if n_groups < 1 or g.numel() != n_groups * C or x.shape[1] != D or x.shape[0] % n_groups:
        raise ValueError("dist_linear_forward: x %s, g %s, v %s do not fit" % (tuple(x.shape), tuple(g.shape), tuple(v.shape)))
    y = torch.empty((x.shape[0], C), device=x.device, dtype=torch.float32)
    _lib.call("mft_dist_linear_forward", _p(x), x.stride(0), n_groups, x.shape[0] // n_groups, _p(v), _p(g), C, D, float(scale), _p(y),
              1 if softmax else 0, _stream())
    return y


def dist_linear_backward(x, g, v, scale, dscores, need_dx=True):
    """d(scores) [R, C] -> (dx [R, D] | None, dv [C, D], dg shaped like g) of dist_linear_forward with one group: one launch,
    every output element written once (torch.empty outputs), fixed summation order."""
    _dist_rows(x, "dist_linear_backward")
    _dist_rows(dscores, "dist_linear_backward")
    _f32c(v)
    _f32c(g)
    C, D = v.shape
    if g.numel() != C or x.shape[1] != D or tuple(dscores.shape) != (x.shape[0], C):
        raise ValueError("dist_linear_backward: x %s, g %s, v %s, dscores %s do not fit"
                         % (tuple(x.shape), tuple(g.shape), tuple(v.shape), tuple(dscores.shape)))
    dx = torch.empty((x.shape[0], D), device=x.device, dtype=torch.float32) if need_dx else None
    dv = torch.empty_like(v)
    dg = torch.empty_like(g)
    _lib.call("mft_dist_linear_backward", _p(x), x.stride(0), x.shape[0], _p(v), _p(g), C, D, float(scale), _p(dscores), dscores.stride(0),
              _p(dx), D, _p(dv), _p(dg), _stream())
    return dx, dv, dg


def dist_head_sgd_run(z_support, y_support, table, v, g, scale, lr=0.01, momentum=0.9, dampening=0.9, weight_decay=0.001):
    """BaselineFinetune(loss_type='dist') head training, every step of every group in one launch: z_support [G, S, D],
    y_support [G, S] int32, table [G, T, batch] int32 (support row per mini-batch slot, -1 = empty), v [G, n_way, D] and
    g [G, n_way] updated IN PLACE with torch.optim.SGD semantics."""
    for t in (z_support, v, g):
        _f32c(t)
    for t in (y_support, table):
        if t.dtype != torch.int32 or not t.is_contiguous():
            raise RuntimeError("dist_head_sgd_run: labels and index table must be contiguous int32 tensors")
    G, S, D = z_support.shape
    n_way = v.shape[1]
    if tuple(v.shape) != (G, n_way, D) or g.numel() != G * n_way or tuple(y_support.shape) != (G, S) or table.dim() != 3 \
            or table.shape[0] != G:
        raise ValueError("dist_head_sgd_run: z %s, y %s, table %s, v %s, g %s do not fit"
                         % (tuple(z_support.shape), tuple(y_support.shape), tuple(table.shape), tuple(v.shape), tuple(g.shape)))
    _lib.call("mft_dist_head_sgd_run", _p(z_support), _p(y_support), _p(table), G, S, D, n_way, table.shape[1], table.shape[2], _p(v),
              _p(g), float(scale), lr, momentum, dampening, weight_decay, _stream())


def dist_head_step(feat, labels, v, g, mv, vv, mg, vg, scale, step, dfeat=None, loss=None, lr=0.01, beta1=0.9, beta2=0.999,
                   eps=1e-8, weight_decay=0.001):
    """One inner step of finetune_linear with a distLinear head for every group, one launch: feat [G * k, D] (row stride free),
    labels [G * k] int32, v [G, n_way, D] and g [G, n_way] with their Adam moments (all six updated IN PLACE with
    torch.optim.Adam semantics, L2 weight decay); ``step`` = the 1-based Adam step.  -> (dfeat [G * k, D] computed with the
    pre-update head, loss [G]); both are written whole (``dfeat`` / ``loss``: caller's buffers)."""
    _dist_rows(feat, "dist_head_step")
    for t in (v, g, mv, vv, mg, vg):
        _f32c(t)
    if labels.dtype != torch.int32 or not labels.is_contiguous():
        raise RuntimeError("dist_head_step: labels must be a contiguous int32 tensor")
    if v.dim() != 3:
        raise ValueError("dist_head_step: v must be [groups, n_way, D], got %s" % (tuple(v.shape),))
    G, n_way, D = v.shape
    k = feat.shape[0] // max(G, 1)
    if G < 1 or feat.shape[0] != G * k or feat.shape[1] != D or labels.numel() != G * k or g.numel() != G * n_way \
            or any(t.shape != v.shape for t in (mv, vv)) or any(t.numel() != G * n_way for t in (mg, vg)):
        raise ValueError("dist_head_step: feat %s, labels %s, v %s, g %s and their moments do not fit"
                         % (tuple(feat.shape), tuple(labels.shape), tuple(v.shape), tuple(g.shape)))
    if dfeat is None:
        dfeat = torch.empty((G * k, D), device=feat.device, dtype=torch.float32)
    if loss is None:
        loss = torch.empty((G,), device=feat.device, dtype=torch.float32)
    _dist_rows(dfeat, "dist_head_step")
    _lib.call("mft_dist_head_step", _p(feat), feat.stride(0), _p(labels), k, G, n_way, D, float(scale), _p(v), _p(g), _p(mv), _p(vv),
              _p(mg), _p(vg), _p(dfeat), dfeat.stride(0), _p(loss), int(step), lr, beta1, beta2, eps, weight_decay, _stream())
    return dfeat, loss


def _linear_head(W, b, what):
    _f32c(W)
    _f32c(b)
    if W.dim() != 3 or tuple(b.shape) != tuple(W.shape[:2]):
        raise ValueError("%s: W must be [groups, n_way, D] and b [groups, n_way], got %s, %s" % (what, tuple(W.shape), tuple(b.shape)))
    return W.shape


def linear_head_step(feat, labels, W, b, mW, vW, mb, vb, step, dfeat=None, loss=None, lr=0.01, beta1=0.9, beta2=0.999, eps=1e-8,
                     weight_decay=0.001):
    """dist_head_step with finetune_linear's Linear(D, n_way) head: feat [G * k, D] (row stride free), labels [G * k] int32,
    W [G, n_way, D] and b [G, n_way] with their Adam moments, all six updated IN PLACE; ``step`` = the 1-based Adam step.
    -> (dfeat [G * k, D] computed with the pre-update head, loss [G]), both written whole."""
    _dist_rows(feat, "linear_head_step")
    G, n_way, D = _linear_head(W, b, "linear_head_step")
    for t in (mW, vW, mb, vb):
        _f32c(t)
    if labels.dtype != torch.int32 or not labels.is_contiguous():
        raise RuntimeError("linear_head_step: labels must be a contiguous int32 tensor")
    k = feat.shape[0] // G
    if feat.shape[0] != G * k or feat.shape[1] != D or labels.numel() != G * k or any(t.shape != W.shape for t in (mW, vW)) \
            or any(t.shape != b.shape for t in (mb, vb)):
        raise ValueError("linear_head_step: feat %s, labels %s, W %s, b %s and their moments do not fit"
                         % (tuple(feat.shape), tuple(labels.shape), tuple(W.shape), tuple(b.shape)))
    if dfeat is None:
        dfeat = torch.empty((G * k, D), device=feat.device, dtype=torch.float32)
    if loss is None:
        loss = torch.empty((G,), device=feat.device, dtype=torch.float32)
    _dist_rows(dfeat, "linear_head_step")
    _lib.call("mft_linear_head_step", _p(feat), feat.stride(0), _p(labels), k, G, n_way, D, _p(W), _p(b), _p(mW), _p(vW), _p(mb), _p(vb),
              _p(dfeat), dfeat.stride(0), _p(loss), int(step), lr, beta1, beta2, eps, weight_decay, _stream())
    return dfeat, loss


def linear_head_scores(x, W, b, out=None):
    """softmax(x @ W[g]^T + b[g]) of every group's rows, one launch: x [G * rows, D] (row stride free), W [G, n_way, D],
    b [G, n_way] -> [G * rows, n_way] (``out``: caller's contiguous buffer)."""
    _dist_rows(x, "linear_head_scores")
    G, n_way, D = _linear_head(W, b, "linear_head_scores")
    if x.shape[1] != D or x.shape[0] % G:
        raise ValueError("linear_head_scores: x %s, W %s do not fit" % (tuple(x.shape), tuple(W.shape)))
    if out is None:
        out = torch.empty((x.shape[0], n_way), device=x.device, dtype=torch.float32)
    elif tuple(_f32c(out).shape) != (x.shape[0], n_way):
        raise ValueError("linear_head_scores: out must be %s, got %s" % ((x.shape[0], n_way), tuple(out.shape)))
    _lib.call("mft_linear_head_scores", _p(x), x.stride(0), x.shape[0] // G, G, n_way, D, _p(W), _p(b), _p(out), _stream())
    return out


def linear_head_adam_run(z_support, y_support, table, W, b, lr=0.01, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.001):
    """dist_head_sgd_run's twin for finetune_linear(freeze_backbone=True): z_support [G, S, D], y_support [G, S] int32,
    table [G, T, batch] int32 (support row per mini-batch slot, -1 = empty), W [G, n_way, D] and b [G, n_way] updated IN PLACE with
    torch.optim.Adam semantics (L2 weight decay), every step of every group in one launch."""
    _f32c(z_support)
    G, n_way, D = _linear_head(W, b, "linear_head_adam_run")
    for t in (y_support, table):
        if t.dtype != torch.int32 or not t.is_contiguous():
            raise RuntimeError("linear_head_adam_run: labels and index table must be contiguous int32 tensors")
    S = z_support.shape[1] if z_support.dim() == 3 else -1
    if tuple(z_support.shape) != (G, S, D) or tuple(y_support.shape) != (G, S) or table.dim() != 3 or table.shape[0] != G:
        raise ValueError("linear_head_adam_run: z %s, y %s, table %s, W %s do not fit"
                         % (tuple(z_support.shape), tuple(y_support.shape), tuple(table.shape), tuple(W.shape)))
    _lib.call("mft_linear_head_adam_run", _p(z_support), _p(y_support), _p(table), G, S, D, n_way, table.shape[1], table.shape[2], _p(W),
              _p(b), lr, beta1, beta2, eps, weight_decay, _stream())


def adam_hyper_advance(step_i32, hyper, lr=0.01, beta1=0.9, beta2=0.999):
    """Device-side t = ++step; hyper = {lr/(1-beta1^t), 1/sqrt(1-beta2^t)} (one tiny launch; graph-capturable)."""
    _lib.call("mft_adam_hyper_advance", _p(step_i32), _p(hyper), lr, beta1, beta2, _stream())


def adam_step(p, g, m, v, step, lr=0.01, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, hyper=None):
    """In-place fused Adam on flat (contiguous) fp32 tensors of equal numel."""
    for t in (p, g, m, v):
        _f32c(t)
    if hyper is not None:
        _lib.call("mft_adam_step_dev", _p(p), _p(g), _p(m), _p(v), p.numel(), _p(hyper), beta1, beta2, eps, weight_decay, _stream())
        return
    _lib.call("mft_adam_step", _p(p), _p(g), _p(m), _p(v), p.numel(), step, lr, beta1, beta2, eps, weight_decay, _stream())


def sgd_step(p, g, buf, first_step, lr=0.01, momentum=0.9, dampening=0.9, weight_decay=0.001):
    _lib.call("mft_sgd_step", _p(p), _p(g), _p(buf), p.numel(), 1 if first_step else 0, lr, momentum, dampening, weight_decay, _stream())


def maml_delta(p, p2, p3):
    _lib.call("mft_maml_delta", _p(p), _p(p2), _p(p3), p.numel(), _stream())


# ------------------------------------------------------------------------------------ gnn glue

def pair_absdiff(x, N, F, ldd):
    """x [n_graphs*N, ldx] -> d [n_graphs*N*N, ldd] = |x_i - x_j| (zero padded beyond F)."""
    _f32c(x)
    n_graphs = x.shape[0] // N
    d = torch.empty((n_graphs * N * N, ldd), device=x.device, dtype=torch.float32)
    _lib.call("mft_pair_absdiff", _p(x), x.shape[1], _p(d), ldd, n_graphs, N, F, _stream())
    return d


def masked_softmax(s, N):
    """s [n_graphs*N*N, lds] (column 0) -> A [n_graphs, N, N]."""
    _f32c(s)
    n_graphs = s.shape[0] // (N * N)
    A = torch.empty((n_graphs, N, N), device=s.device, dtype=torch.float32)
    _lib.call("mft_masked_softmax", _p(s), s.shape[1], _p(A), n_graphs, N, _stream())
    return A


def graph_aggregate(A, x, F, ldy):
    """-> y [n_graphs*N, ldy] = cat(x[:, :F], A@x[:, :F]) zero padded."""
    _f32c(A)
    _f32c(x)
    n_graphs, N, _ = A.shape
    y = torch.empty((n_graphs * N, ldy), device=x.device, dtype=torch.float32)
    _lib.call("mft_graph_aggregate", _p(A), _p(x), x.shape[1], _p(y), ldy, n_graphs, N, F, _stream())
    return y


def copy_cols(x, y, col_off, C, act=ACT_NONE, slope=LRELU_SLOPE):
    _lib.call("mft_copy_cols", _p(x), x.shape[1], _p(y), y.shape[1], col_off, C, x.shape[0], act, slope, _stream())
    return y


def build_graph_nodes(z, n_episodes, n_way, n_support, n_query, ld=256, fold=False):
    """z [n_episodes*n_way*(S+n_query), 128] -> nodes [n_episodes*n_query*n_way*(n_support+1), ld]."""
    _f32c(z)
    rows = n_episodes * n_query * n_way * (n_support + 1)
    nodes = torch.empty((rows, ld), device=z.device, dtype=torch.float32)
    _lib.call("mft_build_graph_nodes", _p(z), z.shape[1], _p(nodes), ld, n_episodes, n_way, n_support, n_query, 1 if fold else 0,
              _stream())
    return nodes


def gather_query_scores(out, n_episodes, n_way, n_support, n_query):
    _f32c(out)
    scores = torch.empty((n_episodes * n_way * n_query, n_way), device=out.device, dtype=torch.float32)
    _lib.call("mft_gather_query_scores", _p(out), out.shape[1], _p(scores), n_episodes, n_way, n_support, n_query, _stream())
    return scores


def gather_rows(src2d, idx_i32, out=None):
    """dst[r] = src2d[idx[r]] for rows of src2d.shape[1] floats."""
    _f32c(src2d)
    n = idx_i32.numel()
    if out is None:
        out = torch.empty((n, src2d.shape[1]), device=src2d.device, dtype=torch.float32)
    _lib.call("mft_gather_rows", _p(src2d), _p(idx_i32), _p(out), n, src2d.shape[1], _stream())
    return out


TOP1_MAX_WAY = 64


def episode_top1(scores, n_episodes, n_way, n_query, need_pred=False):
    """Top-1 count of every episode of a lockstep batch (csrc/feature_eval.hip): scores [n_episodes * n_way * n_query, ld >= n_way]
    float32 with unit column stride, row r of an episode labelled r // n_query -> correct [n_episodes] int32, and with
    ``need_pred`` also the predictions [rows] int32 (first index of the row maximum over the first n_way columns)."""
    _dist_rows(scores, "episode_top1")
    rows = n_episodes * n_way * n_query
    if not 1 <= int(n_way) <= TOP1_MAX_WAY or n_query < 1 or n_episodes < 1 or scores.shape[0] != rows or scores.shape[1] < n_way \
            or scores.stride(0) < scores.shape[1]:
        raise ValueError("episode_top1: scores %s (row stride %d) are not [%d episodes * %d way * %d query, >= n_way] with "
                         "1 <= n_way <= %d" % (tuple(scores.shape), scores.stride(0), n_episodes, n_way, n_query, TOP1_MAX_WAY))
    correct = torch.empty((n_episodes,), device=scores.device, dtype=torch.int32)
    pred = torch.empty((rows,), device=scores.device, dtype=torch.int32) if need_pred else None
    _lib.call("mft_episode_top1", _p(scores), scores.stride(0), n_episodes, n_way, n_query, _p(correct), _p(pred), _stream())
    return (correct, pred) if need_pred else correct


# ---------------------------------------------------------------------------------------------- MatchingNet head (csrc/matchingnet.hip)
MN_D, MN_MAX_S, MN_MAX_WAY = 512, 256, 32
MN_KEYS = ("FCE.lstmcell.weight_ih", "FCE.lstmcell.weight_hh", "FCE.lstmcell.bias_ih", "FCE.lstmcell.bias_hh",
           "G_encoder.weight_ih_l0", "G_encoder.weight_hh_l0", "G_encoder.bias_ih_l0", "G_encoder.bias_hh_l0",
           "G_encoder.weight_ih_l0_reverse", "G_encoder.weight_hh_l0_reverse", "G_encoder.bias_ih_l0_reverse",
           "G_encoder.bias_hh_l0_reverse")


def mn_check(episodes, n_way, n_support, n_query, D=MN_D):
    """The launchers' domain (they return MFT_EINVAL outside it): raise ValueError before anything is launched."""
    if D != MN_D:
        raise ValueError("MatchingNet head: feature dimension %d is not supported (D = %d)" % (D, MN_D))
    if not 1 <= int(n_way) <= MN_MAX_WAY:
        raise ValueError("MatchingNet head: n_way = %d is not supported (1 <= n_way <= %d)" % (int(n_way), MN_MAX_WAY))
    if int(n_support) < 1 or int(n_way) * int(n_support) > MN_MAX_S:
        raise ValueError("MatchingNet head: S = n_way * n_support = %d is not supported (1 <= S <= %d)"
                         % (int(n_way) * int(n_support), MN_MAX_S))
    if int(n_query) < 1 or int(episodes) < 1:
        raise ValueError("MatchingNet head: n_query = %d, episodes = %d (both must be >= 1)" % (int(n_query), int(episodes)))


def mn_gemm(M, N, a1, lda1, b1, ldb1, K1, c, ldc, ta=False, tb=True, batch=1, a1_bs=0, b1_bs=0, b1_alt=None, a2=None, lda2=0,
            a2_bs=0, b2=None, ldb2=0, b2_bs=0, K2=0, c_in=None, ldci=0, ci_bs=0, bias1=None, bias2=None, c_bs=0):
    """mft_mn_gemm: c[z] = c_in[z] + bias1 + bias2 + op(a1[z]) op(b1[z]) + op(a2[z]) op(b2[z]); tensors are passed for their
    addresses only (views carry the offsets), shapes and strides are the integer arguments."""
    _lib.call("mft_mn_gemm", 1 if ta else 0, 1 if tb else 0, M, N, batch, _p(a1), lda1, a1_bs, _p(b1), _p(b1_alt), ldb1, b1_bs, K1, _p(a2),
              lda2, a2_bs, _p(b2), ldb2, b2_bs, K2, _p(c_in), ldci, ci_bs, _p(bias1), _p(bias2), _p(c), ldc, c_bs, _stream())
    return c


def lstm_step_forward(gates, ld_g, c_prev, ld_cp, f_add, c_out, h_out, ld_o, rows, batch=1, bs_g=0, bs_cp=0, bs_o=0):
    _lib.call("mft_lstm_step_forward", _p(gates), ld_g, bs_g, _p(c_prev), ld_cp, bs_cp, _p(f_add), MN_D, _p(c_out), _p(h_out), ld_o, bs_o,
              rows, MN_D, batch, _stream())


def lstm_step_backward(gates, ld_g, c_prev, ld_cp, c_new, ld_cn, dh1, ld_d1, dh2, ld_d2, dc_in, dc_out, ld_dc, rows, batch=1,
                       bs_g=0, bs_cp=0, bs_cn=0, bs_d1=0, bs_d2=0, bs_dc=0, dh_sum=None, dgate_sum=None, accumulate=False):
    _lib.call("mft_lstm_step_backward", _p(gates), ld_g, bs_g, _p(c_prev), ld_cp, bs_cp, _p(c_new), ld_cn, bs_cn, _p(dh1), ld_d1, bs_d1,
              _p(dh2), ld_d2, bs_d2, _p(dc_in), _p(dc_out), ld_dc, bs_dc, _p(dh_sum), _p(dgate_sum), 1 if accumulate else 0, rows, MN_D,
              batch, _stream())


def mn_attention_forward(h, G, episodes, Q, S, a, r):
    _lib.call("mft_mn_attention_forward", _p(h), _p(G), episodes, Q, S, MN_D, _p(a), _p(r), _stream())


def mn_attention_backward(dr, a, G, dh_in, episodes, Q, S, dlogit, dh_out):
    _lib.call("mft_mn_attention_backward", _p(dr), _p(a), _p(G), _p(dh_in), episodes, Q, S, MN_D, _p(dlogit), _p(dh_out), _stream())


def mn_readout_forward(h, G, gnorm, episodes, n_way, n_support, n_query):
    """-> dict(cos, p [M, S], hnorm [M], pc, logp [M, n_way]) for h [M = episodes * n_way * n_query, D], G [episodes, S, D]."""
    mn_check(episodes, n_way, n_support, n_query, h.shape[-1])
    M, S = episodes * n_way * n_query, n_way * n_support
    new = lambda *s: torch.empty(s, device=h.device, dtype=torch.float32)  # noqa: E731
    o = {"cos": new(M, S), "p": new(M, S), "hnorm": new(M), "pc": new(M, n_way), "logp": new(M, n_way)}
    _lib.call("mft_mn_readout_forward", _p(h), _p(G), _p(gnorm), episodes, n_way, n_support, n_query, MN_D, _p(o["cos"]), _p(o["p"]),
              _p(o["hnorm"]), _p(o["pc"]), _p(o["logp"]), _stream())
    return o


def mn_readout_backward(dlogp, h, G, gnorm, ro, episodes, n_way, n_support, n_query):
    """-> (dh [M, D], dG [episodes, S, D]) from d(logp) [M, n_way] and the forward's dict."""
    M, S = episodes * n_way * n_query, n_way * n_support
    new = lambda *s: torch.empty(s, device=h.device, dtype=torch.float32)  # noqa: E731
    dcos, dh, dG = new(M, S), new(M, MN_D), new(episodes, S, MN_D)
    _lib.call("mft_mn_readout_backward", _p(dlogp), dlogp.stride(0), _p(h), _p(G), _p(gnorm), _p(ro["cos"]), _p(ro["p"]), _p(ro["hnorm"]),
              _p(ro["pc"]), episodes, n_way, n_support, n_query, MN_D, _p(dcos), _p(dh), _p(dG), _stream())
    return dh, dG


def mn_colsum(x, rows, C, out=None):
    out = torch.empty(C, device=x.device, dtype=torch.float32) if out is None else out
    _lib.call("mft_mn_colsum", _p(x), C, C, rows, _p(out), _stream())
    return out


def nll_mean(logp, target, loss_sum=None):
    rows, C = logp.shape
    loss = torch.empty((), device=logp.device, dtype=torch.float32)
    _lib.call("mft_nll_mean", _p(logp), logp.stride(0), _p(target), 1 if target.dtype == torch.int64 else 0, C, rows, _p(loss),
              _p(loss_sum), _stream())
    return loss


def nll_mean_backward(target, rows, C, g):
    d = torch.empty((rows, C), device=target.device, dtype=torch.float32)
    _lib.call("mft_nll_mean_backward", _p(target), 1 if target.dtype == torch.int64 else 0, C, rows, _p(g), _p(d), C, _stream())
    return d


def mn_encoder_forward(W, zS, E, S):
    """G_encoder over every episode's support sequence, both directions in lockstep: -> (eg, eh, ec) [2, E, S, 4D | D | D], the gate
    activations, hidden and cell states of every step (direction 1 runs the rows backwards)."""
    D = MN_D
    new = lambda *s: torch.empty(s, device=zS.device, dtype=torch.float32)  # noqa: E731
    eg, eh, ec = new(2, E, S, 4 * D), new(2, E, S, D), new(2, E, S, D)
    for d, sfx in enumerate(("", "_reverse")):          # input parts of all S steps at once
        mn_gemm(E * S, 4 * D, zS, D, W["G_encoder.weight_ih_l0" + sfx], D, D, eg[d], 4 * D,
                bias1=W["G_encoder.bias_ih_l0" + sfx], bias2=W["G_encoder.bias_hh_l0" + sfx])
    for t in range(S):
        r0, r1 = t, S - 1 - t                           # the row each direction writes at step t
        if t > 0:
            p0, p1 = r0 - 1, r1 + 1                     # ... and the row that holds its previous state
            mn_gemm(E, 4 * D, eh[0, :, p0], S * D, W["G_encoder.weight_hh_l0"], D, D, eg[0, :, r0], S * 4 * D, batch=2,
                    a1_bs=(E * S + p1 - p0) * D, b1_alt=W["G_encoder.weight_hh_l0_reverse"], c_in=eg[0, :, r0], ldci=S * 4 * D,
                    ci_bs=(E * S + r1 - r0) * 4 * D, c_bs=(E * S + r1 - r0) * 4 * D)
        lstm_step_forward(eg[0, :, r0], S * 4 * D, ec[0, :, p0] if t > 0 else None, S * D, None, ec[0, :, r0], eh[0, :, r0], S * D, E,
                          batch=2, bs_g=(E * S + r1 - r0) * 4 * D, bs_cp=(E * S + p1 - p0) * D if t > 0 else 0,
                          bs_o=(E * S + r1 - r0) * D)
    return eg, eh, ec


def matching_forward(W, feats, episodes, n_way, n_support, n_query, save=False):
    """MatchingNet head forward: feats [episodes * n_way * (n_support + n_query), 512] (class-major rows, one
    episode after the other), W: the twelve head parameters by state-dict key (MN_KEYS) -> (logp [episodes * n_way * n_query,
    n_way], tape | None).  ``save``: keep the per-step h, c, a, r and gates for matching_backward (S + 1 slots instead of 2)."""
    if feats.dtype != torch.float32 or feats.dim() != 2 or feats.stride(1) != 1:
        raise RuntimeError("MatchingNet head: expected float32 rows [R, D] with unit column stride, got %s %s" % (feats.dtype, tuple(feats.shape)))
    mn_check(episodes, n_way, n_support, n_query, feats.shape[-1])
    E, D, S, Q = episodes, MN_D, n_way * n_support, n_way * n_query
    M = E * Q
    if feats.shape[0] != E * n_way * (n_support + n_query):
        raise ValueError("MatchingNet head: feats %s is not [episodes*n_way*(n_support+n_query) = %d, %d]"
                         % (tuple(feats.shape), E * n_way * (n_support + n_query), D))
    new = lambda *s: torch.empty(s, device=feats.device, dtype=torch.float32)  # noqa: E731
    T = S + 1 if save else 2
    Tg = S if save else 1
    zS, f, fh, fc = new(E, S, D), new(M, D), new(T, M, D), new(T, M, D)
    _lib.call("mft_mn_gather", _p(feats), feats.stride(0), E, n_way, n_support, n_query, D, _p(zS), _p(f), _p(fh[0]), _stream())
    eg, eh, ec = mn_encoder_forward(W, zS, E, S)
    G, gnorm = new(E, S, D), new(E, S)
    _lib.call("mft_mn_encode_combine", _p(zS), _p(eh[0]), _p(eh[1]), E, S, D, _p(G), _p(gnorm), _stream())
    # FCE: the f half of the cell's input part does not change over the S steps
    wih, whh = W["FCE.lstmcell.weight_ih"], W["FCE.lstmcell.weight_hh"]
    Pf = mn_gemm(M, 4 * D, f, D, wih, 2 * D, D, new(M, 4 * D), 4 * D, bias1=W["FCE.lstmcell.bias_ih"], bias2=W["FCE.lstmcell.bias_hh"])
    fg, fa, fr = new(Tg, M, 4 * D), new(Tg, M, S), new(Tg, M, D)
    wih_r = wih[:, D:]
    for k in range(S):
        si, so, sg = k % T, (k + 1) % T, k % Tg
        mn_attention_forward(fh[si], G, E, Q, S, fa[sg], fr[sg])
        mn_gemm(M, 4 * D, fh[si], D, whh, D, D, fg[sg], 4 * D, a2=fr[sg], lda2=D, b2=wih_r, ldb2=2 * D, K2=D, c_in=Pf, ldci=4 * D)
        lstm_step_forward(fg[sg], 4 * D, fc[si] if k > 0 else None, D, f, fc[so], fh[so], D, M)
    hS = fh[S % T]
    ro = mn_readout_forward(hS, G, gnorm, E, n_way, n_support, n_query)
    if not save:
        return ro["logp"], None
    tape = dict(zS=zS, f=f, fh=fh, fc=fc, eg=eg, eh=eh, ec=ec, G=G, gnorm=gnorm, fg=fg, fa=fa, fr=fr, ro=ro,
                shape=(E, n_way, n_support, n_query))
    return ro["logp"], tape


def matching_backward(W, tape, dlogp):
    """d(logp) [M, n_way] -> (dfeats [episodes * n_way * (n_support + n_query), 512], {state-dict key: gradient}).  Consumes the tape:
    the saved gates are overwritten by d(pre-activations), and every weight gradient is ONE transposed GEMM over all steps."""
    E, n_way, n_support, n_query = tape["shape"]
    D, S, Q = MN_D, n_way * n_support, n_way * n_query
    M = E * Q
    zS, f, fh, fc, eg, eh, ec, G, fg, fa, fr = (tape[k] for k in ("zS", "f", "fh", "fc", "eg", "eh", "ec", "G", "fg", "fa", "fr"))
    new = lambda *s: torch.empty(s, device=zS.device, dtype=torch.float32)  # noqa: E731
    wih, whh = W["FCE.lstmcell.weight_ih"], W["FCE.lstmcell.weight_hh"]
    wih_r = wih[:, D:]
    g = {}
    dh, dG = mn_readout_backward(dlogp, fh[S], G, tape["gnorm"], tape["ro"], E, n_way, n_support, n_query)
    # ---- FCE, last step first
    dc, df, dPf, dhl, dr, dlogit, dh2 = new(M, D), new(M, D), new(M, 4 * D), new(M, D), new(M, D), new(M, S), new(M, D)
    for k in range(S - 1, -1, -1):
        first = k == S - 1
        lstm_step_backward(fg[k], 4 * D, fc[k] if k > 0 else None, D, fc[k + 1], D, dh, D, None, 0, None if first else dc, dc, D, M,
                           dh_sum=df, dgate_sum=dPf, accumulate=not first)
        mn_gemm(M, D, fg[k], 4 * D, whh, D, 4 * D, dhl, D, tb=False)
        mn_gemm(M, D, fg[k], 4 * D, wih_r, 2 * D, 4 * D, dr, D, tb=False)
        mn_attention_backward(dr, fa[k], G, dhl, E, Q, S, dlogit, dh2)
        mn_gemm(S, D, fa[k], S, dr, D, Q, dG, D, ta=True, tb=False, batch=E, a1_bs=Q * S, b1_bs=Q * D, a2=dlogit, lda2=S,
                a2_bs=Q * S, b2=fh[k], ldb2=D, b2_bs=Q * D, K2=Q, c_in=dG, ldci=D, ci_bs=S * D, c_bs=S * D)
        dh, dh2 = dh2, dh
    mn_gemm(M, D, dPf, 4 * D, wih, 2 * D, 4 * D, df, D, tb=False, c_in=df, ldci=D)        # df += dPf W_ih[:, :D]; dh is d(h_0 = f)
    gw = new(4 * D, 2 * D)
    mn_gemm(4 * D, D, dPf, 4 * D, f, D, M, gw, 2 * D, ta=True, tb=False)
    mn_gemm(4 * D, D, fg, 4 * D, fr, D, S * M, gw[:, D:], 2 * D, ta=True, tb=False)
    g["FCE.lstmcell.weight_ih"] = gw
    g["FCE.lstmcell.weight_hh"] = mn_gemm(4 * D, D, fg, 4 * D, fh, D, S * M, new(4 * D, D), D, ta=True, tb=False)
    g["FCE.lstmcell.bias_ih"] = mn_colsum(dPf, M, 4 * D)
    g["FCE.lstmcell.bias_hh"] = mn_colsum(dPf, M, 4 * D)
    # ---- G_encoder: d(out_forward) = d(out_reverse) = d(z_S, direct) = dG; direction 0 walks its rows backwards, direction 1 forwards
    edc, edh = new(2, E, D), new(2, E, D)
    for u in range(S):
        r0, r1 = S - 1 - u, u
        more = u < S - 1
        bs = E * S + r1 - r0
        lstm_step_backward(eg[0, :, r0], S * 4 * D, ec[0, :, r0 - 1] if more else None, S * D, ec[0, :, r0], S * D, dG[:, r0], S * D,
                           edh if u > 0 else None, D, edc if u > 0 else None, edc, D, E, batch=2, bs_g=bs * 4 * D,
                           bs_cp=(bs + 2) * D, bs_cn=bs * D, bs_d1=(r1 - r0) * D, bs_d2=E * D, bs_dc=E * D)
        if more:
            mn_gemm(E, D, eg[0, :, r0], S * 4 * D, W["G_encoder.weight_hh_l0"], D, 4 * D, edh, D, tb=False, batch=2, a1_bs=bs * 4 * D,
                    b1_alt=W["G_encoder.weight_hh_l0_reverse"], c_bs=E * D)
    dzS = mn_gemm(E * S, D, eg[0], 4 * D, W["G_encoder.weight_ih_l0"], D, 4 * D, new(E, S, D), D, tb=False, a2=eg[1], lda2=4 * D,
                  b2=W["G_encoder.weight_ih_l0_reverse"], ldb2=D, K2=4 * D, c_in=dG, ldci=D)
    for d, sfx in enumerate(("", "_reverse")):
        g["G_encoder.weight_ih_l0" + sfx] = mn_gemm(4 * D, D, eg[d], 4 * D, zS, D, E * S, new(4 * D, D), D, ta=True, tb=False)
        gh = new(4 * D, D)
        for e in range(E):          # the state a step reads sits one row before (direction 0) / after (direction 1) its own
            a, b = (eg[d, e, 1:], eh[d, e]) if d == 0 else (eg[d, e], eh[d, e, 1:])
            mn_gemm(4 * D, D, a if S > 1 else eg[d, e], 4 * D, b if S > 1 else eh[d, e], D, S - 1, gh, D, ta=True, tb=False,
                    c_in=gh if e > 0 else None, ldci=D)
        g["G_encoder.weight_hh_l0" + sfx] = gh
        g["G_encoder.bias_ih_l0" + sfx] = mn_colsum(eg[d], E * S, 4 * D)
        g["G_encoder.bias_hh_l0" + sfx] = mn_colsum(eg[d], E * S, 4 * D)
    per = n_way * (n_support + n_query)
    dfeats = new(E * per, D)
    _lib.call("mft_mn_scatter_backward", _p(dzS), _p(df), _p(dh), E, n_way, n_support, n_query, D, _p(dfeats), D, _stream())
    return dfeats, g


# ---------------------------------------------------------------------------------------------- MetaOptNet ridge head (csrc/ridge.hip)
RIDGE_D, RIDGE_MAX_S, RIDGE_MAX_WAY = 512, 256, 32
RIDGE_LAMBDA = 50.0


def ridge_check(episodes, n_way, n_support, n_query, D=RIDGE_D):
    """The launchers' domain (they return MFT_EINVAL outside it): raise ValueError before anything is launched."""
    if D != RIDGE_D:
        raise ValueError("MetaOptNet head: feature dimension %d is not supported (D = %d)" % (D, RIDGE_D))
    if not 1 <= int(n_way) <= RIDGE_MAX_WAY:
        raise ValueError("MetaOptNet head: n_way = %d is not supported (1 <= n_way <= %d)" % (int(n_way), RIDGE_MAX_WAY))
    if int(n_support) < 1 or int(n_way) * int(n_support) > RIDGE_MAX_S:
        raise ValueError("MetaOptNet head: S = n_way * n_support = %d is not supported (1 <= S <= %d)"
                         % (int(n_way) * int(n_support), RIDGE_MAX_S))
    if int(n_query) < 1 or int(episodes) < 1:
        raise ValueError("MetaOptNet head: n_query = %d, episodes = %d (both must be >= 1)" % (int(n_query), int(episodes)))


def _ridge_feats(feats, episodes, n_way, n_support, n_query):
    if not feats.is_cuda:
        raise RuntimeError("MetaOptNet head: input is on %s -- the MI355X path has no CPU fallback; call .cuda() first" % feats.device)
    if feats.dtype != torch.float32 or feats.dim() != 2 or feats.stride(1) != 1:
        raise RuntimeError("MetaOptNet head: expected float32 rows [R, D] with unit column stride, got %s %s" % (feats.dtype, tuple(feats.shape)))
    ridge_check(episodes, n_way, n_support, n_query, feats.shape[1])
    if feats.shape[0] != episodes * n_way * (n_support + n_query):
        raise ValueError("MetaOptNet head: feats %s is not [episodes*n_way*(n_support+n_query) = %d, %d]"
                         % (tuple(feats.shape), episodes * n_way * (n_support + n_query), RIDGE_D))
    if feats.stride(0) < RIDGE_D or feats.stride(0) % 4 != 0 or feats.data_ptr() % 16 != 0:
        raise ValueError("MetaOptNet head: row stride %d (must be >= %d and a multiple of 4, rows 16-byte aligned)" % (feats.stride(0), RIDGE_D))


def _ridge_scale(scale):
    if not torch.is_tensor(scale) or not scale.is_cuda or scale.dtype != torch.float32 or scale.numel() != 1:
        raise RuntimeError("MetaOptNet head: scale must be a one-element float32 tensor on the GPU (no CPU fallback)")
    return scale


def ridge_forward(feats, scale, episodes, n_way, n_support, n_query, softmax=False, save=False, lambda_reg=RIDGE_LAMBDA):
    """MetaOptNet-RR head forward: feats [episodes*n_way*(n_support+n_query), 512] (class-major rows, one
    episode after the other, row stride >= 512), scale a one-element device tensor -> (scores [episodes*n_way*n_query, n_way],
    tape | None); ``softmax``: the row softmax of the scores instead.  Three launches whatever the shape: Gram matrix, Cholesky
    factor + alpha + W, scores.  ``save``: keep L, alpha and W for ridge_backward."""
    _ridge_feats(feats, episodes, n_way, n_support, n_query)
    _ridge_scale(scale)
    E, D, S, Q = episodes, RIDGE_D, n_way * n_support, n_way * n_query
    new = lambda *s: torch.empty(s, device=feats.device, dtype=torch.float32)  # noqa: E731
    A, alpha, W, scores = new(E, S, S), new(E, S, n_way), new(E, n_way, D), new(E * Q, n_way)
    ld = feats.stride(0)
    _lib.call("mft_ridge_gram", _p(feats), ld, E, n_way, n_support, n_query, D, float(lambda_reg), _p(A), _stream())
    _lib.call("mft_ridge_factor_solve", _p(feats), ld, E, n_way, n_support, n_query, D, _p(A), _p(alpha), _p(W), _stream())
    _lib.call("mft_ridge_scores", _p(feats), ld, E, n_way, n_support, n_query, D, _p(W), _p(scale), _p(scores), 1 if softmax else 0,
              _stream())
    if not save:
        return scores, None
    return scores, dict(feats=feats, scale=scale, L=A, alpha=alpha, W=W, shape=(E, n_way, n_support, n_query))


def ridge_backward(tape, dscores):
    """d(scores) [episodes*n_way*n_query, n_way] -> (dfeats [rows, 512] with every row written, dscale [1]) from the forward's
    tape.  Two launches whatever the shape: query side (dZ_Q, dW, the shares of dscale), support side (dalpha, B, dZ_S)."""
    E, n_way, n_support, n_query = tape["shape"]
    feats, scale = tape["feats"], tape["scale"]
    D, Q = RIDGE_D, n_way * n_query
    if not dscores.is_cuda:
        raise RuntimeError("MetaOptNet head: d(scores) is on %s -- the MI355X path has no CPU fallback" % dscores.device)
    if dscores.dtype != torch.float32 or dscores.dim() != 2 or dscores.stride(1) != 1:
        raise RuntimeError("MetaOptNet head: expected float32 d(scores) with unit column stride")
    if tuple(dscores.shape) != (E * Q, n_way):
        raise ValueError("ridge_backward: dscores is %s, expected [%d, %d]" % (tuple(dscores.shape), E * Q, n_way))
    new = lambda *s: torch.empty(s, device=feats.device, dtype=torch.float32)  # noqa: E731
    dfeats, dW, dscale = new(feats.shape[0], D), new(E, n_way, D), new(1)
    part = torch.empty(E * 8, device=feats.device, dtype=torch.float64)
    ld = feats.stride(0)
    _lib.call("mft_ridge_backward_query", _p(feats), ld, E, n_way, n_support, n_query, D, _p(tape["W"]), _p(scale), _p(dscores),
              dscores.stride(0), _p(dfeats), D, _p(dW), _p(part), _stream())
    _lib.call("mft_ridge_backward_support", _p(feats), ld, E, n_way, n_support, n_query, D, _p(tape["L"]), _p(tape["alpha"]),
              _p(tape["W"]), _p(dW), _p(part), _p(dfeats), D, _p(dscale), _stream())
    return dfeats, dscale


# ---------------------------------------------------------------------------------------------- TPN head (csrc/tpn.hip)
TPN_D, TPN_MAX_N, TPN_MAX_WAY = 512, 256, 32
TPN_K, TPN_ALPHA = 20, 0.99


def tpn_check(episodes, n_way, n_support, n_query, D=TPN_D, k=TPN_K):
    """The launchers' domain (they return MFT_EINVAL outside it): raise ValueError before anything is launched."""
    if D != TPN_D:
        raise ValueError("TPN head: feature dimension %d is not supported (D = %d)" % (D, TPN_D))
    if not 1 <= int(n_way) <= TPN_MAX_WAY:
        raise ValueError("TPN head: n_way = %d is not supported (1 <= n_way <= %d)" % (int(n_way), TPN_MAX_WAY))
    if int(n_support) < 1 or int(n_query) < 1 or int(episodes) < 1:
        raise ValueError("TPN head: n_support = %d, n_query = %d, episodes = %d (all must be >= 1)"
                         % (int(n_support), int(n_query), int(episodes)))
    if int(n_way) * (int(n_support) + int(n_query)) > TPN_MAX_N:
        raise ValueError("TPN head: N = n_way * (n_support + n_query) = %d nodes is not supported (N <= %d: the factor of one "
                         "episode's graph is kept in one workgroup's LDS)" % (int(n_way) * (int(n_support) + int(n_query)), TPN_MAX_N))
    if not 1 <= int(k) <= TPN_MAX_N:
        raise ValueError("TPN head: k = %d neighbours is not supported (1 <= k <= %d)" % (int(k), TPN_MAX_N))


def _tpn_head(head):
    w3, b3, w4, b4 = head
    for t, shape in ((w3, (8, TPN_D)), (b3, (8,)), (w4, (1, 8)), (b4, (1,))):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise RuntimeError("TPN head: fc3 / fc4 must be float32 tensors on the GPU (no CPU fallback)")
        if t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != shape:
            raise RuntimeError("TPN head: expected contiguous float32 fc3.weight [8, %d], fc3.bias [8], fc4.weight [1, 8], fc4.bias [1]; "
                               "got %s %s" % (TPN_D, t.dtype, tuple(t.shape)))
    return w3, b3, w4, b4


def tpn_forward(feats, head, episodes, n_way, n_support, n_query, k=TPN_K, alpha=TPN_ALPHA, save=False, mask=None):
    """TPN head forward: feats [episodes*n_way*(n_support+n_query), 512] (class-major rows, one episode after
    the other, row stride >= 512), head = (fc3.weight, fc3.bias, fc4.weight, fc4.bias) on the device -> (scores
    [episodes*n_way*n_query, n_way], tape | None).  Three launches whatever the shape: embed, affinity, propagate.  ``save``: keep
    what tpn_backward needs; the tape also exposes ``W`` [episodes, N, N] and ``mask`` [episodes, N, N] (uint8).  ``mask``
    [episodes, N, N] (tests and golden parity only): the neighbour selection instead of the k largest entries per row."""
    if not feats.is_cuda:
        raise RuntimeError("TPN head: input is on %s -- the MI355X path has no CPU fallback; call .cuda() first" % feats.device)
    if feats.dtype != torch.float32 or feats.dim() != 2 or feats.stride(1) != 1:
        raise RuntimeError("TPN head: expected float32 rows [R, D] with unit column stride, got %s %s" % (feats.dtype, tuple(feats.shape)))
    tpn_check(episodes, n_way, n_support, n_query, feats.shape[1], k)
    E, D, N, Q = episodes, TPN_D, n_way * (n_support + n_query), n_way * n_query
    if feats.shape[0] != E * N:
        raise ValueError("TPN head: feats %s is not [episodes*n_way*(n_support+n_query) = %d, %d]" % (tuple(feats.shape), E * N, D))
    if feats.stride(0) < D or feats.stride(0) % 4 != 0 or feats.data_ptr() % 16 != 0:
        raise ValueError("TPN head: row stride %d (must be >= %d and a multiple of 4, rows 16-byte aligned)" % (feats.stride(0), D))
    w3, b3, w4, b4 = _tpn_head(head)
    if mask is not None:
        if not mask.is_cuda:
            raise RuntimeError("TPN head: the forced mask is on %s -- the MI355X path has no CPU fallback" % mask.device)
        if mask.dtype != torch.uint8 or not mask.is_contiguous() or mask.numel() != E * N * N:
            raise ValueError("TPN head: the forced mask must be a contiguous uint8 tensor [episodes, N, N] = [%d, %d, %d]" % (E, N, N))
    dev = feats.device
    new = lambda *s: torch.empty(s, device=dev, dtype=torch.float32)  # noqa: E731
    u, hid, W, scores = new(E * N, D), new(E * N, 8), new(E, N, N), new(E * Q, n_way)
    sig = torch.empty(E * N, device=dev, dtype=torch.float64)
    L = F = mk = rinv = None
    if save:
        L, F, rinv = new(E, N * (N + 1) // 2), new(E, N, n_way), new(E, N)
        mk = torch.empty((E, N, N), device=dev, dtype=torch.uint8)
    _lib.call("mft_tpn_embed", _p(feats), feats.stride(0), E, n_way, n_support, n_query, D, _p(w3), _p(b3), _p(w4), _p(b4), _p(u),
              _p(hid), _p(sig), _stream())
    _lib.call("mft_tpn_affinity", E, n_way, n_support, n_query, D, _p(u), _p(W), _stream())
    _lib.call("mft_tpn_propagate", E, n_way, n_support, n_query, D, _p(W), int(k), float(alpha), _p(mask), _p(L), _p(F), _p(mk),
              _p(rinv), _p(scores), _stream())
    if not save:
        return scores, None
    return scores, dict(feats=feats, head=(w3, b3, w4, b4), u=u, hid=hid, sig=sig, W=W, L=L, F=F, mask=mk, rinv=rinv, alpha=float(alpha),
                        shape=(E, n_way, n_support, n_query))


def tpn_backward(tape, dscores):
    """d(scores) [episodes*n_way*n_query, n_way] -> (dfeats [rows, 512] with every row written, dW3 [8, 512], db3 [8], dW4 [1, 8],
    db4 [1]) from the forward's tape.  Three launches whatever the shape: propagate backward, affinity backward, the parameter
    sums."""
    E, n_way, n_support, n_query = tape["shape"]
    feats = tape["feats"]
    w3, b3, w4, b4 = tape["head"]
    D, N, Q = TPN_D, n_way * (n_support + n_query), n_way * n_query
    if not dscores.is_cuda:
        raise RuntimeError("TPN head: d(scores) is on %s -- the MI355X path has no CPU fallback" % dscores.device)
    if dscores.dtype != torch.float32 or dscores.dim() != 2 or dscores.stride(1) != 1:
        raise RuntimeError("TPN head: expected float32 d(scores) with unit column stride")
    if tuple(dscores.shape) != (E * Q, n_way):
        raise ValueError("tpn_backward: dscores is %s, expected [%d, %d]" % (tuple(dscores.shape), E * Q, n_way))
    dev = feats.device
    new = lambda *s: torch.empty(s, device=dev, dtype=torch.float32)  # noqa: E731
    dd, dfeats, dw3, db3, dw4, db4 = new(E, N, N), new(E * N, D), new(8, D), new(8), new(1, 8), new(1)
    dnode = torch.empty((E * N, 9), device=dev, dtype=torch.float64)
    _lib.call("mft_tpn_propagate_backward", E, n_way, n_support, n_query, D, _p(tape["W"]), tape["alpha"], _p(tape["L"]), _p(tape["F"]),
              _p(tape["mask"]), _p(tape["rinv"]), _p(dscores), dscores.stride(0), _p(dd), _stream())
    _lib.call("mft_tpn_affinity_backward", E, n_way, n_support, n_query, D, _p(tape["u"]), _p(tape["hid"]), _p(tape["sig"]), _p(dd),
              _p(w3), _p(w4), _p(dfeats), D, _p(dnode), _stream())
    _lib.call("mft_tpn_param_backward", _p(feats), feats.stride(0), E, n_way, n_support, n_query, D, _p(tape["hid"]), _p(dnode),
              _p(dw3), _p(db3), _p(dw4), _p(db4), _stream())
    return dfeats, dw3, db3, dw4, db4


# ---------------------------------------------------------------------------------------------- FEAT head (csrc/feat.hip)
FEAT_D, FEAT_MAX_WAY, FEAT_MAX_T = 512, 32, 128
FEAT_TEMPERATURE, FEAT_TEMPERATURE2, FEAT_BALANCE, FEAT_P_ATT, FEAT_P_OUT = 64.0, 32.0, 0.01, 0.1, 0.5
FEAT_HEAD_SHAPES = ((FEAT_D, FEAT_D), (FEAT_D, FEAT_D), (FEAT_D, FEAT_D), (FEAT_D,), (FEAT_D,), (FEAT_D, FEAT_D), (FEAT_D,))


def feat_check(episodes, n_way, n_support, n_query, D=FEAT_D):
    """The launchers' domain (they return MFT_EINVAL outside it): raise ValueError before anything is launched."""
    if D != FEAT_D:
        raise ValueError("FEAT head: feature dimension %d is not supported (D = %d)" % (D, FEAT_D))
    if not 1 <= int(n_way) <= FEAT_MAX_WAY:
        raise ValueError("FEAT head: n_way = %d is not supported (1 <= n_way <= %d)" % (int(n_way), FEAT_MAX_WAY))
    if int(n_support) < 1 or int(n_query) < 1 or int(episodes) < 1:
        raise ValueError("FEAT head: n_support = %d, n_query = %d, episodes = %d (all must be >= 1)"
                         % (int(n_support), int(n_query), int(episodes)))
    T = int(n_support) + int(n_query)
    if T > FEAT_MAX_T:
        raise ValueError("FEAT head: T = n_support + n_query = %d tokens per class is not supported (T <= %d: one wave holds a "
                         "softmax row)" % (T, FEAT_MAX_T))
    rows = int(episodes) * int(n_way) * (T + 1)
    if rows * FEAT_D >= 2 ** 31 or int(episodes) * int(n_way) * (int(n_way) + T * T) >= 2 ** 31:
        raise ValueError("FEAT head: episodes * n_way * (T + 1) = %d token rows is not supported (32-bit element counts)" % rows)


def feat_counts(episodes, n_way, n_support, n_query, train):
    """(Ntok, number of [t, t] block elements) of a step: the prototype sets, then -- in train mode -- the class sets."""
    T, NP = n_support + n_query, episodes * n_way
    return NP + (NP * T if train else 0), NP * n_way + (NP * T * T if train else 0)


def _feat_head(head):
    head = tuple(head)
    if len(head) != 7:
        raise RuntimeError("FEAT head: expected the seven tensors w_qs, w_ks, w_vs, layer_norm.weight, layer_norm.bias, fc.weight, fc.bias")
    for t, shape in zip(head, FEAT_HEAD_SHAPES):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise RuntimeError("FEAT head: the slf_attn tensors must be float32 tensors on the GPU (no CPU fallback)")
        if t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != shape:
            raise RuntimeError("FEAT head: expected contiguous float32 %s, got %s %s" % (shape, t.dtype, tuple(t.shape)))
    return head


def feat_draw(episodes, n_way, n_support, n_query, seed, index, p_att=FEAT_P_ATT, p_out=FEAT_P_OUT, masks_in=None):
    """The two dropout multipliers of a train-mode step in one launch: (m_att [blocks], m_out [Ntok, 512]), each 0 or 1 / (1 - p),
    from Philox4x32-10 keyed by ``seed`` at the draw index read from ``index`` (int64 [1] on the device; the launch stores
    index + 1, so a replayed hipGraph draws fresh masks).  ``masks_in`` = (m_att, m_out) replaces the draw (tests, golden parity)."""
    feat_check(episodes, n_way, n_support, n_query)
    if not index.is_cuda or index.dtype != torch.int64 or index.numel() != 1:
        raise RuntimeError("FEAT head: the draw index must be an int64 tensor of one element on the GPU")
    ntok, nblk = feat_counts(episodes, n_way, n_support, n_query, True)
    m_att = torch.empty(nblk, device=index.device, dtype=torch.float32)
    m_out = torch.empty((ntok, FEAT_D), device=index.device, dtype=torch.float32)
    ia = io = None
    if masks_in is not None:
        ia, io = masks_in
        for t, n in ((ia, nblk), (io, ntok * FEAT_D)):
            if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != n:
                raise ValueError("FEAT head: forced masks must be contiguous float32 tensors on the GPU with %d and %d elements"
                                 % (nblk, ntok * FEAT_D))
    _lib.call("mft_feat_draw", episodes, n_way, n_support, n_query, FEAT_D, float(p_att), float(p_out), int(seed) & 0xFFFFFFFFFFFFFFFF,
              _p(index), _p(ia), _p(io), _p(m_att), _p(m_out), _stream())
    return m_att, m_out


def feat_forward(feats, head, episodes, n_way, n_support, n_query, train, masks=None, save=False,
                 temperature=FEAT_TEMPERATURE, temperature2=FEAT_TEMPERATURE2):
    """FEAT head forward: feats [episodes*n_way*(n_support+n_query), 512] (class-major rows, one episode after
    the other, row stride >= 512), head = the seven slf_attn tensors in state-dict order -> (scores [episodes*n_way*n_query, n_way],
    reg [episodes*n_way*(n_support+n_query), n_way] | None, tape | None).  ``train``: also the auxiliary sets (one per class) and
    their scores ``reg``.  ``masks`` = (m_att, m_out) multipliers (train mode only; None: all 1).  Six launches whatever the shape:
    tokens, project, attention, fc, norm, scores.  ``save``: keep what feat_backward needs."""
    if not feats.is_cuda:
        raise RuntimeError("FEAT head: input is on %s -- the MI355X path has no CPU fallback; call .cuda() first" % feats.device)
    if feats.dtype != torch.float32 or feats.dim() != 2 or feats.stride(1) != 1:
        raise RuntimeError("FEAT head: expected float32 rows [R, D] with unit column stride, got %s %s" % (feats.dtype, tuple(feats.shape)))
    feat_check(episodes, n_way, n_support, n_query, feats.shape[1])
    E, D, T, train = episodes, FEAT_D, n_support + n_query, bool(train)
    rows, Q = E * n_way * T, n_way * n_query
    if feats.shape[0] != rows:
        raise ValueError("FEAT head: feats %s is not [episodes*n_way*(n_support+n_query) = %d, %d]" % (tuple(feats.shape), rows, D))
    if feats.stride(0) < D or feats.stride(0) % 4 != 0 or feats.data_ptr() % 16 != 0:
        raise ValueError("FEAT head: row stride %d (must be >= %d and a multiple of 4, rows 16-byte aligned)" % (feats.stride(0), D))
    wq, wk, wv, ln_w, ln_b, wfc, bfc = head = _feat_head(head)
    ntok, nblk = feat_counts(E, n_way, n_support, n_query, train)
    m_att = m_out = None
    if masks is not None:
        if not train:
            raise ValueError("FEAT head: dropout multipliers exist in train mode only")
        m_att, m_out = masks
        for t, n in ((m_att, nblk), (m_out, ntok * D)):
            if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != n:
                raise ValueError("FEAT head: the multipliers must be contiguous float32 tensors on the GPU with %d and %d elements"
                                 % (nblk, ntok * D))
    dev = feats.device
    new = lambda *s: torch.empty(s, device=dev, dtype=torch.float32)  # noqa: E731
    X, qkv, P, o, y, A = new(ntok, D), new(3, ntok, D), new(nblk), new(ntok, D), new(ntok, D), new(ntok, D)
    mean, rstd, scores = new(ntok), new(ntok), new(E * Q, n_way)
    centre, reg = (new(E * n_way, D), new(rows, n_way)) if train else (None, None)
    sh = (E, n_way, n_support, n_query, D, 1 if train else 0)
    _lib.call("mft_feat_tokens", _p(feats), feats.stride(0), *sh, _p(X), _stream())
    _lib.call("mft_feat_project", _p(X), *sh, _p(wq), _p(wk), _p(wv), _p(qkv), _stream())
    _lib.call("mft_feat_attention", _p(qkv), *sh, _p(m_att), _p(P), _p(o), _stream())
    _lib.call("mft_feat_fc", _p(o), *sh, _p(wfc), _p(bfc), _p(y), _stream())
    _lib.call("mft_feat_norm", _p(y), _p(X), *sh, _p(m_out), _p(ln_w), _p(ln_b), _p(A), _p(mean), _p(rstd), _stream())
    _lib.call("mft_feat_scores", _p(feats), feats.stride(0), *sh, _p(A), float(temperature), float(temperature2), _p(scores), _p(centre),
              _p(reg), _stream())
    if not save:
        return scores, reg, None
    return scores, reg, dict(feats=feats, head=head, X=X, qkv=qkv, P=P, o=o, y=y, A=A, mean=mean, rstd=rstd, centre=centre, m_att=m_att,
                             m_out=m_out, temps=(float(temperature), float(temperature2)), shape=(E, n_way, n_support, n_query), train=train)


def feat_backward(tape, dscores, dreg=None):
    """d(scores) [episodes*n_way*n_query, n_way] and -- for a train-mode tape -- d(reg) [rows, n_way] (None: zero) -> (dfeats
    [rows, 512] with every row written once, then the gradients of the seven head tensors in state-dict order).  Six launches
    whatever the shape: scores, norm, fc, attention, project backward and the dfeats assembly."""
    E, n_way, n_support, n_query = tape["shape"]
    train, feats = tape["train"], tape["feats"]
    wq, wk, wv, ln_w, ln_b, wfc, bfc = tape["head"]
    D, T, Q = FEAT_D, n_support + n_query, n_way * n_query
    rows = E * n_way * T
    for d, shape, name in ((dscores, (E * Q, n_way), "dscores"), (dreg, (rows, n_way), "dreg")):
        if d is None:
            continue
        if not d.is_cuda:
            raise RuntimeError("FEAT head: %s is on %s -- the MI355X path has no CPU fallback" % (name, d.device))
        if d.dtype != torch.float32 or not d.is_contiguous() or tuple(d.shape) != shape:
            raise ValueError("feat_backward: %s must be contiguous float32 %s, got %s %s" % (name, shape, d.dtype, tuple(d.shape)))
    dev = feats.device
    if train and dreg is None:
        dreg = torch.zeros((rows, n_way), device=dev, dtype=torch.float32)
    if not train and dreg is not None:
        raise ValueError("feat_backward: d(reg) for an eval-mode tape")
    ntok, nblk = feat_counts(E, n_way, n_support, n_query, train)
    new = lambda *s: torch.empty(s, device=dev, dtype=torch.float32)  # noqa: E731
    ddirect, dA, dy, dXres, d_o, dS, dqkv, dX = new(rows, D), new(ntok, D), new(ntok, D), new(ntok, D), new(ntok, D), new(nblk), new(3, ntok, D), new(ntok, D)
    dfeats, dW, dln_w, dln_b, dwfc, dbfc = new(rows, D), new(3, D, D), new(D), new(D), new(D, D), new(D)
    sh = (E, n_way, n_support, n_query, D, 1 if train else 0)
    t1, t2 = tape["temps"]
    _lib.call("mft_feat_scores_backward", _p(feats), feats.stride(0), *sh, _p(tape["A"]), _p(tape["centre"]), _p(dscores), _p(dreg), t1, t2,
              _p(ddirect), _p(dA), _stream())
    _lib.call("mft_feat_norm_backward", _p(dA), _p(tape["y"]), _p(tape["X"]), *sh, _p(tape["m_out"]), _p(ln_w), _p(tape["mean"]),
              _p(tape["rstd"]), _p(dy), _p(dXres), _p(dln_w), _p(dln_b), _p(dbfc), _stream())
    _lib.call("mft_feat_fc_backward", _p(dy), _p(tape["o"]), *sh, _p(wfc), _p(d_o), _p(dwfc), _stream())
    _lib.call("mft_feat_attention_backward", _p(d_o), _p(tape["qkv"]), _p(tape["P"]), _p(tape["m_att"]), *sh, _p(dS), _p(dqkv), _stream())
    _lib.call("mft_feat_project_backward", _p(dqkv), _p(tape["X"]), _p(dXres), *sh, _p(wq), _p(wk), _p(wv), _p(dX), _p(dW), _stream())
    _lib.call("mft_feat_dfeats", _p(ddirect), _p(dX), *sh, _p(dfeats), D, _stream())
    return dfeats, dW[0], dW[1], dW[2], dln_w, dln_b, dwfc, dbfc


def feat_loss(scores, reg, episodes, n_way, n_support, n_query, balance=FEAT_BALANCE, loss_sum=None):
    """out [3] = (CE(scores) + balance CE(reg), CE(scores), CE(reg)), means, the label of a row being its class, in one launch;
    ``reg`` None: the main term alone.  ``loss_sum`` (float64 device scalar) += the main term."""
    out = torch.empty(3, device=scores.device, dtype=torch.float32)
    _lib.call("mft_feat_loss", _p(scores), _p(reg), episodes, n_way, n_support, n_query, float(balance), _p(out), _p(loss_sum), _stream())
    return out


def feat_loss_backward(scores, reg, episodes, n_way, n_support, n_query, grad_loss, balance=FEAT_BALANCE):
    """(dscores, dreg | None) of out[0] * grad_loss (a float32 device scalar, None = 1), one launch."""
    dscores = torch.empty_like(scores)
    dreg = torch.empty_like(reg) if reg is not None else None
    _lib.call("mft_feat_loss_backward", _p(scores), _p(reg), episodes, n_way, n_support, n_query, float(balance), _p(grad_loss),
              _p(dscores), _p(dreg), _stream())
    return dscores, dreg


# ---------------------------------------------------------------------------------------------- DKT head (csrc/dkt.hip)
DKT_D, DKT_MAX_M, DKT_MAX_WAY = 512, 256, 32
DKT_KERNELS = ("cossim", "linear")
DKT_NOISE_FLOOR, DKT_NOISE_INIT = 1e-4, 0.1        # noise = DKT_NOISE_FLOOR + softplus(raw_noise); the constructor's noise
DKT_LOSS_LAUNCHES, DKT_BACKWARD_LAUNCHES, DKT_SCORES_LAUNCHES = 3, 3, 4


def dkt_check(episodes, n_way, n_support, n_query, D=DKT_D, loss=True):
    """The launchers' domain (they return MFT_EINVAL outside it): raise ValueError before anything is launched.  ``loss``: the
    marginal likelihood conditions on all N = n_way * (n_support + n_query) rows of the episode; the scores (``loss=False``) on
    the S = n_way * n_support support rows only, with any n_query."""
    if D != DKT_D:
        raise ValueError("DKT head: feature dimension %d is not supported (D = %d)" % (D, DKT_D))
    if not 1 <= int(n_way) <= DKT_MAX_WAY:
        raise ValueError("DKT head: n_way = %d is not supported (1 <= n_way <= %d)" % (int(n_way), DKT_MAX_WAY))
    if int(n_support) < 1 or int(n_query) < 1 or int(episodes) < 1:
        raise ValueError("DKT head: n_support = %d, n_query = %d, episodes = %d (all must be >= 1)"
                         % (int(n_support), int(n_query), int(episodes)))
    if loss and int(n_way) * (int(n_support) + int(n_query)) > DKT_MAX_M:
        raise ValueError("DKT loss: N = n_way * (n_support + n_query) = %d rows is not supported (N <= %d: the factor of one episode's "
                         "kernel matrix is kept in one workgroup's LDS)" % (int(n_way) * (int(n_support) + int(n_query)), DKT_MAX_M))
    if int(n_way) * int(n_support) > DKT_MAX_M:
        raise ValueError("DKT head: S = n_way * n_support = %d is not supported (S <= %d)" % (int(n_way) * int(n_support), DKT_MAX_M))


def dkt_kernel_id(kernel):
    if kernel not in DKT_KERNELS:
        raise ValueError("DKT head: kernel %r (%s)" % (kernel, " or ".join(DKT_KERNELS)))
    return DKT_KERNELS.index(kernel)


def _dkt_args(feats, hyper, episodes, n_way, n_support, n_query, loss):
    if not feats.is_cuda:
        raise RuntimeError("DKT head: input is on %s -- the MI355X path has no CPU fallback; call .cuda() first" % feats.device)
    if feats.dtype != torch.float32 or feats.dim() != 2 or feats.stride(1) != 1:
        raise RuntimeError("DKT head: expected float32 rows [R, D] with unit column stride, got %s %s" % (feats.dtype, tuple(feats.shape)))
    dkt_check(episodes, n_way, n_support, n_query, feats.shape[1], loss)
    N = n_way * (n_support + n_query)
    if feats.shape[0] != episodes * N:
        raise ValueError("DKT head: feats %s is not [episodes*n_way*(n_support+n_query) = %d, %d]" % (tuple(feats.shape), episodes * N, DKT_D))
    if feats.stride(0) < DKT_D or feats.stride(0) % 4 != 0 or feats.data_ptr() % 16 != 0:
        raise ValueError("DKT head: row stride %d (must be >= %d and a multiple of 4, rows 16-byte aligned)" % (feats.stride(0), DKT_D))
    if len(hyper) != 3:
        raise ValueError("DKT head: hyper = (mean, raw_outputscale, raw_noise)")
    for t in hyper:
        if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float32 or t.numel() != 1:
            raise RuntimeError("DKT head: mean, raw_outputscale and raw_noise must be one-element float32 tensors on the GPU (no CPU fallback)")
    return tuple(hyper)


def dkt_loss_forward(feats, hyper, episodes, n_way, n_support, n_query, kernel="cossim", save=False, loss_sum=None):
    """DKT training loss: feats [episodes*n_way*(n_support+n_query), 512] (class-major rows, one episode after
    the other, row stride >= 512), hyper = (mean, raw_outputscale, raw_noise) one-element device tensors -> (loss [1] = the mean
    over the episodes of the negative marginal log-likelihood of the n_way one-vs-rest processes over N, tape | None).  Three
    launchers whatever the shape: normalise, Gram, factor (which queues the one-thread mean behind it).  ``save``: keep U, the
    row norms, the packed factor, A and the per-episode sums for dkt_loss_backward.  ``loss_sum`` (float64 device scalar) += loss."""
    mean, ros, rno = _dkt_args(feats, hyper, episodes, n_way, n_support, n_query, True)
    lin = dkt_kernel_id(kernel)
    E, D, N = episodes, DKT_D, n_way * (n_support + n_query)
    dev = feats.device
    new = lambda *s: torch.empty(s, device=dev, dtype=torch.float32)  # noqa: E731
    U, K, A, loss = new(E * N, D), new(E, N, N), new(E, N, n_way), new(1)
    nrm = torch.empty(E * N, device=dev, dtype=torch.float64)
    stats = torch.empty((E, 4), device=dev, dtype=torch.float64)
    L = new(E, N * (N + 1) // 2) if save else None
    _lib.call("mft_dkt_normalise", _p(feats), feats.stride(0), E, n_way, n_support, n_query, D, lin, _p(U), _p(nrm), _stream())
    _lib.call("mft_dkt_gram", E, n_way, n_support, n_query, D, 0, _p(U), _p(ros), _p(rno), _p(K), _stream())
    _lib.call("mft_dkt_factor", E, n_way, n_support, n_query, D, 0, _p(U), _p(K), _p(mean), _p(ros), _p(L), _p(A), _p(stats), _p(loss),
              _p(loss_sum), None, _stream())
    if not save:
        return loss, None
    return loss, dict(feats=feats, hyper=(mean, ros, rno), U=U, nrm=nrm, L=L, A=A, stats=stats, linear=lin,
                      shape=(E, n_way, n_support, n_query))


def dkt_loss_backward(tape, grad_loss=None):
    """(dfeats [rows, 512] with every row written, (dmean, draw_outputscale, draw_noise) [1] each) from the forward's
    tape, times ``grad_loss`` (a one-element float32 device tensor; None = 1).  Three launches whatever the shape: the 512
    right-hand sides V = K^-1 U against the saved factor with B = A^T U and tr K^-1, the feature gradient, the three scalar sums."""
    E, n_way, n_support, n_query = tape["shape"]
    mean, ros, rno = tape["hyper"]
    D, N = DKT_D, n_way * (n_support + n_query)
    dev = tape["U"].device
    if grad_loss is not None:
        if not grad_loss.is_cuda:
            raise RuntimeError("DKT head: d(loss) is on %s -- the MI355X path has no CPU fallback" % grad_loss.device)
        if grad_loss.dtype != torch.float32 or grad_loss.numel() != 1:
            raise RuntimeError("DKT head: expected a one-element float32 d(loss)")
    new = lambda *s: torch.empty(s, device=dev, dtype=torch.float32)  # noqa: E731
    V, B, dfeats, dhyper = new(E, N, D), new(E, n_way, D), new(E * N, D), (new(1), new(1), new(1))
    part = torch.empty(E * N, device=dev, dtype=torch.float64)
    trace = torch.empty((E, 16), device=dev, dtype=torch.float64)
    _lib.call("mft_dkt_solve", E, n_way, n_support, n_query, D, _p(tape["U"]), _p(tape["L"]), _p(tape["A"]), _p(V), _p(B), _p(trace),
              _stream())
    _lib.call("mft_dkt_backward", E, n_way, n_support, n_query, D, tape["linear"], _p(tape["U"]), _p(tape["nrm"]), _p(tape["A"]), _p(V),
              _p(B), _p(ros), _p(grad_loss), _p(dfeats), D, _p(part), _stream())
    _lib.call("mft_dkt_hyper_backward", E, n_way, n_support, n_query, D, _p(part), _p(trace), _p(tape["stats"]), _p(ros), _p(rno), _p(grad_loss),
              _p(dhyper[0]), _p(dhyper[1]), _p(dhyper[2]), _stream())
    return dfeats, dhyper


def dkt_scores(feats, hyper, episodes, n_way, n_support, n_query, kernel="cossim"):
    """DKT posterior mean: the process conditioned on the S support rows of each episode, evaluated at its
    queries -> scores [episodes*n_way*n_query, n_way], row = class * n_query + q.  Four launches whatever the shape: normalise,
    Gram of the support rows, factor + A_S + W, scores.  A prediction: nothing is saved and nothing is differentiable."""
    mean, ros, rno = _dkt_args(feats, hyper, episodes, n_way, n_support, n_query, False)
    lin = dkt_kernel_id(kernel)
    E, D, N, S, Q = episodes, DKT_D, n_way * (n_support + n_query), n_way * n_support, n_way * n_query
    dev = feats.device
    new = lambda *s: torch.empty(s, device=dev, dtype=torch.float32)  # noqa: E731
    U, K, A, W, scores = new(E * N, D), new(E, S, S), new(E, S, n_way), new(E, n_way, D), new(E * Q, n_way)
    nrm = torch.empty(E * N, device=dev, dtype=torch.float64)
    _lib.call("mft_dkt_normalise", _p(feats), feats.stride(0), E, n_way, n_support, n_query, D, lin, _p(U), _p(nrm), _stream())
    _lib.call("mft_dkt_gram", E, n_way, n_support, n_query, D, 1, _p(U), _p(ros), _p(rno), _p(K), _stream())
    _lib.call("mft_dkt_factor", E, n_way, n_support, n_query, D, 1, _p(U), _p(K), _p(mean), _p(ros), None, _p(A), None, None, None, _p(W),
              _stream())
    _lib.call("mft_dkt_scores", E, n_way, n_support, n_query, D, _p(U), _p(W), _p(mean), _p(scores), _stream())
    return scores


# ---------------------------------------------------------------------------------------------- ANIL head (csrc/anil.hip)
ANIL_D, ANIL_MAX_WAY, ANIL_MAX_S, ANIL_MAX_STEPS = 512, 32, 256, 16
ANIL_MAX_EPISODES, ANIL_MAX_ROWS = 65535, (1 << 31) // ANIL_D   # per call: a grid dimension, and 32-bit element offsets of the rows
ANIL_FORWARD_LAUNCHES, ANIL_BACKWARD_LAUNCHES = 2, 3        # device kernels, at every shape


def anil_check(episodes, n_way, n_support, n_query, inner_steps, inner_lr, D=ANIL_D):
    """The launchers' domain (they return MFT_EINVAL outside it): raise ValueError before anything is launched."""
    if D != ANIL_D:
        raise ValueError("ANIL head: feature dimension %d is not supported (D = %d)" % (D, ANIL_D))
    if not 1 <= int(n_way) <= ANIL_MAX_WAY:
        raise ValueError("ANIL head: n_way = %d is not supported (1 <= n_way <= %d)" % (int(n_way), ANIL_MAX_WAY))
    if int(n_support) < 1 or int(n_query) < 1 or int(episodes) < 1:
        raise ValueError("ANIL head: n_support = %d, n_query = %d, episodes = %d (all must be >= 1)"
                         % (int(n_support), int(n_query), int(episodes)))
    if int(n_way) * int(n_support) > ANIL_MAX_S:
        raise ValueError("ANIL head: S = n_way * n_support = %d is not supported (S <= %d: one workgroup walks the inner steps of an "
                         "episode with its softmax panel in LDS)" % (int(n_way) * int(n_support), ANIL_MAX_S))
    rows = int(episodes) * int(n_way) * (int(n_support) + int(n_query))
    if int(episodes) > ANIL_MAX_EPISODES or rows >= ANIL_MAX_ROWS:
        raise ValueError("ANIL head: episodes = %d, %d feature rows in all are not supported (episodes <= %d, rows < %d per call)"
                         % (int(episodes), rows, ANIL_MAX_EPISODES, ANIL_MAX_ROWS))
    if int(inner_steps) != inner_steps or not 1 <= int(inner_steps) <= ANIL_MAX_STEPS:
        raise ValueError("ANIL head: inner_steps = %r is not supported (1 <= inner_steps <= %d)" % (inner_steps, ANIL_MAX_STEPS))
    if not 0.0 < float(inner_lr) < float("inf"):
        raise ValueError("ANIL head: inner_lr = %r (must be positive and finite)" % (inner_lr,))


def _anil_rows(t, what):
    if not t.is_cuda:
        raise RuntimeError("ANIL head: %s is on %s -- the MI355X path has no CPU fallback; call .cuda() first" % (what, t.device))
    if t.dtype != torch.float32:
        raise RuntimeError("ANIL head: expected float32 %s, got %s" % (what, t.dtype))


def anil_forward(feats, W0, b0, episodes, n_way, n_support, n_query, inner_steps, inner_lr, save=False):
    """ANIL head: feats [episodes*n_way*(n_support+n_query), 512] (class-major rows, one episode after the
    other, row stride >= 512), W0 [n_way, 512], b0 [n_way] -> (scores [episodes*n_way*n_query, n_way], tape | None).  Two launches
    whatever the shape: the walk of the ``inner_steps`` gradient steps of size ``inner_lr`` on each episode's support rows (one
    workgroup per episode), the scores of the adapted classifier.  ``save``: keep the classifiers and softmaxes of every step for
    anil_backward."""
    _anil_rows(feats, "feats")
    _anil_rows(W0, "W0")
    _anil_rows(b0, "b0")
    if feats.dim() != 2 or feats.stride(1) != 1:
        raise RuntimeError("ANIL head: expected rows [R, D] with unit column stride, got %s" % (tuple(feats.shape),))
    anil_check(episodes, n_way, n_support, n_query, inner_steps, inner_lr, feats.shape[1])
    E, D, K = int(episodes), ANIL_D, int(inner_steps)
    N, S, Q = n_way * (n_support + n_query), n_way * n_support, n_way * n_query
    if feats.shape[0] != E * N:
        raise ValueError("ANIL head: feats %s is not [episodes*n_way*(n_support+n_query) = %d, %d]" % (tuple(feats.shape), E * N, D))
    if feats.stride(0) < D or feats.stride(0) % 4 != 0 or feats.data_ptr() % 16 != 0:
        raise ValueError("ANIL head: row stride %d (must be >= %d and a multiple of 4, rows 16-byte aligned)" % (feats.stride(0), D))
    if tuple(W0.shape) != (n_way, D) or tuple(b0.shape) != (n_way,):
        raise ValueError("ANIL head: W0 %s, b0 %s are not [%d, %d], [%d]" % (tuple(W0.shape), tuple(b0.shape), n_way, D, n_way))
    if not W0.is_contiguous() or not b0.is_contiguous() or W0.data_ptr() % 16 != 0:
        raise ValueError("ANIL head: W0 and b0 must be contiguous, W0 16-byte aligned")
    dev = feats.device
    new = lambda *s: torch.empty(s, device=dev, dtype=torch.float32)  # noqa: E731
    Wt, bt, scores = new(E, K + 1, n_way, D), new(E, K + 1, n_way), new(E * Q, n_way)
    P = new(E, K, S, n_way) if save else None
    lr = float(inner_lr)
    _lib.call("mft_anil_adapt", _p(feats), feats.stride(0), E, n_way, n_support, n_query, D, _p(W0), _p(b0), K, lr, _p(Wt), _p(bt), _p(P),
              _stream())
    _lib.call("mft_anil_scores", _p(feats), feats.stride(0), E, n_way, n_support, n_query, D, K, _p(Wt), _p(bt), _p(scores), _stream())
    if not save:
        return scores, None
    return scores, dict(feats=feats, W=Wt, b=bt, P=P, shape=(E, n_way, n_support, n_query), inner_steps=K, inner_lr=lr)


def anil_backward(tape, dscores):
    """(dfeats [rows, 512] with every row written, dW0 [n_way, 512], db0 [n_way]) from the forward's tape and ``dscores``
    [episodes*n_way*n_query, n_way] (float32, read on the device).  Three device kernels whatever the shape: the query side (dZ_Q and
    each episode's gW, gb behind the last step), the reverse walk with the softmax Jacobian (one workgroup per episode), and behind
    it dZ_S from the tapes with the sum of the episodes' gradients in episode order."""
    E, n_way, n_support, n_query = tape["shape"]
    K, lr, feats = tape["inner_steps"], tape["inner_lr"], tape["feats"]
    D, N, S, Q = ANIL_D, n_way * (n_support + n_query), n_way * n_support, n_way * n_query
    _anil_rows(dscores, "d(scores)")
    if tuple(dscores.shape) != (E * Q, n_way) or not dscores.is_contiguous():
        raise ValueError("ANIL head: d(scores) %s is not a contiguous [%d, %d]" % (tuple(dscores.shape), E * Q, n_way))
    dev = feats.device
    new = lambda *s: torch.empty(s, device=dev, dtype=torch.float32)  # noqa: E731
    gW, gb, R = new(E, K + 1, n_way, D), new(E, K + 1, n_way), new(E, K, S, n_way)
    dfeats, dW0, db0 = new(E * N, D), new(n_way, D), new(n_way)
    _lib.call("mft_anil_scores_backward", _p(feats), feats.stride(0), E, n_way, n_support, n_query, D, K, _p(tape["W"]), _p(dscores),
              _p(dfeats), D, _p(gW), _p(gb), _stream())
    _lib.call("mft_anil_adapt_backward", _p(feats), feats.stride(0), E, n_way, n_support, n_query, D, K, lr, _p(tape["W"]), _p(tape["P"]),
              _p(gW), _p(gb), _p(R), _p(dfeats), D, _p(dW0), _p(db0), _stream())
    return dfeats, dW0, db0


# ---------------------------------------------------------------------------------------------- Mahalanobis head (csrc/mahalanobis.hip)
MAHALANOBIS_D, MAHALANOBIS_MAX_WAY, MAHALANOBIS_MAX_S = 512, 32, 256
MAHALANOBIS_MAX_EPISODES, MAHALANOBIS_MAX_ROWS = 65535, (1 << 31) // MAHALANOBIS_D   # per call: a grid dimension, 32-bit row offsets
MAHALANOBIS_BETA = 1.0                                              # the ridge on every class covariance; a constant of the kernels
MAHALANOBIS_FORWARD_LAUNCHES, MAHALANOBIS_BACKWARD_LAUNCHES = 3, 3  # device kernels, at every shape


def mahalanobis_check(episodes, n_way, n_support, n_query, D=MAHALANOBIS_D):
    """The launchers' domain (they return MFT_EINVAL outside it): raise ValueError before anything is launched."""
    if D != MAHALANOBIS_D:
        raise ValueError("Mahalanobis head: feature dimension %d is not supported (D = %d)" % (D, MAHALANOBIS_D))
    if not 1 <= int(n_way) <= MAHALANOBIS_MAX_WAY:
        raise ValueError("Mahalanobis head: n_way = %d is not supported (1 <= n_way <= %d)" % (int(n_way), MAHALANOBIS_MAX_WAY))
    if int(n_support) < 1 or int(n_query) < 1 or int(episodes) < 1:
        raise ValueError("Mahalanobis head: n_support = %d, n_query = %d, episodes = %d (all must be >= 1)"
                         % (int(n_support), int(n_query), int(episodes)))
    if int(n_way) * int(n_support) > MAHALANOBIS_MAX_S:
        raise ValueError("Mahalanobis head: S = n_way * n_support = %d is not supported (S <= %d: one workgroup keeps the packed S x S "
                         "factor of a class in LDS)" % (int(n_way) * int(n_support), MAHALANOBIS_MAX_S))
    rows = int(episodes) * int(n_way) * (int(n_support) + int(n_query))
    if int(episodes) > MAHALANOBIS_MAX_EPISODES or rows >= MAHALANOBIS_MAX_ROWS:
        raise ValueError("Mahalanobis head: episodes = %d, %d feature rows in all are not supported (episodes <= %d, rows < %d per call)"
                         % (int(episodes), rows, MAHALANOBIS_MAX_EPISODES, MAHALANOBIS_MAX_ROWS))


def _mahalanobis_rows(t, what):
    if not t.is_cuda:
        raise RuntimeError("Mahalanobis head: %s is on %s -- the MI355X path has no CPU fallback; call .cuda() first" % (what, t.device))
    if t.dtype != torch.float32:
        raise RuntimeError("Mahalanobis head: expected float32 %s, got %s" % (what, t.dtype))


def mahalanobis_forward(feats, episodes, n_way, n_support, n_query, save=False):
    """Mahalanobis head: feats [episodes*n_way*(n_support+n_query), 512] (class-major rows, one episode after
    the other, row stride >= 512) -> (scores [episodes*n_way*n_query, n_way], tape | None).  Three launches whatever the shape: the
    class means and the centred support rows, their Gram matrix, and the factor-and-solve launch (one workgroup per episode and
    class).  ``save``: keep the solutions w of every (query, class) pair for mahalanobis_backward."""
    _mahalanobis_rows(feats, "feats")
    if feats.dim() != 2 or feats.stride(1) != 1:
        raise RuntimeError("Mahalanobis head: expected rows [R, D] with unit column stride, got %s" % (tuple(feats.shape),))
    mahalanobis_check(episodes, n_way, n_support, n_query, feats.shape[1])
    E, D = int(episodes), MAHALANOBIS_D
    N, S, Q = n_way * (n_support + n_query), n_way * n_support, n_way * n_query
    if feats.shape[0] != E * N:
        raise ValueError("Mahalanobis head: feats %s is not [episodes*n_way*(n_support+n_query) = %d, %d]" % (tuple(feats.shape), E * N, D))
    if feats.stride(0) < D or feats.stride(0) % 4 != 0 or feats.data_ptr() % 16 != 0:
        raise ValueError("Mahalanobis head: row stride %d (must be >= %d and a multiple of 4, rows 16-byte aligned)" % (feats.stride(0), D))
    dev = feats.device
    new = lambda *s: torch.empty(s, device=dev, dtype=torch.float32)  # noqa: E731
    T, Mu, scores = new(E, S, D), new(E, n_way, D), new(E * Q, n_way)
    G = torch.empty((E, S, S), device=dev, dtype=torch.float64)
    W = new(E, Q, n_way, S) if save else None
    shape = (E, n_way, n_support, n_query, D)
    _lib.call("mft_mahalanobis_centre", _p(feats), feats.stride(0), *shape, _p(T), _p(Mu), _stream())
    _lib.call("mft_mahalanobis_gram", *shape, _p(T), _p(G), _stream())
    _lib.call("mft_mahalanobis_scores", _p(feats), feats.stride(0), *shape, _p(T), _p(Mu), _p(G), _p(scores), _p(W), _stream())
    if not save:
        return scores, None
    return scores, dict(feats=feats, T=T, Mu=Mu, W=W, shape=(E, n_way, n_support, n_query))


def mahalanobis_backward(tape, dscores):
    """dfeats [rows, 512] (every row written) from the forward's tape and ``dscores`` [episodes*n_way*n_query, n_way] (float32, read
    on the device).  Three device kernels whatever the shape: the coefficient matrices of the gradient rows from dscores and w, the
    gradient rows as combinations of the rows of Z_Q, Mu and T (dZ_Q, and dT and the class-mean terms into a work array), and the
    support rows from that array with the two mean corrections."""
    E, n_way, n_support, n_query = tape["shape"]
    feats = tape["feats"]
    D, N, S, Q = MAHALANOBIS_D, n_way * (n_support + n_query), n_way * n_support, n_way * n_query
    _mahalanobis_rows(dscores, "d(scores)")
    if tuple(dscores.shape) != (E * Q, n_way) or not dscores.is_contiguous():
        raise ValueError("Mahalanobis head: d(scores) %s is not a contiguous [%d, %d]" % (tuple(dscores.shape), E * Q, n_way))
    dev = feats.device
    new64 = lambda *s: torch.empty(s, device=dev, dtype=torch.float64)  # noqa: E731
    Om, Ph, Ps = new64(E, Q, S), new64(E, n_way, S), new64(E, S, S)
    X = torch.empty((E, S + n_way, D), device=dev, dtype=torch.float32)
    dfeats = torch.empty((E * N, D), device=dev, dtype=torch.float32)
    shape = (E, n_way, n_support, n_query, D)
    _lib.call("mft_mahalanobis_coef", *shape, _p(tape["W"]), _p(dscores), _p(Om), _p(Ph), _p(Ps), _stream())
    _lib.call("mft_mahalanobis_backward", _p(feats), feats.stride(0), *shape, _p(tape["T"]), _p(tape["Mu"]), _p(dscores), _p(Om), _p(Ph),
              _p(Ps), _p(X), _p(dfeats), D, _stream())
    return dfeats


# ---------------------------------------------------------------------------------------------- MetaOptNet SVM head (csrc/svm.hip)
SVM_C = 0.1                        # the published C_reg; a constant of the kernels
SVM_MAX_PRODUCTS = 65536            # MFT_SVM_MAX_PRODUCTS: products M x [S, n_way] per episode before status = 1
_SVM_WORK = 1024 * 16               # float64 workspace of mft_svm_solve per episode

svm_check = ridge_check             # the SVM launchers' domain is the ridge head's


def _svm_gram(feats, E, n_way, n_support, n_query):
    S = n_way * n_support
    M = torch.empty((E, S, S), device=feats.device, dtype=torch.float64)
    _lib.call("mft_svm_gram", _p(feats), feats.stride(0), E, n_way, n_support, n_query, RIDGE_D, _p(M), _stream())
    return M


def svm_forward(feats, scale, episodes, n_way, n_support, n_query, softmax=False, save=False):
    """MetaOptNet-SVM head forward: feats and scale as for ridge_forward -> (scores
    [episodes*n_way*n_query, n_way], tape); ``softmax``: the row softmax of the scores instead.  Three launches whatever the shape:
    float64 Gram matrix, the dual solve (alpha, free mask, W, status), mft_ridge_scores.  The tape always holds ``status``
    [episodes] int32 (0 = the optimality test passed) and ``products`` [episodes] (the solve's products M x [S, n_way]), neither
    read back here; ``save``: also alpha, the free mask and W for svm_backward."""
    _ridge_feats(feats, episodes, n_way, n_support, n_query)
    _ridge_scale(scale)
    E, D, S, Q = episodes, RIDGE_D, n_way * n_support, n_way * n_query
    dev = feats.device
    new = lambda *s: torch.empty(s, device=dev, dtype=torch.float32)  # noqa: E731
    alpha, W, scores = new(E, S, n_way), new(E, n_way, D), new(E * Q, n_way)
    free = torch.empty((E, S, n_way), device=dev, dtype=torch.uint8)
    status = torch.empty((E,), device=dev, dtype=torch.int32)
    work = torch.empty((E, _SVM_WORK), device=dev, dtype=torch.float64)
    M = _svm_gram(feats, E, n_way, n_support, n_query)
    ld = feats.stride(0)
    _lib.call("mft_svm_solve", _p(feats), ld, E, n_way, n_support, n_query, D, _p(M), _p(work), _p(alpha), _p(free), _p(W), _p(status),
              _stream())
    _lib.call("mft_ridge_scores", _p(feats), ld, E, n_way, n_support, n_query, D, _p(W), _p(scale), _p(scores), 1 if softmax else 0,
              _stream())
    products = work[:, 0]               # float64 [episodes]: products M x [S, n_way] the solve used
    if not save:
        return scores, dict(status=status, products=products)
    return scores, dict(feats=feats, scale=scale, alpha=alpha, free=free, W=W, status=status, products=products,
                        shape=(E, n_way, n_support, n_query))


def svm_backward(tape, dscores):
    """d(scores) [episodes*n_way*n_query, n_way] -> (dfeats [rows, 512] with every row written, dscale [1]) from svm_forward's
    tape.  Three launches whatever the shape: the float64 Gram matrix again (it is not kept), mft_ridge_backward_query (dZ_Q, dW,
    the shares of dscale), the support side (A, the adjoint solve for U on the saved free mask, dZ_S)."""
    E, n_way, n_support, n_query = tape["shape"]
    feats, scale = tape["feats"], tape["scale"]
    D, Q = RIDGE_D, n_way * n_query
    if not dscores.is_cuda:
        raise RuntimeError("MetaOptNet head: d(scores) is on %s -- the MI355X path has no CPU fallback" % dscores.device)
    if dscores.dtype != torch.float32 or dscores.dim() != 2 or dscores.stride(1) != 1:
        raise RuntimeError("MetaOptNet head: expected float32 d(scores) with unit column stride")
    if tuple(dscores.shape) != (E * Q, n_way):
        raise ValueError("svm_backward: dscores is %s, expected [%d, %d]" % (tuple(dscores.shape), E * Q, n_way))
    new = lambda *s: torch.empty(s, device=feats.device, dtype=torch.float32)  # noqa: E731
    dfeats, dW, dscale = new(feats.shape[0], D), new(E, n_way, D), new(1)
    part = torch.empty(E * 8, device=feats.device, dtype=torch.float64)
    M = _svm_gram(feats, E, n_way, n_support, n_query)
    ld = feats.stride(0)
    _lib.call("mft_ridge_backward_query", _p(feats), ld, E, n_way, n_support, n_query, D, _p(tape["W"]), _p(scale), _p(dscores),
              dscores.stride(0), _p(dfeats), D, _p(dW), _p(part), _stream())
    _lib.call("mft_svm_backward_support", _p(feats), ld, E, n_way, n_support, n_query, D, _p(M), _p(tape["alpha"]), _p(tape["free"]),
              _p(tape["W"]), _p(dW), _p(part), _p(dfeats), D, _p(dscale), _stream())
    return dfeats, dscale
