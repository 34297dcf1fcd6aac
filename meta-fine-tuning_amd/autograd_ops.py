"""Bridge between the reference-shaped nn.Modules (OIHW nn.Parameters, autograd, optimisers) and the
HIP functional layer.  Parameters are repacked into the kernels' layouts lazily (cache keyed on the
tensors' autograd version counters) and gradients are handed back in the reference's layouts.
"""
import contextlib

import torch

from . import functional as Fn
from . import functional_bwd as FB
from . import ops

_ARENAS = {}


def arena_for(device):
    a = _ARENAS.get(device)
    if a is None:
        a = Fn.Arena(device)
        _ARENAS[device] = a
    return a


def _require_cuda(x, what):
    if not x.is_cuda:
        raise RuntimeError("%s: input is on %s -- the MI355X path has no CPU fallback; call .cuda() first" % (what, x.device))


def module_weights(mod):
    """Packed ResNet10Weights of a backbone.ResNet module, rebuilt only when a parameter changed."""
    params = list(mod.parameters())
    key = tuple((p.data_ptr(), p._version) for p in params)
    cache = mod.__dict__.get("_mft_pack")
    if cache is None or cache[0] != key:
        if cache is not None and cache[1].can_repack() and _same_storage(cache[0], key):
            cache[1].repack()             # same tensors, new values (optimizer.step): one launch refreshes every packed copy
            W = cache[1]
        else:
            sd = {k: v for k, v in mod.state_dict().items()}
            W = Fn.ResNet10Weights(sd, params[0].device)
        cache = (key, W)
        mod.__dict__["_mft_pack"] = cache
    return cache[1]


def _same_storage(old_key, new_key):
    return len(old_key) == len(new_key) and all(a[0] == b[0] for a, b in zip(old_key, new_key))


def _running(mod):
    """name -> (running_mean, running_var, num_batches_tracked) of every tracking BatchNorm2d: the statistics launch of each layer
    advances all three (mft_bn_stats), so a forward costs no counter launch of its own."""
    run = {}
    for name, m in mod.named_modules():
        if isinstance(m, torch.nn.BatchNorm2d) and m.track_running_stats:
            run[name] = (m.running_mean, m.running_var, m.num_batches_tracked)
    return run


def _eval_weights(mod, W):
    """Eval-mode BatchNorm: statistics come from the running buffers."""
    stats = {}
    for name, m in mod.named_modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            rstd = torch.empty_like(m.running_var)
            ops._lib.call("mft_var_to_rstd", ops._p(m.running_var), ops._p(rstd), rstd.numel(), m.eps, ops._stream())
            stats[name] = (m.running_mean.view(1, -1), rstd.view(1, -1))
    return stats


# ---------------------------------------------------------------------------------------------- feature-wise transformation

def is_feature_wise(mod):
    """A backbone.ResNet built from SimpleBlock2 (ResNet10_FW)."""
    return bool(getattr(mod, "feature_wise", False))


def _base_params(mod):
    """The parameters ResNet10 has too, in its order (the feature-wise transformation's gamma / beta sit in between)."""
    if not is_feature_wise(mod):
        return list(mod.parameters())
    return [p for n, p in mod.named_parameters() if not n.endswith((".gamma", ".beta"))]


def fwt_seed(mod):
    """The generator key of this process: the module's ``fwt_seed`` with the rank mixed in, so that ranks draw different noise and
    the same (rank, seed, draw index) reproduces it."""
    from . import parallel
    return (int(mod.fwt_seed) + 0x9E3779B97F4A7C15 * parallel.world()[0]) & 0xFFFFFFFFFFFFFFFF


def fwt_draw(mod, groups):
    """Draw the noise of one train-mode forward of a ResNet10_FW module (``groups`` independent sets: one per lockstep episode, as
    each episode is a forward call of its own in the reference) and fold it into the seven layers' affine parameters: ONE launch,
    which also advances the module's draw index on the device."""
    from . import backbone
    named = dict(mod.named_parameters())
    layers, need = [], []
    for name, C, col in backbone.FWT_LAYERS:
        w, b, gamma, beta = (named["%s.%s" % (name, k)] for k in ("weight", "bias", "gamma", "beta"))
        for p in (w, b, gamma, beta):
            if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
                raise RuntimeError("ResNet10_FW: %s parameters must be contiguous float32 tensors on the GPU (no CPU fallback)" % name)
        layers.append((name, C, col, w.detach(), b.detach(), gamma.detach().view(-1), beta.detach().view(-1)))
        if gamma.requires_grad or beta.requires_grad:
            need.append(name)
    return FB.FwtState(layers, groups, backbone.FWT_COLS, fwt_seed(mod), mod.fwt_draw_index, noise_in=mod.__dict__.get("_fwt_forced"),
                       need_gamma_beta=need)


@contextlib.contextmanager
def fwt_forced_noise(mod, noise):
    """Tests and golden parity only: inside the block every train-mode forward of ``mod`` takes its normals from ``noise``
    [groups, 2, 1856] (float32, on the module's device) instead of the generator; the draw index still advances."""
    if not is_feature_wise(mod):
        raise ValueError("fwt_forced_noise: not a ResNet10_FW module")
    mod.__dict__["_fwt_forced"] = noise
    try:
        yield mod
    finally:
        mod.__dict__.pop("_fwt_forced", None)


class _ResNet10Fn(torch.autograd.Function):
    """ResNet10 forward on HIP; backward through the last block only (the inner-loop regime: everything
    below trunk.7 is frozen -- finetune.py:242-252)."""

    @staticmethod
    def forward(ctx, mod, x_nhwc, *params):
        W = module_weights(mod)
        arena = arena_for(x_nhwc.device)
        n = x_nhwc.shape[0]
        slab = Fn.LastBlockSlab(1, x_nhwc.device, zero=False)
        slab.load_shared(W)
        tape = {}
        feat = Fn.resnet10_forward(W, x_nhwc, arena, ipg=n, slab=slab, tape=tape, running=_running(mod), tag="mod%d" % n)
        ctx.tape, ctx.slab, ctx.n, ctx.mod = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in tape.items()}, slab, n, mod
        return feat.clone()

    @staticmethod
    def backward(ctx, dfeat):
        mod = ctx.mod
        names = [n for n, _ in mod.named_parameters()]
        need = [p.requires_grad for p in mod.parameters()]
        if any(need[:-9]):
            raise NotImplementedError(
                "backward below trunk.7 requested (%s): use methods.gnnnet.GnnNet.set_forward_loss for the "
                "meta-train path" % [n for n, r in zip(names, need) if r][0])
        grads = Fn.LastBlockSlab(1, dfeat.device)
        arena = arena_for(dfeat.device)
        Fn.last_block_backward(ctx.tape, dfeat.contiguous(), ctx.slab, grads, arena, ipg=ctx.n, tag="modbw%d" % ctx.n)
        g = grads.export(0)
        out = [None] * len(names)
        for i, nm in enumerate(names):
            if nm in g and need[i]:
                out[i] = g[nm]
        return (None, None) + tuple(out)


class _ResNet10FullFn(torch.autograd.Function):
    """ResNet10 forward + full backward on HIP (meta-training: every parameter receives a gradient,
    train.py:28; meta_template.py:76-92)."""

    @staticmethod
    def forward(ctx, mod, x_nhwc, groups, *params):
        W = module_weights(mod)
        fwt = fwt_draw(mod, groups) if is_feature_wise(mod) else None
        feat, tape = FB.resnet10_forward_taped(W, x_nhwc, running=_running(mod), groups=groups, fwt=fwt)
        ctx.tape, ctx.W, ctx.mod = tape, W, mod
        return feat

    @staticmethod
    def backward(ctx, dfeat):
        mod = ctx.mod
        names = [n for n, _ in mod.named_parameters()]
        need = [p.requires_grad for p in mod.parameters()]
        g = FB.resnet10_backward(ctx.W, ctx.tape, dfeat.contiguous().float(), set(names))
        out = [g[nm] if r else None for nm, r in zip(names, need)]         # (gamma / beta of a feature-wise layer: frozen by default)
        return (None, None, None) + tuple(out)


class _HeadFn(torch.autograd.Function):
    """GnnNet.fc + graph assembly + GNN_nl + score gather with a hand-written backward (gnnnet.py:76-87,210-217)."""

    @staticmethod
    def forward(ctx, model, feats, n_support, n_query, fold, episodes, *params):
        G = head_weights(model.gnn, model.fc, model.n_way)
        scores, tape = FB.head_forward_taped(G, feats.contiguous().float(), model.n_way, n_support, n_query, fold, episodes)
        ctx.tape, ctx.G, ctx.model = tape, G, model
        ctx.feats_need = feats.requires_grad
        return scores

    @staticmethod
    def backward(ctx, dscores):
        model = ctx.model
        dfeats, g = FB.head_backward(ctx.G, ctx.tape, dscores.contiguous().float())
        names = ["fc." + n for n, _ in model.fc.named_parameters()] + ["gnn." + n for n, _ in model.gnn.named_parameters()]
        plist = list(model.fc.parameters()) + list(model.gnn.parameters())
        out = [g[nm].view_as(p) if p.requires_grad else None for nm, p in zip(names, plist)]
        return (None, dfeats if ctx.feats_need else None, None, None, None, None) + tuple(out)


class _CrossEntropyFn(torch.autograd.Function):
    """nn.CrossEntropyLoss()(scores, y) = mean_r(logsumexp(scores_r) - scores_r[y_r]) with ONE launch each way
    (mft_cross_entropy_mean / _backward; gnnnet.py:219-231, baselinetrain.py:38-45).  Labels are read as given (int64 or int32)."""

    @staticmethod
    def forward(ctx, logits, target, loss_sum):
        rows, C = logits.shape
        loss = torch.empty((), device=logits.device, dtype=torch.float32)
        ops._lib.call("mft_cross_entropy_mean", ops._p(logits), logits.stride(0), ops._p(target), 1 if target.dtype == torch.int64 else 0,
                      C, rows, ops._p(loss), ops._p(loss_sum), ops._stream())
        ctx.save_for_backward(logits, target)
        return loss

    @staticmethod
    def backward(ctx, g):
        logits, target = ctx.saved_tensors
        rows, C = logits.shape
        d = torch.empty((rows, C), device=logits.device, dtype=torch.float32)
        g = g.contiguous().float()
        ops._lib.call("mft_cross_entropy_mean_backward", ops._p(logits), logits.stride(0), ops._p(target),
                      1 if target.dtype == torch.int64 else 0, C, rows, ops._p(g), ops._p(d), C, ops._stream())
        return d, None, None


class CrossEntropyLoss(torch.nn.CrossEntropyLoss):
    """``nn.CrossEntropyLoss()`` as the episode / pre-training losses use it (gnnnet.py:43, baselinetrain.py:20: default arguments,
    [rows, C] float scores against [rows] class indices), computed by the HIP library.  Same class hierarchy and attributes as
    torch's module; anything outside that use (class weights, label smoothing, probabilities as targets, a CPU tensor) raises --
    there is no torch fallback on the product path."""

    def forward(self, input, target):
        if (self.weight is not None or self.reduction != "mean" or self.label_smoothing != 0.0 or input.dim() != 2 or target.dim() != 1
                or target.dtype not in (torch.int64, torch.int32) or target.shape[0] != input.shape[0]):
            raise NotImplementedError("CrossEntropyLoss on the HIP path: default options, [rows, C] scores, [rows] int64 / int32 labels")
        _require_cuda(input, "CrossEntropyLoss")
        if not target.is_cuda:
            raise RuntimeError("CrossEntropyLoss: labels are on the CPU -- the MI355X path has no CPU fallback; call .cuda() first")
        if input.dtype != torch.float32 or input.stride(1) != 1:
            input = input.float().contiguous()
        return _CrossEntropyFn.apply(input, target.contiguous(), self.loss_sum(input.device))

    def loss_sum(self, device=None):
        """float64 device scalar that every forward of this module adds its loss to (one per device, never re-created: a recorded
        hipGraph keeps writing it).  The episode loops print running means from differences of it -- one read-back per printed
        line instead of one per step (meta_template.py:91-93)."""
        sums = self.__dict__.setdefault("_mft_loss_sums", {})
        if device is None:
            return next(iter(sums.values()), None)
        key = torch.device(device).index
        t = sums.get(key)
        if t is None:
            t = sums[key] = torch.zeros((), device=device, dtype=torch.float64)
        return t


def resnet10_module_forward(mod, x, groups=1):
    """backbone.ResNet.forward: x NCHW [n,3,H,W] on the GPU -> [n,512].  ``groups`` > 1 (meta-training only): the n images are
    ``groups`` episodes one after the other, each a BatchNorm mini-batch of its own (GnnNet.set_forward_loss_lockstep)."""
    _require_cuda(x, "ResNet10.forward")
    if groups != 1 and not (mod.training and torch.is_grad_enabled() and all(p.requires_grad for p in _base_params(mod))):
        raise NotImplementedError("several BatchNorm groups per call exist on the meta-training path only (train mode, every "
                                  "backbone parameter trainable)")
    if x.dim() == 4 and x.dtype == torch.float32 and x.permute(0, 2, 3, 1).is_contiguous():
        xn = x.permute(0, 2, 3, 1)            # already NHWC in memory (train.ResidentEpisodeLoader: mft_augment_views writes NHWC)
    else:
        x = x.contiguous().float()
        xn = ops.nchw_to_nhwc(x)
    params = list(mod.parameters())
    if not mod.training:
        # eval-mode BatchNorm (finetune(freeze_backbone=True), finetune.py:265-266): running statistics, no buffer updates
        if torch.is_grad_enabled() and any(p.requires_grad for p in params):
            raise NotImplementedError("autograd through an eval-mode backbone is not on the HIP hot path (the reference only "
                                      "evaluates it: the frozen-backbone loop has no optimiser, finetune.py:253-299)")
        W = module_weights(mod)
        n = xn.shape[0]
        return Fn.resnet10_forward(W, xn, arena_for(xn.device), ipg=n, fixed=_eval_weights(mod, W), tag="evl%d" % n).clone()
    if is_feature_wise(mod):
        # train-mode ResNet10_FW: always the taped launches (the only ones that take a per-group affine); without autograd the
        # tape is dropped.  The noise stays on: the reference draws in every train-mode forward.
        base = _base_params(mod)
        if torch.is_grad_enabled() and any(p.requires_grad for p in params):
            if not any(p.requires_grad for p in base[:-9]):
                raise NotImplementedError("ResNet10_FW: the last-block-only backward (the inner-loop regime) is not built for the "
                                          "feature-wise transformation backbone; train it with every parameter trainable")
            return _ResNet10FullFn.apply(mod, xn, groups, *params)
        return FB.resnet10_forward_taped(module_weights(mod), xn, running=_running(mod), groups=groups, fwt=fwt_draw(mod, groups))[0]
    if torch.is_grad_enabled() and any(p.requires_grad for p in params):
        if any(p.requires_grad for p in params[:-9]):
            out = _ResNet10FullFn.apply(mod, xn, groups, *params)       # meta-training: gradients for the whole backbone
        else:
            out = _ResNet10Fn.apply(mod, xn, *params)           # inner loop: last block only
    else:
        W = module_weights(mod)
        n = xn.shape[0]
        out = Fn.resnet10_forward(W, xn, arena_for(xn.device), ipg=n, running=_running(mod), tag="mod%d" % n).clone()
    return out            # (every BatchNorm's num_batches_tracked was advanced by its own statistics launch: _running)


# ---------------------------------------------------------------------------------------------- packing

def pad_rows(x2d, ld):
    out = torch.zeros((x2d.shape[0], ld), device=x2d.device)
    out[:, :x2d.shape[1]] = x2d
    return out


def _version_key(mod):
    return tuple((p.data_ptr(), p._version) for p in mod.parameters())


def head_weights(gnn_mod, fc_mod=None, n_way=None):
    """Packed GnnHeadWeights for a GNN_nl (and optionally GnnNet.fc), cached on the parameter versions."""
    key = _version_key(gnn_mod) + (() if fc_mod is None else _version_key(fc_mod))
    cache = gnn_mod.__dict__.get("_mft_pack")
    if cache is not None and cache[0] != key and fc_mod is not None and cache[1].can_repack() and _same_storage(cache[0], key):
        cache[1].repack()
        cache = (key, cache[1])
        gnn_mod.__dict__["_mft_pack"] = cache
    if cache is None or cache[0] != key:
        sd = {"gnn." + k: v for k, v in gnn_mod.state_dict().items()}
        if fc_mod is not None:
            sd.update({"fc." + k: v for k, v in fc_mod.state_dict().items()})
        else:
            dev = next(gnn_mod.parameters()).device
            sd.update({"fc.0.weight": torch.zeros(128, 512, device=dev), "fc.0.bias": torch.zeros(128, device=dev),
                       "fc.1.weight": torch.ones(128, device=dev), "fc.1.bias": torch.zeros(128, device=dev)})
        G = Fn.GnnHeadWeights(sd, next(gnn_mod.parameters()).device, gnn_mod.train_N_way if n_way is None else n_way)
        cache = (key, G)
        gnn_mod.__dict__["_mft_pack"] = cache
    return cache[1]


class _Solo:
    """GnnHeadWeights-shaped view of a single Wcompute / Gconv module (stand-alone module calls)."""

    def __init__(self):
        self.wc, self.gc, self.n_way = {}, {}, 0


def solo_weights(mod, kind):
    key = _version_key(mod)
    cache = mod.__dict__.get("_mft_pack")
    if cache is None or cache[0] != key:
        dev = next(mod.parameters()).device
        S = _Solo()

        def d(t):
            return t.detach().to(dev).float().contiguous()
        if kind == "wc":
            layers = []
            for li in range(1, 5):
                conv, bn = getattr(mod, "conv2d_%d" % li), getattr(mod, "bn_%d" % li)
                layers.append((ops.pack_conv_weight(d(conv.weight)), d(conv.bias), d(bn.weight), d(bn.bias), conv.weight.shape[0]))
            S.wc["solo"] = (layers, (ops.pack_conv_weight(d(mod.conv2d_last.weight)), d(mod.conv2d_last.bias)))
        else:
            g = b = None
            if mod.bn_bool:
                g, b = d(mod.bn.weight), d(mod.bn.bias)
            S.gc["solo"] = (ops.pack_conv_weight(d(mod.fc.weight)), d(mod.fc.bias), g, b, mod.fc.weight.shape[0])
        cache = (key, S)
        mod.__dict__["_mft_pack"] = cache
    return cache[1]


def invalidate(mod):
    """Drop cached packed weights after an in-place parameter update done behind autograd's back."""
    for m in mod.modules():
        m.__dict__.pop("_mft_pack", None)


def touch(mod):
    """Mark the cached packed weights stale but keep them: the next lookup refreshes every packed copy IN PLACE (one launch) instead
    of rebuilding the pack -- for in-place parameter updates that do not bump autograd's version counters (kernels writing
    ``p.data``).  Anything recorded against the pack's buffers (a captured inner loop) stays valid."""
    for m in mod.modules():
        c = m.__dict__.get("_mft_pack")
        if c is not None:
            m.__dict__["_mft_pack"] = (tuple((k[0], -1) for k in c[0]), c[1])


def gnnnet_head(model, feats, n_support, n_query, fold=False, episodes=1):
    """GnnNet.fc + z_stack + forward_gnn (gnnnet.py:76-87,210-217): feats [episodes*n_way*(S+n_query), 512] (one episode after
    the other) -> scores [episodes*n_way*n_query, n_way].  Differentiable (hand-written backward) when autograd is recording."""
    _require_cuda(feats, "GnnNet head")
    plist = list(model.fc.parameters()) + list(model.gnn.parameters())
    if torch.is_grad_enabled() and (feats.requires_grad or any(p.requires_grad for p in plist)):
        return _HeadFn.apply(model, feats, n_support, n_query, fold, episodes, *plist)
    G = head_weights(model.gnn, model.fc, model.n_way)
    f = feats.detach().contiguous().float()
    return Fn.gnnnet_scores(G, f, episodes, model.n_way, n_support, n_query, arena_for(f.device), fold=fold, tag="head%d" % episodes).clone()


class _ProtoHeadFn(torch.autograd.Function):
    """ProtoNet prototypes + negative squared euclidean distances (protonet.py set_forward / euclidean_dist) with a HIP backward:
    one mft_proto_scores launch forward, one mft_proto_backward launch back, all episodes at once."""

    @staticmethod
    def forward(ctx, feats, n_way, n_support, n_query, episodes):
        ctx.save_for_backward(feats)
        ctx.shape = (episodes, n_way, n_support, n_query)
        return ops.proto_scores(feats, episodes, n_way, n_support, n_query)

    @staticmethod
    def backward(ctx, dscores):
        feats, = ctx.saved_tensors
        episodes, n_way, n_support, n_query = ctx.shape
        d = dscores if (dscores.dtype == torch.float32 and dscores.is_contiguous()) else dscores.contiguous().float()
        return ops.proto_backward(feats, d, episodes, n_way, n_support, n_query), None, None, None, None


def protonet_head(feats, n_way, n_support, n_query, episodes=1):
    """ProtoNet.set_forward tail (protonet.py): feats [episodes*n_way*(n_support+n_query), D] (class-major rows, one episode after
    the other) -> scores [episodes*n_way*n_query, n_way] = -||q - mean(support_c)||^2.  Differentiable when autograd records."""
    _require_cuda(feats, "ProtoNet head")
    if feats.dtype != torch.float32 or not feats.is_contiguous():
        feats = feats.contiguous().float()
    if torch.is_grad_enabled() and feats.requires_grad:
        return _ProtoHeadFn.apply(feats, n_way, n_support, n_query, episodes)
    return ops.proto_scores(feats.detach(), episodes, n_way, n_support, n_query)


class _DistLinearFn(torch.autograd.Function):
    """Baseline++ head (backbone.distLinear): one mft_dist_linear_forward launch forward, one mft_dist_linear_backward launch
    back for dx, dg and dv together."""

    @staticmethod
    def forward(ctx, x, g, v, scale):
        ctx.save_for_backward(x, g, v)
        ctx.scale = scale
        return ops.dist_linear_forward(x, g, v, scale)

    @staticmethod
    def backward(ctx, dscores):
        x, g, v = ctx.saved_tensors
        d = dscores if (dscores.dtype == torch.float32 and dscores.stride(1) == 1) else dscores.contiguous().float()
        dx, dv, dg = ops.dist_linear_backward(x, g, v, ctx.scale, d, need_dx=ctx.needs_input_grad[0])
        return dx, dg, dv, None


def dist_linear(x, g, v, scale):
    """backbone.distLinear.forward: x [R, D], g [C, 1], v [C, D] -> scale * cosine scores [R, C].  Differentiable in x, g and v
    when autograd records."""
    _require_cuda(x, "distLinear")
    _require_cuda(v, "distLinear")
    if x.dtype != torch.float32 or x.dim() != 2 or x.stride(1) != 1:
        x = x.contiguous().float()
    if torch.is_grad_enabled() and (x.requires_grad or g.requires_grad or v.requires_grad):
        return _DistLinearFn.apply(x, g.contiguous(), v.contiguous(), float(scale))
    return ops.dist_linear_forward(x.detach(), g.detach().contiguous(), v.detach().contiguous(), float(scale))


def matchingnet_params(model):
    """The twelve head parameters of a MatchingNet in state-dict order (ops.MN_KEYS): FCE.lstmcell.*, G_encoder.*"""
    named = dict(model.FCE.lstmcell.named_parameters(prefix="FCE.lstmcell"))
    named.update(model.G_encoder.named_parameters(prefix="G_encoder"))
    return [named[k] for k in ops.MN_KEYS]


def _mn_weights(plist):
    for k, p in zip(ops.MN_KEYS, plist):
        if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
            raise RuntimeError("MatchingNet head: parameter %s must be a contiguous float32 tensor on the GPU (no CPU fallback)" % k)
    return {k: p.detach() for k, p in zip(ops.MN_KEYS, plist)}       # read in torch's own layout: no packed copies to refresh


class _MatchingHeadFn(torch.autograd.Function):
    """MatchingNet head (G_encoder, FCE, cosine read-out) with a hand-written backward: ops.matching_forward keeps the per-step
    h, c, a, r and gates, ops.matching_backward walks the S FCE steps and the S encoder steps back and returns the gradients of the
    features and of the twelve head parameters."""

    @staticmethod
    def forward(ctx, feats, n_way, n_support, n_query, episodes, *plist):
        W = _mn_weights(plist)
        logp, tape = ops.matching_forward(W, feats, episodes, n_way, n_support, n_query, save=True)
        ctx.tape, ctx.W = tape, W
        ctx.need = (feats.requires_grad,) + tuple(p.requires_grad for p in plist)
        return logp

    @staticmethod
    def backward(ctx, dlogp):
        if ctx.tape is None:
            raise RuntimeError("MatchingNet head: backward called twice (the saved gates are consumed by the first pass)")
        d = dlogp if (dlogp.dtype == torch.float32 and dlogp.stride(1) == 1) else dlogp.contiguous().float()
        dfeats, g = ops.matching_backward(ctx.W, ctx.tape, d)
        ctx.tape = None
        out = [g[k] if need else None for k, need in zip(ops.MN_KEYS, ctx.need[1:])]
        return (dfeats if ctx.need[0] else None, None, None, None, None) + tuple(out)


def matchingnet_head(model, feats, n_support, n_query, episodes=1):
    """MatchingNet.set_forward tail: feats [episodes*n_way*(n_support+n_query), 512] (class-major rows, one
    episode after the other) -> log-probabilities [episodes*n_way*n_query, n_way].  Differentiable (features and the twelve head
    parameters) when autograd records; the no-grad path keeps two state slots and saves nothing."""
    _require_cuda(feats, "MatchingNet head")
    ops.mn_check(episodes, model.n_way, n_support, n_query, feats.shape[-1])
    if feats.dtype != torch.float32 or not feats.is_contiguous():
        feats = feats.contiguous().float()
    plist = matchingnet_params(model)
    if torch.is_grad_enabled() and (feats.requires_grad or any(p.requires_grad for p in plist)):
        return _MatchingHeadFn.apply(feats, model.n_way, n_support, n_query, episodes, *plist)
    return ops.matching_forward(_mn_weights(plist), feats.detach(), episodes, model.n_way, n_support, n_query)[0]


class _RidgeHeadFn(torch.autograd.Function):
    """MetaOptNet ridge-regression head with a hand-written backward: ops.ridge_forward keeps the Cholesky
    factor, alpha and W, ops.ridge_backward returns the gradients of every feature row and of ``scale``."""

    @staticmethod
    def forward(ctx, feats, scale, n_way, n_support, n_query, episodes):
        scores, tape = ops.ridge_forward(feats, scale.detach(), episodes, n_way, n_support, n_query, save=True)
        tape.pop("feats")
        tape.pop("scale")
        ctx.save_for_backward(feats, scale)
        ctx.tape = tape
        return scores

    @staticmethod
    def backward(ctx, dscores):
        feats, scale = ctx.saved_tensors
        d = dscores if (dscores.dtype == torch.float32 and dscores.stride(1) == 1) else dscores.contiguous().float()
        dfeats, dscale = ops.ridge_backward(dict(ctx.tape, feats=feats, scale=scale.detach()), d)
        return (dfeats if ctx.needs_input_grad[0] else None, dscale.view(scale.shape) if ctx.needs_input_grad[1] else None,
                None, None, None, None)


def metaoptnet_head(feats, scale, n_way, n_support, n_query, episodes=1):
    """MetaOptNet.set_forward tail: feats [episodes*n_way*(n_support+n_query), 512] (class-major rows, one
    episode after the other), scale the head's one-element parameter -> scores [episodes*n_way*n_query, n_way] = scale * Z_Q W of
    the ridge regression on the support rows.  Differentiable (features and scale) when autograd records; the no-grad path saves
    nothing."""
    _require_cuda(feats, "MetaOptNet head")
    _require_cuda(scale, "MetaOptNet head")
    ops.ridge_check(episodes, n_way, n_support, n_query, feats.shape[-1])
    if feats.dtype != torch.float32 or not feats.is_contiguous():
        feats = feats.contiguous().float()
    if torch.is_grad_enabled() and (feats.requires_grad or scale.requires_grad):
        return _RidgeHeadFn.apply(feats, scale, n_way, n_support, n_query, episodes)
    return ops.ridge_forward(feats.detach(), scale.detach(), episodes, n_way, n_support, n_query)[0]


class _SvmHeadFn(torch.autograd.Function):
    """MetaOptNet SVM head with a hand-written backward: ops.svm_forward keeps alpha, the free mask and W,
    ops.svm_backward solves the adjoint system on that mask and returns the gradients of every feature row and of ``scale``."""

    @staticmethod
    def forward(ctx, feats, scale, n_way, n_support, n_query, episodes):
        scores, tape = ops.svm_forward(feats, scale.detach(), episodes, n_way, n_support, n_query, save=True)
        ctx.save_for_backward(feats, scale, tape["alpha"], tape["free"], tape["W"])
        ctx.shape = tape["shape"]
        _SVM_STATUS[0] = tape["status"]
        return scores

    @staticmethod
    def backward(ctx, dscores):
        feats, scale, alpha, free, W = ctx.saved_tensors
        d = dscores if (dscores.dtype == torch.float32 and dscores.stride(1) == 1) else dscores.contiguous().float()
        dfeats, dscale = ops.svm_backward(dict(feats=feats, scale=scale.detach(), alpha=alpha, free=free, W=W, shape=ctx.shape), d)
        return (dfeats if ctx.needs_input_grad[0] else None, dscale.view(scale.shape) if ctx.needs_input_grad[1] else None,
                None, None, None, None)


_SVM_STATUS = [None]


def metaoptnet_svm_status():
    """``status`` [episodes] int32 of the last metaoptnet_svm_head call (0 = the solve's optimality test passed), still on the
    device: reading it is the caller's host sync, none is made here.  None before the first call."""
    return _SVM_STATUS[0]


def metaoptnet_svm_head(feats, scale, n_way, n_support, n_query, episodes=1):
    """MetaOptNet(head="svm").set_forward tail: as metaoptnet_head, with W from the Crammer-Singer dual of
    the support rows in the place of the ridge regression.  Differentiable (features and scale) when autograd records; the
    no-grad path saves nothing.  metaoptnet_svm_status() returns the call's status tensor."""
    _require_cuda(feats, "MetaOptNet head")
    _require_cuda(scale, "MetaOptNet head")
    ops.svm_check(episodes, n_way, n_support, n_query, feats.shape[-1])
    if feats.dtype != torch.float32 or not feats.is_contiguous():
        feats = feats.contiguous().float()
    if torch.is_grad_enabled() and (feats.requires_grad or scale.requires_grad):
        return _SvmHeadFn.apply(feats, scale, n_way, n_support, n_query, episodes)
    scores, tape = ops.svm_forward(feats.detach(), scale.detach(), episodes, n_way, n_support, n_query)
    _SVM_STATUS[0] = tape["status"]
    return scores


class _TpnHeadFn(torch.autograd.Function):
    """TPN head with a hand-written backward: ops.tpn_forward keeps the packed Cholesky factor, F, the
    neighbour mask and D^-1/2, ops.tpn_backward returns the gradients of every feature row and of the four head parameters (the
    mask is a constant of the backward)."""

    @staticmethod
    def forward(ctx, feats, w3, b3, w4, b4, n_way, n_support, n_query, episodes):
        head = tuple(p.detach() for p in (w3, b3, w4, b4))
        scores, tape = ops.tpn_forward(feats, head, episodes, n_way, n_support, n_query, save=True, mask=_TPN_FORCED[0])
        ctx.save_for_backward(feats, *head)
        ctx.tape = {k: v for k, v in tape.items() if k not in ("feats", "head")}
        _TPN_LAST[0] = (tape["mask"], tape["W"])
        return scores

    @staticmethod
    def backward(ctx, dscores):
        feats, *head = ctx.saved_tensors
        d = dscores if (dscores.dtype == torch.float32 and dscores.stride(1) == 1) else dscores.contiguous().float()
        dfeats, dw3, db3, dw4, db4 = ops.tpn_backward(dict(ctx.tape, feats=feats, head=tuple(head)), d)
        need = ctx.needs_input_grad
        return (dfeats if need[0] else None, dw3 if need[1] else None, db3 if need[2] else None, dw4 if need[3] else None,
                db4 if need[4] else None, None, None, None, None)


_TPN_FORCED = [None]
_TPN_LAST = [None]


@contextlib.contextmanager
def tpn_forced_graph(mask):
    """Tests and golden parity only: inside the block every tpn_head call takes its neighbour selection from ``mask``
    [episodes, N, N] (uint8, on the device; non-zero = selected) instead of the k largest entries per row."""
    _TPN_FORCED[0] = mask
    try:
        yield mask
    finally:
        _TPN_FORCED[0] = None


def tpn_last_graph():
    """(mask [episodes, N, N] uint8, W [episodes, N, N]) of the last recorded tpn_head call, still on the device; None before it."""
    return _TPN_LAST[0]


def tpn_head(feats, fc3_w, fc3_b, fc4_w, fc4_b, n_way, n_support, n_query, episodes=1):
    """TPN.set_forward tail: feats [episodes*n_way*(n_support+n_query), 512] (class-major rows, one episode
    after the other), the four parameters of the relation module's fc3 / fc4 -> scores [episodes*n_way*n_query, n_way] = the query
    rows of (I - alpha S)^-1 Y on the episode's k-nearest-neighbour graph.  Differentiable (features and the four parameters)
    when autograd records; the no-grad path saves nothing."""
    plist = (fc3_w, fc3_b, fc4_w, fc4_b)
    _require_cuda(feats, "TPN head")
    for p in plist:
        _require_cuda(p, "TPN head")
    ops.tpn_check(episodes, n_way, n_support, n_query, feats.shape[-1])
    if feats.dtype != torch.float32 or not feats.is_contiguous():
        feats = feats.contiguous().float()
    if torch.is_grad_enabled() and (feats.requires_grad or any(p.requires_grad for p in plist)):
        return _TpnHeadFn.apply(feats, *plist, n_way, n_support, n_query, episodes)
    return ops.tpn_forward(feats.detach(), tuple(p.detach() for p in plist), episodes, n_way, n_support, n_query,
                           mask=_TPN_FORCED[0])[0]


class _FeatHeadFn(torch.autograd.Function):
    """FEAT head with a hand-written backward: ops.feat_forward keeps the tokens, the projections, the
    attention rows before dropout and the LayerNorm statistics; ops.feat_backward returns the gradients of every feature row and of
    the seven head parameters.  Train mode returns (scores, reg), eval mode scores alone."""

    @staticmethod
    def forward(ctx, feats, wq, wk, wv, ln_w, ln_b, wfc, bfc, n_way, n_support, n_query, episodes, train, masks, temps):
        head = tuple(p.detach() for p in (wq, wk, wv, ln_w, ln_b, wfc, bfc))
        scores, reg, tape = ops.feat_forward(feats, head, episodes, n_way, n_support, n_query, train, masks=masks, save=True,
                                             temperature=temps[0], temperature2=temps[1])
        ctx.save_for_backward(feats, *head)
        ctx.tape = {k: v for k, v in tape.items() if k not in ("feats", "head")}
        ctx.set_materialize_grads(False)                 # an unused output's gradient stays None: no fill launch
        return (scores, reg) if train else scores

    @staticmethod
    def backward(ctx, dscores, dreg=None):
        feats, *head = ctx.saved_tensors
        fix = lambda d: d if (d is None or (d.dtype == torch.float32 and d.is_contiguous())) else d.contiguous().float()  # noqa: E731
        if dscores is None:
            dscores = torch.zeros((ctx.tape["shape"][0] * ctx.tape["shape"][1] * ctx.tape["shape"][3], ctx.tape["shape"][1]),
                                  device=feats.device, dtype=torch.float32)
        grads = ops.feat_backward(dict(ctx.tape, feats=feats, head=tuple(head)), fix(dscores), fix(dreg))
        need = ctx.needs_input_grad
        return tuple(g if need[i] else None for i, g in enumerate(grads)) + (None,) * 7


_FEAT_FORCED = [None]


@contextlib.contextmanager
def feat_forced_masks(masks):
    """Tests and golden parity only: inside the block every train-mode FEAT head call takes its dropout multipliers (m_att, m_out)
    from ``masks`` (float32, on the device, the layout of ops.feat_draw) instead of the generator."""
    _FEAT_FORCED[0] = masks
    try:
        yield masks
    finally:
        _FEAT_FORCED[0] = None


def feat_forced():
    return _FEAT_FORCED[0]


def feat_head(feats, head, n_way, n_support, n_query, episodes=1, train=False, masks=None,
              temperature=ops.FEAT_TEMPERATURE, temperature2=ops.FEAT_TEMPERATURE2):
    """FEAT.set_forward tail: feats [episodes*n_way*(n_support+n_query), 512] (class-major rows, one episode
    after the other), the seven slf_attn parameters in state-dict order -> scores [episodes*n_way*n_query, n_way]; ``train``:
    (scores, reg [rows, n_way]) with the auxiliary sets, ``masks`` = (m_att, m_out) their dropout multipliers (None: 1).
    Differentiable (features and the seven parameters) when autograd records; the no-grad path saves nothing."""
    plist = tuple(head)
    _require_cuda(feats, "FEAT head")
    for p in plist:
        _require_cuda(p, "FEAT head")
    ops.feat_check(episodes, n_way, n_support, n_query, feats.shape[-1])
    if feats.dtype != torch.float32 or not feats.is_contiguous():
        feats = feats.contiguous().float()
    temps = (float(temperature), float(temperature2))
    if torch.is_grad_enabled() and (feats.requires_grad or any(p.requires_grad for p in plist)):
        return _FeatHeadFn.apply(feats, *plist, n_way, n_support, n_query, episodes, bool(train), masks, temps)
    scores, reg, _ = ops.feat_forward(feats.detach(), tuple(p.detach() for p in plist), episodes, n_way, n_support, n_query, train,
                                      masks=masks, temperature=temps[0], temperature2=temps[1])
    return (scores, reg) if train else scores


class _FeatLossFn(torch.autograd.Function):
    """CE(scores) + balance CE(reg) (means; a row's label is its class) with ONE launch each way (mft_feat_loss / _backward).
    Returns the 0-dim tensors (total, main term, auxiliary term); only the total is differentiable."""

    @staticmethod
    def forward(ctx, scores, reg, shape, balance, loss_sum):
        out = ops.feat_loss(scores, reg, *shape, balance=balance, loss_sum=loss_sum)
        ctx.save_for_backward(scores, reg)
        ctx.shape, ctx.balance = shape, balance
        total, main, aux = out[0], out[1], out[2]        # views of the launch's output: no device work
        ctx.mark_non_differentiable(main, aux)
        ctx.set_materialize_grads(False)
        return total, main, aux

    @staticmethod
    def backward(ctx, g, _gm=None, _ga=None):
        scores, reg = ctx.saved_tensors
        if g is not None and (g.dtype != torch.float32 or g.numel() != 1):
            g = g.reshape(-1)[:1].float()
        dscores, dreg = ops.feat_loss_backward(scores, reg, *ctx.shape, g, balance=ctx.balance)
        return dscores, dreg, None, None, None


def feat_loss(scores, reg, episodes, n_way, n_support, n_query, balance=ops.FEAT_BALANCE, loss_sum=None):
    """(loss, main, aux): loss = CE(scores, y_query) + balance CE(reg, y_all) as a 0-dim tensor (``reg`` None: the main term alone)
    and its two terms (0-dim, not differentiable).  ``loss_sum`` (float64 device scalar) += the main term."""
    _require_cuda(scores, "FEAT loss")
    if scores.dtype != torch.float32 or not scores.is_contiguous():
        scores = scores.contiguous().float()
    if reg is not None and (reg.dtype != torch.float32 or not reg.is_contiguous()):
        reg = reg.contiguous().float()
    return _FeatLossFn.apply(scores, reg, (episodes, n_way, n_support, n_query), float(balance), loss_sum)


class _DktLossFn(torch.autograd.Function):
    """DKT's negative marginal log-likelihood with a hand-written backward: ops.dkt_loss_forward keeps the
    normalised rows, the packed Cholesky factor, A = K^-1 R and the per-episode sums; ops.dkt_loss_backward returns the gradients of
    every feature row and of the three hyperparameters, with the upstream gradient read on the device."""

    @staticmethod
    def forward(ctx, feats, mean, raw_outputscale, raw_noise, shape, kernel, loss_sum):
        hyper = tuple(p.detach() for p in (mean, raw_outputscale, raw_noise))
        loss, tape = ops.dkt_loss_forward(feats, hyper, *shape, kernel=kernel, save=True, loss_sum=loss_sum)
        ctx.tape = {k: v for k, v in tape.items() if k != "feats"}       # (the backward reads U and |z|, not the rows themselves)
        ctx.shapes = tuple(p.shape for p in (mean, raw_outputscale, raw_noise))
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        if g.dtype != torch.float32 or g.numel() != 1:
            g = g.reshape(-1)[:1].float()
        dfeats, dhyper = ops.dkt_loss_backward(ctx.tape, g)
        need = ctx.needs_input_grad
        return (dfeats if need[0] else None,) + tuple(dhyper[i].view(ctx.shapes[i]) if need[1 + i] else None for i in range(3)) \
            + (None, None, None)


def _dkt_inputs(what, feats, hyper, episodes, n_way, n_support, n_query, loss):
    _require_cuda(feats, what)
    for p in hyper:
        _require_cuda(p, what)
    ops.dkt_check(episodes, n_way, n_support, n_query, feats.shape[-1], loss)
    if feats.dtype != torch.float32 or not feats.is_contiguous():
        feats = feats.contiguous().float()
    return feats


def dkt_loss(feats, mean, raw_outputscale, raw_noise, n_way, n_support, n_query, episodes=1, kernel="cossim", loss_sum=None):
    """DKT.set_forward_loss tail: feats [episodes*n_way*(n_support+n_query), 512] (class-major rows, one
    episode after the other) and the three one-element hyperparameters -> the 0-dim loss: the negative marginal log-likelihood of
    the n_way one-vs-rest Gaussian processes over ALL rows of the episode, divided by their number, averaged over the episodes.
    Differentiable (features and the three hyperparameters) when autograd records; the no-grad path saves nothing.  ``loss_sum``
    (float64 device scalar) += the loss."""
    hyper = (mean, raw_outputscale, raw_noise)
    feats = _dkt_inputs("DKT loss", feats, hyper, episodes, n_way, n_support, n_query, True)
    ops.dkt_kernel_id(kernel)
    if torch.is_grad_enabled() and (feats.requires_grad or any(p.requires_grad for p in hyper)):
        return _DktLossFn.apply(feats, *hyper, (episodes, n_way, n_support, n_query), kernel, loss_sum)
    return ops.dkt_loss_forward(feats.detach(), tuple(p.detach() for p in hyper), episodes, n_way, n_support, n_query, kernel=kernel,
                                loss_sum=loss_sum)[0].view(())


def dkt_scores(feats, mean, raw_outputscale, raw_noise, n_way, n_support, n_query, episodes=1, kernel="cossim"):
    """DKT.set_forward tail: the posterior mean of the process conditioned on each episode's support rows, at its queries ->
    scores [episodes*n_way*n_query, n_way].  A prediction: the returned tensor never requires grad (the method trains through
    ``dkt_loss`` and never differentiates through its scores)."""
    hyper = (mean, raw_outputscale, raw_noise)
    feats = _dkt_inputs("DKT head", feats, hyper, episodes, n_way, n_support, n_query, False)
    return ops.dkt_scores(feats.detach(), tuple(p.detach() for p in hyper), episodes, n_way, n_support, n_query, kernel=kernel)


class _AnilHeadFn(torch.autograd.Function):
    """ANIL head with a hand-written second-order backward: ops.anil_forward keeps the classifier and the
    softmax of every inner step, ops.anil_backward returns the gradients of every feature row (support rows through the inner
    steps, query rows through the scores) and of the classifier's initialisation."""

    @staticmethod
    def forward(ctx, feats, W0, b0, n_way, n_support, n_query, episodes, inner_steps, inner_lr):
        scores, tape = ops.anil_forward(feats, W0.detach(), b0.detach(), episodes, n_way, n_support, n_query, inner_steps, inner_lr,
                                        save=True)
        ctx.save_for_backward(feats)
        ctx.tape = {k: v for k, v in tape.items() if k != "feats"}
        return scores

    @staticmethod
    def backward(ctx, dscores):
        feats, = ctx.saved_tensors
        d = dscores if (dscores.dtype == torch.float32 and dscores.is_contiguous()) else dscores.contiguous().float()
        dfeats, dW0, db0 = ops.anil_backward(dict(ctx.tape, feats=feats), d)
        need = ctx.needs_input_grad
        return (dfeats if need[0] else None, dW0 if need[1] else None, db0 if need[2] else None, None, None, None, None, None, None)


def anil_scores(feats, W0, b0, n_way, n_support, n_query, episodes=1, inner_steps=5, inner_lr=0.01):
    """ANIL.set_forward tail: feats [episodes*n_way*(n_support+n_query), 512] (class-major rows, one episode
    after the other), the classifier's initialisation W0 [n_way, 512], b0 [n_way] -> scores [episodes*n_way*n_query, n_way] of the
    classifier after ``inner_steps`` gradient steps of size ``inner_lr`` on the episode's support rows.  Differentiable (features
    and initialisation, exactly, through the inner steps) when autograd records; the no-grad path saves nothing."""
    _require_cuda(feats, "ANIL head")
    _require_cuda(W0, "ANIL head")
    _require_cuda(b0, "ANIL head")
    ops.anil_check(episodes, n_way, n_support, n_query, inner_steps, inner_lr, feats.shape[-1])
    if feats.dtype != torch.float32 or not feats.is_contiguous():
        feats = feats.contiguous().float()
    if torch.is_grad_enabled() and (feats.requires_grad or W0.requires_grad or b0.requires_grad):
        return _AnilHeadFn.apply(feats, W0, b0, n_way, n_support, n_query, episodes, inner_steps, inner_lr)
    return ops.anil_forward(feats.detach(), W0.detach(), b0.detach(), episodes, n_way, n_support, n_query, inner_steps, inner_lr)[0]


class _MahalanobisHeadFn(torch.autograd.Function):
    """Mahalanobis head with a hand-written backward: ops.mahalanobis_forward keeps the class means, the
    centred support rows and the solution w of every (query, class) pair, ops.mahalanobis_backward returns the gradient of every
    feature row (query rows through d, support rows through the class means, the task mean and T)."""

    @staticmethod
    def forward(ctx, feats, n_way, n_support, n_query, episodes):
        scores, tape = ops.mahalanobis_forward(feats, episodes, n_way, n_support, n_query, save=True)
        ctx.save_for_backward(feats)
        ctx.tape = {k: v for k, v in tape.items() if k != "feats"}
        return scores

    @staticmethod
    def backward(ctx, dscores):
        feats, = ctx.saved_tensors
        d = dscores if (dscores.dtype == torch.float32 and dscores.is_contiguous()) else dscores.contiguous().float()
        return ops.mahalanobis_backward(dict(ctx.tape, feats=feats), d), None, None, None, None


def mahalanobis_scores(feats, n_way, n_support, n_query, episodes=1):
    """Mahalanobis.set_forward tail: feats [episodes*n_way*(n_support+n_query), 512] (class-major rows, one
    episode after the other) -> scores [episodes*n_way*n_query, n_way] = minus half the squared Mahalanobis distance of every query
    to every class mean under the class's regularised covariance.  Differentiable (support and query features, exactly) when
    autograd records; the no-grad path saves nothing."""
    _require_cuda(feats, "Mahalanobis head")
    ops.mahalanobis_check(episodes, n_way, n_support, n_query, feats.shape[-1])
    if feats.dtype != torch.float32 or not feats.is_contiguous():
        feats = feats.contiguous().float()
    if torch.is_grad_enabled() and feats.requires_grad:
        return _MahalanobisHeadFn.apply(feats, n_way, n_support, n_query, episodes)
    return ops.mahalanobis_forward(feats.detach(), episodes, n_way, n_support, n_query)[0]


class _NLLFn(torch.autograd.Function):
    """nn.NLLLoss()(logp, y) = -mean_r logp[r, y_r], one launch each way (mft_nll_mean / _backward)."""

    @staticmethod
    def forward(ctx, logp, target, loss_sum):
        ctx.save_for_backward(target)
        ctx.shape = tuple(logp.shape)
        return ops.nll_mean(logp, target, loss_sum)

    @staticmethod
    def backward(ctx, g):
        target, = ctx.saved_tensors
        return ops.nll_mean_backward(target, ctx.shape[0], ctx.shape[1], g.contiguous().float()), None, None


class NLLLoss(torch.nn.NLLLoss):
    """``nn.NLLLoss()`` as MatchingNet uses it (default arguments, [rows, C] float log-probabilities against [rows] class indices),
    computed by the HIP library; anything else raises.  ``loss_sum`` as CrossEntropyLoss.loss_sum: the float64 device scalar every
    forward adds its loss to."""

    loss_sum = CrossEntropyLoss.loss_sum

    def forward(self, input, target):
        if (self.weight is not None or self.reduction != "mean" or self.ignore_index != -100 or input.dim() != 2 or target.dim() != 1
                or target.dtype not in (torch.int64, torch.int32) or target.shape[0] != input.shape[0]):
            raise NotImplementedError("NLLLoss on the HIP path: default options, [rows, C] log-probabilities, [rows] int64 / int32 labels")
        _require_cuda(input, "NLLLoss")
        if not target.is_cuda:
            raise RuntimeError("NLLLoss: labels are on the CPU -- the MI355X path has no CPU fallback; call .cuda() first")
        if input.dtype != torch.float32 or input.stride(1) != 1:
            input = input.float().contiguous()
        return _NLLFn.apply(input, target.contiguous(), self.loss_sum(input.device))
