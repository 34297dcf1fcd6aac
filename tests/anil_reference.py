"""The ANIL definition of DESIGN.md section 21 restated for the tests: ``anil_chain`` is the plain torch chain in its input's dtype
(the inner gradient by torch.autograd.grad with create_graph=True, so that autograd differentiates through the inner steps), and
``anil_closed_form`` is the recursion the kernels of csrc/anil.hip run (softmax Jacobians and Hessian-vector products written out).
Shared by tests/test_anil_cpu.py and tests/test_anil_gpu.py; tools/make_golden_anil.py holds its own copy on the reference's
MetaTemplate."""
import numpy as np
import torch
import torch.nn.functional as F

HEAD = ["classifier.weight", "classifier.bias"]


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


def step_size(inner_lr):
    """The launchers take inner_lr as a C float: every chain here steps with that number."""
    return float(np.float32(inner_lr))


def split(feats, n_way, n_support, n_query, episodes=1):
    """feats [episodes*n_way*(n_support+n_query), D], class-major -> (Z_S [episodes, S, D], Z_Q [episodes, Q, D])."""
    z = feats.reshape(episodes, n_way, n_support + n_query, -1)
    return z[:, :, :n_support].reshape(episodes, n_way * n_support, -1), z[:, :, n_support:].reshape(episodes, n_way * n_query, -1)


def labels(n_way, per):
    return torch.arange(n_way).repeat_interleave(per)


def anil_chain(feats, W0, b0, n_way, n_support, n_query, episodes=1, inner_steps=5, inner_lr=0.01):
    """-> (loss, scores [episodes*n_way*n_query, n_way]); the loss is the mean cross entropy of the scores over all query rows (the
    mean of the episodes' losses).  Differentiable in feats, W0 and b0 through the inner steps."""
    a = step_size(inner_lr)
    ZS, ZQ = split(feats, n_way, n_support, n_query, episodes)
    yS, yQ = labels(n_way, n_support), labels(n_way, n_query)
    scores = []
    with torch.enable_grad():
        for e in range(episodes):
            W = W0 if W0.requires_grad else W0.detach().requires_grad_(True)
            b = b0 if b0.requires_grad else b0.detach().requires_grad_(True)
            for _ in range(inner_steps):
                inner = F.cross_entropy(ZS[e] @ W.t() + b, yS)
                gW, gb = torch.autograd.grad(inner, (W, b), create_graph=True)
                W, b = W - a * gW, b - a * gb
            scores.append(ZQ[e] @ W.t() + b)
        scores = torch.cat(scores)
        loss = F.cross_entropy(scores, yQ.repeat(episodes))
    return loss, scores


def anil_closed_form(feats, W0, b0, n_way, n_support, n_query, episodes=1, inner_steps=5, inner_lr=0.01, dscores=None):
    """The forward steps and the reverse recursion of DESIGN.md section 21, no autograd -> (loss, scores, dfeats, dW0, db0).
    ``dscores``: the upstream gradient G [episodes*Q, n_way]; None = that of the mean cross entropy."""
    a = step_size(inner_lr)
    dt = feats.dtype
    ZS, ZQ = split(feats.detach(), n_way, n_support, n_query, episodes)
    S, Q = n_way * n_support, n_way * n_query
    YS = F.one_hot(labels(n_way, n_support), n_way).to(dt)
    YQ = F.one_hot(labels(n_way, n_query), n_way).to(dt)
    tapes, scores = [], []
    for e in range(episodes):
        W, b, tape = W0.detach().clone(), b0.detach().clone(), []
        for _ in range(inner_steps):
            P = torch.softmax(ZS[e] @ W.t() + b, dim=1)
            tape.append((W, P))
            W = W - a * (P - YS).t() @ ZS[e] / S
            b = b - a * (P - YS).sum(0) / S
        tapes.append((tape, W))
        scores.append(ZQ[e] @ W.t() + b)
    scores = torch.cat(scores)
    logp = torch.log_softmax(scores, dim=1)
    loss = -(logp * YQ.repeat(episodes, 1)).sum() / (episodes * Q)
    G = (torch.softmax(scores, dim=1) - YQ.repeat(episodes, 1)) / (episodes * Q) if dscores is None else dscores.to(dt)
    D = feats.shape[1]
    dfeats = torch.zeros(episodes, n_way, n_support + n_query, D, dtype=dt)
    dW0, db0 = torch.zeros_like(W0), torch.zeros_like(b0)
    for e in range(episodes):
        tape, WK = tapes[e]
        Ge = G[e * Q:(e + 1) * Q]
        dZQ = Ge @ WK
        gW, gb = Ge.t() @ ZQ[e], Ge.sum(0)
        dZS = torch.zeros(S, D, dtype=dt)
        for Wt, P in reversed(tape):
            U = ZS[e] @ gW.t() + gb
            R = P * (U - (P * U).sum(1, keepdim=True))
            dZS -= (a / S) * ((P - YS) @ gW + R @ Wt)
            gW = gW - (a / S) * R.t() @ ZS[e]
            gb = gb - (a / S) * R.sum(0)
        dfeats[e, :, :n_support] = dZS.reshape(n_way, n_support, D)
        dfeats[e, :, n_support:] = dZQ.reshape(n_way, n_query, D)
        dW0 += gW
        db0 += gb
    return loss, scores, dfeats.reshape(-1, D), dW0, db0
