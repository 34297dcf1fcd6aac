"""The Mahalanobis head of DESIGN.md section 22 restated for the tests: ``dense_chain`` is the definition with torch.linalg.inv on the
D x D matrices Q_c in its input's dtype (autograd gives its gradients), and ``closed_form`` is the span form and the backward the
kernels of csrc/mahalanobis.hip run, without autograd.  Shared by tests/test_mahalanobis_cpu.py and tests/test_mahalanobis_gpu.py;
tools/make_golden_mahalanobis.py holds its own copy of the definition on the reference's MetaTemplate."""
import torch
import torch.nn.functional as F

BETA = 1.0


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


def split(feats, n_way, n_support, n_query, episodes=1):
    """feats [episodes*n_way*(n_support+n_query), D], class-major -> (Z_S [episodes, S, D], Z_Q [episodes, Q, D])."""
    z = feats.reshape(episodes, n_way, n_support + n_query, -1)
    return z[:, :, :n_support].reshape(episodes, n_way * n_support, -1), z[:, :, n_support:].reshape(episodes, n_way * n_query, -1)


def labels(n_way, per):
    return torch.arange(n_way).repeat_interleave(per)


def dense_chain(feats, n_way, n_support, n_query, episodes=1):
    """-> (loss, scores [episodes*n_way*n_query, n_way]); the loss is the mean cross entropy of the scores over all query rows (the
    mean of the episodes' losses).  Differentiable in feats."""
    n, S = n_support, n_way * n_support
    D = feats.shape[1]
    lam = n / (n + 1.0)
    ZS, ZQ = split(feats, n_way, n_support, n_query, episodes)
    eye = torch.eye(D, dtype=feats.dtype)
    scores = []
    for e in range(episodes):
        T = ZS[e] - ZS[e].mean(0, keepdim=True)
        St = T.t() @ T / (S - 1) if S > 1 else torch.zeros(D, D, dtype=feats.dtype)
        cols = []
        for c in range(n_way):
            zc = ZS[e][c * n:(c + 1) * n]
            mu = zc.mean(0)
            Sc = (zc - mu).t() @ (zc - mu) / (n - 1) if n > 1 else torch.zeros(D, D, dtype=feats.dtype)
            Qinv = torch.linalg.inv(lam * Sc + (1.0 - lam) * St + BETA * eye)
            d = ZQ[e] - mu
            cols.append(-0.5 * ((d @ Qinv) * d).sum(1))
        scores.append(torch.stack(cols, dim=1))
    scores = torch.cat(scores)
    return F.cross_entropy(scores, labels(n_way, n_query).repeat(episodes)), scores


def closed_form(feats, n_way, n_support, n_query, episodes=1, dscores=None):
    """The span form of DESIGN.md section 22 and its backward, no autograd -> (loss, scores, dfeats).  ``dscores``: the upstream
    gradient [episodes*Q, n_way]; None = that of the mean cross entropy."""
    dt = feats.dtype
    n, S, Q = n_support, n_way * n_support, n_way * n_query
    D = feats.shape[1]
    lam = n / (n + 1.0)
    ZS, ZQ = split(feats.detach(), n_way, n_support, n_query, episodes)
    YQ = F.one_hot(labels(n_way, n_query), n_way).to(dt)
    tapes, scores = [], []
    for e in range(episodes):
        mu_c = ZS[e].reshape(n_way, n, D).mean(1)
        T = ZS[e] - ZS[e].mean(0, keepdim=True)
        G = T @ T.t()
        sc, Ws = [], []
        for c in range(n_way):
            d = ZQ[e] - mu_c[c]                                   # [Q, D]
            if S > 1:
                a, b = (1.0 - lam) / (S - 1), (lam / (n - 1) if n > 1 else 0.0)
                P = torch.zeros(S, S, dtype=dt)
                P[c * n:(c + 1) * n, c * n:(c + 1) * n] = torch.eye(n, dtype=dt) - 1.0 / n
                Minv = (torch.eye(S, dtype=dt) - P) / a + P / (a + b)
                w = torch.linalg.solve(BETA * Minv + G, T @ d.t()).t()        # [Q, S]
            else:
                w = torch.zeros(Q, S, dtype=dt)
            r = d - w @ T
            sc.append(-(d * r).sum(1) / (2.0 * BETA))
            Ws.append(w)
        scores.append(torch.stack(sc, dim=1))
        tapes.append((mu_c, T, torch.stack(Ws, dim=1)))              # w [Q, n_way, S]
    scores = torch.cat(scores)
    logp = torch.log_softmax(scores, dim=1)
    loss = -(logp * YQ.repeat(episodes, 1)).sum() / (episodes * Q)
    g = (torch.softmax(scores, dim=1) - YQ.repeat(episodes, 1)) / (episodes * Q) if dscores is None else dscores.to(dt)
    dfeats = torch.zeros(episodes, n_way, n_support + n_query, D, dtype=dt)
    for e in range(episodes):
        mu_c, T, w = tapes[e]
        ge = g[e * Q:(e + 1) * Q]
        dZQ, dT, dZS = torch.zeros(Q, D, dtype=dt), torch.zeros(S, D, dtype=dt), torch.zeros(S, D, dtype=dt)
        for c in range(n_way):
            r = ZQ[e] - mu_c[c] - w[:, c] @ T
            gr = ge[:, c:c + 1] * r / BETA
            dZQ -= gr
            dT += w[:, c].t() @ gr
            dZS[c * n:(c + 1) * n] += gr.sum(0) / n              # through mu_c
        dZS += dT - dT.mean(0, keepdim=True)                      # through T = Z_S - mu_t
        dfeats[e, :, :n_support] = dZS.reshape(n_way, n_support, D)
        dfeats[e, :, n_support:] = dZQ.reshape(n_way, n_query, D)
    return loss, scores, dfeats.reshape(-1, D)
