"""DESIGN.md section 20 (the DKT head) as plain torch chains in the dtype of their input: the yardsticks of tests/test_dkt_cpu.py and
tests/test_dkt_gpu.py.  ``dkt_chain`` is the definition (autograd gives its gradients); ``dkt_closed_form`` restates the loss's
gradients the way csrc/dkt.hip computes them."""
import math

import torch
import torch.nn.functional as F

HEAD = ["gp.mean", "gp.raw_outputscale", "gp.raw_noise"]
NOISE_FLOOR = 1e-4
RAW_NOISE_INIT = math.log(math.expm1(0.1 - NOISE_FLOOR))


def raw_noise_for(noise):
    """raw_noise with NOISE_FLOOR + softplus(raw_noise) = noise."""
    return math.log(math.expm1(noise - NOISE_FLOOR))


def normalise(z, kernel):
    if kernel == "cossim":
        return F.normalize(z, dim=1, eps=1e-12)              # z / max(|z|, 1e-12)
    if kernel == "linear":
        return z / math.sqrt(z.shape[1])
    raise ValueError(kernel)


def hyper_values(hyper):
    mean, raw_os, raw_noise = (h.reshape(()) for h in hyper)
    return mean, F.softplus(raw_os), NOISE_FLOOR + F.softplus(raw_noise)


def targets(n_way, per_class, dtype):
    """Y [n_way * per_class, n_way]: +1 on the row's class, -1 elsewhere (rows class-major)."""
    cls = torch.arange(n_way * per_class) // per_class
    return 2.0 * F.one_hot(cls, n_way).to(dtype) - 1.0


def episode_loss(z, hyper, n_way, kernel):
    """z [N, D] class-major -> the negative marginal log-likelihood of the n_way one-vs-rest processes over N (0-dim)."""
    N = z.shape[0]
    mean, s, noise = hyper_values(hyper)
    U = normalise(z, kernel)
    K = s * (U @ U.t()) + noise * torch.eye(N, dtype=z.dtype)
    R = targets(n_way, N // n_way, z.dtype) - mean
    L = torch.linalg.cholesky(K)
    A = torch.cholesky_solve(R, L)
    logdet = 2.0 * torch.log(torch.diagonal(L)).sum()
    return (0.5 * (R * A).sum() + 0.5 * n_way * logdet + 0.5 * n_way * N * math.log(2.0 * math.pi)) / N


def episode_scores(z_support, z_query, hyper, n_way, kernel):
    """Posterior mean at the queries of the processes conditioned on the support rows -> [Q, n_way]."""
    S = z_support.shape[0]
    mean, s, noise = hyper_values(hyper)
    US, UQ = normalise(z_support, kernel), normalise(z_query, kernel)
    K = s * (US @ US.t()) + noise * torch.eye(S, dtype=z_support.dtype)
    A = torch.cholesky_solve(targets(n_way, S // n_way, z_support.dtype) - mean, torch.linalg.cholesky(K))
    return mean + UQ @ (s * (US.t() @ A))


def dkt_chain(feats, hyper, n_way, n_support, n_query, episodes=1, kernel="cossim", loss=True, scores=True):
    """feats [episodes*n_way*(n_support+n_query), D] (class-major rows, one episode after the other), hyper = (mean,
    raw_outputscale, raw_noise) -> (loss: mean over the episodes | None, scores [episodes*n_way*n_query, n_way] | None,
    per-episode losses | None)."""
    T = n_support + n_query
    z_all = feats.view(episodes, n_way, T, -1)
    losses, out = [], []
    for e in range(episodes):
        if loss:
            losses.append(episode_loss(z_all[e].reshape(n_way * T, -1), hyper, n_way, kernel))
        if scores:
            out.append(episode_scores(z_all[e, :, :n_support].reshape(n_way * n_support, -1),
                                      z_all[e, :, n_support:].reshape(n_way * n_query, -1), hyper, n_way, kernel))
    per = torch.stack(losses) if loss else None
    return (per.mean() if loss else None), (torch.cat(out) if scores else None), per


def dkt_closed_form(feats, hyper, n_way, n_support, n_query, episodes=1, kernel="cossim"):
    """The gradients of ``dkt_chain``'s loss without autograd and without K^-1: with G = (C K^-1 - A A^T) / (2 N),
    G U = (C V - A (A^T U)) / (2 N), V = K^-1 U, and tr K^-1 = (N - s sum_i <u_i, V_i>) / noise.
    -> (dfeats, dmean, draw_outputscale, draw_noise)."""
    T = n_support + n_query
    N, C = n_way * T, n_way
    mean, s, noise = hyper_values(hyper)
    z_all = feats.view(episodes, N, -1)
    dz, dmean, dos, dnoise = [], 0.0, 0.0, 0.0
    for e in range(episodes):
        z = z_all[e]
        U = normalise(z, kernel)
        K = s * (U @ U.t()) + noise * torch.eye(N, dtype=z.dtype)
        L = torch.linalg.cholesky(K)
        A = torch.cholesky_solve(targets(C, T, z.dtype) - mean, L)
        V = torch.cholesky_solve(U, L)
        GU = (C * V - A @ (A.t() @ U)) / (2 * N)
        dmean = dmean - A.sum() / N
        dos = dos + (GU * U).sum()
        dnoise = dnoise + (C * (N - s * (U * V).sum()) / noise - (A * A).sum()) / (2 * N)
        dU = 2 * s * GU
        if kernel == "cossim":
            n = z.norm(dim=1, keepdim=True)
            big = n >= 1e-12
            dz.append(torch.where(big, (dU - U * (U * dU).sum(1, keepdim=True)) / n.clamp_min(1e-12), dU / 1e-12))
        else:
            dz.append(dU / math.sqrt(z.shape[1]))
    raw_os, raw_noise = hyper[1].reshape(()), hyper[2].reshape(())
    return (torch.cat(dz) / episodes, dmean / episodes, torch.sigmoid(raw_os) * dos / episodes,
            torch.sigmoid(raw_noise) * dnoise / episodes)


def rel(a, b):
    """Relative L2 distance of a to b, in float64."""
    a, b = a.detach().double().reshape(-1).cpu(), b.detach().double().reshape(-1).cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))
