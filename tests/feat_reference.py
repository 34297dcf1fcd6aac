"""The FEAT definition of DESIGN.md section 19 restated as a plain differentiable torch chain in the dtype of its inputs (float64:
the reference; float32 on the CPU: the yardstick), and the host restatement of the dropout draw.  Shared by tests/test_feat_cpu.py
and tests/test_feat_gpu.py; nothing here touches the library."""
import math

import numpy as np
import torch
import torch.nn.functional as F

D = 512
TEMPERATURE, TEMPERATURE2, BALANCE, P_ATT, P_OUT = 64.0, 32.0, 0.01, 0.1, 0.5
HEAD = ["slf_attn.w_qs.weight", "slf_attn.w_ks.weight", "slf_attn.w_vs.weight", "slf_attn.layer_norm.weight",
        "slf_attn.layer_norm.bias", "slf_attn.fc.weight", "slf_attn.fc.bias"]


def set_to_set(X, head, m_att=None, m_out=None, taps=None):
    """A(X) for X [sets, t, D]; m_att [sets, t, t] and m_out [sets, t, D] are multipliers (None: 1).  ``taps``: a list that receives
    a dict of the call's intermediates, those a parameter gradient sums over keeping their gradients."""
    wq, wk, wv, ln_w, ln_b, wfc, bfc = head
    q, k, v = X @ wq.t(), X @ wk.t(), X @ wv.t()
    P = torch.softmax(q @ k.transpose(1, 2) / math.sqrt(X.shape[-1]), dim=2)
    o = (P if m_att is None else P * m_att) @ v
    y = o @ wfc.t() + bfc
    h = (y if m_out is None else y * m_out) + X
    A = F.layer_norm(h, (X.shape[-1],), ln_w, ln_b, 1e-5)
    if taps is not None:
        for t in (q, k, v, y, A):
            t.retain_grad()
        taps.append(dict(X=X, q=q, k=k, v=v, P=P, o=o, y=y, h=h, A=A))
    return A


def term_sums(taps):
    """Per head parameter (state-dict order): the norm of the sum of the absolute values of the terms its gradient adds up over
    the token rows of every set_to_set call in ``taps`` (after backward)."""
    ab = lambda t: t.detach().double().abs().reshape(-1, t.shape[-1])  # noqa: E731
    den = [0.0] * 7
    for tp in taps:
        X, o, h = ab(tp["X"]), ab(tp["o"]), tp["h"].detach().double().reshape(-1, tp["h"].shape[-1])
        xhat = ((h - h.mean(1, keepdim=True)) / torch.sqrt(h.var(1, unbiased=False, keepdim=True) + 1e-5)).abs()
        dq, dk, dv, dy, dA = (ab(tp[n].grad) for n in ("q", "k", "v", "y", "A"))
        for i, t in enumerate((dq.t() @ X, dk.t() @ X, dv.t() @ X, (dA * xhat).sum(0), dA.sum(0), dy.t() @ o, dy.sum(0))):
            den[i] = den[i] + t
    return [float(t.norm()) for t in den]


def split_masks(masks, episodes, n_way, T, dtype):
    """(m_att, m_out) in the layout of ops.feat_draw -> ((prototype sets' m_att [E, n_way, n_way], m_out [E, n_way, D]),
    (class sets' m_att [E * n_way, T, T], m_out [E * n_way, T, D]))."""
    if masks is None:
        return (None, None), (None, None)
    m_att, m_out = (m.to(dtype) for m in masks)
    NP = episodes * n_way
    return ((m_att[:NP * n_way].view(episodes, n_way, n_way), m_out[:NP].view(episodes, n_way, -1)),
            (m_att[NP * n_way:].view(NP, T, T), m_out[NP:].view(NP, T, -1)))


def feat_chain(feats, head, n_way, n_support, n_query, episodes=1, train=False, masks=None, taps=None):
    """feats [episodes*n_way*T, D] -> (scores [episodes*n_way*n_query, n_way], reg [episodes*n_way*T, n_way] | None)."""
    T = n_support + n_query
    z = feats.view(episodes, n_way, T, -1)
    (pa, po), (ca, co) = split_masks(masks if train else None, episodes, n_way, T, feats.dtype)
    proto = z[:, :, :n_support].sum(2) / n_support                         # [E, n_way, D]
    adapted = set_to_set(proto, head, pa, po, taps)
    zq = z[:, :, n_support:].reshape(episodes, n_way * n_query, -1)
    scores = -((zq.unsqueeze(2) - adapted.unsqueeze(1)) ** 2).sum(3) / TEMPERATURE
    reg = None
    if train:
        A = set_to_set(z.reshape(episodes * n_way, T, -1), head, ca, co, taps)
        centre = (A.sum(1) / T).view(episodes, n_way, -1)
        za = z.reshape(episodes, n_way * T, -1)
        reg = (-((za.unsqueeze(2) - centre.unsqueeze(1)) ** 2).sum(3) / TEMPERATURE2).reshape(episodes * n_way * T, n_way)
    return scores.reshape(episodes * n_way * n_query, n_way), reg


def labels(n_way, n_query, n_support, episodes=1):
    yq = torch.from_numpy(np.tile(np.repeat(np.arange(n_way), n_query), episodes))
    ya = torch.from_numpy(np.tile(np.repeat(np.arange(n_way), n_support + n_query), episodes))
    return yq, ya


def feat_loss(scores, reg, n_way, n_support, n_query, episodes=1):
    """(total, main, aux | None): CE(scores, y_query) + BALANCE * CE(reg, y_all), both means."""
    yq, ya = labels(n_way, n_query, n_support, episodes)
    main = F.cross_entropy(scores, yq)
    if reg is None:
        return main, main, None
    aux = F.cross_entropy(reg, ya)
    return main + BALANCE * aux, main, aux


# ------------------------------------------------------------------------------------------------ the dropout draw on the host
def philox4x32_10(ctr, key):
    """Philox4x32-10 (Salmon et al., SC'11): ctr [..., 4], key [..., 2] uint32 -> [..., 4] uint32."""
    c = [np.asarray(ctr[..., i], dtype=np.uint64) for i in range(4)]
    k = [np.asarray(key[..., i], dtype=np.uint64) for i in range(2)]
    m32 = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & m32]
        k = [(k[0] + np.uint64(0x9E3779B9)) & m32, (k[1] + np.uint64(0xBB67AE85)) & m32]
    return np.stack(c, axis=-1).astype(np.uint32)


def draw_words(seed, index, mask_id, n):
    """Word 0 of the blocks of elements 0 .. n-1 of mask ``mask_id``: counter = (i low, i high | id << 31, index low, index high)."""
    i = np.arange(n, dtype=np.uint64)
    ctr = np.zeros((n, 4), dtype=np.uint32)
    ctr[:, 0] = (i & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    ctr[:, 1] = ((i >> np.uint64(32)).astype(np.uint32)) | np.uint32(mask_id << 31)
    ctr[:, 2] = index & 0xFFFFFFFF
    ctr[:, 3] = (index >> 32) & 0xFFFFFFFF
    key = np.zeros((n, 2), dtype=np.uint32)
    key[:, 0] = seed & 0xFFFFFFFF
    key[:, 1] = (seed >> 32) & 0xFFFFFFFF
    return philox4x32_10(ctr, key)[:, 0]


def draw_masks(seed, index, episodes, n_way, n_support, n_query, p_att=P_ATT, p_out=P_OUT):
    """(m_att, m_out) float32 numpy arrays as mft_feat_draw writes them: kept iff word * 2^-32 >= p (p as float32 holds it)."""
    T, NP = n_support + n_query, episodes * n_way
    out = []
    for mask_id, n, p in ((0, NP * n_way + NP * T * T, p_att), (1, (NP + NP * T) * D, p_out)):
        pf = float(np.float32(p))
        w = draw_words(seed, index, mask_id, n).astype(np.float64) * 2.0 ** -32
        out.append(np.where(w >= pf, np.float32(1.0 / (1.0 - pf)), np.float32(0.0)).astype(np.float32))
    return out[0], out[1].reshape(-1, D)
