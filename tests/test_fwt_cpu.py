"""ResNet10_FW (feature-wise transformation backbone) without a GPU: the module contract against the
reference's golden G28, a float64 restatement of the forward fed G28's recorded noise, a numpy restatement of the generator of
csrc/fwt.hip (Philox4x32-10 known answers, statistics), plain_state_dict, and the refusals."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import meta_fine_tuning_amd  # noqa: F401
from meta_fine_tuning_amd import backbone, synthetic
from meta_fine_tuning_amd.backbone import FWT_COLS, FWT_LAYERS
from meta_fine_tuning_amd.io_utils import model_dict
from oracle import mft_oracle as O

torch.set_num_threads(8)
FWT_COL = {name: (C, col) for name, C, col in FWT_LAYERS}


def g28(golden_dir):
    return np.load(os.path.join(golden_dir, "g28_resnet10_fw.npz"))


# ------------------------------------------------------------------------------------------------ the generator, restated in numpy
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


def fwt_words(seed, index, groups, ld=FWT_COLS):
    """The generator words of one draw: counter = (column, group, index low, index high), key = seed -> (w0, w1) [groups, ld]."""
    ctr = np.zeros((groups, ld, 4), dtype=np.uint32)
    ctr[..., 0] = np.arange(ld, dtype=np.uint32)[None, :]
    ctr[..., 1] = np.arange(groups, dtype=np.uint32)[:, None]
    ctr[..., 2] = index & 0xFFFFFFFF
    ctr[..., 3] = (index >> 32) & 0xFFFFFFFF
    key = np.zeros((groups, ld, 2), dtype=np.uint32)
    key[..., 0] = seed & 0xFFFFFFFF
    key[..., 1] = (seed >> 32) & 0xFFFFFFFF
    out = philox4x32_10(ctr, key)
    return out[..., 0], out[..., 1]


def fwt_normals(seed, index, groups, ld=FWT_COLS):
    """noise [groups, 2, ld] in float64 (the kernel rounds it to fp32 once): Box-Muller on the two 24-bit uniforms."""
    w0, w1 = fwt_words(seed, index, groups, ld)
    u1 = ((w0 >> 8).astype(np.float64) + 0.5) * 2.0 ** -24
    u2 = ((w1 >> 8).astype(np.float64) + 0.5) * 2.0 ** -24
    r = np.sqrt(-2.0 * np.log(u1))
    return np.stack([r * np.cos(2.0 * np.pi * u2), r * np.sin(2.0 * np.pi * u2)], axis=1)


def test_philox_known_answers():
    def run(ctr, key):
        return ["%08x" % v for v in philox4x32_10(np.array(ctr, dtype=np.uint32), np.array(key, dtype=np.uint32))]
    assert run([0, 0, 0, 0], [0, 0]) == ["6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"]
    assert run([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2) == ["408f276d", "41c83b0e", "a20bc7c6", "6d5451fd"]
    assert run([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0]) == ["d16cfe09", "94fdcceb", "5001e420", "24126ea1"]


def test_generator_statistics():
    draws = np.stack([fwt_normals(0, i, 1) for i in range(64)])          # [64, 1, 2, 1856]
    N = draws.size
    assert N == 237568 and np.isfinite(draws).all()
    assert abs(draws.mean()) <= 5.0 / np.sqrt(N), draws.mean()
    assert abs(draws.var() - 1.0) <= 5.0 * np.sqrt(2.0 / N), draws.var()
    flat = draws.reshape(64, -1).astype(np.float32)
    assert len({row.tobytes() for row in flat}) == 64                    # no two draw indices give equal noise
    # groups and seeds are independent streams too
    a, b = fwt_normals(0, 0, 2), fwt_normals(1, 0, 1)
    assert not np.array_equal(a[0], a[1]) and not np.array_equal(a[0], b[0])
    assert np.array_equal(a[0], fwt_normals(0, 0, 1)[0])                  # same (seed, index, group): the same noise


# ------------------------------------------------------------------------------------------------ the forward, restated in torch
def softplus100(x):
    return F.softplus(x, beta=100)


def fw_forward(sd, x, noise, prefix="", train=True, track=False):
    """ResNet10_FW.forward (backbone.py:90-130,313-350 of the reference) on state-dict tensors, in x's dtype: ``noise`` [2, 1856]
    is the noise of this one forward (row 0 = n_g, row 1 = n_b).  Eval mode: the plain ResNet10."""
    if not train:
        return O.resnet10_forward(sd, x, prefix, train=False)
    bsd = sd if track else None

    def bn(t, name):
        return O.batchnorm_train(t, sd[prefix + name + ".weight"], sd[prefix + name + ".bias"], bsd, prefix + name)

    def fwt(t, name):
        C, col = FWT_COL[name]
        z = bn(t, name)
        n_g = noise[0, col:col + C].to(t.dtype).view(1, C, 1, 1)
        n_b = noise[1, col:col + C].to(t.dtype).view(1, C, 1, 1)
        return (1 + n_g * softplus100(sd[prefix + name + ".gamma"])) * z + n_b * softplus100(sd[prefix + name + ".beta"])

    c0 = F.conv2d(x, sd[prefix + "trunk.0.weight"], None, stride=2, padding=3)
    out = F.max_pool2d(F.relu(bn(c0, "trunk.1")), kernel_size=3, stride=2, padding=1)
    for idx in (4, 5, 6, 7):
        indim, outdim, half = O.STAGES[idx]
        p = "trunk.%d" % idx
        s = 2 if half else 1
        r1 = F.relu(bn(F.conv2d(out, sd[prefix + p + ".C1.weight"], None, stride=s, padding=1), p + ".BN1"))
        b2 = fwt(F.conv2d(r1, sd[prefix + p + ".C2.weight"], None, stride=1, padding=1), p + ".BN2")
        short = out if indim == outdim else fwt(F.conv2d(out, sd[prefix + p + ".shortcut.weight"], None, stride=s, padding=0),
                                                p + ".BNshortcut")
        out = F.relu(b2 + short)
    return out.mean(dim=(2, 3))


def g28_state():
    sd = synthetic.resnet10_fw_state_dict(28, prefix="feature.")
    sd.update(synthetic.gnn_head_state_dict(29, 5))
    return sd


def test_float64_restatement_reproduces_g28(golden_dir):
    g = g28(golden_dir)
    sd = O.clone_state(g28_state(), torch.float64)
    x = synthetic.train_episode(28, 5, 5, 16, 84).double()
    noise = torch.from_numpy(g["noise"])[0]
    assert noise.shape == (2, FWT_COLS) and noise.dtype == torch.float32
    with torch.no_grad():
        feats = fw_forward(sd, x.reshape(-1, 3, 84, 84), noise, "feature.")
        z = O.fc_project(sd, feats).view(5, 21, -1)
        sc = O.gnnnet_scores_from_z(sd, z, 5, 5, 16)
        loss = F.cross_entropy(sc, torch.from_numpy(np.repeat(np.arange(5), 16)))
        ev = fw_forward(sd, x.reshape(-1, 3, 84, 84)[:10], None, "feature.", train=False)
    assert float((sc - torch.from_numpy(g["scores"])).abs().max()) < 1e-9
    assert abs(float(loss) - float(g["loss"])) < 1e-9
    assert float((ev - torch.from_numpy(g["eval_feats"])).abs().max()) < 1e-9


def test_folded_affine_is_the_layer():
    """The design of csrc/fwt.hip: per-channel noise makes the layer a BatchNorm with the affine (gm w, gm b + bt)."""
    rs = np.random.RandomState(5)
    x = torch.from_numpy(rs.standard_normal((6, 128, 5, 5)))
    w, b = torch.from_numpy(rs.uniform(0.5, 1.5, 128)), torch.from_numpy(rs.standard_normal(128) * 0.1)
    n_g, n_b = torch.from_numpy(rs.standard_normal(128)).view(1, -1, 1, 1), torch.from_numpy(rs.standard_normal(128)).view(1, -1, 1, 1)
    gamma, beta = torch.full((1, 128, 1, 1), 0.3, dtype=torch.float64), torch.full((1, 128, 1, 1), 0.5, dtype=torch.float64)
    gm, bt = 1 + n_g * softplus100(gamma), n_b * softplus100(beta)
    layer = gm * F.batch_norm(x, None, None, w, b, True) + bt
    folded = F.batch_norm(x, None, None, gm.view(-1) * w, gm.view(-1) * b + bt.view(-1), True)
    assert float((layer - folded).abs().max()) < 1e-13


# ------------------------------------------------------------------------------------------------ the module contract
def test_state_dict_keys_order_and_flags_equal_g28(golden_dir):
    from meta_fine_tuning_amd.methods.gnnnet import GnnNet
    g = g28(golden_dir)
    m = GnnNet(model_dict['ResNet10_FW'], n_way=5, n_support=5)
    assert list(m.state_dict().keys()) == [str(k) for k in g["state_keys"]]
    named = list(m.named_parameters())
    assert [n for n, _ in named] == [str(k) for k in g["param_names"]]
    assert [bool(p.requires_grad) for _, p in named] == [bool(v) for v in g["param_requires_grad"]]
    sd = m.feature.state_dict()
    assert len(sd) == 86 and list(sd.keys()) == list(synthetic.resnet10_fw_state_dict(0).keys())
    plain = list(synthetic.resnet10_state_dict(0).keys())
    assert [k for k in sd if not k.endswith((".gamma", ".beta"))] == plain and len(plain) == 72
    for name, C, _ in FWT_LAYERS:
        i = list(sd.keys()).index(name + ".bias")
        assert list(sd.keys())[i + 1:i + 3] == [name + ".gamma", name + ".beta"]
        assert tuple(sd[name + ".gamma"].shape) == (1, C, 1, 1)
        assert float(sd[name + ".gamma"].min()) == float(sd[name + ".gamma"].max()) == pytest.approx(0.3)
        assert float(sd[name + ".beta"].min()) == float(sd[name + ".beta"].max()) == pytest.approx(0.5)
        assert float(sd[name + ".weight"].min()) == 1.0 and float(sd[name + ".bias"].abs().max()) == 0.0
    m.load_state_dict(g28_state())
    # neither the seed nor the draw index is part of the checkpoint; both survive a deepcopy
    import copy
    m.feature.fwt_seed = 7
    c = copy.deepcopy(m.feature)
    assert c.fwt_seed == 7 and c.fwt_draw_index.dtype == torch.int64 and "fwt_draw_index" not in c.state_dict()


def test_filtered_last_nine_names():
    m = backbone.ResNet10_FW()
    names = [n for n, p in m.named_parameters() if p.requires_grad]
    assert names[-9:] == [n for n, _ in backbone.ResNet10().named_parameters()][-9:]
    assert [n for n, _ in m.named_parameters()][-9:] != names[-9:]          # ... the unfiltered list ends in gamma / beta


def test_plain_state_dict_round_trips_into_resnet10():
    from meta_fine_tuning_amd.methods.protonet import ProtoNet
    fw = synthetic.resnet10_fw_state_dict(3, prefix="feature.")
    plain = backbone.plain_state_dict(fw)
    ref = synthetic.resnet10_state_dict(3, prefix="feature.")
    assert list(plain.keys()) == list(ref.keys()) and all(torch.equal(plain[k], ref[k]) for k in ref)
    assert backbone.has_fwt_keys(fw) and not backbone.has_fwt_keys(plain)
    m = ProtoNet(model_dict['ResNet10'], n_way=5, n_support=5)
    m.load_state_dict(plain)
    with pytest.raises(RuntimeError):
        m.load_state_dict(fw)


# ------------------------------------------------------------------------------------------------ refusals
def test_train_main_refuses_fine_tune():
    from meta_fine_tuning_amd import train
    with pytest.raises(NotImplementedError, match="ResNet10_FW"):
        train.main(["--model", "ResNet10_FW", "--method", "gnnnet", "--fine_tune", "--stop_epoch", "1"])


def test_finetune_main_and_entry_points_refuse():
    import argparse
    from meta_fine_tuning_amd import engine, finetune
    with pytest.raises(NotImplementedError, match="plain_state_dict"):
        finetune.main(["--model", "ResNet10_FW", "--method", "gnnnet"])
    sd = synthetic.resnet10_fw_state_dict(3, prefix="feature.")
    with pytest.raises(NotImplementedError, match="plain_state_dict"):
        engine.FinetuneEngine(sd, mode="proto")
    with pytest.raises(NotImplementedError, match="plain_state_dict"):
        engine.adapt_last_block(backbone.ResNet10_FW(), torch.zeros(5, 3, 84, 84), np.zeros(5, dtype=np.int32), 1, 4)
    finetune.params = argparse.Namespace(model="ResNet10_FW", fine_tune_epoch=0)
    try:
        with pytest.raises(NotImplementedError, match="plain_state_dict"):
            finetune.finetune([torch.zeros(5, 20, 3, 84, 84)] * 2, None, None, sd, None)
    finally:
        finetune.params = None


def test_rank_enters_the_seed(monkeypatch):
    from meta_fine_tuning_amd import autograd_ops as AG
    from meta_fine_tuning_amd import parallel
    m = backbone.ResNet10_FW()
    monkeypatch.setattr(parallel, "world", lambda: (0, 2))
    s0 = AG.fwt_seed(m)
    monkeypatch.setattr(parallel, "world", lambda: (1, 2))
    s1 = AG.fwt_seed(m)
    assert s0 == 0 and s1 != s0 and 0 <= s1 < 2 ** 64 and AG.fwt_seed(m) == s1       # same rank and seed: the same key
    assert not np.array_equal(fwt_normals(s0, 0, 1), fwt_normals(s1, 0, 1))         # ranks draw different noise
    m.fwt_seed = 5
    assert AG.fwt_seed(m) == (s1 + 5) % 2 ** 64
