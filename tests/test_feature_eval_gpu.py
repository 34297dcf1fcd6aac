"""save_features / test on a real MI355X: mft_episode_top1 against numpy (exact), the lockstep evaluation
against a loop over the per-episode API from the same seeds, and the two drivers end to end."""
import os
import random
import re

import numpy as np
import pytest
import torch

import meta_fine_tuning_amd  # noqa: F401
from meta_fine_tuning_amd import _lib, backbone, configs, feature_eval, ops, save_features, synthetic
from meta_fine_tuning_amd import test as test_driver
from meta_fine_tuning_amd.data.feature_loader import init_loader
from meta_fine_tuning_amd.io_utils import model_dict

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1, 4), (1, 5, 15, 5), (3, 2, 1, 8), (2, 33, 2, 36), (7, 64, 3, 64), (1, 64, 17, 68), (601, 5, 15, 8)]
PATTERNS = ("random", "ties", "neg_inf", "one_nan", "several_nan", "padding")


def _scores(shape, pattern):
    """float32 [rows, ld] for one value pattern; columns n_way .. ld-1 are padding."""
    E, n_way, n_query, ld = shape
    rows = E * n_way * n_query
    rs = np.random.RandomState(sum(shape) + len(pattern))
    s = rs.standard_normal((rows, ld)).astype(np.float32)
    if pattern == "ties":                                   # the maximum repeated at several columns: the lowest index wins
        s = rs.randint(0, 3, size=(rows, ld)).astype(np.float32)
    elif pattern == "neg_inf":                              # every other row all -inf: prediction 0
        s[::2] = -np.inf
    elif pattern == "one_nan":
        s[np.arange(rows), rs.randint(0, n_way, size=rows)] = np.nan
    elif pattern == "several_nan":                          # the first NaN wins, whatever follows it
        s[rs.uniform(size=(rows, ld)) < 0.4] = np.nan
        s[1::3, 0] = np.inf                                 # ... also a +inf in front of it: a later NaN still wins
    elif pattern == "padding":                              # must not be read into the comparison
        s[:, n_way:] = np.where(rs.uniform(size=(rows, ld - n_way)) < 0.5, np.inf, np.nan)
    return s


def _numpy_top1(s, shape):
    E, n_way, n_query, _ = shape
    pred = np.argmax(s[:, :n_way], axis=1).astype(np.int32)           # first index of the maximum, a NaN counting as the maximum
    label = np.tile(np.repeat(np.arange(n_way), n_query), E)
    return pred, (pred == label).reshape(E, -1).sum(axis=1).astype(np.int32)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_episode_top1_equals_numpy_exactly(shape):
    E, n_way, n_query, ld = shape
    for pattern in PATTERNS:
        if pattern == "padding" and ld == n_way:
            continue
        s = _scores(shape, pattern)
        want_pred, want_correct = _numpy_top1(s, shape)
        dev = torch.from_numpy(s).cuda()
        correct, pred = ops.episode_top1(dev, E, n_way, n_query, need_pred=True)
        assert np.array_equal(pred.cpu().numpy(), want_pred), pattern
        assert np.array_equal(correct.cpu().numpy(), want_correct), pattern
        only = ops.episode_top1(dev, E, n_way, n_query)                # pred = NULL
        assert np.array_equal(only.cpu().numpy(), want_correct), pattern
        again = ops.episode_top1(dev, E, n_way, n_query)               # fixed summation order: the same bytes
        assert torch.equal(only, again)


def test_episode_top1_reads_a_strided_view_and_refuses_bad_arguments():
    E, n_way, n_query, ld = 2, 5, 3, 8
    s = _scores((E, n_way, n_query, ld), "random")
    want_pred, want_correct = _numpy_top1(s, (E, n_way, n_query, ld))
    dev = torch.from_numpy(s).cuda()
    correct, pred = ops.episode_top1(dev[:, :n_way], E, n_way, n_query, need_pred=True)      # a view: 5 columns, row stride 8
    assert np.array_equal(pred.cpu().numpy(), want_pred) and np.array_equal(correct.cpu().numpy(), want_correct)
    lib = _lib.lib()
    c = torch.zeros(E, dtype=torch.int32, device="cuda")
    p = torch.zeros(E * n_way * n_query, dtype=torch.int32, device="cuda")

    def call(ld_, e_, w_, q_):
        return lib.mft_episode_top1(ops._p(dev), ld_, e_, w_, q_, ops._p(c), ops._p(p), ops._stream())
    assert call(ld, E, n_way, n_query) == 0
    for bad in ((ld, E, 0, n_query), (ld, E, 65, n_query), (ld, E, -1, n_query), (n_way - 1, E, n_way, n_query), (ld, E, n_way, 0),
                (ld, 0, n_way, n_query), (ld, -3, n_way, n_query), (64, 1, 65, 1)):
        assert call(*bad) == _lib.MFT_EINVAL, bad
    with pytest.raises(ValueError, match="episode_top1"):
        ops.episode_top1(dev, E + 1, n_way, n_query)


# ------------------------------------------------------------------------------------------------ lockstep == sequential
N_WAY, N_SHOT, N_QUERY, EPISODES, PER_BATCH = 5, 5, 15, 6, 4
POOL = "ISIC"                       # 7 classes of 64 x 64 pool images
CASES = [("baseline", False), ("baseline++", False), ("gnnnet", False), ("protonet", False), ("matchingnet", False),
         ("metaoptnet", False), ("protonet", True)]


def _state(method):
    """A stand-in checkpoint state: the seeded backbone and the method's seeded head."""
    sd = synthetic.resnet10_state_dict(16, prefix="feature.")
    if method == "gnnnet":
        sd.update(synthetic.gnn_head_state_dict(17, N_WAY))
    elif method == "matchingnet":
        sd.update(synthetic.matchingnet_head_state())
    elif method == "metaoptnet":
        sd.update(synthetic.metaoptnet_head_state())
    return sd


def _argv(method, extra=()):
    return ["--dataset", "miniImageNet", "--method", method, "--test_dataset", POOL] + list(extra)


def _write_checkpoint(method, state, model="ResNet10"):
    from meta_fine_tuning_amd.io_utils import parse_args
    d = save_features.checkpoint_dir(parse_args('save_features', _argv(method, ["--model", model])))
    os.makedirs(d, exist_ok=True)
    torch.save({'epoch': 0, 'state': state}, os.path.join(d, "0.tar"))


def _env(monkeypatch, episodes=EPISODES, per_batch=PER_BATCH):
    monkeypatch.setenv("MFT_POOL_PER_CLASS", "24")
    monkeypatch.setenv("MFT_IMAGE_SIZE", "64")
    monkeypatch.setenv("MFT_EPISODES", str(episodes))
    monkeypatch.setenv("MFT_EPISODES_PER_BATCH", str(per_batch))
    monkeypatch.delenv("MFT_STANDIN_WEIGHTS", raising=False)


def _seed():
    random.seed(10)
    np.random.seed(10)
    torch.manual_seed(10)


def _sequential(model, method, adaptation, cl_data_file):
    """The yardstick: the sequential protocol over the same table through the existing per-episode API."""
    kind = feature_eval.adaptation_kind(method, adaptation)
    model.n_way, model.n_support, model.n_query = N_WAY, N_SHOT, N_QUERY
    y = np.repeat(range(N_WAY), N_QUERY)
    scores, accs, z_alls = [], [], []
    _seed()
    for _ in range(EPISODES):
        chosen = random.sample(sorted(cl_data_file), N_WAY)
        z_all = []
        for c in chosen:
            rows = cl_data_file[c]
            perm = np.random.permutation(len(rows))
            z_all.append([np.squeeze(rows[perm[i]]) for i in range(N_SHOT + N_QUERY)])
        z_all = torch.from_numpy(np.array(z_all))
        with torch.no_grad():
            s = model.set_forward_adaptation(z_all, is_feature=True) if kind is not None else model.set_forward(z_all, is_feature=True)
        s = s.cpu().numpy()
        scores.append(s)
        z_alls.append(z_all)
        accs.append(np.mean(np.argmax(s, axis=1) == y) * 100)
    return scores, np.asarray(accs), z_alls


def run_case(method, adaptation, tmp_path, monkeypatch):
    """-> dict: lockstep scores / accuracies (test.main and feature_eval.evaluate), sequential scores / accuracies, episodes' z_all."""
    monkeypatch.setattr(configs, "save_dir", str(tmp_path))
    _env(monkeypatch)
    _write_checkpoint(method, _state(method))
    argv = _argv(method)
    featfile = save_features.main(argv)
    acc_main = test_driver.main(argv + (["--adaptation"] if adaptation else []))
    from meta_fine_tuning_amd.io_utils import parse_args
    params = parse_args('test', argv)
    model, loaded = test_driver.load_model(params)
    assert loaded is not None or method in save_features.BASELINES
    cl = init_loader(featfile)
    _seed()
    acc_lock, s_lock = feature_eval.evaluate(model, method, feature_eval.FeatureTable(cl), N_WAY, N_SHOT, N_QUERY, EPISODES, PER_BATCH,
                                             adaptation=adaptation, return_scores=True)
    s_seq, acc_seq, z_alls = _sequential(model, method, adaptation, cl)
    return dict(acc_main=acc_main, acc_lock=acc_lock, s_lock=s_lock, s_seq=s_seq, acc_seq=acc_seq, z=z_alls, model=model)


@pytest.mark.parametrize("method,adaptation", CASES, ids=["%s%s" % (m, "_adaptation" if a else "") for m, a in CASES])
def test_lockstep_equals_sequential(method, adaptation, tmp_path, monkeypatch):
    """6 episodes in batches of 4 + 2 against the per-episode API from the same seeds.  Measured on an MI355X: the scores of all
    seven cases are bit-identical (the proto, ridge, matching, GNN, linear and cosine launchers keep a fixed per-episode summation
    order whatever the number of episodes in the launch), so equality is what is asserted -- no tolerance, no excused episode."""
    r = run_case(method, adaptation, tmp_path, monkeypatch)
    assert len(r["s_lock"]) == len(r["s_seq"]) == EPISODES
    for e, (a, b) in enumerate(zip(r["s_lock"], r["s_seq"])):
        assert a.shape == b.shape == (N_WAY * N_QUERY, N_WAY)
        assert np.array_equal(a, b), (method, e, float(np.abs(a - b).max()))
    assert np.array_equal(r["acc_lock"], r["acc_seq"])
    assert np.array_equal(r["acc_main"], r["acc_seq"])                 # what test.main returned, through its own seeding
    assert r["acc_main"].dtype == np.float64 and r["acc_main"].shape == (EPISODES,)
    # the features are not degenerate: the episodes differ and the heads tell classes apart better than chance on average
    assert not np.array_equal(r["z"][0].numpy(), r["z"][1].numpy()) and r["acc_seq"].mean() > 100.0 / N_WAY


def test_a_shape_outside_the_heads_domain_raises_before_any_launch(monkeypatch):
    table = feature_eval.FeatureTable({c: [np.ones(512, np.float32)] * 20 for c in range(40)})
    monkeypatch.setattr(ops, "gather_rows", lambda *a, **k: pytest.fail("a launch was made"))
    model = feature_eval.build_model("matchingnet", model_dict["ResNet10"], 5, 5).cuda()
    with pytest.raises(ValueError, match="MatchingNet head"):
        feature_eval.evaluate(model, "matchingnet", table, 5, 5, 0, 2, 2)
    model = feature_eval.build_model("baseline", model_dict["ResNet10"], 17, 1).cuda()
    with pytest.raises(ValueError, match="linear-head adaptation"):
        feature_eval.evaluate(model, "baseline", table, 17, 1, 15, 2, 2)
    model = feature_eval.build_model("baseline++", model_dict["ResNet10"], 17, 1).cuda()
    with pytest.raises(ValueError, match="cosine-head adaptation"):
        feature_eval.evaluate(model, "baseline++", table, 17, 1, 15, 2, 2)
    model = feature_eval.build_model("gnnnet", model_dict["ResNet10"], 5, 5).cuda()
    with pytest.raises(ValueError, match="n_support \\+ 15"):
        feature_eval.evaluate(model, "gnnnet", table, 5, 5, 4, 2, 2)


# ------------------------------------------------------------------------------------------------ drivers
def test_train_then_save_features_then_test(tmp_path, monkeypatch, capsys):
    from meta_fine_tuning_amd import train
    monkeypatch.setattr(configs, "save_dir", str(tmp_path))
    _env(monkeypatch)
    monkeypatch.setenv("MFT_IMAGE_SIZE", "84")
    train.main(["--dataset", "miniImageNet", "--method", "protonet", "--stop_epoch", "1"], n_episode=2, size=84, pool_images_per_class=24)
    argv = ["--dataset", "miniImageNet", "--method", "protonet", "--split", "base"]
    capsys.readouterr()
    f = save_features.main(argv)
    out = capsys.readouterr().out
    assert "SYNTHETIC" in out and "stand-in" not in out
    assert f == str(tmp_path / "features" / "miniImageNet" / "ResNet10_protonet_5way_5shot" / "base.npz") and os.path.isfile(f)
    with np.load(f) as z:
        n_classes = synthetic.DATASET_SHAPES["miniImageNet"][0]
        assert int(z["count"][0]) == n_classes * 24 and z["all_feats"].shape == (n_classes * 24, 512)
        assert z["all_feats"].dtype == np.float32 and np.isfinite(z["all_feats"]).all()
        assert np.array_equal(z["all_labels"], np.repeat(np.arange(n_classes, dtype=np.int32), 24))
    acc = test_driver.main(argv)
    out = capsys.readouterr().out
    m = re.search(r"^(\d+) Test Acc = (\d+\.\d\d)% \+- (\d+\.\d\d)%", out, flags=re.M)
    assert m and int(m.group(1)) == EPISODES == len(acc)
    assert float(m.group(2)) == float("%4.2f" % np.mean(acc)) and float(m.group(3)) == float("%4.2f" % (1.96 * np.std(acc) / np.sqrt(EPISODES)))
    assert ((acc >= 0) & (acc <= 100)).all()
    # `test` without its feature file, and save_features without a checkpoint, say what is missing
    with pytest.raises(FileNotFoundError, match="save_features"):
        test_driver.main(argv[:-1] + ["novel"])
    with pytest.raises(FileNotFoundError, match="MFT_STANDIN_WEIGHTS"):
        save_features.main(["--dataset", "miniImageNet", "--method", "matchingnet"])


def test_resnet10_fw_features_equal_the_plain_backbone_bit_for_bit(tmp_path, monkeypatch):
    monkeypatch.setattr(configs, "save_dir", str(tmp_path))
    _env(monkeypatch)
    fw = synthetic.resnet10_fw_state_dict(28, prefix="feature.")
    _write_checkpoint("protonet", fw, model="ResNet10_FW")
    _write_checkpoint("protonet", backbone.plain_state_dict(fw))
    f_fw = save_features.main(_argv("protonet", ["--model", "ResNet10_FW"]))
    f_plain = save_features.main(_argv("protonet"))
    assert f_fw != f_plain and "ResNet10_FW_protonet" in f_fw
    with np.load(f_fw) as a, np.load(f_plain) as b:
        assert a["all_feats"].shape == (7 * 24, 512) and np.array_equal(a["all_feats"], b["all_feats"])
        assert np.array_equal(a["all_labels"], b["all_labels"]) and np.abs(a["all_feats"]).max() > 0
    acc = test_driver.main(_argv("protonet", ["--model", "ResNet10_FW"]))           # loads the 86-key checkpoint into ProtoNet(ResNet10_FW)
    assert len(acc) == EPISODES


def test_standin_weights_are_an_opt_in_and_are_tagged(tmp_path, monkeypatch, capsys):
    monkeypatch.setattr(configs, "save_dir", str(tmp_path))
    _env(monkeypatch)
    with pytest.raises(FileNotFoundError):
        save_features.main(_argv("metaoptnet"))
    monkeypatch.setenv("MFT_STANDIN_WEIGHTS", "1")
    save_features.main(_argv("metaoptnet"))
    acc = test_driver.main(_argv("metaoptnet"))
    out = capsys.readouterr().out
    assert out.count("stand-in weights") == 2 and len(acc) == EPISODES
