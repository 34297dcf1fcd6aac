"""CPU-only checks: the C-ABI library loads and exports every symbol include/mft_hip.h declares, the host
mirrors keep the reference's state_dict / flag / sampling contracts, and the product path refuses to run
without a GPU (no silent fallback)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import meta_fine_tuning_amd  # noqa: F401
from meta_fine_tuning_amd import _lib, backbone, engine, io_utils, synthetic
from meta_fine_tuning_amd.methods import gnnnet, gnnnet_copy, baselinefinetune, meta_template

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    hdr = open(os.path.join(ROOT, "include", "mft_hip.h")).read()
    declared = set(re.findall(r"\b(mft_[a-z0-9_]+)\s*\(", hdr))
    assert len(declared) >= 28
    h = _lib.lib()
    for name in declared:
        assert hasattr(h, name), "libmft_hip.so lacks %s" % name
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    assert h.mft_version() >= 100
    # the product header declares launchers only: the form-selection hooks of tests/ and tools/ live in their own header
    assert not [n for n in declared if n.startswith("mft_debug_") or n.endswith(("_set_exact", "_set_xcd"))]
    hooks = set(re.findall(r"\b(mft_[a-z0-9_]+)\s*\(", open(os.path.join(ROOT, "include", "mft_hip_testing.h")).read()))
    assert hooks == set(_lib.TESTING_SIGNATURES) and all(hasattr(h, n) for n in hooks)


_JOB_STRUCTS = ("MftWgradJob", "MftBnStatsJob", "MftBnFwdJob", "MftBnApplyJob", "MftBnBwdJob", "MftFwtJob", "MftFwtGradJob")


def test_binding_is_derived_from_the_header():
    """One pinned launcher per type class of the header: the table is parsed from it, never typed by hand."""
    P, I, L, U, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_ulonglong, ctypes.c_float
    S, R = _lib.SIGNATURES, _lib.RESTYPES
    assert S["mft_fwt_draw_fold"][4] is U and S["mft_fwt_draw_fold"] == [P, I, I, I, U, P, P, P, P, P]
    assert S["mft_gather_rows"] == [P, P, P, I, L, P]
    assert S["mft_adam_step"].count(F) == 5 and S["mft_adam_step"] == [P, P, P, P, L, I, F, F, F, F, F, P]
    ws_floats = [n for n in S if n.endswith("_ws_floats")]
    assert ws_floats and all(R[n] is L for n in ws_floats)
    assert S["mft_version"] == [] and R["mft_version"] is I
    assert _lib.TESTING_SIGNATURES["mft_wgrad_fwd_set_exact"] == [I] and _lib.TESTING_SIGNATURES["mft_wgrad_fwd_set_xcd"] == [I]
    assert R["mft_wgrad_fwd_set_exact"] is None and R["mft_wgrad_fwd_set_xcd"] is None
    assert set(R) == set(S) | set(_lib.TESTING_SIGNATURES)
    h = _lib.lib()                                           # ... and it is what the loaded functions carry
    for n in R:
        assert getattr(h, n).restype is R[n] and list(getattr(h, n).argtypes or []) == {**S, **_lib.TESTING_SIGNATURES}[n], n
    hdr = open(os.path.join(ROOT, "include", "mft_hip.h")).read()
    assert int(re.search(r"#define\s+MFT_EINVAL\s+\((-?\d+)\)", hdr).group(1)) == _lib.MFT_EINVAL


@pytest.mark.parametrize("text, what", [
    ("int mft_a(const float* x, double y, void* stream);", "double y"),
    ("int mft_a(const float* x, size_t n, void* stream);", "size_t n"),
    ("double mft_a(void);", "double"),
    ("int mft_a(int n);\nint mft_b(void);\nint mft_a(int n);", "mft_a is declared twice"),
    ("typedef struct MftJob { const float* x; double eps; } MftJob;\nint mft_a(const MftJob* j);", "double eps"),
    ("int mft_a(int n), mft_b(int n);", "not a prototype"),
    ("", "no prototype"),
    ("/* int mft_a(void); */\n#define MFT_X 1\n", "no prototype"),
])
def test_header_parser_refuses_to_guess(text, what):
    with pytest.raises(RuntimeError) as e:
        _lib.parse_header(text)
    assert what in str(e.value)


def test_header_parser_accepts_the_forms_the_headers_use():
    protos, structs = _lib.parse_header("""
        #ifdef __cplusplus
        extern "C" {
        #endif
        enum { MFT_A = 0, MFT_B = 1 };
        typedef struct MftJob { const float* in; float* out; long long* count;   /* three pointers */
                                int ld, C, rows; float eps, momentum; } MftJob;
        long long mft_ws_floats(int C, long long rows);       // a count
        void mft_set(int on);
        int mft_go(const MftJob* jobs, const float* const* views, unsigned long long seed, unsigned* words, float eps,
                   void* stream);
        #ifdef __cplusplus
        }
        #endif""")
    P, I, L, U, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_ulonglong, ctypes.c_float
    assert protos == {"mft_ws_floats": ([I, L], L), "mft_set": ([I], None), "mft_go": ([P, P, U, P, F, P], I)}
    assert structs == {"MftJob": [("in", P), ("out", P), ("count", P), ("ld", I), ("C", I), ("rows", I), ("eps", F), ("momentum", F)]}


def _host_clang():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    d = os.path.dirname(os.path.realpath(hipcc))
    cands = [os.path.join(d, "amdclang"), os.path.join(d, "clang"), os.path.join(d, "..", "llvm", "bin", "clang"),
             os.path.join(d, "..", "lib", "llvm", "bin", "clang")]
    found = [c for c in cands if os.path.exists(c)]
    assert found, "no host clang beside %s (looked at %s): the build needs one" % (hipcc, cands)
    return found[0]


def test_job_structs_match_the_compilers_layout(tmp_path):
    """sizeof / offsetof of every job typedef as the host compiler lays include/mft_hip.h out == the ctypes classes _lib.struct builds."""
    classes = {n: _lib.struct(n) for n in _JOB_STRUCTS}
    assert _lib.struct("MftBnFwdJob") is classes["MftBnFwdJob"]                      # cached
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "mft_hip.h"', "int main(void) {"]
    for n, c in classes.items():
        lines.append('  printf("%s %%zu\\n", sizeof(%s));' % (n, n))
        lines += ['  printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (n, f, n, f) for f, _ in c._fields_]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines + ["  return 0;", "}"]) + "\n")
    exe = str(tmp_path / "layout")
    subprocess.run([_host_clang(), "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    got = dict(ln.split() for ln in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())
    want = {}
    for n, c in classes.items():
        want[n] = str(ctypes.sizeof(c))
        want.update({"%s.%s" % (n, f): str(getattr(c, f).offset) for f, _ in c._fields_})
    assert got == want
    assert [f for f, _ in classes["MftFwtJob"]._fields_] == ["w", "b", "gamma", "beta", "w_fold", "b_fold", "gm", "C", "col"]


def test_call_and_try_call(monkeypatch):
    class Stub:
        def __init__(self):
            self.seen = []

        def __getattr__(self, name):
            def fn(*args):
                self.seen.append((name, args))
                return {"mft_ok": 0, "mft_refuses": _lib.MFT_EINVAL, "mft_fails": 719}[name]
            return fn

    stub = Stub()
    monkeypatch.setattr(_lib, "_lib", stub)                  # what lib() hands out, as a running LaunchTimer does
    assert _lib.call("mft_ok", 1, 2.5, None) is None and _lib.try_call("mft_ok", 3) is True
    assert stub.seen == [("mft_ok", (1, 2.5, None)), ("mft_ok", (3,))]
    with pytest.raises(RuntimeError, match=r"mft_refuses failed with code -22 "):
        _lib.call("mft_refuses", 1)
    assert _lib.try_call("mft_refuses", 1) is False
    for f in (_lib.call, _lib.try_call):
        with pytest.raises(RuntimeError, match=r"mft_fails failed with code 719 "):
            f("mft_fails")


def test_state_dict_contract():
    """140 entries, 5,307,706 parameters, last nine feature names adaptable."""
    m = gnnnet.GnnNet(backbone.ResNet10, n_way=5, n_support=5)
    sd = m.state_dict()
    assert len(sd) == 140
    assert sum(p.numel() for p in m.parameters()) == 5307706
    assert sum(p.numel() for p in m.feature.parameters()) == 4905792
    ref = synthetic.gnnnet_state_dict(seed=0)
    assert list(sd.keys()) == list(ref.keys())
    for k in sd:
        assert tuple(sd[k].shape) == tuple(ref[k].shape), k
    names = [n for n, _ in m.feature.named_parameters()]
    assert names[-9:] == ["trunk.7.C1.weight", "trunk.7.BN1.weight", "trunk.7.BN1.bias", "trunk.7.C2.weight",
                          "trunk.7.BN2.weight", "trunk.7.BN2.bias", "trunk.7.shortcut.weight",
                          "trunk.7.BNshortcut.weight", "trunk.7.BNshortcut.bias"]
    assert sum(p.numel() for n, p in m.feature.named_parameters() if n in names[-9:]) == 3673088
    m.load_state_dict(ref)
    assert m.feature.final_feat_dim == 512 and m.feat_dim == 512
    assert m.support_label.shape == (1, 30, 5)
    assert float(m.support_label[0, 5].sum()) == 0.0 and float(m.support_label[0, 4, 0]) == 1.0


def test_gnnnet50_contract():
    m = gnnnet_copy.GnnNet(backbone.ResNet10, n_way=5, n_support=50)
    assert m.n_support == 25 and m.support_label.shape == (1, 130, 5)
    assert m._image_support() == 50 and m._graph_support() == 25
    assert isinstance(baselinefinetune.BaselineFinetune(backbone.ResNet10, 5, 5), meta_template.MetaTemplate)


@pytest.mark.parametrize("n_way", [33, 64, 0])
def test_gnnnet_refuses_episode_widths_past_the_node_rows(n_way):
    """The graph-node rows are 256 floats wide (128 fc features + 2 x 48 Gconv outputs + n_way label columns): an n_way the head
    cannot hold is refused with a ValueError naming the limit when the model / the packed head is built, before any launch."""
    from meta_fine_tuning_amd import functional as Fn
    with pytest.raises(ValueError, match="n_way <= 32"):
        gnnnet.GnnNet(io_utils.model_dict["ResNet10"], n_way=n_way, n_support=1)
    with pytest.raises(ValueError, match="n_way <= 32"):
        gnnnet_copy.GnnNet(io_utils.model_dict["ResNet10"], n_way=n_way, n_support=50)
    with pytest.raises(ValueError, match="n_way <= 32"):
        Fn.GnnHeadWeights(synthetic.gnn_head_state_dict(seed=1, n_way=max(n_way, 1)), torch.device("cpu"), n_way)
    assert gnnnet.GnnNet(io_utils.model_dict["ResNet10"], n_way=32, n_support=1).gnn.layer_last.fc.out_features == 32


def test_cli_flags_and_defaults():
    p = io_utils.parse_args('train', [])
    assert (p.dataset, p.model, p.method, p.train_n_way, p.test_n_way, p.n_shot) == ('miniImagenet', 'ResNet10', 'baseline', 5, 5, 5)
    assert (p.save_iter, p.fine_tune_epoch, p.gen_examples, p.num_classes, p.save_freq, p.start_epoch, p.stop_epoch) == (-1, 100, 10, 200, 50, 0, 400)
    assert not p.fine_tune and not p.train_aug and not p.freeze_backbone
    q = io_utils.parse_args('train', ['--method', 'gnnnet', '--n_shot', '20', '--fine_tune', '--names-list', 'a', 'b'])
    assert q.method == 'gnnnet' and q.n_shot == 20 and q.fine_tune and q.models_to_use == ['a', 'b']
    with pytest.raises(ValueError):
        io_utils.parse_args('bogus', [])
    assert 'ResNet10' in io_utils.model_dict


def test_checkpoint_lookup(tmp_path):
    d = str(tmp_path)
    assert io_utils.get_resume_file(d) is None
    for n in (0, 50, 399):
        open(os.path.join(d, "%d.tar" % n), "w").close()
    assert io_utils.get_resume_file(d).endswith("399.tar")
    assert io_utils.get_best_file(d).endswith("399.tar")
    open(os.path.join(d, "best_model.tar"), "w").close()
    assert io_utils.get_best_file(d).endswith("best_model.tar")
    assert io_utils.get_assigned_file(d, 7).endswith("7.tar")


def test_permutation_draw_order_matches_reference():
    """finetune.py:270-272 draws one permutation per epoch from the global numpy RNG; batching episodes must keep
    the stream order episode by episode."""
    np.random.seed(10)
    a = [engine.draw_perms(500, 5) for _ in range(3)]
    np.random.seed(10)
    b = [[np.random.permutation(500) for _ in range(5)] for _ in range(3)]
    for x, y in zip(a, b):
        for p, q in zip(x, y):
            assert np.array_equal(p, q)


def test_synthetic_episode_contract():
    ep = synthetic.test_episode(3, 5, 5, 15, 84, gen_examples=2)
    assert len(ep) == 4 and ep[0].shape == (5, 20, 3, 84, 84) and ep[0].dtype == torch.float32
    assert torch.equal(ep[0], ep[1])                      # finetune.py:606
    assert not torch.equal(ep[0], ep[2])
    assert torch.equal(synthetic.test_episode(3, 5, 5, 15, 84, 2)[3], ep[3])      # deterministic
    x = synthetic.train_episode(4, 5, 5, 16, 84)
    assert x.shape == (5, 21, 3, 84, 84)


def test_no_silent_cpu_fallback():
    m = backbone.ResNet10()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(2, 3, 84, 84))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            engine.FinetuneEngine(synthetic.gnnnet_state_dict(), episodes_per_batch=1)


def test_step_tables_shapes():
    if torch.cuda.is_available():
        pytest.skip("host-logic test for the CPU tier")
    e = engine.FinetuneEngine.__new__(engine.FinetuneEngine)
    e.E, e.bs, e.n_total, e.epochs = 2, 5, 75, 2
    e.y_support = np.tile(np.repeat(np.arange(5), 5), 3).astype(np.int32)
    perms = [[np.random.RandomState(i * 10 + ep).permutation(75) for ep in range(2)] for i in range(2)]
    tabs = e.step_tables(perms, 2)
    assert len(tabs) == 2 * 15
    k, idx, lab = tabs[16]
    assert k == 5 and idx.shape == (10,) and lab.shape == (10,)
    assert np.array_equal(idx[:5], perms[0][1][5:10]) and np.array_equal(idx[5:], 75 + perms[1][1][5:10])
    assert np.array_equal(lab[:5], e.y_support[perms[0][1][5:10]])


def test_checkpoints_interchange_with_the_reference(tmp_path):
    """a checkpoint written by this package ({'epoch','state'} .tar, train.py:46-48) loads strictly
    into the REFERENCE's own GnnNet(ResNet10) and a reference-written one loads strictly here, including the extra
    feature2./feature3. copies a meta-fine-tuned reference model carries (train.py:197-202 drops them).  The reference's side
    is its state_dict schema -- key order, shapes, dtypes -- recorded in golden G20 (oracle/make_golden_g20.py): a strict load
    needs exactly these keys with exactly these shapes."""
    g20 = np.load(os.path.join(ROOT, "tests", "golden", "g20_reference_state_dict.npz"))
    ref = [(str(k), tuple(int(d) for d in s_[:n]), str(t)) for k, s_, n, t in zip(g20["keys"], g20["shapes"], g20["ndim"], g20["dtypes"])]
    assert len(ref) == 140
    ours = gnnnet.GnnNet(backbone.ResNet10, n_way=5, n_support=5)
    ours.load_state_dict(synthetic.gnnnet_state_dict(seed=3))
    f = str(tmp_path / "399.tar")
    torch.save({"epoch": 399, "state": ours.state_dict()}, f)
    loaded = torch.load(f)["state"]
    assert [(k, tuple(v.shape), str(v.dtype).replace("torch.", "")) for k, v in loaded.items()] == ref
    for k, v in loaded.items():
        assert torch.equal(v, ours.state_dict()[k]), k
    # the other direction, with the meta-fine-tuning copies present
    gen = torch.Generator().manual_seed(5)
    sd = {k: (torch.randn(s_, generator=gen) if t == "float32" else torch.zeros(s_, dtype=getattr(torch, t))) for k, s_, t in ref}
    sd.update({k.replace("feature.", "feature2.", 1): v.clone() for k, v in sd.items() if k.startswith("feature.")})
    g = str(tmp_path / "600.tar")
    torch.save({"epoch": 600, "state": sd}, g)
    state = {k: v for k, v in torch.load(g)["state"].items() if "feature2." not in k and "feature3." not in k}
    ours2 = gnnnet.GnnNet(backbone.ResNet10, n_way=5, n_support=5)
    ours2.load_state_dict(state, strict=True)
    assert list(ours2.state_dict().keys()) == [k for k, _, _ in ref]
    for k, v in ours2.state_dict().items():
        assert torch.equal(v, sd[k]), k


def test_engine_cache_is_content_keyed():
    """finetune._EngineCache: same bytes -> same engine (deep copies, reloaded checkpoints), in-place updates of the same dict and
    different checkpoints -> different engines; entries pin the dict they were built from; eviction closes engines."""
    import copy
    from meta_fine_tuning_amd import finetune as ft

    class FakeEngine:
        def __init__(self):
            self.closed = False

        def close(self):
            self.closed = True

    built = []

    def build():
        built.append(FakeEngine())
        return built[-1]

    cache = ft._EngineCache(2)
    sd = {"feature.trunk.0.weight": torch.randn(4, 3), "feature.trunk.1.weight": torch.ones(4), "fc.0.weight": torch.randn(2, 2),
          "feature2.trunk.0.weight": torch.zeros(4, 3)}
    e0 = cache.get(sd, ("cfg",), build)
    assert cache.get(sd, ("cfg",), build) is e0 and len(built) == 1                      # identity hit
    assert cache.get(copy.deepcopy(sd), ("cfg",), build) is e0 and len(built) == 1       # content hit
    other_head = dict(sd, **{"fc.0.weight": torch.randn(2, 2)})
    assert cache.get(other_head, ("cfg",), build) is e0                                  # only the backbone tensors count
    assert cache.get(sd, ("cfg2",), build) is not e0 and len(built) == 2                 # another configuration
    with torch.no_grad():
        sd["feature.trunk.0.weight"].mul_(2.0)                                           # same dict object, new weights
    e2 = cache.get(sd, ("cfg",), build)
    assert e2 is not e0 and len(built) == 3
    assert len(cache.entries) == 2 and built[0].closed                                   # capacity 2: the oldest was evicted + closed
    assert all(ent["pins"] for ent in cache.entries)
    cache.clear()
    assert all(b.closed for b in built) and not cache.entries


def test_batched_permutation_draws_follow_the_sequential_order():
    """scores_batched draws every episode's permutations up front, in the order the reference's sequential calls consume the
    global numpy stream: per episode finetune_linear's 20 permutations of the support set (finetune.py:139-141), then
    finetune's fine_tune_epoch permutations of n_way*n_support*(views+1) (finetune.py:269-272)."""
    from meta_fine_tuning_amd import finetune as ft
    np.random.seed(10)
    got = [ft.draw_episode_perms("all", 5, 5, 4, 3) for _ in range(3)]
    np.random.seed(10)
    for lin, gnn in got:
        for p in lin:
            assert np.array_equal(p, np.random.permutation(25))
        for p in gnn:
            assert np.array_equal(p, np.random.permutation(25 * 5))
    assert len(got[0][0]) == ft.LINEAR_EPOCHS and len(got[0][1]) == 3
    np.random.seed(3)
    lin, gnn = ft.draw_episode_perms("gnnnet", 5, 20, 19, 5)
    assert lin is None and len(gnn) == 5 and gnn[0].shape == (2000,)
    lin, gnn = ft.draw_episode_perms("baseline", 5, 50, 2, 1)
    assert gnn is None and lin[0].shape == (250,)
    # per-episode generators (sharded evaluation): a pure function of (seed, episode index)
    from meta_fine_tuning_amd import parallel
    a = ft.draw_episode_perms("gnnnet", 5, 5, 3, 2, parallel.episode_rng(10, 7))
    b = ft.draw_episode_perms("gnnnet", 5, 5, 3, 2, parallel.episode_rng(10, 7))
    c = ft.draw_episode_perms("gnnnet", 5, 5, 3, 2, parallel.episode_rng(10, 8))
    assert all(np.array_equal(x, y) for x, y in zip(a[1], b[1])) and not np.array_equal(a[1][0], c[1][0])
    assert parallel.episode_torch_seed(10, 7) != parallel.episode_torch_seed(10, 8)


def test_finetune_50_and_train_50_mirror_surface():
    """finetune_50 / train_50 export what the reference's 50-shot drivers define (finetune_50.py:20,48,182; train_50.py:30) and keep
    their own module-global ``params``."""
    import inspect
    from meta_fine_tuning_amd import finetune as ft, finetune_50 as ft50, train_50
    from meta_fine_tuning_amd.methods import gnnnet_copy
    assert ft50.GnnNet is gnnnet_copy.GnnNet and ft50.params is None
    ref_sig = ["liz_x", "y", "model", "state_in", "save_it", "linear", "flatten", "n_query", "ds", "pretrained_dataset",
               "freeze_backbone", "n_way", "n_support"]
    assert list(inspect.signature(ft50.finetune).parameters) == ref_sig == list(inspect.signature(ft.finetune).parameters)
    assert list(inspect.signature(ft50.finetune_linear).parameters)[:13] == ["liz_x", "y", "state_in", "save_it", "linear", "flatten",
                                                                              "n_query", "ds", "pretrained_dataset", "freeze_backbone",
                                                                              "n_way", "n_support", "classifier"]
    assert list(inspect.signature(train_50.train).parameters) == ["base_loader", "model", "optimization", "start_epoch", "stop_epoch", "params"]
    m = gnnnet_copy.GnnNet(lambda: __import__("meta_fine_tuning_amd").backbone.ResNet10(), n_way=5, n_support=50)
    assert m.n_support == 25 and m.support_label.shape == (1, 130, 5) and hasattr(m, "train_loop50") and hasattr(m, "train_loop_finetune50")


def test_bench_helpers_and_pmc_provenance(tmp_path, monkeypatch):
    """bench.py's host-side helpers: the algorithmic FLOP count of SURVEY.md §8(d), and the rule that `roofline.traffic` is only
    quoted from a PMC pass measured on byte-identical kernel source (profiles/pmc_traffic.json carries commit + source hash)."""
    import json
    import bench
    # C2: P = 2500 image passes, 100-image final pass, GNN (15, 30): 1.0228 TFLOP per episode at 84x84 ("1.02")
    fl = bench.episode_flops(5, 5, 15, 19, 5)
    assert abs(fl / 1e12 - 1.0228) < 2e-3
    assert bench.episode_flops(5, 20, 15, 19, 5) > 3.9e12 and bench.episode_flops(5, 50, 15, 19, 5) > 9.9e12
    assert len(bench.kernel_source_sha()) == 16 and bench.kernel_source_sha(True) != bench.kernel_source_sha(False)
    # the refusal logic: a record is quoted only for its own episodes-per-step AND byte-identical kernel source.  Whether the
    # COMMITTED record is fresh is a profiling-job matter (any edit of the kernel file stales it until the PMC passes are re-run
    # on a GPU box): a stale record only warns here, and bench.py then reports traffic = null.
    with open(os.path.join(bench.ROOT, "profiles", "pmc_traffic.json")) as f:
        rec = json.load(f)
    fused = rec["kernel"].startswith("wgrad_adam_fwd_kernel")          # which of the two dominant-kernel forms the record was taken on
    sha = bench.kernel_source_sha(fused)
    if rec["kernel_source_sha16"] != sha:
        import warnings
        warnings.warn("profiles/pmc_traffic.json was measured on other kernel source (%s, now %s): bench.py reports "
                      "roofline.traffic = null until tools/final_profiles.sh is re-run" % (rec["kernel_source_sha16"], sha))
        assert bench.pmc_traffic(rec["episodes_per_step"], fused) is None
    else:
        assert bench.pmc_traffic(rec["episodes_per_step"], fused) is not None      # the committed record belongs to THIS tree's kernel
    monkeypatch.setattr(bench, "kernel_source_sha", lambda fused=False: rec["kernel_source_sha16"])
    t = bench.pmc_traffic(rec["episodes_per_step"])
    assert t is not None and 1.0 <= t["mb_per_launch"] / t["algorithmic_mb_per_launch"] < 1.1
    assert bench.pmc_traffic(rec["episodes_per_step"] + 1) is None
    # a record with a foreign hash is refused
    monkeypatch.setattr(bench, "kernel_source_sha", lambda fused=False: "0" * 16)
    assert bench.pmc_traffic(rec["episodes_per_step"]) is None
    # the power sampler reads hwmon files: fake one GPU under load and one idle
    import time
    ps = bench.PowerSampler()
    for i, (uw, hz) in enumerate(((1378e6, 2140e6), (95e6, 132e6))):
        d = tmp_path / ("hw%d" % i)
        d.mkdir()
        (d / "power1_input").write_text("%d\n" % uw)
        (d / "freq1_input").write_text("%d\n" % hz)
        (d / "power1_cap").write_text("1400000000\n")
    ps.cards = [(str(tmp_path / "hw1" / "power1_input"), str(tmp_path / "hw1" / "freq1_input"), str(tmp_path / "hw1" / "power1_cap")),
                (str(tmp_path / "hw0" / "power1_input"), str(tmp_path / "hw0" / "freq1_input"), str(tmp_path / "hw0" / "power1_cap"))]
    ps.start()
    time.sleep(0.2)
    r = ps.stop()
    assert r["socket_w_median"] == 1378 and r["shader_mhz_median"] == 2140 and r["power_cap_w"] == 1400 and r["samples"] >= 2
    empty = bench.PowerSampler()
    empty.cards = []
    empty.start()
    assert empty.stop() is None


def test_bench_dump_outputs_and_arguments(tmp_path):
    """bench.dump_outputs writes float32 (float64 stays float64) DIR/<name>.npy files and refuses more than 64 MB in all; --steps
    below 1 is refused before anything runs."""
    import subprocess
    import sys
    import bench
    bench.dump_outputs(str(tmp_path / "d"), {"scores": torch.ones(2, 3, dtype=torch.float16), "loss": np.array([0.5]),
                                             "params": torch.arange(4, dtype=torch.float32)})
    got = {f: np.load(str(tmp_path / "d" / f)) for f in sorted(os.listdir(str(tmp_path / "d")))}
    assert sorted(got) == ["loss.npy", "params.npy", "scores.npy"]
    assert got["scores.npy"].dtype == np.float32 and got["scores.npy"].shape == (2, 3) and got["loss.npy"].dtype == np.float64
    assert np.array_equal(got["params.npy"], np.arange(4, dtype=np.float32))
    with pytest.raises(SystemExit):
        bench.dump_outputs(str(tmp_path / "big"), {"x": np.zeros((64 << 20) // 4 + 1, dtype=np.float32)})
    assert not (tmp_path / "big").exists()
    r = subprocess.run([sys.executable, os.path.join(bench.ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--steps" in r.stderr


def test_slab_placement_choice():
    """engine.pick_slab_buffers: from measured triple rates pick (w, m, v) and a second weight buffer sharing (m, v) -- synthetic rates
    with two 'regions' (triples inside region {0, 1, 2, 3} are slow, as the first allocations of a process typically are)."""
    import itertools
    from meta_fine_tuning_amd import engine as eng
    K = 8
    rates = {}
    for t in itertools.combinations(range(K), 3):
        slow = sum(1 for i in t if i < 4)
        rates[t] = {3: 5.0, 2: 5.6, 1: 6.1, 0: 6.2}[slow] + 0.001 * sum(t)
    w, m, v, w2 = eng.pick_slab_buffers(rates, K)
    assert len({w, m, v, w2}) == 4 and min(w, m, v, w2) >= 4                 # everything out of the slow region
    assert rates[tuple(sorted((w, m, v)))] >= 6.2 and rates[tuple(sorted((w2, m, v)))] >= 6.2
    # one dominant triple does not win if its (m, v) pair has no good second weight buffer
    rates2 = {t: 5.0 for t in itertools.combinations(range(5), 3)}
    rates2[(0, 1, 2)] = 6.4
    rates2[(2, 3, 4)] = 6.0
    rates2[(1, 3, 4)] = 6.0
    w, m, v, w2 = eng.pick_slab_buffers(rates2, 5)
    assert {m, v} == {3, 4} and {w, w2} == {1, 2}


# ------------------------------------------------------------------------------------------------ round 3 host logic

def test_meta_training_loader_gives_every_rank_the_same_number_of_steps(monkeypatch):
    """Every step of episode-parallel meta-training is one collective (train.AllReduceAdam.step): with n_episode % W != 0 (the
    CLI default 100 episodes on 8 GPUs) the ranks must still run the SAME number of steps, over disjoint episodes."""
    from meta_fine_tuning_amd import train
    drawn = []
    monkeypatch.setattr(train.synthetic, "train_episode", lambda seed, *a, **k: drawn.append(seed) or seed)
    for n_episode, W in ((100, 8), (7, 2), (5, 3), (4, 4), (100, 1)):
        seen, lens = [], []
        for r in range(W):
            ld = train.SyntheticEpisodeLoader(5, 5, 16, 84, n_episode, rank=r, world=W)
            got = [x for x, _ in ld]
            assert len(got) == len(ld) == n_episode // W
            lens.append(len(got))
            seen += got
            assert [x for x, _ in ld] == [g + n_episode for g in got]          # the next epoch continues the stream
        assert len(set(lens)) == 1 and len(set(seen)) == len(seen) and max(seen) < n_episode
        assert len(seen) == n_episode - n_episode % W


def test_checkpoint_lookup_mirrors_the_reference(tmp_path, monkeypatch):
    """finetune.checkpoint_files against the paths the reference's __main__ opens (finetune.py:448-527, io_utils.py:49-69)."""
    from meta_fine_tuning_amd import configs, finetune as ft
    monkeypatch.setattr(configs, "save_dir", str(tmp_path))
    base = str(tmp_path) + "/checkpoints/miniImageNet/"
    P = lambda *a: io_utils.parse_args('train', list(a))
    # gnnnet: <model>_gnnnet[_aug]_<n>way_<k>shot/<save_iter>.tar                                      (finetune.py:486-498)
    assert ft.checkpoint_files(P("--method", "gnnnet", "--save_iter", "600")) == (base + "ResNet10_gnnnet_5way_5shot/600.tar", None)
    assert ft.checkpoint_files(P("--method", "gnnnet", "--save_iter", "7", "--train_aug", "--n_shot", "20", "--train_n_way", "3")) == \
        (base + "ResNet10_gnnnet_aug_3way_20shot/7.tar", None)
    # --save_iter -1: best_model.tar if present, else the newest epoch, else None                     (io_utils.py:53-69)
    d = tmp_path / "checkpoints" / "miniImageNet" / "ResNet10_gnnnet_5way_5shot"
    assert ft.checkpoint_files(P("--method", "gnnnet")) == (None, None)
    d.mkdir(parents=True)
    for name in ("3.tar", "12.tar"):
        (d / name).write_bytes(b"")
    assert ft.checkpoint_files(P("--method", "gnnnet"))[0] == str(d / "12.tar")
    (d / "best_model.tar").write_bytes(b"")
    assert ft.checkpoint_files(P("--method", "gnnnet"))[0] == str(d / "best_model.tar")
    # baseline: literal 400.tar when --save_iter is given, newest epoch otherwise                       (finetune.py:448-462)
    assert ft.checkpoint_files(P("--method", "baseline", "--save_iter", "9")) == (None, base + "ResNet10_baseline/400.tar")
    db = tmp_path / "checkpoints" / "miniImageNet" / "ResNet10_baseline_aug"
    db.mkdir(parents=True)
    for name in ("100.tar", "399.tar", "best_model.tar"):
        (db / name).write_bytes(b"")
    assert ft.checkpoint_files(P("--method", "baseline", "--train_aug")) == (None, str(db / "399.tar"))      # get_resume_file skips best_model
    # all: the GNN file is ALWAYS ..._gnnnet_aug_<n>way_<k>shot/600.tar; the baseline file uses get_best_file   (:464-480,508-514)
    assert ft.checkpoint_files(P("--method", "all", "--train_aug")) == (base + "ResNet10_gnnnet_aug_5way_5shot/600.tar", str(db / "best_model.tar"))
    assert ft.checkpoint_files(P("--method", "all", "--save_iter", "5")) == (base + "ResNet10_gnnnet_aug_5way_5shot/600.tar",
                                                                             base + "ResNet10_baseline/400.tar")
    # loading strips what a --fine_tune run leaves in the state dict                                   (finetune.py:501-511)
    f = tmp_path / "x.tar"
    torch.save({"epoch": 1, "state": {"feature.a": torch.ones(2), "feature2.a": torch.zeros(2), "feature3.trunk.b": torch.zeros(1),
                                      "fc.0.weight": torch.ones(1)}}, str(f))
    assert sorted(ft.load_checkpoint_state(str(f))) == ["fc.0.weight", "feature.a"]
    # a missing checkpoint is an error, as the reference's torch.load is (finetune.py:498) -- named epoch or not, directory or not
    monkeypatch.delenv("MFT_STANDIN_WEIGHTS", raising=False)
    for path, explicit in ((str(d / "77.tar"), True), (str(tmp_path / "nowhere" / "1.tar"), True), (None, False)):
        with pytest.raises(FileNotFoundError):
            ft._resolve_state("gnnnet", path, 5, explicit, False)
    # the stand-in weights are an explicit opt-in
    monkeypatch.setenv("MFT_STANDIN_WEIGHTS", "1")
    sd, used = ft._resolve_state("gnnnet", str(tmp_path / "nowhere" / "1.tar"), 5, True, False)
    assert used is None and len(sd) == 140
    hz = np.load(os.path.join(ROOT, "tests", "golden", "g9_head.npz"))
    assert all(torch.equal(sd[k], torch.from_numpy(hz[k])) for k in hz.files)          # not a random head


def test_balanced_batches_and_lookahead_guard():
    from meta_fine_tuning_amd import finetune as ft
    assert [ft.balanced_batch(n, 128) for n in (600, 300, 150, 75, 128, 129, 1)] == [120, 100, 75, 75, 128, 65, 1]
    # where the engine's fused inner loop applies (it wants E % 32 == 0): round the equal size up to a multiple of 32 when the padded
    # slots cost less than running unfused -- 600 -> 5 x 128, 300 -> 3 x 100 stays (128 would pad 28 %), 75 stays, 250 -> 2 x 128
    assert [ft.balanced_batch(n, 128, fused=True) for n in (600, 300, 150, 75, 128, 129, 250, 1)] == [128, 100, 75, 75, 128, 65, 128, 1]
    for n in range(1, 700, 37):
        e = ft.balanced_batch(n, 128, fused=True)
        assert e <= 128 and e * ((n + 127) // 128) >= n
    for n in range(1, 700, 37):
        e = ft.balanced_batch(n, 128)
        nb = (n + 127) // 128
        assert e <= 128 and e * nb >= n and (e - 1) * nb < n
    # a parked score is handed out only to the call it was computed for
    x = torch.zeros(1)
    st, st2, model = {"a": 1}, {"a": 1}, object()
    ctx = {"freeze_backbone": False, "state_gnn": st, "state_b": st2, "model": model}
    ft._READY[id(x)] = {"pin": x, "gnn": "G", "linear": "L", "ctx": ctx}
    with pytest.raises(RuntimeError):
        ft._take_ready([x], "gnn", True, st, model)                  # --freeze_backbone call against non-frozen parked scores
    with pytest.raises(RuntimeError):
        ft._take_ready([x], "gnn", False, st2, model)                # another state dict
    assert ft._take_ready([x], "linear", False, st2) == "L" and ft._take_ready([x], "gnn", False, st, model) == "G"
    assert not ft._READY
    # the frozen branches train nothing: the wrapper passes the loader through untouched
    la = ft.LookaheadLoader([1, 2, 3], "gnnnet", None, fine_tune_epoch=1, freeze_backbone=True)
    assert list(la) == [1, 2, 3] and not ft._READY


def test_fuse_next_policy():
    """MFT_FUSE_NEXT=auto: the fused next-step forward only where it measured faster (whole waves of the walking kernel, light trunk)."""
    f = engine.fuse_next_policy
    assert f("1", 7, False, 224, False) is True and f("0", 128, True, 84, True) is False
    assert [E for E in (1, 16, 31, 32, 64, 96, 120, 128, 160) if f("auto", E, True, 84, True)] == [32, 64, 96, 128, 160]
    assert not f("auto", 128, False, 84, True) and not f("auto", 128, True, 224, True) and not f("auto", 128, True, 84, False)


def test_placement_hint_roundtrip(tmp_path, monkeypatch):
    import json
    import stat
    monkeypatch.setenv("HOME", str(tmp_path))                         # -> ~/.cache/mft under the test's own directory
    engine._PLACEMENT_HINTS.clear()
    assert engine._placement_hint("k") is None
    good = {"chosen": [1, 2, 3, 4], "chosen_gbs": 6.1, "chosen_alt_gbs": 6.0}
    engine._placement_hint("k", good)
    d = engine._hint_dir()
    assert d.startswith(str(tmp_path)) and stat.S_IMODE(os.lstat(d).st_mode) == 0o700
    path = os.path.join(d, "slab_placement.json")
    assert stat.S_IMODE(os.lstat(path).st_mode) == 0o600 and sorted(os.listdir(d)) == ["slab_placement.json"]   # no temp file left
    engine._PLACEMENT_HINTS.clear()                                   # another process: the file answers
    assert engine._placement_hint("k")["chosen"] == [1, 2, 3, 4] and engine._placement_hint("other") is None
    assert engine._placement_hint("k", K=4) is None                   # an index beyond this engine's candidates: no hint
    # a stale, foreign or truncated-schema entry is "no hint", never an exception in FinetuneEngine's constructor
    bad = [{"chosen": [1, 2, 3]}, {"chosen": [1, 1, 2, 3], "chosen_gbs": 6.0, "chosen_alt_gbs": 6.0}, {"chosen": "1234"}, [1, 2, 3, 4],
           {"chosen": [1, 2, 3, 4], "chosen_gbs": "fast", "chosen_alt_gbs": 6.0}, {"chosen": [1, 2, 3, 4], "chosen_gbs": 6.0},
           {"chosen": [1.0, 2, 3, 4], "chosen_gbs": 6.0, "chosen_alt_gbs": 6.0}, {"chosen": [-1, 2, 3, 4], "chosen_gbs": 6.0, "chosen_alt_gbs": 6.0},
           None, 7]
    for b in bad:
        with open(path, "w") as f:
            json.dump({"k": b}, f)
        engine._PLACEMENT_HINTS.clear()
        assert engine._placement_hint("k") is None, b
    for raw in ("", "{", "[1, 2]", '"x"'):
        with open(path, "w") as f:
            f.write(raw)
        engine._PLACEMENT_HINTS.clear()
        assert engine._placement_hint("k") is None
        engine._placement_hint("k2", good)                            # and recording over a broken file repairs it
        engine._PLACEMENT_HINTS.clear()
        assert engine._placement_hint("k2")["chosen"] == [1, 2, 3, 4]
    # a hint directory somebody else could write into is not used
    os.chmod(d, 0o777)
    assert engine._hint_dir() != d
    os.chmod(d, 0o700)


def test_graphed_step_is_only_offered_where_it_can_replay(monkeypatch):
    """graph_step.for_loop: a hipGraph replay of the episode's forward + backward exists only for CUDA models and only for the two
    loss functions it knows (plain set_forward_loss; the differentiable half of set_forward_loss_finetune) -- a CPU model or a
    disabled switch get None and MetaTemplate's loop runs the reference's eager body."""
    import torch
    from meta_fine_tuning_amd import graph_step
    from meta_fine_tuning_amd.io_utils import model_dict
    from meta_fine_tuning_amd.methods.gnnnet import GnnNet
    model = GnnNet(model_dict['ResNet10'], n_way=5, n_support=5)          # parameters on the CPU
    assert graph_step.for_loop(model, model.set_forward_loss) is None
    assert graph_step.for_loop(model, model.set_forward_loss_finetune) is None
    assert "_mft_graph_steps" not in model.__dict__ or not model.__dict__["_mft_graph_steps"]
    monkeypatch.setattr(graph_step, "ENABLED", False)
    assert graph_step.for_loop(model, model.set_forward_loss) is None
    # a step that gave up (capture refused, or a loader that keeps changing the episode shape) runs the eager body
    st = graph_step.GraphedLossBackward(model, model.set_forward_loss)
    calls = []
    monkeypatch.setattr(st, "_eager", lambda x, stream=None: calls.append(tuple(x.shape)) or "eager")
    st.failed = True
    assert st(torch.zeros(5, 21, 3, 8, 8)) == "eager" and calls


def test_resident_episode_loader_draws_like_the_reference_sampler():
    """train.ResidentEpisodeLoader (datasets/miniImageNet_few_shot.py:53-74,105-107): n_way DISTINCT classes of the pool per
    episode, per class n_support + n_query DISTINCT images; episode i is a pure function of (seed, epoch, i), so W ranks walking
    i = r, r + W, ... see together exactly the episodes one rank sees, and every rank runs floor(n_episode / W) steps."""
    from meta_fine_tuning_amd import train
    pool = torch.zeros((64, 30, 4, 4, 3), dtype=torch.uint8)            # host stand-in: only the index logic is exercised here
    one = train.ResidentEpisodeLoader(pool, 5, 5, 16, 84, n_episode=10, seed=3)
    seen = set()
    for i in range(10):
        classes, images, _ = one.indices(0, i)
        assert len(set(classes.tolist())) == 5 and max(classes) < 64
        assert images.shape == (5, 21) and all(len(set(r.tolist())) == 21 and max(r) < 30 for r in images)
        seen.add(tuple(classes.tolist()))
        c2, i2, _ = one.indices(0, i)
        assert np.array_equal(classes, c2) and np.array_equal(images, i2)
    assert len(seen) > 5                                                  # episodes differ
    assert not np.array_equal(one.indices(0, 0)[0], one.indices(1, 0)[0]) or not np.array_equal(one.indices(0, 0)[1], one.indices(1, 0)[1])
    ranks = [train.ResidentEpisodeLoader(pool, 5, 5, 16, 84, n_episode=10, seed=3, rank=r, world=3) for r in range(3)]
    assert [len(r) for r in ranks] == [3, 3, 3]
    with pytest.raises(ValueError):
        train.ResidentEpisodeLoader(pool, 5, 20, 16, 84)                  # 36 images per class from a pool of 30
    with pytest.raises(ValueError):
        train.ResidentEpisodeLoader(pool.float(), 5, 5, 16, 84)


def test_training_side_view_parameters():
    """augment.sample_train_view_params: the un-augmented box of Resize(1.15 s) + CenterCrop(s), or RandomResizedCrop with
    torchvision's default scale (0.08, 1) / ratio (3/4, 4/3) + ImageJitter(.4, .4, .4) + horizontal flip only
    (datasets/miniImageNet_few_shot.py:108-141)."""
    from meta_fine_tuning_amd import augment
    P0 = augment.sample_train_view_params(np.random.RandomState(0), 50, 84, 84, 84, aug=False)
    assert P0.shape == (1, 50, augment.NPARAM)
    assert np.allclose(P0[0, :, 0:4], np.asarray(augment.noaug_box(84, 84, 84), dtype=np.float32)[None]) and np.all(P0[0, :, 4:7] == 1.0)
    assert np.all(P0[0, :, 7:10] == 0.0)
    P1 = augment.sample_train_view_params(np.random.RandomState(0), 4000, 84, 84, 84, aug=True)
    y0, x0, h, w = P1[0, :, 0], P1[0, :, 1], P1[0, :, 2], P1[0, :, 3]
    assert np.all(h >= 1) and np.all(w >= 1) and np.all(y0 >= 0) and np.all(x0 >= 0) and np.all(y0 + h <= 84) and np.all(x0 + w <= 84)
    area = h * w / (84.0 * 84.0)
    assert area.min() < 0.2 and area.max() > 0.9 and 0.07 <= area.min()          # scale (0.08, 1), not the test-time (0.5, 0.9)
    ratio = w / h
    assert ratio.min() >= 0.70 and ratio.max() <= 1.40
    assert np.all(np.abs(P1[0, :, 4:7] - 1.0) <= 0.4 + 1e-6) and np.abs(P1[0, :, 4:7] - 1.0).max() > 0.3
    assert 0.4 < P1[0, :, 7].mean() < 0.6 and np.all(P1[0, :, 8] == 0.0) and np.all(P1[0, :, 9] == 1.0)


def test_settings_object_is_the_single_typed_source_of_knobs(monkeypatch):
    """settings.Settings: one typed field per MFT_* knob (KNOBS table == dataclass fields), parsed and validated in one place;
    current() follows the environment (tests change variables), bad values raise with the variable's name, and no module of the
    package parses an MFT_* variable on its own any more (build-time MFT_EXPERIMENTS / MFT_BUILD_JOBS excepted)."""
    import dataclasses
    from meta_fine_tuning_amd import settings
    for v in [k[1] for k in settings.KNOBS]:
        monkeypatch.delenv(v, raising=False)
    s = settings.current()
    assert dataclasses.is_dataclass(s) and s == settings.Settings()            # defaults ARE the product
    assert [f.name for f in dataclasses.fields(s)] == [k[0] for k in settings.KNOBS]
    assert len({k[1] for k in settings.KNOBS}) == len(settings.KNOBS)
    with pytest.raises(dataclasses.FrozenInstanceError):
        s.fuse_next = "1"
    monkeypatch.setenv("MFT_EPISODES", "7")
    monkeypatch.setenv("MFT_TRUNK_F16X2", "0")
    s2 = settings.current()
    assert s2.episodes == 7 and s2.trunk_f16x2 is False and s2.fuse_next == "auto"
    monkeypatch.setenv("MFT_FUSE_NEXT", "yes")
    with pytest.raises(ValueError, match="MFT_FUSE_NEXT"):
        settings.current()
    monkeypatch.setenv("MFT_FUSE_NEXT", "0")
    monkeypatch.setenv("MFT_SLAB_BALLAST_GB", "lots")
    with pytest.raises(ValueError, match="MFT_SLAB_BALLAST_GB"):
        settings.current()
    # every knob is documented, and the package holds no stray parser
    assert all(len(k[4]) > 10 for k in settings.KNOBS) and "MFT_FUSE_NEXT" in settings.describe()
    pkg = os.path.dirname(os.path.abspath(settings.__file__))
    stray = []
    for root, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py") and f not in ("settings.py", "build.py"):
                txt = open(os.path.join(root, f)).read()
                stray += [(f, m) for m in re.findall(r"environ[^\n]*?(MFT_[A-Z0-9_]+)", txt)]
    assert not stray, stray


def test_bench_work_table_matches_the_header():
    """bench.LAUNCH_WORK derives the algorithmic bytes / flops of a launch from the launcher's C-ABI arguments BY POSITION: every
    launcher it names must exist in include/mft_hip.h, and evaluating its formula on arguments built from the header's parameter
    NAMES must give the textbook figure -- a signature change cannot silently shift an index."""
    import bench
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(root, "include", "mft_hip.h")).read(), flags=re.S)
    vals = {"n_img": 640, "H": 6, "W": 6, "Cin": 256, "Cout": 512, "KH": 3, "KW": 3, "stride": 2, "pad": 1, "imgs_per_group": 5}
    for name, (family, work) in bench.LAUNCH_WORK.items():
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % re.escape(name), hdr, flags=re.S)
        assert m, "launcher %s is not declared in include/mft_hip.h" % name
        params = [re.sub(r"[\*\s]", " ", q).split()[-1] for q in m.group(1).split(",")]
        v = dict(vals)
        if "KH" not in params:                                  # the 3x3 / stride-1 / pad-1 (or fixed 3x3) forms carry no kernel geometry
            v.update(KH=3, KW=3, stride=1, pad=1)
        args = [v.get(q, 0) for q in params]
        assert {"n_img", "Cin", "Cout"} <= set(params), (name, params)
        got = work(args)
        oh = (v["H"] + 2 * v["pad"] - v["KH"]) // v["stride"] + 1
        if family == "adam":
            want = 24.0 * (v["n_img"] // v["imgs_per_group"]) * v["Cout"] * v["KH"] * v["KW"] * v["Cin"]
        else:
            want = 2.0 * v["n_img"] * oh * oh * v["Cout"] * v["KH"] * v["KW"] * v["Cin"]
        assert got == want, (name, params, got, want)
    assert {f for f, _ in bench.LAUNCH_WORK.values()} == {"adam", "f32", "x3"}


def test_round6_host_pieces():
    """Host-side pieces of round 6 that need no GPU: LockstepLoader groups k consecutive episodes (a short tail is not drawn), version
    bumps happen without a launch, ZeroLease hands a buffer out once at a time and takes it back when the tape dies -- still zero in
    the padding its users never write --, and WgradBatch in its disabled form refuses nothing silently."""
    import gc
    from meta_fine_tuning_amd import functional_bwd as FB, graph_step
    from meta_fine_tuning_amd.methods.meta_template import LockstepLoader
    eps = [(torch.full((5, 21, 3, 4, 4), float(i)), None) for i in range(7)]
    ll = LockstepLoader(eps, 3)
    got = list(ll)
    assert len(ll) == 2 == len(got) and got[0][0].shape == (3, 5, 21, 3, 4, 4)
    assert [float(x[j, 0, 0, 0, 0, 0]) for x, _ in got for j in range(3)] == [0.0, 1.0, 2.0, 3.0, 4.0, 5.0]
    p = [torch.nn.Parameter(torch.zeros(3)) for _ in range(2)]
    v0 = [q._version for q in p]
    graph_step.bump_versions(p)
    assert [q._version for q in p] == [v + 1 for v in v0] and all(float(q.sum()) == 0.0 for q in p)
    graph_step.bump_versions([])
    FB.ZeroLease._free.clear()
    a = FB.ZeroLease()
    b1 = a.take((4, 8), torch.device("cpu"))
    b2 = a.take((4, 8), torch.device("cpu"))
    assert b1.data_ptr() != b2.data_ptr() and float(b1.abs().sum()) == 0.0
    b1[:, :5] = 1.0                                  # a user writes its valid columns only
    ptrs = {b1.data_ptr(), b2.data_ptr()}
    del a
    gc.collect()
    c = FB.ZeroLease()
    r1, r2 = c.take((4, 8), torch.device("cpu")), c.take((4, 8), torch.device("cpu"))
    assert {r1.data_ptr(), r2.data_ptr()} == ptrs       # the same two buffers come back: no new allocation, no fill
    back = r1 if float(r1.abs().sum()) > 0 else r2
    assert float(back[:, 5:].abs().sum()) == 0.0        # ... with the padding still zero
    r3 = c.take((4, 8), torch.device("cpu"))
    assert r3.data_ptr() not in ptrs and float(r3.abs().sum()) == 0.0


def test_round6_late_knobs_and_form_predicates():
    """The kernel-form knobs added late in round 6 exist with their measured defaults, every knob of settings.KNOBS has its row in
    README's table (variable name and default), and the host-side predicates that pick a small-problem kernel form answer without a
    GPU call where they can (the register-K GEMM rule is pure host logic; the one-launch BatchNorm rule asks the library for its limit)."""
    import inspect
    from meta_fine_tuning_amd import functional_bwd as FB, ops, settings
    s = settings.Settings()
    assert s.pair_rk_rows == 16384 and s.gemm_rk_rows == 4096 and s.wgrad_batch is True and s.pair_f16x2 is False
    readme = open(os.path.join(ROOT, "README.md")).read()
    for field, var, _, default, _doc in settings.KNOBS:
        assert "`%s`" % var in readme, "README knob table lacks %s" % var
    assert FB.GEMM_RK_ROWS == settings.current().gemm_rk_rows and FB.PAIR_RK_ROWS == settings.current().pair_rk_rows
    src = inspect.getsource(FB._gemm_fwd)
    assert "GEMM_RK_ROWS" in src and "ops.gemm_rk" in src and "ops.gemm(" in src          # both forms reachable, chosen by size
    assert ops.bn_forward_small_ok(48, 480) and ops.bn_forward_small_ok(128, 105)          # the head's BatchNorm1d layers
    assert not ops.bn_forward_small_ok(512, 945) and not ops.bn_forward_small_ok(6, 100)   # trunk.7 (measured slower), C % 4 != 0


def test_head_method_table_and_episodic_methods_agree():
    """train.HEAD_METHODS and finetune.EPISODIC_METHODS name the same head methods, every one of them refuses --fine_tune by its
    own name, and no two share a FinetuneEngine mode."""
    from meta_fine_tuning_amd import finetune, train
    for name in train.HEAD_METHODS:
        with pytest.raises(NotImplementedError, match="first-order-MAML") as e:
            train.main(['--method', name, '--fine_tune', '--stop_epoch', '1'])
        assert name in str(e.value)
    assert finetune.EPISODIC_METHODS == ("gnnnet",) + tuple(train.HEAD_METHODS)
    modes = [cls.ENGINE_MODE for cls in train.HEAD_METHODS.values()]
    assert len(set(modes)) == len(modes) == 3 and all(modes)
    assert [cls.METHOD for cls in train.HEAD_METHODS.values()] == list(train.HEAD_METHODS)
