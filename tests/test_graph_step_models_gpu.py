"""The graphed training step (common/graph_step.py) of EVERY plugin that can take it, against the eager step.

`hip_graph_step: auto` (the default) replays the step of the plugins in DEFAULT as a hipGraph, `hip_graph_step: True` also that
of the plugins in ADMITTED; the plugins in OPTED_OUT never replay.  A host-only test keeps the three lists complete, so a new
plugin cannot slip past the rest of this file.  For every plugin of DEFAULT + ADMITTED one process does a discarded eager
warm-up run (the first library GEMM of a process can pick another algorithm, see tests/test_models_gpu.py), two eager runs
E1, E2 and one graphed run G from the same seed in deterministic mode: two epochs each, driven the way `Trainer.fit` drives
them, with a learning-rate decay between them and at least five full batches plus a short last one per epoch.

What is checked of G: the step was captured once per epoch and replayed for every full batch after the eager ones (counted,
not assumed), no capture failed, the optimizer's device counter saw every batch.  What is compared between G and E1: every
per-batch loss, every parameter after the row-lazy tables are flushed, both Adam moments.  The tolerance is measured against
EAGER: with n_t = max |E2 - E1| of a tensor t, G must equal E1 bit for bit where n_t == 0 (what deterministic mode promises
for a step made only of this project's kernels) and stay within 4 n_t otherwise (a library GEMM inside the step; the 4
because n_t is one sample of a maximum over many elements, not a bound), never beyond rtol 1e-4 / atol 2e-5 on parameters and
rtol 1e-5 on losses.  The measured figures are printed and tabulated in EXPERIMENTS.md ("Graphed step against eager, every
plugin").  `test_frozen_host_state_is_noticed` shows the comparison rejecting a replay that froze host state."""
import os
import re

import numpy as np
import pytest
import torch

from tests.test_models_gpu import _golden, _write_user_graph, build

# the plugins of `hip_graph_step: auto` (graph_capturable = True), of `hip_graph_step: True` (no flag), and those that opt out
DEFAULT = ("LayerGCN", "LightGCN", "BPR", "VBPR", "FREEDOM", "BM3", "MMGCN", "LATTICE")
ADMITTED = ("GRCN", "DualGNN", "DRAGON", "MGCN", "SMORE", "PGL", "SLMRec", "MMGCF")
OPTED_OUT = ("LGMRec", "MVGAE", "DAMRS", "SELFCFED_LGN")
NOT_TRAINED = ("ItemKNNCBF",)       # the one plugin without a training step (req_training: False)

# hyper-parameters: each plugin's own test in tests/test_models_gpu.py or its tests/test_*_models_gpu.py file
EXTRA = {
    "LayerGCN": {"n_layers": 4, "reg_weight": 1e-3, "dropout": 0.1},
    "LightGCN": {"n_layers": 3, "reg_weight": 1e-4},
    "BPR": {"reg_weight": 1e-2},
    "VBPR": {"reg_weight": 1e-3},
    "FREEDOM": {"dropout": 0.8, "reg_weight": 1e-3},
    "BM3": {"n_layers": 2, "reg_weight": 0.1, "dropout": 0.3},
    "MMGCN": {"reg_weight": 1e-3, "learning_rate": 1e-3},
    "LATTICE": {"reg_weight": 1e-3, "learning_rate": 1e-3},
    "GRCN": {"reg_weight": 1e-3, "learning_rate": 1e-3, "n_layers": 3},
    "DualGNN": {"reg_weight": 1e-3, "learning_rate": 1e-3, "aggr_mode": "add"},
    "DRAGON": {"reg_weight": 1e-3, "learning_rate": 1e-3, "aggr_mode": "add", "n_mm_layers": 1, "knn_k": 10, "mm_image_weight": 0.1},
    "MGCN": {"cl_loss": 0.01, "learning_rate": 1e-3},
    "SMORE": {"cl_loss": 0.01, "learning_rate": 1e-3, "n_ui_layers": 3, "image_knn_k": 10, "text_knn_k": 15, "reg_weight": 1e-4,
              "dropout_rate": 0.1},
    "PGL": {"dropout": 0.2, "reg_weight": 0.1, "mode": "local"},
    "SLMRec": {"learning_rate": 1e-3, "ssl_temp": 0.5, "ssl_alpha": 0.1, "reg": 1e-3, "layer_num": 3, "adj_type": "pre",
               "mm_fusion_mode": "concat"},
    "MMGCF": {"reg_weight": 1e-3, "learning_rate": 1e-3, "n_ui_layers": 2, "fusion_mode": "concat", "weighting": "alpha",
              "dropout": 0.5},
    "SELFCFED_LGN": {"n_layers": 2, "dropout": 0.2, "reg_weight": 1e-3},
    "LGMRec": {"n_ui_layers": 2, "n_mm_layers": 2, "n_hyper_layer": 1, "hyper_num": 4, "keep_rate": 0.5, "alpha": 0.3,
               "cl_weight": 1e-4, "reg_weight": 1e-6},
    "MVGAE": {"learning_rate": 1e-3, "beta": 0.1, "n_layers": 2},
    "DAMRS": {"kl_weight": 1, "neighbor_weight": 0.01, "n_mm_layers": 1, "n_ui_layers": 2, "knn_k": 10},
}
# the opt-in fused ops that sit inside a step (each from the file that tests the op in its model): captured as well
FUSED = {
    "MMGCN+fused_layers": {"fused_layers": True},
    "GRCN+fused_attention": {"fused_attention": True, "fused_attention_backward": True},
    "MGCN+fused_fusion": {"fused_fusion": True},
    "SMORE+fused_spectrum": {"fused_spectrum": True},
    "PGL+fused_ssl": {"fused_ssl": True},
}
CASES = DEFAULT + ADMITTED + tuple(FUSED)
# plugins that re-draw a pruned graph every epoch: the same edges in every run and epoch (golden file, key)
PINNED = {"LayerGCN": ("tiny", "lay_keep_idx"), "FREEDOM": ("tiny", "fr_keep_idx"), "PGL": ("pgl", "keep_idx"),
          "MMGCF": ("mmgcf", "b_keep_idx")}

BATCH = 192            # 1182 training interactions: six full batches and a short one of 30
EPOCHS = 2
DECAY = [0.5, 1]       # learning_rate_scheduler: the second epoch runs at half the rate
PARAM_CAP = (1e-4, 2e-5)        # rtol, atol of tests/test_models_gpu.py::test_graphed_train_step_equals_eager
LOSS_CAP = (1e-5, 0.0)


def _models_dir():
    import mmrec_amd
    return os.path.join(os.path.dirname(os.path.abspath(mmrec_amd.__file__)))


def _all_plugin_names():
    """every name `get_model` can return a class for: one configs/model/<Name>.yaml and one models/<name>.py each"""
    root = _models_dir()
    names = sorted(f[:-5] for f in os.listdir(os.path.join(root, "configs", "model")) if f.endswith(".yaml"))
    modules = sorted(f[:-3] for f in os.listdir(os.path.join(root, "models")) if f.endswith(".py") and not f.startswith("_"))
    assert sorted(n.lower() for n in names) == modules, (names, modules)
    return names


def test_the_three_lists_are_complete():
    """Every trainable plugin is in exactly one of DEFAULT / ADMITTED / OPTED_OUT, its class attribute says the same, the one
    plugin that does not train is named, and the overall.yaml comment on `hip_graph_step` lists DEFAULT."""
    import yaml
    from mmrec_amd.utils.utils import get_model
    names = _all_plugin_names()
    listed = DEFAULT + ADMITTED + OPTED_OUT + NOT_TRAINED
    assert len(set(listed)) == len(listed), "a plugin is in two lists"
    assert sorted(listed) == names, (sorted(set(names) - set(listed)), sorted(set(listed) - set(names)))
    assert set(EXTRA) == set(DEFAULT + ADMITTED + OPTED_OUT)
    root = _models_dir()
    for name in names:
        cls = get_model(name)
        with open(os.path.join(root, "configs", "model", name + ".yaml")) as f:
            trains = (yaml.safe_load(f) or {}).get("req_training", True)
        assert trains is not (name in NOT_TRAINED), name
        flag = getattr(cls, "graph_capturable", None)
        if name in NOT_TRAINED:
            continue
        want = True if name in DEFAULT else False if name in OPTED_OUT else None
        assert flag is want, (name, flag, want)
    with open(os.path.join(root, "configs", "overall.yaml")) as f:
        lines = f.read().split("\n")
    at = [i for i, ln in enumerate(lines) if ln.startswith("hip_graph_step:")]
    assert len(at) == 1
    comment = lines[at[0]].split("#", 1)[1]
    for ln in lines[at[0] + 1:]:
        if not ln.lstrip().startswith("#") or not ln.startswith(" "):
            break
        comment += " " + ln.lstrip()[1:]
    said = re.search(r"graph_capturable = True \(([^)]*)\)", comment)
    assert said, comment
    found = [n for n in names if re.search(r"\b%s\b" % re.escape(n), said.group(1))]
    assert sorted(found) == sorted(DEFAULT), (found, comment)


class _Stub:
    """what `Trainer._graph_wanted` looks at, without a device: the config, the two trainer variants, the model's flag"""
    def __init__(self, cls, value):
        flag = getattr(cls, "graph_capturable", None)

        class Model:
            graph_capturable = flag

            def parameters(self):
                return [type("P", (), {"is_cuda": True})()]
        self.model, self.mg, self.clip_grad_norm = Model(), False, None
        self.config = {"hip_graph_step": value}


@pytest.mark.parametrize("name", OPTED_OUT)
def test_opted_out_plugins_never_replay(name):
    """`hip_graph_step: True` admits every plugin that does not opt out: for the plugins of OPTED_OUT `_graph_wanted` stays
    False under every value of the key (and the same stub says True for an admitted and a default plugin, so it can)."""
    from mmrec_amd.common.trainer import Trainer
    from mmrec_amd.utils.utils import get_model
    for value in (True, "auto", None, False):
        assert Trainer._graph_wanted(_Stub(get_model(name), value)) is False, value
    assert Trainer._graph_wanted(_Stub(get_model(ADMITTED[0]), True)) is True
    assert Trainer._graph_wanted(_Stub(get_model(ADMITTED[0]), "auto")) is False
    assert Trainer._graph_wanted(_Stub(get_model(DEFAULT[0]), None)) is True


@pytest.mark.gpu
@pytest.mark.parametrize("name", OPTED_OUT)
def test_opted_out_plugins_train_eagerly_on_the_device(tmp_path, golden, name):
    """the same on the real model and Trainer: no graphed step, an optimizer that is not capturable"""
    from mmrec_amd.common.trainer import Trainer
    _side_files(tmp_path, name)
    config, _, _, model = build(tmp_path, golden, name, dict(_extra(name), hip_graph_step=True))
    config["hip_graph_step"] = True
    trainer = Trainer(config, model)
    assert trainer._graph_wanted() is False and trainer._graphed_step(model.calculate_loss) is None
    assert not trainer.optimizer.capturable


def _extra(case):
    """the hyper-parameters of a case; the learning rate is a grid in most plugins' yaml files: one value"""
    extra = dict(EXTRA[case.split("+")[0]], **FUSED.get(case, {}))
    extra.setdefault("learning_rate", 1e-3)
    return extra


def _side_files(tmp_path, name):
    if name in ("DualGNN", "DRAGON"):
        _write_user_graph(tmp_path, _golden(name.lower()))
    if name == "DAMRS":
        os.makedirs(os.path.join(str(tmp_path), "baby"), exist_ok=True)
        np.save(os.path.join(str(tmp_path), "baby", "item_graph_dict_2.npy"),
                {i: [[(i + 1) % 90, (i + 7) % 90], [1.0, 1.0]] for i in range(0, 90, 2)}, allow_pickle=True)


class _Recorded:
    """the training loader, with the shape of every batch it hands out written down"""
    def __init__(self, loader):
        self.loader, self.shapes = loader, []

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        for batch in self.loader:
            self.shapes.append(tuple(batch.shape))
            yield batch


def _state(model, optimizer):
    """parameters (row-lazy tables flushed) and both Adam moments, on the host"""
    from mmrec_amd.common.lazy_rows import flush_lazy_tables
    flush_lazy_tables(model)
    torch.cuda.synchronize()
    out = {}
    for n, p in model.named_parameters():
        out["p:" + n] = p.detach().cpu().numpy().copy()
        st = optimizer.state.get(p)
        if st:
            out["m:" + n] = st["exp_avg"].detach().cpu().numpy().copy()
            out["v:" + n] = st["exp_avg_sq"].detach().cpu().numpy().copy()
    return out


def _run(tmp_path, golden, case, mode, counts):
    """two epochs of `case` the way Trainer.fit drives them -> {tensor name: array}; mode: the value of `hip_graph_step`
    (None leaves the key at the default 'auto').  counts: {'captures': n, 'replays': n}, advanced by the wrapped methods."""
    from mmrec_amd import hip_ops
    from mmrec_amd.common.trainer import Trainer
    from mmrec_amd.utils.utils import init_seed
    name = case.split("+")[0]
    extra = _extra(case)
    extra.update(hip_deterministic=True, learning_rate_scheduler=DECAY, train_batch_size=BATCH)
    if mode is not None:
        extra["hip_graph_step"] = mode
    _side_files(tmp_path, name)
    config, train_data, _, model = build(tmp_path, golden, name, extra)
    assert (config["hip_graph_step"] in (None, "auto")) == (mode is None)
    train_data.batch_size = train_data.step = BATCH          # the loader takes its size from the caller, not from the config
    loader = _Recorded(train_data)
    n_batches, n_full = len(loader), len(loader) - 1
    init_seed(123)
    trainer = Trainer(config, model)
    assert hip_ops.DETERMINISTIC
    graphed = mode is not False
    assert trainer.optimizer.capturable == graphed and trainer._graph_wanted() == graphed
    keep = None
    if name in PINNED:
        src, key = PINNED[name]
        keep = torch.as_tensor((golden if src == "tiny" else _golden(src))[key]).to(model.device)
    out, eager_first = {}, int(getattr(model, "graph_eager_batches", 0) or 0)
    for epoch in range(EPOCHS):
        before = dict(counts)
        model.pre_epoch_processing()
        if keep is not None:
            model.set_kept_edges(keep)
        total, per_batch = trainer._train_epoch(loader, epoch)
        assert not torch.is_tensor(total), "NaN loss"
        trainer.lr_scheduler.step()
        model.post_epoch_processing()
        # at least five full batches and a short last one -- from what the loader really handed out
        shapes = loader.shapes[epoch * n_batches:]
        assert len(shapes) == n_batches == len(per_batch) and n_full >= 5
        assert all(s == (shapes[0][0], BATCH) for s in shapes[:-1]) and 0 < shapes[-1][1] < BATCH, shapes
        out["loss:epoch%d" % epoch] = torch.stack([x.reshape(()) for x in per_batch]).cpu().numpy().copy()
        step = trainer._graphed_step(model.calculate_loss)
        captures, replays = counts["captures"] - before["captures"], counts["replays"] - before["replays"]
        if not graphed:
            assert step is None and captures == 0 and replays == 0
            continue
        # the graphed run really replays: the first batch of the run is eager (library handles), a plugin's declared eager
        # batches follow (LATTICE: 1), the short last batch is eager, every other one is a replay of this epoch's one capture
        assert step is not None
        assert not step.failed and step.graph is not None, "the capture failed: the epoch ran eagerly"
        assert captures == 1, captures
        assert replays == n_full - eager_first - (1 if epoch == 0 else 0) and replays >= 4, (replays, n_full)
        out.setdefault("counts", []).append((captures, replays))
    lrs = [g["lr"] for g in trainer.optimizer.param_groups]
    assert all(abs(lr - extra["learning_rate"] * DECAY[0] ** EPOCHS) <= 1e-12 for lr in lrs), lrs     # the decay was applied
    if graphed:
        steps = [int(v[0].item()) for v in trainer.optimizer._dev.values()]
        assert steps and all(s == EPOCHS * n_batches for s in steps), (steps, EPOCHS * n_batches)
    out.update(_state(model, trainer.optimizer))
    return out


def _differences(e1, e2, g):
    """-> [(tensor name, n_t = max |E2 - E1|, max |G - E1|, allowed, indices beyond it)] for every compared tensor"""
    assert set(e1) == set(e2)
    # (the graphed run allocates the moments of every trainable parameter before its first capture, an eager run those of
    # the parameters that received a gradient: a moment only one side has is compared as zeros)
    assert {k for k in e1 if k[:2] not in ("m:", "v:")} == {k for k in g if k[:2] not in ("m:", "v:")}
    rows = []
    for key in sorted(set(e1) | set(g)):
        some = e1[key] if key in e1 else g[key]
        a, b, c = (np.asarray(x.get(key, np.zeros_like(some)), dtype=np.float64) for x in (e1, e2, g))
        assert a.shape == b.shape == c.shape and np.isfinite(a).all() and np.isfinite(c).all(), key
        noise = float(np.abs(b - a).max()) if a.size else 0.0
        diff = np.abs(c - a)
        rtol, atol = LOSS_CAP if key.startswith("loss:") else PARAM_CAP
        allowed = np.minimum(4.0 * noise, atol + rtol * np.abs(a))            # n_t == 0: bit for bit
        bad = np.argwhere(diff > allowed)
        rows.append((key, noise, float(diff.max()) if a.size else 0.0, 4.0 * noise, [tuple(i) for i in bad]))
    return rows


def _report(case, rows, counts=None):
    worst = lambda kind, col: max([r[col] for r in rows if r[0].startswith(kind)] or [0.0])
    print("graph-vs-eager %-22s captures/replays per epoch %s | n_t loss %.3e param %.3e m %.3e v %.3e | G-E1 loss %.3e param %.3e "
          "m %.3e v %.3e" % (case, counts, worst("loss:", 1), worst("p:", 1), worst("m:", 1), worst("v:", 1),
                             worst("loss:", 2), worst("p:", 2), worst("m:", 2), worst("v:", 2)))
    for key, noise, diff, allowed, bad in rows:
        if noise > 0 or diff > 0:
            print("    %-44s n_t %.3e  |G - E1| %.3e  allowed %.3e  beyond: %d" % (key, noise, diff, allowed, len(bad)))


@pytest.fixture
def counted(monkeypatch):
    """captures and replays, counted where they happen"""
    from mmrec_amd.common.graph_step import GraphedTrainStep
    counts = {"captures": 0, "replays": 0}
    capture, replay = GraphedTrainStep._capture, torch.cuda.CUDAGraph.replay

    def counting_capture(self, batch):
        counts["captures"] += 1
        return capture(self, batch)

    def counting_replay(self):
        counts["replays"] += 1
        return replay(self)
    monkeypatch.setattr(GraphedTrainStep, "_capture", counting_capture)
    monkeypatch.setattr(torch.cuda.CUDAGraph, "replay", counting_replay)
    return counts


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_graphed_epochs_equal_eager_epochs(tmp_path, golden, counted, case):
    from mmrec_amd import hip_ops
    name = case.split("+")[0]
    mode = None if name in DEFAULT else True         # DEFAULT: the config's own 'auto'; ADMITTED: hip_graph_step: True
    try:
        _run(tmp_path, golden, case, False, counted)                          # discarded: settles the library's choices
        e1 = _run(tmp_path, golden, case, False, counted)
        e2 = _run(tmp_path, golden, case, False, counted)
        g = _run(tmp_path, golden, case, mode, counted)
    finally:
        hip_ops.set_deterministic(hip_ops.DETERMINISTIC_DEFAULT)               # the switch is process-wide
    counts = g.pop("counts")
    assert "counts" not in e1 and "counts" not in e2
    rows = _differences(e1, e2, g)
    _report(case, rows, counts)
    assert any(r[0].startswith("m:") for r in rows) and any(r[0].startswith("loss:") for r in rows)
    moved = [k for k in e1 if k.startswith("m:") and np.abs(e1[k]).max() > 0]
    assert moved, "no parameter received a gradient"
    wrong = [(key, noise, diff, allowed, bad[:8]) for key, noise, diff, allowed, bad in rows if bad]
    assert not wrong, wrong


@pytest.mark.gpu
def test_frozen_host_state_is_noticed(counted):
    """The comparison can fail: a step that multiplies its loss by a Python-side counter bakes the counter's value at capture
    time into the graph.  The first replay (the capture batch itself) is right, every later one is not -- and `_differences`
    says so, from the second replay on, while the same comparison of the eager run with itself is clean."""
    from mmrec_amd.common.graph_step import GraphedTrainStep
    from mmrec_amd.common.optim import HipAdam
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(3)
    w0 = torch.randn(50, 16, generator=gen)
    # (ids without duplicates: the gather's backward then adds nothing twice, so the eager runs repeat bit for bit)
    batches = [torch.randperm(50, generator=gen)[:32 if b < 6 else 7].reshape(1, -1).to(dev) for b in range(7)]

    class Counting(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.table = torch.nn.Parameter(w0.clone())
            self.calls = 0

        def calculate_loss(self, batch):
            self.calls += 1                                   # host state: frozen at capture
            return (self.table[batch[0]] ** 2).sum() * float(self.calls)

    def run(graphed):
        net = Counting().to(dev)
        opt = HipAdam(net.parameters(), lr=1e-2, capturable=graphed)
        step = GraphedTrainStep(net, opt, steps_per_capture=len(batches) + 2)
        step.invalidate()
        losses = []
        for b in batches:
            if graphed:
                losses.append(step(b).detach().clone())
            else:
                losses.append(step._eager(b).detach())
        if graphed:
            assert not step.failed and step.graph is not None
        torch.cuda.synchronize()
        out = {"loss:epoch0": torch.stack(losses).cpu().numpy().copy(), "p:table": net.table.detach().cpu().numpy().copy()}
        for tag, key in (("m", "exp_avg"), ("v", "exp_avg_sq")):
            out[tag + ":table"] = opt.state[net.table][key].cpu().numpy().copy()
        return out
    e1, e2, g = run(False), run(False), run(True)
    assert counted == {"captures": 1, "replays": 5}
    assert not any(bad for *_, bad in _differences(e1, e2, e1))
    rows = {key: bad for key, _, _, _, bad in _differences(e1, e2, g)}
    # batch 0 is eager, batch 1 the capture and first replay; the replays of batches 2 .. 5 carry the stale counter (the
    # short batch 6 runs eagerly with a Python counter that stood still during the replays: wrong as well)
    assert [i[0] for i in rows["loss:epoch0"]] == [2, 3, 4, 5, 6], rows["loss:epoch0"]
    assert rows["v:table"], "the second moment is not scale-free: it must differ too"


@pytest.mark.gpu
def test_a_parameter_outside_the_captured_step_keeps_its_own_count(counted):
    """LATTICE's case in small: `late` receives a gradient only in the eager first batch of an epoch (`graph_eager_batches`),
    so it is no part of the captured step and only eager steps update it.  Its bias corrections are those of its OWN count
    (second update: step 2, as in torch.optim.Adam and in the eager run), not of the group's device counter (step 8): two
    epochs replayed equal two epochs eager bit for bit, in the parameters and in both moments."""
    from mmrec_amd.common.graph_step import GraphedTrainStep
    from mmrec_amd.common.optim import HipAdam
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(4)
    w0, l0 = torch.randn(50, 16, generator=gen), torch.randn(16, generator=gen)
    epochs = [[torch.randperm(50, generator=gen)[:32 if b < 6 else 7].reshape(1, -1).to(dev) for b in range(7)] for _ in range(2)]

    class Net(torch.nn.Module):
        graph_eager_batches = 1

        def __init__(self):
            super().__init__()
            self.table, self.late = torch.nn.Parameter(w0.clone()), torch.nn.Parameter(l0.clone())
            self.first = False

        def calculate_loss(self, batch):
            loss = (self.table[batch[0]] ** 2).sum()
            if self.first:                                    # set per epoch, outside the step: like LATTICE's graph build
                self.first = False
                loss = loss + (self.late ** 2).sum() * 0.5
            return loss

    def run(graphed):
        net = Net().to(dev)
        opt = HipAdam(net.parameters(), lr=1e-2, capturable=graphed)
        step = GraphedTrainStep(net, opt, steps_per_capture=9)
        out = {}
        for e, batches in enumerate(epochs):
            for group in opt.param_groups:
                group["lr"] = 1e-2 * 0.5 ** e
            step.invalidate()
            net.first = True
            losses = [(step(b) if graphed else step._eager(b)).detach().clone() for b in batches]
            out["loss:epoch%d" % e] = torch.stack(losses).cpu().numpy().copy()
            assert not step.failed and (step.graph is not None) == graphed
        torch.cuda.synchronize()
        for name, p in net.named_parameters():
            out["p:" + name] = p.detach().cpu().numpy().copy()
            out["m:" + name] = opt.state[p]["exp_avg"].cpu().numpy().copy()
            out["v:" + name] = opt.state[p]["exp_avg_sq"].cpu().numpy().copy()
        assert opt.state[net.late]["step"] == 2
        return out
    e1, e2, g = run(False), run(False), run(True)
    assert counted == {"captures": 2, "replays": 4 + 5}
    rows = _differences(e1, e2, g)
    _report("toy: late parameter", rows)
    assert not np.array_equal(e1["p:late"], l0.numpy()) and all(r[1] == 0 for r in rows)
    assert not [r for r in rows if r[4]], [r[:4] for r in rows if r[4]]
