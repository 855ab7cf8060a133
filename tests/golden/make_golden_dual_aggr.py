#!/usr/bin/env python3
"""Golden vectors for DualGNN and DRAGON with `aggr_mode` 'mean' and 'max' from the unmodified reference
-> tests/golden/dualgnn_mean.npz, dragon_mean.npz, dualgnn_max.npz, dragon_max.npz (+ dualgnn_max_ops.npz, dragon_max_ops.npz).
      python tests/golden/make_golden_dual_aggr.py

The runs are those of make_golden_dualgnn.py with one configuration value changed: same dataset, same user co-occurrence
graph, same seed, and -- Base_gcn has no parameters -- the same initial parameters and RNG positions.  The script CHECKS that
against dualgnn.npz / dragon.npz and stores only what those files do not hold: `loss1`, `result`, every `g_*`,
`scores_first_batch`.

'mean' runs on the committed torch_geometric stand-in (_shims/) as it is.

'max': THE STAND-IN FOR `aggr='max'` IS THIS SCRIPT'S, NOT THE REFERENCE'S.  The committed stand-in has no max and stays
untouched; `propagate_max` below is installed for `aggr == 'max'` inside this process only.  It implements, in plain torch,
the SELECTION RULE of mmrec_neighbor_max_f32 (include/mmrec_hip.h): per (target node, column) the first edge in `edge_index`
order whose message is NaN, else the first that attains the maximum (-0 = +0); the output is that message's bits, a node
without messages gets 0, and the whole gradient goes to the chosen edge's source.
Why the rule is ours to fix: PyG routes a CUDA max with gradients through `torch_scatter.scatter_max`, which sends the
gradient to a SINGLE, UNSPECIFIED entry among tied ones (whichever thread's atomic won); PyG without torch_scatter falls
back to `scatter_reduce('amax')`, whose backward SPLITS the gradient evenly among the tied entries.  The forward value is the
same under all three; only the routing of the gradient among exactly tied entries differs, and there the reference itself
has no single answer.  Ties are the norm in the second hop (two neighbours that copied the same x[k][c] in the first), so a
rule has to be fixed, and it is the same in the kernel, in `hip_ops.neighbor_max_torch` and here.

For 'max' each of the four Base_gcn calls of the training step (modality v / t, hop 1 / 2) is recorded as `op_<m><hop>_*`:
  in <name>_max.npz      argsrc  int32 [n, 64]  the source node chosen (-1: none)
                         margin  fp32  [n, 64]  maximum minus the largest strictly smaller candidate (inf if there is none)
  in <name>_max_ops.npz  x       fp32  [n, 64]  the conv's input (hop 2: bitwise hop 1's output)
                         gy      int8  [n, 64]  a recorded upstream gradient, in eighths (gy / 8 is the gradient)
                         gx      fp32  [n, 64]  autograd's gradient w.r.t. x for that upstream gradient
(two files per model: a committed file stays below 1 MiB).  The upstream gradients come from a private RandomState: the global
numpy / torch streams the run reads are not touched.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
from make_golden_dualgnn import make_user_graph, pack_dict  # noqa: E402

RECORDS = []            # one dict per propagate_max call, in call order
GY_RNG = np.random.RandomState(20240607)


def propagate_max(self, edge_index, size=None, **kwargs):
    """MessagePassing.propagate for aggr == 'max' (see the module docstring: this script's stand-in)"""
    x = kwargs['x']
    src, dst = edge_index[0], edge_index[1]
    n, d = (size[1] if size is not None else x.size(0)), x.size(1)
    sel = torch.full((n, d), -1, dtype=torch.int64)
    margin = torch.full((n, d), float('inf'), dtype=x.dtype)
    xd = x.detach()
    for r in range(n):
        e = torch.nonzero(dst == r).flatten()                   # the node's edges, in edge_index order
        if not e.numel():
            continue
        m = xd[src[e]]                                          # [deg, d]
        isn = m.isnan()
        top = torch.where(isn, torch.full_like(m, float('-inf')), m).max(0)[0]
        cand = torch.where(isn.any(0, keepdim=True), isn, m == top)
        order = torch.arange(e.numel()).unsqueeze(1).expand_as(m)
        first = torch.where(cand, order, torch.full_like(order, e.numel())).min(0)[0]
        sel[r] = src[e[first]]
        below = torch.where(m < top, m, torch.full_like(m, float('-inf'))).max(0)[0]
        margin[r] = top - below                                  # (inf where nothing is strictly smaller)
    some = sel >= 0
    col = torch.arange(d).unsqueeze(0).expand(n, d)
    out = torch.where(some, x[sel.clamp(min=0), col], torch.zeros((), dtype=x.dtype))
    rec = {"x": xd.numpy().copy(), "argsrc": sel.numpy().astype(np.int32), "margin": margin.numpy().copy()}
    if x.requires_grad:
        gy8 = GY_RNG.randint(-8, 9, size=(n, d)).astype(np.int8)
        (gx,) = torch.autograd.grad(out, x, torch.from_numpy(gy8.astype(np.float32) / 8.0), retain_graph=True)
        rec["gy"], rec["gx"] = gy8, gx.numpy().copy()
    RECORDS.append(rec)
    return self.update(out)


def install_max():
    from torch_geometric.nn.conv import MessagePassing
    stock = MessagePassing.propagate

    def propagate(self, edge_index, size=None, **kwargs):
        if self.aggr == 'max':
            return propagate_max(self, edge_index, size=size, **kwargs)
        return stock(self, edge_index, size=size, **kwargs)
    MessagePassing.propagate = propagate


def run(name, tmp, ug, extra, mode):
    from utils.configurator import Config
    from utils.dataset import RecDataset
    from utils.dataloader import TrainDataLoader, EvalDataLoader
    from utils.utils import init_seed, get_model
    base = dict(np.load(os.path.join(HERE, name.lower() + ".npz")))
    cd = {"gpu_id": 0, "use_gpu": False, "data_path": tmp + "/", "train_batch_size": mg.BATCH,
          "save_recommended_topk": False, "epochs": 1, "reg_weight": 1e-3, "learning_rate": 1e-3, "aggr_mode": mode}
    cd.update(extra)
    config = Config(name, "baby", cd)
    for k, v in cd.items():
        config[k] = v
    config["seed"] = mg.SEED
    dataset = RecDataset(config)
    str(dataset)
    tr, va, te = dataset.split()
    str(tr), str(va), str(te)
    train_data = TrainDataLoader(config, tr, batch_size=mg.BATCH, shuffle=True)
    valid_data = EvalDataLoader(config, va, additional_dataset=tr, batch_size=config["eval_batch_size"])
    init_seed(mg.SEED)
    train_data.pretrain_setup()
    model = get_model(name)(config, train_data)
    assert model.aggr_mode == mode and model.v_gcn.conv_embed_1.aggr == mode
    # everything the <name>.npz of the 'add' run holds about the state before the step is the same here
    rp, ids, cnt = pack_dict(ug)
    assert np.array_equal(rp, base["ug_rowptr"]) and np.array_equal(ids, base["ug_ids"]) and np.array_equal(cnt, base["ug_cnt"])
    assert np.array_equal(model.edge_index.numpy(), base["edge_index"])
    init = model.result_embed.detach().numpy().copy()
    assert np.array_equal(init, base["result_embed_init"])
    del model._parameters["result_embed"]                    # make_golden_dualgnn.py's harness note
    model.result_embed = torch.as_tensor(init)
    for pname, p in model.named_parameters():
        assert np.array_equal(p.detach().numpy(), base["p_" + pname]), pname
    assert int(np.random.get_state()[2]) == int(base["np_pos_after_init"])
    model.pre_epoch_processing()
    assert np.array_equal(np.asarray(model.epoch_user_graph, dtype=np.int64), base["epoch_user_graph"])
    assert int(np.random.get_state()[2]) == int(base["np_pos_after_epoch"])
    b1 = next(iter(train_data))
    for _ in train_data:
        pass
    assert np.array_equal(b1.numpy(), base["batch1"])
    del RECORDS[:]
    out = {}
    loss = model.calculate_loss(b1.clone())
    loss.backward()
    out["loss1"] = np.float32(loss.item())
    out["result"] = model.result_embed.detach().numpy().copy()
    for pname, p in model.named_parameters():
        if p.grad is not None:
            out["g_" + pname] = p.grad.numpy().copy()
            assert np.abs(out["g_" + pname]).max() > 0, pname
    assert {k[2:] for k in out if k.startswith("g_")} == {k[2:] for k in base if k.startswith("g_")}
    with torch.no_grad():
        users, mask = next(iter(valid_data))
        out["scores_first_batch"] = model.full_sort_predict([users, mask]).numpy()
    ops = {}
    if mode == 'max':
        assert len(RECORDS) == 4                             # v hop 1, v hop 2, t hop 1, t hop 2
        for tag, rec in zip(("v1", "v2", "t1", "t2"), RECORDS):
            assert (rec["argsrc"] >= 0).all()                # no isolated node
            out["op_%s_argsrc" % tag], out["op_%s_margin" % tag] = rec["argsrc"], rec["margin"]
            for k in ("x", "gy", "gx"):
                ops["op_%s_%s" % (tag, k)] = rec[k]
        for m in "vt":                                       # hop 2 reads hop 1's output, bit for bit
            a, x1 = RECORDS["vt".index(m) * 2]["argsrc"], RECORDS["vt".index(m) * 2]["x"]
            assert np.array_equal(x1[a, np.arange(64)[None, :]].view(np.int32), RECORDS["vt".index(m) * 2 + 1]["x"].view(np.int32))
        ties = [int((rec["margin"] == 0).sum()) for rec in RECORDS]
        print("  exact ties (margin == 0) per call:", ties, "of", RECORDS[0]["margin"].size)
    for suffix, d in (("_" + mode, out), ("_" + mode + "_ops", ops)):
        if not d:
            continue
        dst = os.path.join(HERE, name.lower() + suffix + ".npz")
        np.savez_compressed(dst, **d)
        print("wrote", dst, os.path.getsize(dst) // 1024, "KiB", len(d), "arrays")
        assert os.path.getsize(dst) < (1 << 20), "a committed file stays below 1 MiB"
    print("  %s %s loss %.6f" % (name, mode, out["loss1"]))


def main():
    import tempfile
    tmp = tempfile.mkdtemp(prefix="mmrec_golden_dual_aggr_")
    mg.make_dataset(tmp)
    ug = make_user_graph(tmp)
    mg.install_shims()
    install_max()
    os.chdir(mg.REF_SRC)
    for mode in ("mean", "max"):
        run("DualGNN", tmp, ug, {}, mode)
        run("DRAGON", tmp, ug, {"n_mm_layers": 1, "knn_k": 10, "mm_image_weight": 0.1}, mode)


if __name__ == "__main__":
    main()
