#!/usr/bin/env python3
"""Fused edge attention (hip_ops.edge_attention, mmrec_edge_attention_f32: scores, softmax and aggregation in one kernel)
against the three ops it replaces (edge_dot -> edge_softmax -> spmm_vals, hip_ops.EDGE_ATTENTION off) in ONE process, each leg
as a hipGraph replay:

    forward             Y, alpha = edge_attention(x, x, dyn)
    forward_backward    the same + d / d x of sum(Y dY) + sum(alpha dA)   (the fused op's backward is composed of the
                        existing kernels: no fused backward kernel exists)
    grcn_step           GRCN.calculate_loss + backward at Amazon-Baby shape with `fused_attention` True against False

Shapes: GRCN at Amazon-Baby shape -- both directions of the synthetic Baby training interactions over the 19,445 + 7,050 nodes,
rows = the target node, d = 64 -- and a hub-heavy graph of the same size in which 32 nodes receive a third of the edges.  HIP
events around windows of replays: median / min / max over five windows after warm-up, windows of the two paths alternating.  A
leg is "slower" when its median exceeds the three ops' by more than their own min-max spread.  Results as JSON (default
profiles/edge_attention_ab.json).

    python tools/prof_edge_attention.py [out.json]
"""
import json
import os
import shutil
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.prof_edge_dot import REPLAYS, captured, shapes, window  # noqa: E402

WINDOWS = 5


def measure(name, legs, result):
    """legs: (leg, fused fn, three-op fn)"""
    import numpy as np
    for leg, fused, three in legs:
        graphs = (("fused", captured(fused)), ("three_ops", captured(three)))
        per = {k: [] for k, _ in graphs}
        for _ in range(WINDOWS):
            for k, graph in graphs:
                per[k].append(window(graph))
        med = {k: float(np.median(v)) for k, v in per.items()}
        spread = max(per["three_ops"]) - min(per["three_ops"])
        entry = {k: {"median_us": med[k], "min_us": min(v), "max_us": max(v)} for k, v in per.items()}
        entry["fused_minus_three_ops_us"] = med["fused"] - med["three_ops"]
        entry["three_ops_spread_us"] = spread
        entry["verdict"] = "SLOWER than the spread allows" if med["fused"] - med["three_ops"] > spread else "not slower"
        result["legs"][leg] = entry
        print("%-10s %-17s fused %9.2f us [%.2f, %.2f]   three ops %9.2f us [%.2f, %.2f]   %s" % (
            name, leg, med["fused"], min(per["fused"]), max(per["fused"]), med["three_ops"], min(per["three_ops"]),
            max(per["three_ops"]), entry["verdict"]), flush=True)
        del graphs


def with_switch(on, fn):
    from mmrec_amd import hip_ops

    def run():
        hip_ops.EDGE_ATTENTION = on
        try:
            return fn()
        finally:
            hip_ops.EDGE_ATTENTION = True
    return run


def hub_heavy(n, ne, hubs=32, seed=1):
    """ne edges over n nodes; a third of them arrive at `hubs` nodes"""
    import numpy as np
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, n, ne)
    rows[: ne // 3] = rng.integers(0, hubs, ne // 3)
    return rng.permutation(rows), rng.integers(0, n, ne)


def one(name, n, rows_h, cols_h):
    import numpy as np
    import torch
    import torch.nn.functional as F
    from mmrec_amd import hip_ops
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    rows, cols = torch.from_numpy(rows_h).to(dev), torch.from_numpy(cols_h).to(dev)
    ne = rows.numel()
    x = F.normalize(torch.rand(n, 64, device=dev, generator=gen) - 0.5).requires_grad_()      # row-normalised, as in GRCN
    dY = torch.rand(n, 64, device=dev, generator=gen) - 0.5
    dA = torch.rand(ne, device=dev, generator=gen) - 0.5
    dyn = hip_ops.DynGraph(rows, cols, n, n)
    assert hip_ops.edge_attention_served(x, x, dyn)
    y_on, a_on = hip_ops.edge_attention(x, x, dyn)                    # builds the long-row list outside any capture
    y_off, a_off = with_switch(False, lambda: hip_ops.edge_attention(x, x, dyn))()
    diff = (float((y_on - y_off).abs().max()), float((a_on - a_off).abs().max()))
    assert max(diff) <= 1e-5, diff

    def forward():
        with torch.no_grad():
            return hip_ops.edge_attention(x, x, dyn)

    def forward_backward():
        y, a = hip_ops.edge_attention(x, x, dyn)
        return torch.autograd.grad((y * dY).sum() + (a * dA).sum(), x)
    deg = np.bincount(rows_h, minlength=n)
    result = {"shape": name, "n_nodes": int(n), "n_edges": int(ne), "max_edges_on_a_row": int(deg.max()),
              "rows_beyond_group_max": int((deg > hip_ops.edge_attention_group_max()).sum()),
              "group_max": hip_ops.edge_attention_group_max(), "max_abs_diff_Y_alpha": diff,
              "windows": WINDOWS, "replays_per_window": REPLAYS, "legs": {}}
    measure(name, [(leg, with_switch(True, fn), with_switch(False, fn))
                   for leg, fn in (("forward", forward), ("forward_backward", forward_backward))], result)
    torch.cuda.empty_cache()
    return result


def grcn_step(result):
    """GRCN on the synthetic Amazon-Baby dataset: calculate_loss + backward of one training batch, key on against off"""
    import torch
    from mmrec_amd import synth
    root = tempfile.mkdtemp(prefix="mmrec_baby_")
    synth.write_dataset(root, "baby", seed=0)
    from mmrec_amd.utils.configurator import Config
    from mmrec_amd.utils.dataloader import TrainDataLoader
    from mmrec_amd.utils.dataset import RecDataset
    from mmrec_amd.utils.utils import get_model, init_seed
    steps = {}
    for fused in (True, False):
        cd = dict(n_layers=3, reg_weight=1e-3, learning_rate=1e-3, gpu_id=0, use_gpu=True, data_path=root + "/", epochs=1,
                  save_recommended_topk=False, fused_attention=fused)
        config = Config("GRCN", "baby", cd)
        for k, v in cd.items():
            config[k] = v
        config["seed"] = 999
        data = RecDataset(config)
        str(data)
        tr, _, _ = data.split()
        str(tr)
        train_data = TrainDataLoader(config, tr, batch_size=config["train_batch_size"], shuffle=True)
        init_seed(999)
        train_data.pretrain_setup()
        model = get_model("GRCN")(config, train_data).to(config["device"])
        model.train()
        model.pre_epoch_processing()
        batch = next(iter(train_data)).clone()
        params = [p for p in model.parameters() if p.requires_grad]
        steps[fused] = (lambda model=model, batch=batch, params=params:
                        torch.autograd.grad(model.calculate_loss(batch), params, allow_unused=True))
        result["grcn_batch"] = int(batch.shape[1])
    measure("grcn_baby", [("grcn_step", steps[True], steps[False])], result)
    shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "edge_attention_ab.json")
    name, n, rows_h, cols_h = shapes()[0]
    results = [one(name, n, rows_h, cols_h), one("hub_heavy", n, *hub_heavy(n, rows_h.size))]
    grcn_step(results[0])
    with open(path, "w") as f:
        json.dump(results, f, indent=1)
    print("wrote", path)
