#!/usr/bin/env python3
"""Softmax over the edges that share a target node: the kernel path (hip_ops.EDGE_SOFTMAX on: mmrec_segment_softmax_f32 /
_bwd_f32) against the scatter / gather composition (the switch off: scatter-max, gathers, exp, index_add, divide and stock
autograd) in ONE process, each leg as a hipGraph replay:

    forward             alpha = edge_softmax(score, dyn)
    forward_backward    the same + d alpha / d score
    grcn_step           GRCN.calculate_loss + backward at the shape's own size (grcn_baby only): both content GCNs' softmax

Shapes: GRCN at Amazon-Baby shape -- both directions of the synthetic Baby training interactions over the 26,495 nodes,
segments = the target node -- and LATTICE's 7,050 x 10 kNN pairs, segments = the item.  HIP events around windows of replays:
median / min / max over five windows after warm-up, windows of the two paths alternating.  A leg is "slower" when its median
exceeds the composition's by more than the composition's own min-max spread.  Results as JSON (default
profiles/edge_softmax_ab.json).

    python tools/prof_edge_softmax.py [out.json]
"""
import json
import os
import shutil
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.prof_edge_dot import captured, shapes, window  # noqa: E402

WINDOWS = 5


def with_switch(on, fn):
    from mmrec_amd import hip_ops

    def run():
        hip_ops.EDGE_SOFTMAX = on
        try:
            return fn()
        finally:
            hip_ops.EDGE_SOFTMAX = True
    return run


def measure(name, legs, result):
    import numpy as np
    for leg, fn in legs:
        graphs = (("kernel", captured(with_switch(True, fn))), ("composition", captured(with_switch(False, fn))))
        per = {k: [] for k, _ in graphs}
        for _ in range(WINDOWS):
            for k, graph in graphs:
                per[k].append(window(graph))
        med = {k: float(np.median(v)) for k, v in per.items()}
        spread = max(per["composition"]) - min(per["composition"])
        entry = {k: {"median_us": med[k], "min_us": min(v), "max_us": max(v)} for k, v in per.items()}
        entry["kernel_minus_composition_us"] = med["kernel"] - med["composition"]
        entry["composition_spread_us"] = spread
        entry["verdict"] = "SLOWER than the spread allows" if med["kernel"] - med["composition"] > spread else "not slower"
        result["legs"][leg] = entry
        print("%-12s %-17s kernel %9.2f us [%.2f, %.2f]   composition %9.2f us [%.2f, %.2f]   %s" % (
            name, leg, med["kernel"], min(per["kernel"]), max(per["kernel"]), med["composition"], min(per["composition"]),
            max(per["composition"]), entry["verdict"]), flush=True)
        del graphs


def one(name, n, rows_h, cols_h):
    import numpy as np
    import torch
    from mmrec_amd import hip_ops
    from tools.prof_edge_dot import REPLAYS
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    rows, cols = torch.from_numpy(rows_h).to(dev), torch.from_numpy(cols_h).to(dev)
    ne = rows.numel()
    score = ((torch.rand(ne, device=dev, generator=gen) - 0.5) * 4).requires_grad_()
    g = torch.rand(ne, device=dev, generator=gen) - 0.5
    dyn = hip_ops.DynGraph(rows, cols, n, n)
    assert hip_ops.edge_softmax_served(score, dyn)
    # Without autograd.  With it, and the results kept, the first device run of this tool ended in a segmentation fault in the
    # captured forward_backward leg, after torch's warning that an AccumulateGrad node and the gradient's producer were on
    # different streams; supposed, not shown: autograd state of `score` bound to the default stream outlived these calls and
    # the backward captured on the side stream then synchronised the default stream with the capture.
    with torch.no_grad():
        on = hip_ops.edge_softmax(score, dyn)                         # builds the long-row list outside any capture
        off = with_switch(False, lambda: hip_ops.edge_softmax(score, dyn))()
    diff = float((on - off).abs().max())
    assert diff <= 1e-5, diff

    def forward():
        with torch.no_grad():
            return hip_ops.edge_softmax(score, dyn)

    def forward_backward():
        return torch.autograd.grad(hip_ops.edge_softmax(score, dyn), score, g)
    deg = np.bincount(rows_h)
    result = {"shape": name, "n_nodes": int(n), "n_edges": int(ne), "max_edges_on_a_row": int(deg.max()),
              "rows_beyond_group_max": int((deg > hip_ops.segment_softmax_group_max()).sum()),
              "group_max": hip_ops.segment_softmax_group_max(), "max_abs_diff_kernel_vs_composition": diff,
              "windows": WINDOWS, "replays_per_window": REPLAYS, "legs": {}}
    measure(name, (("forward", forward), ("forward_backward", forward_backward)), result)
    torch.cuda.empty_cache()
    return result


def grcn_step(result):
    """GRCN on the synthetic Amazon-Baby dataset: calculate_loss + backward of one training batch"""
    import torch
    from mmrec_amd import synth
    root = tempfile.mkdtemp(prefix="mmrec_baby_")
    synth.write_dataset(root, "baby", seed=0)
    from mmrec_amd.utils.configurator import Config
    from mmrec_amd.utils.dataloader import TrainDataLoader
    from mmrec_amd.utils.dataset import RecDataset
    from mmrec_amd.utils.utils import get_model, init_seed
    cd = dict(n_layers=3, reg_weight=1e-3, learning_rate=1e-3, gpu_id=0, use_gpu=True, data_path=root + "/", epochs=1,
              save_recommended_topk=False)
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

    def step():
        return torch.autograd.grad(model.calculate_loss(batch), params, allow_unused=True)
    result["grcn_batch"] = int(batch.shape[1])
    measure("grcn_baby", (("grcn_step", step),), result)
    shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "edge_softmax_ab.json")
    results = [one(*s) for s in shapes()]
    grcn_step(results[0])
    with open(path, "w") as f:
        json.dump(results, f, indent=1)
    print("wrote", path)
