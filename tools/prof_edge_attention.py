#!/usr/bin/env python3
"""Fused edge attention (hip_ops.edge_attention, mmrec_edge_attention_f32: scores, softmax and aggregation in one kernel)
against the three ops it replaces (edge_dot -> edge_softmax -> spmm_vals, hip_ops.EDGE_ATTENTION off) in ONE process, each leg
as a hipGraph replay:

    forward             Y, alpha = edge_attention(x, x, dyn)
    forward_backward    the same + d / d x of sum(Y dY) + sum(alpha dA)   (the fused op's backward composed of the older kernels)
    grcn_step           GRCN.calculate_loss + backward at Amazon-Baby shape with `fused_attention` True against False

and the fused op's ONE-CALL backward (edge_attention(fused_backward=True), mmrec_edge_attention_bwd_f32) against its composed
backward, the forward being the fused kernel in both:

    backward            d / d x of sum(Y dY) + sum(alpha dA) alone: the forward runs once, outside the replayed graph
    grcn_step_bwd       GRCN.calculate_loss + backward with `fused_attention` on and `fused_attention_backward` True against False
                        (at Baby shape only, as grcn_step: GRCN's graph is its dataset's)

Shapes: GRCN at Amazon-Baby shape -- both directions of the synthetic Baby training interactions over the 19,445 + 7,050 nodes,
rows = the target node, d = 64 -- and a hub-heavy graph of the same size in which 32 nodes receive a third of the edges.  HIP
events around windows of replays: median / min / max over five windows after warm-up, windows of the two paths alternating.  A
leg is "slower" when its median exceeds the other path's by more than that path's own min-max spread.  Results as JSON (default
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


def measure(name, legs, result, new="fused", old="three_ops"):
    """legs: (leg, fn of the path `new`, fn of the path `old`)"""
    import numpy as np
    for leg, fused, three in legs:
        graphs = ((new, captured(fused)), (old, captured(three)))
        per = {k: [] for k, _ in graphs}
        for _ in range(WINDOWS):
            for k, graph in graphs:
                per[k].append(window(graph))
        med = {k: float(np.median(v)) for k, v in per.items()}
        spread = max(per[old]) - min(per[old])
        entry = {k: {"median_us": med[k], "min_us": min(v), "max_us": max(v)} for k, v in per.items()}
        entry["%s_minus_%s_us" % (new, old)] = med[new] - med[old]
        entry["%s_spread_us" % old] = spread
        entry["verdict"] = "SLOWER than the spread allows" if med[new] - med[old] > spread else "not slower"
        entry["faster_by_more_than_the_spread"] = bool(med[old] - med[new] > spread)
        result["legs"][leg] = entry
        print("%-10s %-17s %s %9.2f us [%.2f, %.2f]   %s %9.2f us [%.2f, %.2f]   %s" % (
            name, leg, new, med[new], min(per[new]), max(per[new]), old, med[old], min(per[old]), max(per[old]),
            entry["verdict"]), flush=True)
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
    # Without autograd, as in prof_edge_softmax.py, whose captured backward ended in a segmentation fault after such calls;
    # supposed, not shown: autograd state of `x` bound to the default stream outlived them and the backward captured on the
    # side stream then synchronised the default stream with the capture.
    with torch.no_grad():
        y_on, a_on = hip_ops.edge_attention(x, x, dyn)                # builds the long-row list outside any capture
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

    def backward_alone(fused_backward):
        held = []

        def run():
            # the forward runs once, at the first call: a warm-up call, so outside the graph (it builds both long lists), and on
            # the stream the graph is then captured on (a backward runs on its forward's stream)
            if not held:
                y, a = hip_ops.edge_attention(x, x, dyn, fused_backward=fused_backward)
                held.append((y * dY).sum() + (a * dA).sum())
            return torch.autograd.grad(held[0], x, retain_graph=True)
        return run
    g_new, g_old = backward_alone(True)()[0], backward_alone(False)()[0]
    result["max_abs_diff_grad_fused_backward"] = float((g_new - g_old).abs().max())
    assert result["max_abs_diff_grad_fused_backward"] <= 1e-4 * float(g_old.abs().max()), result
    measure(name, [("backward", backward_alone(True), backward_alone(False))], result, "fused_backward", "composed_backward")
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
    for fused, fused_bwd in ((True, False), (False, False), (True, True)):
        cd = dict(n_layers=3, reg_weight=1e-3, learning_rate=1e-3, gpu_id=0, use_gpu=True, data_path=root + "/", epochs=1,
                  save_recommended_topk=False, fused_attention=fused, fused_attention_backward=fused_bwd)
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
        steps[fused, fused_bwd] = (lambda model=model, batch=batch, params=params:
                                   torch.autograd.grad(model.calculate_loss(batch), params, allow_unused=True))
        result["grcn_batch"] = int(batch.shape[1])
    measure("grcn_baby", [("grcn_step", steps[True, False], steps[False, False])], result)
    measure("grcn_baby", [("grcn_step_bwd", steps[True, True], steps[True, False])], result, "fused_backward", "composed_backward")
    shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "edge_attention_ab.json")
    name, n, rows_h, cols_h = shapes()[0]
    results = [one(name, n, rows_h, cols_h), one("hub_heavy", n, *hub_heavy(n, rows_h.size))]
    grcn_step(results[0])
    with open(path, "w") as f:
        json.dump(results, f, indent=1)
    print("wrote", path)
