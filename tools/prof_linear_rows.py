#!/usr/bin/env python3
"""Forward + backward of the projection of a batch's feature rows as a hipGraph replay, the two forms in ONE process:

    two-step   hip_ops.linear(table.index_select(0, ids), W, b)     (LazyRowEmbedding.rows: the [n, F] copy is written, then read twice)
    gathered   hip_ops.linear_rows(table, ids, W, b)                (LazyRowEmbedding.project_rows: the kernels read the table's rows)

through the row-lazy table, as FREEDOM / BM3 run them under `lazy_feature_adam` (the rows' gradient stays compact: no dense
table gradient on either side).  Shapes (n_table, F, n): the tables of Amazon-Baby / Sports / Clothing (text) and config 5 with
a batch of 2 x 2048 rows.  Median of five replay windows with min and max, windows of the two forms alternating.

    python tools/prof_linear_rows.py                      # the four shapes
    python tools/prof_linear_rows.py n_table F n          # one shape
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((7050, 4096, 4096), (18357, 4096, 4096), (23033, 384, 4096), (500000, 4096, 4096))
WINDOWS, REPLAYS = 5, 200


def captured(fb):
    import torch
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(5):
            fb()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            fb()
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(10):
        graph.replay()
    return graph


def window(graph):
    import torch
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(REPLAYS):
        graph.replay()
    e.record()
    torch.cuda.synchronize()
    return a.elapsed_time(e) / REPLAYS * 1e3


def one(n_table, F, n):
    import numpy as np
    import torch
    from mmrec_amd import hip_ops
    from mmrec_amd.common.lazy_rows import LazyRowEmbedding
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    emb = LazyRowEmbedding.from_pretrained(torch.rand(n_table, F, device=dev, generator=gen), freeze=False)
    ids = torch.randint(0, n_table, (n,), device=dev, generator=gen)
    W = (torch.rand(64, F, device=dev, generator=gen) - 0.5).requires_grad_()
    b = torch.zeros(64, device=dev, requires_grad=True)
    G = torch.rand(n, 64, device=dev, generator=gen) - 0.5
    assert hip_ops.linear_rows_served(emb.weight, ids, W)

    def two_step():
        W.grad = b.grad = None
        emb._pending = []
        hip_ops.linear(emb.rows(ids), W, b).backward(G)

    def gathered():
        W.grad = b.grad = None
        emb._pending = []
        emb.project_rows(ids, W, b).backward(G)
    forms = (("two-step", captured(two_step)), ("gathered", captured(gathered)))
    per = {name: [] for name, _ in forms}
    for _ in range(WINDOWS):
        for name, graph in forms:
            per[name].append(window(graph))
    for name, _ in forms:
        t = per[name]
        print("n_table=%d F=%d n=%d %-8s fwd+bwd replay: median %.2f us  min %.2f  max %.2f" %
              (n_table, F, n, name, float(np.median(t)), min(t), max(t)), flush=True)
    a, g = per["two-step"], per["gathered"]
    diff, spread = float(np.median(g)) - float(np.median(a)), max(a) - min(a)
    print("n_table=%d F=%d n=%d gathered - two-step = %+.2f us (%+.1f %%); spread of the two-step windows %.2f us -> %s" %
          (n_table, F, n, diff, 100.0 * diff / float(np.median(a)), spread,
           "SLOWER than the spread allows" if diff > spread else "not slower"), flush=True)
    del emb, forms
    torch.cuda.empty_cache()


if __name__ == "__main__":
    if len(sys.argv) == 4:
        one(*(int(a) for a in sys.argv[1:4]))
    else:
        for shape in SHAPES:
            one(*shape)
