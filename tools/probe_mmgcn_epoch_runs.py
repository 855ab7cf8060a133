#!/usr/bin/env python3
"""MMGCN's epoch on the tiny golden dataset (tests/golden/tiny.npz, the setup of
tests/test_models_gpu.py::test_graphed_train_step_equals_eager[MMGCN]) run several times in ONE process, eagerly (E) and with the
step replayed as a hipGraph (G): after every run, the largest parameter difference against every earlier run and the parameter
that holds it, and whether the graphed step was really captured.  Shows which runs agree with which: in the default mode the
epoch has two outcomes that the BPR scatter's atomics choose between, whatever E / G and `fused_layers` are; with
`hip_deterministic` every run has the same bits (profiles/gcn_layer_fuzz.log, last part).

    python tools/probe_mmgcn_epoch_runs.py [SEQUENCE, default EEGEGGE] [on|off: fused_layers] [det: hip_deterministic]
"""
import os
import pathlib
import shutil
import sys
import tempfile

import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.test_models_gpu import build  # noqa: E402
from mmrec_amd.common.trainer import Trainer  # noqa: E402

golden = dict(np.load(os.path.join(ROOT, "tests", "golden", "tiny.npz"), allow_pickle=False))
seq = sys.argv[1] if len(sys.argv) > 1 else "EEGEGGE"
fused = len(sys.argv) > 2 and sys.argv[2] == "on"
runs = []
for i, kind in enumerate(seq):
    graphed = kind == "G"
    tmp = pathlib.Path(tempfile.mkdtemp())
    extra = {"reg_weight": 1e-3, "learning_rate": 1e-3, "hip_graph_step": graphed}
    if fused:
        extra["fused_layers"] = True
    if len(sys.argv) > 3 and sys.argv[3] == "det":
        extra["hip_deterministic"] = True
    config, train_data, _, model = build(tmp, golden, "MMGCN", extra)
    config["hip_graph_step"] = graphed
    torch.manual_seed(123)
    trainer = Trainer(config, model)
    model.pre_epoch_processing()
    total, _ = trainer._train_epoch(train_data, 0)
    torch.cuda.synchronize()
    names = [k for k, _ in model.named_parameters()]
    runs.append((kind, total, [p.detach().cpu().numpy().copy() for p in model.parameters()]))
    line = []
    for j, (k2, t2, p2) in enumerate(runs[:-1]):
        d = [float(np.abs(a - b).max()) for a, b in zip(p2, runs[-1][2])]
        w = int(np.argmax(d))
        line.append("%s%d %.1e(%s)" % (k2, j, max(d), names[w] if max(d) > 2e-5 else "-"))
    step = trainer._graphed_step(model.calculate_loss)
    line.append("captured=%s" % (None if step is None else (step.graph is not None and not step.failed)))
    print("run %d %s fused=%s loss %.9g | vs %s" % (i, kind, fused, total, "  ".join(line)), flush=True)
    del trainer, model, train_data
    shutil.rmtree(tmp, ignore_errors=True)
