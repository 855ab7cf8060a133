#!/usr/bin/env python3
"""Golden facts about the reference's API surface -> tests/golden/reference_api.json + reference_knn_helpers.npz
(tests/test_host_logic.py reads them; the reference itself is not needed there).

    python tests/golden/make_golden_reference_api.py      # build container only (needs the reference checkout)

reference_api.json
  models           the names of the reference's `src/models/*.py`
  config_files     for each `configs/{model,dataset}/*.yaml` and `configs/overall.yaml`: key -> digest of its parsed value
  final_configs    for each model, with and without the Mirror-Gradient file: key -> digest of every value of the merged
                   `Config(name, "sports", overrides, mg).final_config_dict` (device as its string), and whether a missing
                   key reads None
Values are kept as digests (tests/_env.py: config_digest), not copied: equal digests <=> equal values.
reference_knn_helpers.npz
  the seeded inputs and the outputs of the reference's utils/utils.py kNN-graph helpers on them."""
import importlib.util
import json
import os
import sys
import tempfile

import numpy as np
import torch
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden as mg  # noqa: E402
from tests._env import config_digest  # noqa: E402

MODEL_OVERRIDES = {"gpu_id": 0, "use_gpu": False, "learning_rate": 0.123, "brand_new_key": [1, 2]}


def load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def digests(d):
    return {str(k): config_digest(v) for k, v in d.items()}


def api_facts():
    out = {"models": sorted(f[:-3] for f in os.listdir(os.path.join(mg.REF_SRC, "models")) if f.endswith(".py")),
           "config_files": {}, "final_configs": {}}
    for sub in ("model", "dataset"):
        for f in sorted(os.listdir(os.path.join(mg.REF_SRC, "configs", sub))):
            with open(os.path.join(mg.REF_SRC, "configs", sub, f)) as fh:
                out["config_files"][sub + "/" + f] = digests(yaml.safe_load(fh))
    with open(os.path.join(mg.REF_SRC, "configs", "overall.yaml")) as fh:
        out["config_files"]["overall.yaml"] = digests(yaml.safe_load(fh))
    # the reference resolves ./configs from the working directory: a scratch directory whose `configs` links to its own
    tmp = tempfile.mkdtemp(prefix="mmrec_golden_api_")
    os.symlink(os.path.join(mg.REF_SRC, "configs"), os.path.join(tmp, "configs"))
    os.chdir(tmp)
    ref = load("_ref_configurator", os.path.join(mg.REF_SRC, "utils", "configurator.py"))
    for name in sorted(f[:-5] for f in os.listdir(os.path.join(mg.REF_SRC, "configs", "model"))):
        for m in (False, True):
            a = ref.Config(name, "sports", dict(MODEL_OVERRIDES), m)
            d = dict(a.final_config_dict)
            d["device"] = str(d["device"])
            out["final_configs"]["%s/mg=%d" % (name, m)] = {"values": digests(d),
                                                            "missing_key_is_none": a["no_such_key"] is None}
    return out


def knn_helper_vectors():
    sys.path.insert(0, os.path.join(HERE, "_shims"))         # torch_scatter, imported lazily by the sparse helper
    ref = load("_ref_utils_utils", os.path.join(mg.REF_SRC, "utils", "utils.py"))
    g = torch.Generator().manual_seed(3)
    v = {}
    feats = torch.randn(40, 12, generator=g)
    v["feats"] = feats.clone()
    sim = ref.build_sim(feats)
    v["sim"] = sim
    v["neighbourhood_5"] = ref.build_knn_neighbourhood(sim, 5)
    adj = torch.relu(torch.randn(30, 30, generator=g))
    adj[4] = 0.0                                               # an empty row: 0, not inf / nan
    v["adj"] = adj.clone()
    v["normalized_laplacian"] = ref.compute_normalized_laplacian(adj)
    for norm in ("sym", "rw", "none"):
        v["dense_laplacian_" + norm] = ref.get_dense_laplacian(adj, norm)
        v["knn_dense_" + norm] = ref.build_knn_normalized_graph(adj, 4, False, norm)
        b = ref.build_knn_normalized_graph(adj, 4, True, norm)
        v["knn_sparse_indices_" + norm], v["knn_sparse_values_" + norm] = b._indices(), b._values()
        ei = torch.randint(0, 30, (2, 200), generator=g)
        w = torch.rand(200, generator=g)
        v["edge_index_" + norm], v["edge_weight_" + norm] = ei.clone(), w.clone()
        i2, w2 = ref.get_sparse_laplacian(ei, w.clone(), 30, norm)
        v["sparse_laplacian_indices_" + norm], v["sparse_laplacian_weights_" + norm] = i2, w2
    return {k: t.numpy() for k, t in v.items()}


def main():
    knn = knn_helper_vectors()
    facts = api_facts()
    with open(os.path.join(HERE, "reference_api.json"), "w") as f:
        json.dump(facts, f, indent=1, sort_keys=True)
        f.write("\n")
    np.savez_compressed(os.path.join(HERE, "reference_knn_helpers.npz"), **knn)
    print("wrote reference_api.json (%d models, %d config files, %d final configs), reference_knn_helpers.npz (%d arrays)"
          % (len(facts["models"]), len(facts["config_files"]), len(facts["final_configs"]), len(knn)))


if __name__ == "__main__":
    main()
