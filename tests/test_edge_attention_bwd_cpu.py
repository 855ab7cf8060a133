"""CPU: the fused edge attention backward (mmrec_edge_attention_bwd_f32, hip_ops.edge_attention(fused_backward=True), GRCN's
`fused_attention_backward`) as far as it goes without a device: the entry point's host argument checks in their stated order,
the keyword on CPU tensors (not served: the three-op composition, bit for bit), and the config key's default."""
import os

import numpy as np
import pytest
import torch

import tests.test_models_gpu as G
from mmrec_amd import _lib
from tests._cpu_ops import cpu_ops  # noqa: F401  (fixture)
from tests.test_edge_attention_cpu import _graph, _three_ops, deterministic_torch  # noqa: F401  (fixture)

BAD_ARG, UNSUPPORTED = 10001, 10002


def _entry():
    if not os.path.exists(_lib.LIB_PATH):
        from mmrec_amd.build import build
        build(verbose=False)
    return _lib.load().mmrec_edge_attention_bwd_f32


def test_argument_errors():
    """(no launch: runs without a GPU) the stated codes, in the stated order"""
    f = _entry()
    one = np.zeros(4, np.int32).ctypes.data_as(_lib._P)
    two = np.zeros(4, np.int32).ctypes.data_as(_lib._P)

    def call(rowptr=one, n_rows=3, colidx=one, long_rows=None, n_long=0, rowptr_t=one, rowidx_t=one, long_cols=None, n_long_t=0,
             Q=one, n_q=3, KV=one, n_kv=5, Y=one, alpha=one, dY=one, dAlpha=one, d=64, ne=5, ds=one, dQ=one, dKV=two, base=None):
        return f(rowptr, n_rows, colidx, None, long_rows, n_long, rowptr_t, rowidx_t, None, long_cols, n_long_t, Q, n_q, KV, n_kv,
                 Y, alpha, dY, dAlpha, d, ne, ds, dQ, dKV, base, None)
    none = dict(rowptr=None, colidx=None, rowptr_t=None, rowidx_t=None, Q=None, KV=None, Y=None, alpha=None, dY=None, dAlpha=None,
                ds=None, dQ=None, dKV=None)
    for d in (0, 8, 32, 63, 65, 128):
        assert call(d=d) == UNSUPPORTED                               # d == 64 only ...
        assert call(d=d, n_rows=-1, **none) == UNSUPPORTED            # ... and before everything else
    for kw in ({"n_rows": -1}, {"ne": -1}, {"n_long": -1}, {"n_long_t": -1}, {"n_q": -1}, {"n_kv": -1}):
        assert call(**kw) == BAD_ARG
        assert call(**dict(kw, **none)) == BAD_ARG
    assert call(n_rows=0, **none) == 0 and call(ne=0, **none) == 0    # nothing to launch: pointers may be NULL
    assert call(n_rows=0, n_kv=2 ** 31) == 0                          # ... before the size limits
    assert call(ne=2 ** 31) == UNSUPPORTED and call(n_kv=2 ** 31) == UNSUPPORTED
    assert call(ne=2 ** 31, **none) == UNSUPPORTED and call(ne=2 ** 31, n_q=2) == UNSUPPORTED
    assert call(n_q=2) == BAD_ARG                                     # fewer rows of Q than rows
    for k in ("rowptr", "colidx", "KV", "alpha", "ds"):               # needed by every call
        assert call(**{k: None}) == BAD_ARG, k
    assert call(dY=None, dAlpha=None) == BAD_ARG                      # no gradient arrives
    assert call(Y=None) == BAD_ARG                                    # dY without the forward's Y
    assert call(dQ=None, dKV=None) == BAD_ARG                         # nothing asked for
    for k in ("rowptr_t", "rowidx_t", "Q"):                           # the column side, when dKV is wanted
        assert call(**{k: None}) == BAD_ARG, k
    assert call(base=two) == BAD_ARG                                  # the base must not be dKV
    assert call(n_long=2) == BAD_ARG and call(n_long_t=2) == BAD_ARG  # a long count without its list
    assert call(n_long=2, KV=None) == BAD_ARG


@pytest.mark.parametrize("same", [False, True], ids=["distinct", "Q_is_KV"])
def test_keyword_on_cpu_tensors_is_the_three_op_composition(cpu_ops, deterministic_torch, same):  # noqa: F811
    """not served on the CPU: `fused_backward` is ignored -- values and gradients are those of edge_dot -> edge_softmax ->
    spmm_vals, bit for bit, as without the keyword"""
    from mmrec_amd import hip_ops
    rng = np.random.default_rng(12)
    n = 40
    dyn = _graph(rng, n, n, 700)
    dY = torch.from_numpy(rng.standard_normal((n, 64)).astype(np.float32))
    dA = torch.from_numpy(rng.standard_normal(700).astype(np.float32))
    runs = []
    for fn in (lambda Q, KV, d: hip_ops.edge_attention(Q, KV, d, fused_backward=True),
               lambda Q, KV, d: hip_ops.edge_attention(Q, KV, d, 1e-16, False),
               lambda Q, KV, d: _three_ops(hip_ops, Q, KV, d)):
        Q = torch.from_numpy((np.random.default_rng(2).standard_normal((n, 64)) * 0.5).astype(np.float32)).requires_grad_()
        KV = Q if same else torch.from_numpy((np.random.default_rng(3).standard_normal((n, 64)) * 0.5).astype(np.float32)).requires_grad_()
        assert not hip_ops.edge_attention_served(Q, KV, dyn)
        Y, alpha = fn(Q, KV, dyn)
        ((Y * dY).sum() + (alpha * dA).sum()).backward()
        runs.append((Y.detach(), alpha.detach(), Q.grad, KV.grad))
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert torch.equal(a, b)
    assert float(runs[0][2].abs().max()) > 0


def test_switch_and_keyword_defaults():
    import inspect
    from mmrec_amd import hip_ops
    from mmrec_amd.models.grcn import CGCN
    assert hip_ops.EDGE_ATTENTION_BWD is True
    assert inspect.signature(hip_ops.edge_attention).parameters["fused_backward"].default is False
    feats = torch.rand(5, 8)
    assert CGCN(feats, 3, 64, 1).fused_attention_backward is False
    assert CGCN(feats, 3, 64, 1, True).fused_attention_backward is False
    assert CGCN(feats, 3, 64, 1, True, True).fused_attention_backward is True


def test_grcn_key_absent_is_off_and_on_the_cpu_changes_nothing(tmp_path, golden, cpu_ops, deterministic_torch, monkeypatch):  # noqa: F811
    """GRCN on the tiny golden dataset: with the key absent `CGCN.fused_attention_backward` is False; the key reaches
    `hip_ops.edge_attention` only together with `fused_attention`; on the CPU (nothing served) loss and gradients are the same bits"""
    from mmrec_amd import hip_ops
    monkeypatch.setattr(G, "USE_GPU", False)
    asked = []
    real = hip_ops.edge_attention
    monkeypatch.setattr(hip_ops, "edge_attention", lambda *a, **k: asked.append(k.get("fused_backward")) or real(*a, **k))
    out = []
    for i, extra in enumerate(({}, {"fused_attention": True}, {"fused_attention_backward": True},
                               {"fused_attention": True, "fused_attention_backward": True})):
        config, train_data, _, model = G.build(tmp_path / str(i), golden, "GRCN",
                                               dict({"reg_weight": 1e-3, "learning_rate": 1e-3, "n_layers": 3}, **extra))
        want = bool(extra.get("fused_attention_backward"))
        assert model.v_gcn.fused_attention_backward is want and model.t_gcn.fused_attention_backward is want
        batch = next(iter(train_data)).clone() if i == 0 else batch
        model.train()
        model.pre_epoch_processing()
        torch.manual_seed(77)
        loss = model.calculate_loss(batch.clone())
        loss.backward()
        out.append((loss.detach(), {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}))
    assert asked == [False, False, True, True]                        # asked by the two runs with `fused_attention` only
    for loss, g in out[1:]:
        assert torch.equal(loss, out[0][0]) and set(g) == set(out[0][1])
        for n in g:
            assert torch.equal(g[n], out[0][1][n]), n
