"""CPU: the segment softmax over a graph's edges (mmrec_segment_softmax_*, hip_ops.edge_softmax) without a GPU -- the three
exports, the argument checks that happen on the host before any launch, the torch composition that everything the kernels do
not serve (here: CPU tensors) still takes, bit for bit what GRCN ran before, and the long-row list the wrapper hands to the
kernel."""
import os
import types

import numpy as np
import pytest
import torch

from mmrec_amd import _lib

EXPORTS = ("mmrec_segment_softmax_group_max", "mmrec_segment_softmax_f32", "mmrec_segment_softmax_bwd_f32")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from mmrec_amd.build import build
        build(verbose=False)
    return _lib.load()


def test_exports_in_header_signatures_and_library(lib):
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mmrec_hip.h")).read()
    for name in EXPORTS:
        assert name in _lib.SIGNATURES and name in src and hasattr(lib, name), name
    assert "#define MMREC_ABI_VERSION 16" in src and lib.mmrec_abi_version() == 16       # additive: the version stays
    assert lib.mmrec_segment_softmax_group_max() >= 64


def test_argument_errors_without_gpu(lib):
    fwd, bwd = lib.mmrec_segment_softmax_f32, lib.mmrec_segment_softmax_bwd_f32
    one = (np.zeros(4, np.int32)).ctypes.data_as(_lib._P)            # any non-NULL pointer: nothing is read before the checks end
    # negative sizes
    assert fwd(None, -1, None, None, 0, None, 5, 1e-16, None, None) == 10001
    assert fwd(None, 3, None, None, 0, None, -5, 1e-16, None, None) == 10001
    assert fwd(None, 3, None, None, -1, None, 5, 1e-16, None, None) == 10001
    assert bwd(None, -1, None, None, 0, None, None, 5, None, None) == 10001
    assert bwd(None, 3, None, None, 0, None, None, -5, None, None) == 10001
    assert bwd(None, 3, None, None, -1, None, None, 5, None, None) == 10001
    # nothing to do: 0 with NULL pointers
    assert fwd(None, 3, None, None, 0, None, 0, 1e-16, None, None) == 0
    assert fwd(None, 0, None, None, 0, None, 5, 1e-16, None, None) == 0
    assert bwd(None, 3, None, None, 0, None, None, 0, None, None) == 0
    assert bwd(None, 0, None, None, 0, None, None, 5, None, None) == 0
    # more edges than the launch indexes
    assert fwd(None, 3, None, None, 0, None, 2 ** 31, 1e-16, None, None) == 10002
    assert bwd(None, 3, None, None, 0, None, None, 2 ** 31, None, None) == 10002
    # NULL rowptr / score / out (alpha / g / ds)
    assert fwd(None, 3, None, None, 0, None, 5, 1e-16, None, None) == 10001
    assert fwd(None, 3, None, None, 0, one, 5, 1e-16, one, None) == 10001
    assert fwd(one, 3, None, None, 0, None, 5, 1e-16, one, None) == 10001
    assert fwd(one, 3, None, None, 0, one, 5, 1e-16, None, None) == 10001
    assert bwd(None, 3, None, None, 0, one, one, 5, one, None) == 10001
    assert bwd(one, 3, None, None, 0, None, one, 5, one, None) == 10001
    assert bwd(one, 3, None, None, 0, one, None, 5, one, None) == 10001
    assert bwd(one, 3, None, None, 0, one, one, 5, None, None) == 10001
    # a long-row count without a list
    assert fwd(one, 3, None, None, 2, one, 5, 1e-16, one, None) == 10001
    assert bwd(one, 3, None, None, 2, one, one, 5, one, None) == 10001


def _graph(rng, n_rows, n_cols, ne):
    rows = torch.from_numpy(rng.integers(0, n_rows, ne))
    cols = torch.from_numpy(rng.integers(0, n_cols, ne))
    return types.SimpleNamespace(rows=rows, cols=cols, n_rows=n_rows, n_cols=n_cols)


@pytest.mark.parametrize("by", ["row", "col"])
def test_cpu_tensors_take_the_composition_bit_for_bit(by):
    from mmrec_amd import hip_ops
    from mmrec_amd.models import grcn
    assert hip_ops.EDGE_SOFTMAX is True
    rng = np.random.default_rng(5)
    dyn = _graph(rng, 40, 25, 600)
    index, n = (dyn.rows, 40) if by == "row" else (dyn.cols, 25)
    score = torch.from_numpy((rng.standard_normal(600) * 5).astype(np.float32)).requires_grad_()
    g = torch.from_numpy(rng.standard_normal(600).astype(np.float32))
    assert not hip_ops.edge_softmax_served(score, dyn)
    out = hip_ops.edge_softmax(score, dyn, by=by)
    assert out.shape == (600,) and out.dtype == torch.float32
    assert torch.equal(out.detach(), grcn.segment_softmax(score.detach(), index, n))
    out.backward(g)
    s64 = score.detach().double().requires_grad_()
    ref = hip_ops.segment_softmax_torch(s64, index, n)
    ref.backward(g.double())
    assert float((out.detach().double() - ref.detach()).abs().max()) <= 1e-6
    assert float((score.grad.double() - s64.grad).abs().max()) <= 1e-6 * float(s64.grad.abs().max())
    # the backward formula of the kernel IS this derivative: ds = alpha (g - sum alpha g) over the segment (float64)
    a, g64 = ref.detach(), g.double()
    dot = torch.zeros(n, dtype=torch.float64).index_add_(0, index, a * g64)
    assert float((a * (g64 - dot[index]) - s64.grad).abs().max()) <= 1e-15
    with pytest.raises(ValueError):
        hip_ops.edge_softmax(score, dyn, by="edge")


def test_non_finite_rule_of_the_composition():
    """the rule the kernel copies: [0, 1 | -inf, -inf | inf, 2 | nan, 3 | 1, -200]"""
    from mmrec_amd import hip_ops
    inf, nan = float("inf"), float("nan")
    s = torch.tensor([0, 1, -inf, -inf, inf, 2, nan, 3, 1, -200], dtype=torch.float32)
    dyn = types.SimpleNamespace(rows=torch.arange(10) // 2, cols=torch.arange(10), n_rows=5, n_cols=10)
    out = hip_ops.edge_softmax(s, dyn).numpy()
    assert np.isfinite(out[:2]).all() and abs(out[:2].sum() - 1) < 1e-6
    assert np.isnan(out[2:8]).all()
    assert out[8] == 1.0 and out[9] == 0.0


def test_served_is_about_device_dtype_shape_and_the_switch(monkeypatch):
    from mmrec_amd import hip_ops
    rng = np.random.default_rng(1)
    dyn = _graph(rng, 6, 6, 12)

    class OnDevice(torch.Tensor):                                    # a stand-in that says it lives on the device
        is_cuda = True
    for t, ok in ((torch.zeros(12), True), (torch.zeros(12, dtype=torch.float64), False), (torch.zeros(11), False),
                  (torch.zeros(12, 1), False), (torch.zeros(24)[::2], False)):
        assert not hip_ops.edge_softmax_served(t, dyn)                # CPU tensors: never
        assert hip_ops.edge_softmax_served(t.as_subclass(OnDevice), dyn) == ok, (t.shape, t.dtype)
    assert not hip_ops.edge_softmax_served(None, dyn)
    monkeypatch.setattr(hip_ops, "EDGE_SOFTMAX", False)
    assert not hip_ops.edge_softmax_served(torch.zeros(12).as_subclass(OnDevice), dyn)


def test_long_row_list_is_the_rows_beyond_the_group_maximum(lib):
    from mmrec_amd import hip_ops
    gm = hip_ops.segment_softmax_group_max()
    assert gm == lib.mmrec_segment_softmax_group_max()
    lens = [0, 1, gm, gm + 1, 5000]
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    lr = hip_ops.segment_long_rows(rp)
    assert lr.dtype == np.int32 and lr.tolist() == [3, 4]
    assert hip_ops.segment_long_rows(np.array([0, 0, 1, 1 + gm], np.int32)).size == 0
    assert hip_ops.segment_long_rows(np.zeros(1, np.int32)).size == 0              # no rows at all
