"""CPU: the per-edge dot products (SDDMM, ABI 16) without a GPU -- the argument checks of mmrec_edge_dot_f32 /
mmrec_edge_dot_bwd_f32 happen on the host before any launch, and `hip_ops.edge_dot` on anything the kernels do not serve
(here: CPU tensors) is the torch composition `(A[rows] * B[cols]).sum(-1)` with stock autograd, `A is B` included."""
import os

import numpy as np
import pytest
import torch

from mmrec_amd import _lib


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from mmrec_amd.build import build
        build(verbose=False)
    return _lib.load()


def test_abi_version_is_16(lib):
    assert _lib.ABI_VERSION == 16 and lib.mmrec_abi_version() == 16
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mmrec_hip.h")).read()
    assert "#define MMREC_ABI_VERSION 16" in src
    for name in ("mmrec_edge_dot_f32", "mmrec_edge_dot_bwd_f32"):
        assert name in _lib.SIGNATURES and name in src and hasattr(lib, name)


def test_argument_errors_without_gpu(lib):
    fwd, bwd = lib.mmrec_edge_dot_f32, lib.mmrec_edge_dot_bwd_f32
    # the width is checked before the pointers: 8 / 16 / 32 and the multiples of 64 up to 384, nothing else
    assert fwd(None, 10, None, 10, None, None, 5, 24, None, None) == 10002
    assert fwd(None, 10, None, 10, None, None, 5, 448, None, None) == 10002
    assert fwd(None, 10, None, 10, None, None, 5, 0, None, None) == 10002
    assert fwd(None, 10, None, 10, None, None, 5, 64, None, None) == 10001        # served width: NULL pointers
    assert fwd(None, 10, None, 10, None, None, 0, 64, None, None) == 0            # no edges: nothing to launch
    assert fwd(None, 10, None, 10, None, None, -1, 64, None, None) == 10001       # negative sizes
    assert fwd(None, -1, None, 10, None, None, 5, 64, None, None) == 10001
    assert fwd(None, 10, None, 10, None, None, 2 ** 31, 64, None, None) == 10002  # more edges than the launch indexes
    for d in (8, 16, 32, 64, 128, 192, 256, 320, 384):
        assert fwd(None, 10, None, 10, None, None, 5, d, None, None) == 10001
        assert bwd(None, None, 10, None, 10, None, None, 5, d, None, None, None) == 10001
    assert bwd(None, None, 10, None, 10, None, None, 5, 40, None, None, None) == 10002
    assert bwd(None, None, 10, None, 10, None, None, 5, 448, None, None, None) == 10002
    assert bwd(None, None, 10, None, 10, None, None, 0, 64, None, None, None) == 0
    assert bwd(None, None, 10, None, 10, None, None, 5, 64, None, None, None) == 10001
    assert bwd(None, None, 10, None, 10, None, None, 2 ** 31, 64, None, None, None) == 10002


def _tables(rng, n_a, n_b, d, ne):
    A = torch.from_numpy(rng.standard_normal((n_a, d)).astype(np.float32))
    B = torch.from_numpy(rng.standard_normal((n_b, d)).astype(np.float32))
    rows = torch.from_numpy(rng.integers(0, n_a, ne))
    cols = torch.from_numpy(rng.integers(0, n_b, ne))
    rows[1], cols[1] = rows[0], cols[0]                       # a duplicate edge
    g = torch.from_numpy(rng.standard_normal(ne).astype(np.float32))
    return A, B, rows, cols, g


def _rel(got, want):
    return float((got.double() - want).abs().max() / want.abs().max())


@pytest.mark.parametrize("d", [64, 40])
def test_cpu_tensors_take_the_torch_composition(d):
    from mmrec_amd import hip_ops
    assert hip_ops.EDGE_DOT is True
    rng = np.random.default_rng(d)
    A, B, rows, cols, g = _tables(rng, 30, 20, d, 200)
    assert not hip_ops.edge_dot_served(A, B, rows, cols)
    A.requires_grad_(), B.requires_grad_()
    out = hip_ops.edge_dot(A, B, rows, cols)
    assert out.shape == (200,) and out.dtype == torch.float32
    out.backward(g)
    A64, B64 = A.detach().double().requires_grad_(), B.detach().double().requires_grad_()
    ref = (A64[rows] * B64[cols]).sum(-1)
    ref.backward(g.double())
    assert _rel(out.detach(), ref.detach()) <= 1e-6
    assert _rel(A.grad, A64.grad) <= 1e-6 and _rel(B.grad, B64.grad) <= 1e-6


def test_cpu_fallback_with_one_table_on_both_sides():
    from mmrec_amd import hip_ops
    rng = np.random.default_rng(1)
    A, _, rows, cols, g = _tables(rng, 25, 25, 64, 300)
    A.requires_grad_()
    out = hip_ops.edge_dot(A, A, rows, cols)
    out.backward(g)
    A64 = A.detach().double().requires_grad_()
    ref = (A64[rows] * A64[cols]).sum(-1)
    ref.backward(g.double())
    assert _rel(out.detach(), ref.detach()) <= 1e-6 and _rel(A.grad, A64.grad) <= 1e-6       # both gradients, summed


def test_served_is_about_device_dtype_width_and_the_switch(monkeypatch):
    from mmrec_amd import hip_ops
    A = torch.zeros(4, 64)
    ids = torch.zeros(3, dtype=torch.int64)
    assert not hip_ops.edge_dot_served(A, A, ids, ids)                    # CPU tensors
    assert not hip_ops.edge_dot_served(None, A, ids, ids)
    for d, ok in ((8, True), (16, True), (32, True), (64, True), (384, True), (24, False), (40, False), (448, False), (0, False)):
        assert hip_ops._edge_width_served(d) == ok
    monkeypatch.setattr(hip_ops, "EDGE_DOT", False)
    assert not hip_ops.edge_dot_served(A, A, ids, ids)
