"""The config-5 SpMM layer in ONE launch: multi-chunk rows finished by the last-arriving chunk block at every graph size
(mmrec_spmm_csr_f32 `long_tickets`), bit for bit the two-launch form (tickets withheld), launch after launch, inside a
hipGraph replay, in the LayerGCN epilogue, and after a failed launch's ticket re-zeroing."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def c5(dev):
    from mmrec_amd import hip_ops, synth
    nu, ni, eu, ei = synth.shaped_edges("c5", seed=0)
    r, c, v = synth.sym_norm_coo(eu, ei, nu, ni)
    n = nu + ni
    g = hip_ops.CsrGraph.from_coo_device(torch.from_numpy(r.astype(np.int32)).to(dev), torch.from_numpy(c.astype(np.int32)).to(dev),
                                         torch.from_numpy(v).to(dev), n, n, symmetric=True)
    X = torch.rand(n, 64, device=dev, generator=torch.Generator(device=dev).manual_seed(0)) - 0.5
    return g, X


def without_tickets(g, fn):
    tickets, g.long_tickets = g.long_tickets, None
    try:
        return fn()
    finally:
        g.long_tickets = tickets


def tickets_zero(g):
    return int(g.long_tickets.abs().sum()) == 0


def test_c5_one_launch_equals_two_launches(dev, c5):
    from mmrec_amd import hip_ops
    g, X = c5
    assert g.n_rows > (1 << 18) and g.n_chunks > g.n_long > 10_000 and g.long_tickets is not None
    Z = torch.rand(X.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(1)) - 0.5
    A0 = torch.rand(X.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(2)) - 0.5

    def run():
        Y, acc = torch.empty_like(X), torch.empty_like(X)
        hip_ops.spmm_raw(g, X, Y=Y, Z=Z, acc_in=A0, acc_out=acc, alpha=0.5, beta=2.0, acc_scale=0.25)
        return Y, acc
    ref = without_tickets(g, run)
    for _ in range(3):
        got = run()
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
        assert tickets_zero(g)


def test_c5_one_launch_in_graph_replay(dev, c5):
    from mmrec_amd import hip_ops
    g, X = c5
    Yref = torch.empty_like(X)
    without_tickets(g, lambda: hip_ops.spmm_raw(g, X, Y=Yref))
    Y = torch.empty_like(X)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        hip_ops.spmm_raw(g, X, Y=Y)
        cg = torch.cuda.CUDAGraph()
        with torch.cuda.graph(cg, stream=side):
            hip_ops.spmm_raw(g, X, Y=Y)
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(3):
        Y.fill_(float("nan"))
        cg.replay()
        torch.cuda.synchronize()
        assert torch.equal(Y, Yref)
        assert tickets_zero(g)
    del cg


def test_c5_layergcn_one_launch_equals_two_launches(dev, c5):
    from mmrec_amd import hip_ops
    g, X = c5
    a = hip_ops.layergcn_sum(g, X, 2)
    assert tickets_zero(g)
    b = without_tickets(g, lambda: hip_ops.layergcn_sum(g, X, 2))
    assert torch.equal(a, b)


def test_c5_failed_launch_rezeroes_tickets(dev, c5):
    """CsrGraph.checked(): a launch that reports an error may have left tickets counted; they are re-zeroed, and the next
    launch gives the two-launch form's bits again."""
    from mmrec_amd import _lib, hip_ops
    g, X = c5
    g.long_tickets.fill_(1)                    # what an interrupted launch could leave behind
    with pytest.raises(_lib.MMRecHipError):
        g.checked(_lib.load().mmrec_spmm_csr_f32(None, None, None, None, None, None, None, None, g.n_rows, 64, 1.0, 0.0, 1.0,
                                                  g.long_row_threshold, None, None, g.n_long, g.n_chunks, None, None, None),
                  "spmm_csr_f32")
    assert tickets_zero(g)
    Y, Yref = torch.empty_like(X), torch.empty_like(X)
    hip_ops.spmm_raw(g, X, Y=Y)
    without_tickets(g, lambda: hip_ops.spmm_raw(g, X, Y=Yref))
    assert torch.equal(Y, Yref) and tickets_zero(g)
