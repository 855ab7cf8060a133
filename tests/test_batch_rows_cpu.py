"""CPU: the cases of tests/test_batch_rows_fuzz_gpu.py (drawn here, the same ones) through the torch-CPU stand-ins of
tests/_cpu_ops.py -- the body the GPU box runs and its float64 references are known to be sound, a correct fp32
implementation stays within the bound on every case and exact mode is exact -- and the checker against planted errors.

The stand-ins have one path each: the path switches change the case's data only (the item-item row beyond ROWS_MAX_CHUNKS),
nothing is asserted about paths, and N comes from sequential chain lengths (`cpu_depths`: a row's or a column's whole length,
so the hub cases' N is above the 1024 the device paths are held to)."""
import numpy as np
import pytest
import torch

from tests._cpu_ops import cpu_ops  # noqa: F401  (fixture)
from tests.test_batch_rows_fuzz_gpu import (CASES, LAYERGCN_CASES, accept, case, cpu_depths, describe, gpu_depths, reference,
                                            rounded, run_case, run_layergcn)
from tests.test_batch_rows_fuzz_gpu import test_cases_span_every_axis  # noqa: F401  (collected here as well)
from tests.test_spmm_fuzz_gpu import gamma


@pytest.mark.parametrize("k", range(CASES))
def test_cases_on_the_cpu_stand_ins(cpu_ops, k):  # noqa: F811
    from mmrec_amd import hip_ops
    c = case(k)
    got = run_case(c, hip_ops, torch.device("cpu"), False)
    print(describe(c, accept(c, got, cpu_depths(c))))


@pytest.mark.parametrize("storage,grads,L", LAYERGCN_CASES[::3])
def test_layergcn_sum_parts_on_the_cpu_stand_in(cpu_ops, storage, grads, L):  # noqa: F811
    from mmrec_amd import hip_ops
    run_layergcn(hip_ops, lambda a: torch.from_numpy(np.ascontiguousarray(a)), storage, grads, L)


def _find(cond):
    for k in range(CASES):
        c = case(k)
        if cond(c):
            return c
    raise AssertionError("no such case")


def _rejected(c, got):
    with pytest.raises(AssertionError):
        accept(c, got, gpu_depths(c))


def test_checker_rejects_planted_errors():
    """each error is planted into a correct fp32 result -- the float64 reference rounded to fp32 -- of a case that can show it,
    and checked as the GPU fuzz checks (the device path's N)"""
    rows_op = lambda c: c.op in ("then", "parts_rows")      # noqa: E731
    # a duplicated listed row counted once in the backward
    c = _find(lambda c: rows_op(c) and c.list == "dup_users" and c.grads in ("both", "one_buffer", "noncontig"))
    good = rounded(reference(c))
    accept(c, good, gpu_depths(c))
    _rejected(c, {**good, **{k: v for k, v in rounded(reference(c, dedup=True)).items() if k in ("dU", "dI")}})
    # A used for A^T on a directed graph; one s G term of the recurrence dropped; s = 1 / L
    c = _find(lambda c: rows_op(c) and not c.symmetric and c.L >= 2 and c.B > 1)
    good = rounded(reference(c))
    accept(c, good, gpu_depths(c))
    _rejected(c, rounded(reference(c, no_transpose=True)))
    for term in range(c.L + 1):
        _rejected(c, rounded(reference(c, drop=term)))
    bad = rounded(reference(c, s=1.0 / c.L))
    _rejected(c, {**good, "dU": bad["dU"], "dI": bad["dI"]})
    _rejected(c, {**bad, "dU": good["dU"], "dI": good["dI"]})
    # ... in exact mode too (L = 1, every plan)
    c = _find(lambda c: c.op == "then" and c.exact and c.L == 1 and not c.symmetric and c.plan == "multi" and c.B > 1)
    good = rounded(reference(c))
    accept(c, good, gpu_depths(c))
    _rejected(c, rounded(reference(c, no_transpose=True)))
    _rejected(c, rounded(reference(c, drop=0)))
    _rejected(c, rounded(reference(c, s=1.0)))
    # the item-item push omitted; the user / item split shifted by one row
    for exact in (True, False):
        c = _find(lambda c: c.op == "then" and c.exact == exact and c.B > 1 and c.grads != "user_only")
        good = rounded(reference(c))
        accept(c, good, gpu_depths(c))
        _rejected(c, rounded(reference(c, no_item_push=True)))
        _rejected(c, rounded(reference(c, shift=True)))
        wrong = np.concatenate([good["dU"], good["dI"]])
        _rejected(c, {**good, "dU": wrong[1:c.nu + 1], "dI": np.concatenate([wrong[c.nu + 1:], wrong[:1]])})
    # a 1e-4 relative error in one element of a hub row
    c = _find(lambda c: rows_op(c) and not c.exact and c.positive and c.plan == "multi" and c.B >= 16 and c.L >= 2)
    ref = reference(c)
    good = rounded(ref)
    accept(c, good, gpu_depths(c))
    name = "ia" if c.op == "then" else "at"
    hub = max(c.hubs, key=c.hubs.get)
    at = int(np.flatnonzero(c.item_rows == hub)[0]) + (c.B if name == "at" else 0)
    r, mag = ref[name]
    col = int(np.argmax(np.abs(r[at]) / mag[at]))
    assert abs(r[at, col]) / mag[at, col] > 0.99 and gamma(gpu_depths(c)[name]) < 6.2e-5      # positive case: no cancellation
    bad = good[name].copy()
    bad[at, col] = np.float32(r[at, col] * (1 + 1e-4))
    _rejected(c, {**good, name: bad})
    # a non-zero gradient row for an id outside an empty batch
    c = _find(lambda c: rows_op(c) and c.list == "empty_batch")
    good = rounded(reference(c))
    accept(c, good, gpu_depths(c))
    for name in ("dU", "dI"):
        bad = good[name].copy()
        bad[7, 3] = 1e-30
        _rejected(c, {**good, name: bad})
