"""CPU: the C-ABI library loads and exports exactly what include/mmrec_hip.h declares; host-only
entry points (plan helpers, workspace sizes) behave.  No GPU compute is called here."""
import ctypes
import os
import re

import numpy as np
import pytest

from mmrec_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(ROOT, "include", "mmrec_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(mmrec_[a-z0-9_]+)\s*\(", src)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from mmrec_amd.build import build
        build(verbose=False)
    return _lib.load()


def test_header_symbols_exported_and_typed(lib):
    names = _declared()
    assert len(names) >= 20
    for n in names:
        assert hasattr(lib, n), "library does not export %s" % n
        assert n in _lib.SIGNATURES, "ctypes binding lacks %s" % n
    assert sorted(_lib.SIGNATURES) == names
    assert lib.mmrec_abi_version() == _lib.ABI_VERSION
    assert lib.mmrec_error_string(0) == b"ok"
    assert b"bad argument" in lib.mmrec_error_string(10001)


def test_row_group_ops_share_one_threshold(lib):
    """one long-row list per CSR serves the segment softmax, the edge attention and the neighbour max"""
    assert (lib.mmrec_segment_softmax_group_max() == lib.mmrec_edge_attention_group_max()
            == lib.mmrec_neighbor_max_group_max())


def test_every_included_header_is_a_build_dependency():
    """an edit of any header a source includes must recompile: build()'s dependency set holds them all"""
    from mmrec_amd import build
    deps = {os.path.basename(h) for h in build.header_deps()}
    csrc = os.path.join(ROOT, "mmrec_amd", "csrc")
    included = set()
    for name in os.listdir(csrc):
        if name.endswith((".hip", ".h")):
            included |= {os.path.basename(h) for h in re.findall(r'#include\s+"([^"]+\.h)"', open(os.path.join(csrc, name)).read())}
    assert "common.h" in included and "mmrec_hip.h" in included
    assert included <= deps, "not a build dependency: %s" % sorted(included - deps)
    assert all(os.path.exists(h) for h in build.header_deps())


def test_missing_library_fails_loudly(monkeypatch):
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", "/nonexistent/libmmrec_hip.so")
    with pytest.raises(_lib.MMRecHipError):
        _lib.load()


def test_cpu_tensor_is_rejected():
    import torch
    from mmrec_amd import hip_ops
    with pytest.raises(_lib.MMRecHipError):
        hip_ops.gather_sqnorm(torch.zeros(4, 64), torch.zeros(2, dtype=torch.int64))


def test_spmm_plan_host(lib):
    deg = np.array([0, 3, 300, 5000, 256, 257, 2048 + 1], dtype=np.int64)
    rp = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    nl, nc = ctypes.c_int32(), ctypes.c_int32()
    assert lib.mmrec_spmm_plan_count(rp.ctypes.data_as(ctypes.c_void_p), len(deg), 256,
                                     ctypes.byref(nl), ctypes.byref(nc)) == 0
    assert nl.value == 4 and nc.value == 1 + 10 + 1 + 5   # ceil(deg / 512)
    lr = np.empty(nl.value, np.int32)
    cp = np.empty(nl.value + 1, np.int32)
    assert lib.mmrec_spmm_plan_fill(rp.ctypes.data_as(ctypes.c_void_p), len(deg), 256,
                                    lr.ctypes.data_as(ctypes.c_void_p),
                                    cp.ctypes.data_as(ctypes.c_void_p)) == 0
    assert lr.tolist() == [2, 3, 5, 6] and cp.tolist() == [0, 1, 11, 12, 17]
    assert lib.mmrec_spmm_plan_count(None, 3, 256, ctypes.byref(nl), ctypes.byref(nc)) == 10001


def test_workspace_sizes(lib):
    assert lib.mmrec_bpr_workspace_bytes(2048) == 2048 * 4
    assert lib.mmrec_linear_workspace_bytes(7050, 4096, 64) > 0
    assert lib.mmrec_linear_workspace_bytes(7050, 4096, 32) == 0


def test_argument_errors_without_gpu(lib):
    # argument validation happens on the host before any launch
    assert lib.mmrec_spmm_csr_f32(None, None, None, None, None, None, None, None, 10, 24, 1.0, 0.0, 1.0,
                                  256, None, None, 0, 0, None, None, None) == 10002   # d: not a multiple of 64, not a slice width
    assert lib.mmrec_spmm_csr_f32(None, None, None, None, None, None, None, None, 10, 32, 1.0, 0.0, 1.0,
                                  256, None, None, 0, 0, None, None, None) == 10001   # d = 32 is a feature slice: NULL pointers
    assert lib.mmrec_score_topk_f32(None, None, 4, 10, 64, None, None, 65, None, None, None, 0, None) == 10001
    assert lib.mmrec_score_topk_f32(None, None, 4, 10, 64, None, None, 5, None, None, None, 2, None) == 10001   # unknown flag
    assert lib.mmrec_linear_fwd_f32(None, None, None, None, 4, 6, 64, None, None) == 10002  # F % 4
    # the product at listed rows and its transposed push (ABI 10): widths 8 / 16 / 32 / 64
    assert lib.mmrec_spmm_rows_f32(None, None, None, None, None, 0, None, 5, 128, 32, None, None) == 10002
    assert lib.mmrec_spmm_rows_f32(None, None, None, None, None, 0, None, 5, 64, 32, None, None) == 10001
    assert lib.mmrec_spmm_rows_f32(None, None, None, None, None, 0, None, 0, 64, 32, None, None) == 0          # empty list
    assert lib.mmrec_spmm_push_rows_f32(None, None, None, None, 1.0, None, 5, 24, None, None, None) == 10002
    assert lib.mmrec_spmm_push_rows_f32(None, None, None, None, 1.0, None, 5, 16, None, None, None) == 10001
    # sampled scoring on a column slice: widths 8 / 16 / 32 / 64 k, nothing else
    assert lib.mmrec_bpr_dots_f32(None, None, None, None, None, None, 5, 24, None, None) == 10002
    assert lib.mmrec_bpr_dots_f32(None, None, None, None, None, None, 5, 16, None, None) == 10001
    assert lib.mmrec_bpr_dots_f32(None, None, None, None, None, None, 0, 8, None, None) == 0            # empty batch
    assert lib.mmrec_bpr_loss_from_dots_f32(None, 5, 7, 1.0, None, None, None, None) == 10001           # unknown variant
    assert lib.mmrec_bpr_bwd_f32(None, None, None, None, None, None, 5, 40, None, None, 1.0, None, None, None, None) == 10002
    assert lib.mmrec_bpr_bwd_f32(None, None, None, None, None, None, 5, 8, None, None, 1.0, None, None, None, None) == 10001


def test_topk_workspace_covers_both_kd64_paths(lib):
    """kd = 64 calls may be served by the fp16 filter path or the materialised path (the `flags` argument
    decides at launch): the workspace query must cover both, grow with the problem, and stay far below the 4 nq nc bytes of a
    full score matrix at evaluation scale."""
    prev = 0
    for nq, nc in ((100, 1500), (4096, 7050), (19445, 7050), (39387, 23033)):
        b = lib.mmrec_topk_workspace_bytes(nq, nc, 64, 50)
        assert b > 0 and b >= prev
        prev = b
    big = lib.mmrec_topk_workspace_bytes(20000, 500000, 64, 50)
    assert 0 < big <= 9 * 2 ** 30            # one 8 GB score block of the materialised path at most
    assert lib.mmrec_topk_workspace_bytes(0, 10, 64, 5) == 0


def test_tile_and_sweep_plans(lib):
    """The plan exports of the ops on tile64.h and mfma_sweep.h, which launch nothing.  The literals follow from the plans'
    definitions: a fuser's workgroup takes 64 rows while `cap` workgroups cover the table (spectrum 1024, modal fusion 256), then
    ceil(n / (64 cap)) tiles of 64; a sweep has ceil(own / 128) own tiles, asks for ceil(target / own tiles) splits, at most its
    cap and at most the ceil(other / 64) tiles there are, and gives a split ceil(tiles / splits) tiles of 64 rows."""
    rows = lib.mmrec_spectrum_rows_per_block
    assert [rows(n) for n in (0, 1, 65536)] == [64, 64, 64]       # 1024 blocks of 64 rows
    assert rows(65537) == 128
    assert rows(2 ** 30) == 1048576                                # 2^30 / 65,536 = 16,384 tiles of 64
    assert rows(2 ** 30 + 1) == 0 and rows(-1) == 0
    rows = lib.mmrec_modal_fusion_rows_per_block
    assert rows(16384) == 64 and rows(16385) == 128                # 256 blocks of 64 rows
    assert rows(2 ** 30) == 4194304                                # 2^30 / 16,384 = 65,536 tiles of 64
    # 65,537 rows in blocks of 128: 513 blocks of 198 floats; 16,385 rows in blocks of 128: 129 blocks of 12,544 floats
    assert lib.mmrec_spectrum_workspace_bytes(65537) == 513 * 198 * 4 == 406296
    assert lib.mmrec_modal_fusion_workspace_bytes(16385) == 129 * 12544 * 4 == 6472704
    # one own tile, 1000 tiles of the table: the forward LSE may split 64 ways (16 tiles each), the tri-top-k 32 ways (32 each)
    assert lib.mmrec_score_lse_split_cols(128, 64000, 0) == 1024
    assert lib.mmrec_tri_topk_split_cols(128, 64000) == 2048
    # 16 own tiles, target 512: 32 splits of the 111 tiles, 4 tiles each -- the same plan in both ops
    assert lib.mmrec_score_lse_split_cols(2048, 7050, 0) == 256
    assert lib.mmrec_tri_topk_split_cols(2048, 7050) == 256


def test_row_fusers_share_one_plan(lib):
    """The three whole-table fusers on tile64.h (modal fusion, encoder heads, GCN layer) have ONE plan, 256 workgroups of 64 rows
    and then more tiles each, and differ in the floats of a block's partial only.  16,385 rows: 129 blocks of 128 rows, of 12,544
    floats (3 (64 64 + 64) + 64), of 2 heads x 12,480 (3 (64 64 + 64)) and of 16,512 (4 (64 64) + 2 (64)).  Nothing is launched."""
    plans = (lib.mmrec_modal_fusion_rows_per_block, lib.mmrec_encoder_heads_rows_per_block, lib.mmrec_gcn_layer_rows_per_block)
    for n in (0, 1, 64, 65, 16384, 16385, 20011, 2 ** 30, 2 ** 30 + 1, -1):
        assert len({rows(n) for rows in plans}) == 1, n
    assert lib.mmrec_modal_fusion_workspace_bytes(16385) == 129 * 12544 * 4 == 6472704
    assert lib.mmrec_encoder_heads_workspace_bytes(16385, 2) == 129 * 2 * 12480 * 4 == 12879360
    assert lib.mmrec_gcn_layer_workspace_bytes(16385) == 129 * 16512 * 4 == 8520192


def test_projection_workspace_plans(lib):
    """The workspace exports of the modal projection (gemm.hip), which launch nothing: the split plans and the layouts behind them
    pinned to literals.  Notation: blocks = ceil(n / 128) row blocks; the fp32 plan `pick_split` minimises max(ceil(tiles s / 256),
    2) x (chunk + 128 if s > 1) over at most 64 splits, the streaming plan `pick_split_stream` wants 256 / tiles splits (three
    for 129 ... 170 tiles, one above) of at least two ring tiles each; al256 rounds up to a multiple of 256 bytes."""
    ws, bs, rows = lib.mmrec_linear_workspace_bytes, lib.mmrec_linear_bwd_split_workspace_bytes, lib.mmrec_linear_rows_workspace_bytes
    assert ws(0, 4096, 64) == 0 and ws(128, 4096, 100) == 0 and rows(0, 128, 64) == 0
    # one block, one chunk: no slabs; split W 64 x 20 x 4 = 5,120 + redo flags (1 block + 64 W rows) x 4 = 260
    assert ws(1, 20, 64) == 5120 + 260 == 5380
    # 32 blocks: the fp32 forward splits K 16 ways (2 x (256 + 128) = 768 is its cheapest), the streaming one 8: slabs 16 x 4096 x
    # 64 x 4 = 16,777,216 + split W 1,048,576 + row maxima 16 x 4096 x 4 = 262,144 + flags (32 + 64) x 4 = 384
    assert ws(4096, 4096, 64) == 16777216 + 1048576 + 262144 + 384 == 18088320
    # 180 blocks: 4 chunks of 1024 (3 rounds x 1152 = 3,456), the streaming plan 1: slabs 4 x 23,033 x 256 = 23,585,792 + split W
    # 1,048,576 + row maxima 4 x 23,033 x 4 = 368,528 + flags (180 + 64) x 4 = 976
    assert ws(23033, 4096, 64) == 23585792 + 1048576 + 368528 + 976 == 25003872
    # out = 384, 2 blocks: the forward's 64 chunks of 64 outweigh dW's six groups of one chunk (6 x 64 x 4 = 1,536): slabs 64 x
    # 129 x 256 = 2,113,536 + split W 1,048,576 + row maxima 64 x 129 x 4 = 33,024 + flags (2 + 64) x 4 = 264
    assert ws(129, 4096, 384) == 2113536 + 1048576 + 33024 + 264 == 3195400
    # one column block, 32,769 items: dW asks for 64 chunks of ceil(513 / 32) x 32 = 544 items, which makes 61; per 64-output group
    # 61 slabs of 64 x 128 floats + 61 x 64 db partials = 503,616 floats; the forward (257 blocks, one chunk) needs 34,052 bytes
    assert ws(32769, 128, 128) == 503616 * 4 * 2 == 4028928
    assert ws(32769, 128, 384) == 503616 * 4 * 6 == 12086784
    # backward split, larger than the fp32 calls' 33,032: 3 chunks of 64 items, 5 tiles of 32: W^T 128 x 256 = 32,768 + column
    # scales (128 + 256) x 4 = 1,536 + db partials max(3, 5) x 256 = 1,280 + slabs 3 x 64 x 128 x 4 = 98,304 + dY split 5 x 12,288
    assert ws(129, 128, 64) == 33032
    assert bs(129, 128, 64) == 32768 + 1536 + 1280 + 98304 + 61440 == 195328
    # 32 column blocks: 8 chunks of ceil(7813 / 32) x 32 = 7,840 items, 1,954 tiles, 64 dY-split workgroups: W^T 1,048,576 + scales
    # al256(4,352 x 4) = 17,408 + db partials 64 x 256 = 16,384 + slabs 8 x 64 x 4096 x 4 = 8,388,608 + dY split 1,954 x 12,288
    assert bs(62500, 4096, 64) == 1048576 + 17408 + 16384 + 8388608 + 24010752 == 33481728
    # 3 column blocks, 128 items: 2 chunks of 64, 4 tiles: 98,304 + 2,560 + 1,024 + 2 x 64 x 384 x 4 = 196,608 + 4 x 12,288
    assert bs(128, 384, 64) == 98304 + 2560 + 1024 + 196608 + 49152 == 347648
    assert bs(129, 4096, 384) == ws(129, 4096, 384)            # out > 64: the fp32 calls serve it, and their workspace
    # gathered rows: the backward split's size where it serves the shape (out = 64, F % 128 == 0), else 0
    assert rows(128, 384, 64) == 347648 and rows(62500, 4096, 64) == 33481728
    assert rows(7050, 96, 64) == 0 and rows(7050, 4096, 128) == 0
