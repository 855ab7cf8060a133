"""Encoders shared by models (reference: common/encoders.py).

LightGCN_Encoder: mean_l(A_hat^l E0) with A_hat = sparse_dropout(norm_adj, rate ~ U[0, 1)) drawn per forward
(encoders.py:77-90): the kept entries scaled by 1 / (1 - rate).  The CSR structure never changes, only the per-entry
values do, so one `DynGraph` (structure + transpose permutation, built once) serves every batch and the dropped
entries are zeros of the value vector; the masked matrix is not symmetric, the backward runs on the transposed CSR
with the same values.  `get_embedding` (no dropout) is the fused layer-mean SpMM on the plain normalised CSR.

`fused_edge_dropout: True` (config key, off by default): the dropout branch runs `hip_ops.lightgcn_mean_edge_dropout` -- the
keep mask packed to one bit per entry, dropped entries never gathered, the layer mean in the SpMM's accumulator epilogue (the
arithmetic of the no-dropout path, not the bits of `stack().mean()`).  The draws are the same either way.
"""
import numpy as np
import torch
import torch.nn as nn

from mmrec_amd import hip_ops
from mmrec_amd.graph import norm_adj_graph
from mmrec_amd.models._base import GeneralRecommender


class LightGCN_Encoder(GeneralRecommender):
    def __init__(self, config, dataset):
        super().__init__(config, dataset)
        self.interaction_matrix = dataset.inter_matrix(form='coo').astype(np.float32)
        self.user_count, self.item_count = self.n_users, self.n_items
        self.latent_size = config['embedding_size']
        self.n_layers = 3 if config['n_layers'] is None else config['n_layers']
        self.layers = [self.latent_size] * self.n_layers
        self.drop_ratio = 1.0
        self.drop_flag = True
        init = nn.init.xavier_uniform_
        self.embedding_dict = nn.ParameterDict({
            'user_emb': nn.Parameter(init(torch.empty(self.user_count, self.latent_size))),
            'item_emb': nn.Parameter(init(torch.empty(self.item_count, self.latent_size)))})
        self.sparse_norm_adj = norm_adj_graph(self.interaction_matrix, self.n_users, self.n_items, self.device)
        self._dyn = None
        self.fused_edge_dropout = bool(config['fused_edge_dropout']) if 'fused_edge_dropout' in config else False
        self._edge_graph = None

    def draw_dropout(self):
        """(rate, keep mask over the nnz entries in row-major order) -- encoders.py:77-79,86-88."""
        rate = np.random.random() * self.drop_ratio
        keep = torch.floor(1 - rate + torch.rand(self.sparse_norm_adj.nnz, device=self.device)).to(torch.bool)
        return rate, keep

    def _dropped_values(self):
        g = self.sparse_norm_adj
        if self._dyn is None:
            n = g.n_rows
            rows = torch.repeat_interleave(torch.arange(n, device=g.rowptr.device), torch.diff(g.rowptr.to(torch.int64)))
            self._dyn = hip_ops.DynGraph(rows.contiguous(), g.colidx.to(torch.int64).contiguous(), n, n,
                                         long_row_threshold=g.long_row_threshold)
        rate, keep = self.draw_dropout()
        return self._dyn, (g.vals * keep.to(g.vals.dtype)) * (1. / (1 - rate))

    def _edge_dropout_graph(self):
        """the fixed normalised values on the structure `_dropped_values` uses, built once, next to `_dyn`"""
        g = self.sparse_norm_adj
        if self._edge_graph is None:
            if self._dyn is None:
                n = g.n_rows
                rows = torch.repeat_interleave(torch.arange(n, device=g.rowptr.device), torch.diff(g.rowptr.to(torch.int64)))
                self._dyn = hip_ops.DynGraph(rows.contiguous(), g.colidx.to(torch.int64).contiguous(), n, n,
                                             long_row_threshold=g.long_row_threshold)
            self._edge_graph = hip_ops.EdgeDropoutGraph(self._dyn, g.vals)
        return self._edge_graph

    def all_embeddings(self, dropout):
        ego = torch.cat([self.embedding_dict['user_emb'], self.embedding_dict['item_emb']], 0)
        if not dropout:
            out = hip_ops.lightgcn_mean(self.sparse_norm_adj, ego, self.n_layers)
        elif self.fused_edge_dropout:
            eg = self._edge_dropout_graph()
            rate, keep = self.draw_dropout()
            out = hip_ops.lightgcn_mean_edge_dropout(eg, ego, self.n_layers, keep, 1. / (1 - rate))
        else:
            dyn, vals = self._dropped_values()
            layers = [ego]
            for _ in range(self.n_layers):
                ego = hip_ops.spmm_vals(dyn, ego, vals)
                layers.append(ego)
            out = torch.stack(layers, dim=1).mean(dim=1)
        return out[:self.user_count], out[self.user_count:]

    def forward(self, inputs):
        u_all, i_all = self.all_embeddings(self.drop_flag)
        return u_all[inputs[0], :], i_all[inputs[1], :]

    @torch.no_grad()
    def get_embedding(self):
        return self.all_embeddings(False)
