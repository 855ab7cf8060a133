"""GRCN on the HIP hot path (reference: models/grcn.py, which needs torch_geometric).

Per modality a content GCN scores every user-item edge by attention -- softmax over the incoming edges of a node of
<x_target, x_source> -- and aggregates with those weights; the per-modality edge weights, scaled by a learned
per-node confidence and pruned by relu(max), then weight a two-hop sum aggregation of the id embeddings.  Every
aggregation is the CSR SpMM with DIFFERENTIABLE per-edge values (`hip_ops.spmm_vals`: forward, d/dX through the
transposed structure, d/dvalues as per-edge dot products) over one structure built once -- the bidirectional edge
list never changes; the per-edge scores are the SDDMM kernel (`hip_ops.edge_dot`, its backward the same SpMM over that
structure), the segment softmax over a target's incoming edges is `hip_ops.edge_softmax` over the same structure's CSR
form (no atomics: the attention weights and their gradient repeat bit for bit).  With the config key `fused_attention: True`
(absent / False: the three ops) the content GCN's attention is `hip_ops.edge_attention`: scores, softmax and aggregation in one
kernel that gathers every source row once; with `fused_attention_backward: True` as well (absent / False: the backward composed
of the older kernels) its backward is one call too (`mmrec_edge_attention_bwd_f32`).  BPR runs on the fused kernel over the 192-wide concatenation, evaluation on the fused score + mask +
top-K.

Reference behaviour kept:
  * the routing loop calls the attention layer on the user -> item edges only, so nothing is ever aggregated AT a
    user and `preference + x_hat[:num_user]` adds zeros: three extra row-normalisations of the preference table and
    nothing else (grcn.py:147-155).  Here the loop is those normalisations, without the discarded aggregation;
  * evaluation scores with the `result` of the last training forward (grcn.py:320-327);
  * `n_layers` is the number of routing iterations; weight_mode 'confid', fusion 'concat', pruning on.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from mmrec_amd import hip_ops
from mmrec_amd.models._base import FusedEvalMixin, GeneralRecommender
from mmrec_amd.models.mmgcn import _lin64


def segment_softmax(score, index, n):
    """torch_geometric.utils.softmax: softmax over the entries sharing an index (eps 1e-16 in the denominator) -- the torch
    composition; the model itself calls `hip_ops.edge_softmax` over its edge structure"""
    return hip_ops.segment_softmax_torch(score, index, n)


class EGCN(nn.Module):
    """id embeddings: x + W x + W W x with the refined edge weights W"""

    def __init__(self, num_user, num_item, dim_E):
        super().__init__()
        self.id_embedding = nn.Parameter(nn.init.xavier_normal_(torch.rand((num_user + num_item, dim_E))))

    def forward(self, edges, weight):
        x = F.normalize(self.id_embedding)
        x1 = hip_ops.spmm_vals(edges.dyn, x, weight)
        x2 = hip_ops.spmm_vals(edges.dyn, x1, weight)
        return x + x1 + x2


class CGCN(nn.Module):
    """content embeddings of one modality + the attention weight of every (bidirectional) edge"""

    def __init__(self, features, num_user, dim_C, num_routing, fused_attention=False, fused_attention_backward=False):
        super().__init__()
        self.num_user, self.num_routing, self.fused_attention = num_user, num_routing, bool(fused_attention)
        self.fused_attention_backward = bool(fused_attention_backward)       # only read together with fused_attention
        self.preference = nn.Parameter(nn.init.xavier_normal_(torch.rand((num_user, dim_C))))
        self.features = features
        self.MLP = nn.Linear(features.size(1), dim_C)
        nn.init.xavier_normal_(self.MLP.weight)

    def forward(self, edges):
        features = F.normalize(F.leaky_relu(_lin64(self.MLP, self.features)))
        preference = F.normalize(self.preference)
        for _ in range(self.num_routing):
            preference = F.normalize(preference)          # + the all-zero user rows of the item-side aggregation
        x = torch.cat((preference, features), dim=0)
        if self.fused_attention:                          # scores, softmax and aggregation in one pass over the edges
            agg, alpha = hip_ops.edge_attention(x, x, edges.dyn, fused_backward=self.fused_attention_backward)
            return x + agg, alpha
        score = hip_ops.edge_dot(x, x, edges.dst, edges.src, dyn=edges.dyn)
        alpha = hip_ops.edge_softmax(score, edges.dyn)
        return x + hip_ops.spmm_vals(edges.dyn, x, alpha), alpha


class _Edges:
    """cat(user -> item, item -> user): message sources, targets and the SpMM structure (rows = targets)"""

    def __init__(self, users, items, n, device):
        self.src = torch.cat((users, items)).to(device)
        self.dst = torch.cat((items, users)).to(device)
        self.dyn = hip_ops.DynGraph(self.dst.contiguous(), self.src.contiguous(), n, n)


class GRCN(FusedEvalMixin, GeneralRecommender):
    def __init__(self, config, dataset):
        super().__init__(config, dataset)
        self.num_user, self.num_item = self.n_users, self.n_items
        dim_x, dim_C = config['embedding_size'], config['latent_embedding']
        if dim_x != hip_ops.EMB_DIM or dim_C != hip_ops.EMB_DIM:
            raise NotImplementedError("GRCN: embedding_size / latent_embedding must be %d" % hip_ops.EMB_DIM)
        self.reg_weight = config['reg_weight']
        inter = dataset.inter_matrix(form='coo').astype(np.float32)
        users = torch.from_numpy(inter.row.astype(np.int64))
        items = torch.from_numpy(inter.col.astype(np.int64)) + self.n_users
        self.edge_index = torch.stack((users, items)).to(self.device)
        n = self.n_users + self.n_items
        self.edges = _Edges(users, items, n, self.device)
        self.id_gcn = EGCN(self.n_users, self.n_items, dim_x)
        fused = bool(config['fused_attention'])           # new key, default off: `hip_ops.edge_attention` for the content GCNs
        fused_bwd = bool(config['fused_attention_backward'])      # new key, default off: the attention's backward in one call
        num_model = 0
        if self.v_feat is not None:
            self.v_gcn = CGCN(self.v_feat, self.n_users, dim_C, config['n_layers'], fused, fused_bwd)
            num_model += 1
        if self.t_feat is not None:
            self.t_gcn = CGCN(self.t_feat, self.n_users, dim_C, config['n_layers'], fused, fused_bwd)
            num_model += 1
        if num_model == 0:
            raise ValueError("GRCN needs at least one item feature modality")
        self.model_specific_conf = nn.Parameter(nn.init.xavier_normal_(torch.rand((n, num_model))))
        self.result = nn.init.xavier_normal_(torch.rand((n, dim_x))).to(self.device)

    def _apply(self, fn, *a, **k):
        out = super()._apply(fn, *a, **k)
        self.result = fn(self.result)
        return out

    def forward(self):
        reps, weights = [], []
        for name in ('v_gcn', 't_gcn'):
            if hasattr(self, name):
                rep, alpha = getattr(self, name)(self.edges)
                reps.append(rep)
                weights.append(alpha)
        weight = torch.stack(weights, dim=1) * self.model_specific_conf[self.edges.src]      # confidence of the sender
        weight = torch.relu(weight.max(dim=1).values)                                        # 'confid' + pruning
        id_rep = self.id_gcn(self.edges, weight)
        representation = torch.cat([id_rep] + reps, dim=1)
        self.result = representation.detach()
        return representation

    def eval_embeddings(self):
        return self.result[:self.n_users], self.result[self.n_users:]

    def calculate_loss(self, interaction):
        users = interaction[0]
        pos, neg = interaction[1] + self.n_users, interaction[2] + self.n_users
        out = self.forward().contiguous()
        loss = hip_ops.bpr_loss(out, out, users, pos, neg, hip_ops.BPR_LOGSIG, 'mean')
        B, d = users.shape[0], hip_ops.EMB_DIM
        ids = self.id_gcn.id_embedding
        reg = (2.0 * hip_ops.gather_sqnorm(ids, users) + hip_ops.gather_sqnorm(ids, pos)
               + hip_ops.gather_sqnorm(ids, neg)) / (2.0 * B * d)
        if hasattr(self, 'v_gcn'):
            reg = reg + (self.v_gcn.preference ** 2).mean()
            reg = reg + hip_ops.gather_sqnorm(self.v_gcn.preference, users) / (B * d)
        if hasattr(self, 't_gcn'):
            reg = reg + hip_ops.gather_sqnorm(self.t_gcn.preference, users) / (B * d)
        return loss + self.reg_weight * reg
