"""DRAGON on the HIP hot path (reference: models/dragon.py, which needs torch_geometric).

DualGNN's two modal GCNs (x + A x + A^2 x over the symmetric-normalised user-item graph) with the modalities
CONCATENATED instead of summed (128-wide representations), plus FREEDOM's frozen kNN item-item graph: item
representations are propagated `n_mm_layers` times over `mm_adj` and users over the co-occurrence graph.  Every
propagation is the HIP CSR SpMM at row width 64 (bipartite hops) or 128 (item-item, user-user); the modal MLPs run
on the fp32 MFMA projection kernels; BPR is the fused gather-dot-logsigmoid kernel over the 128-wide table and the
full-rank evaluation the fused score + mask + top-K (kd = 128).

Reference quirks kept: `image_embedding` / `text_embedding` / `image_trs` / `text_trs` / `MLP_v` / `MLP_t` /
`MLP_user` / `weight_i` are created (and saved) but take no part in the loss; `mm_adj_{knn_k}.pt` is cached next to
the data WITHOUT the image weight in its name; evaluation uses the `result_embed` of the last training forward.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from mmrec_amd import hip_ops
from mmrec_amd.models._base import FusedEvalMixin, GeneralRecommender
from mmrec_amd.models.dualgnn import GCN, UserGraphMixin, aggr_graph, check_aggr_mode, np_xavier_normal
from mmrec_amd.models.freedom import load_or_build_mm_adj


class DRAGON(UserGraphMixin, FusedEvalMixin, GeneralRecommender):
    def __init__(self, config, dataset):
        super().__init__(config, dataset)
        dim_x = config['embedding_size']
        self.num_user, self.num_item = self.n_users, self.n_items
        self.feat_embed_dim = config['feat_embed_dim']
        self.n_layers = config['n_mm_layers']
        self.knn_k = config['knn_k']
        self.mm_image_weight = config['mm_image_weight']
        self.aggr_mode = check_aggr_mode(config['aggr_mode'], "DRAGON")
        self.construction = 'cat'
        self.reg_weight = config['reg_weight']
        self.drop_rate = 0.1
        self.dim_latent = 64
        self.MLP_v = nn.Linear(self.dim_latent, self.dim_latent, bias=False)
        self.MLP_t = nn.Linear(self.dim_latent, self.dim_latent, bias=False)
        self.load_user_graph(config, 40)
        if self.v_feat is not None:
            self.image_embedding = nn.Embedding.from_pretrained(self.v_feat, freeze=False)
            self.image_trs = nn.Linear(self.v_feat.shape[1], self.feat_embed_dim)
        if self.t_feat is not None:
            self.text_embedding = nn.Embedding.from_pretrained(self.t_feat, freeze=False)
            self.text_trs = nn.Linear(self.t_feat.shape[1], self.feat_embed_dim)
        self.mm_adj = load_or_build_mm_adj(config, self.v_feat, self.t_feat, self.knn_k, self.mm_image_weight,
                                           self.n_items, self.device, cache_name='mm_adj_{}.pt'.format(self.knn_k))
        inter = dataset.inter_matrix(form='coo').astype(np.float32)
        self.graph = aggr_graph(self.aggr_mode, inter, self.n_users, self.n_items, self.device, "DRAGON")
        self.weight_u = nn.Parameter(np_xavier_normal(self.n_users, 2, 1))
        self.weight_u.data = F.softmax(self.weight_u.data, dim=1)
        self.weight_i = nn.Parameter(np_xavier_normal(self.n_items, 2, 1))
        self.weight_i.data = F.softmax(self.weight_i.data, dim=1)
        np.random.choice(self.n_items, int(self.n_items * self.drop_rate), replace=False)   # the unused item drop
        self.MLP_user = nn.Linear(self.dim_latent * 2, self.dim_latent)
        self.v_preference = self.t_preference = None
        if self.v_feat is not None:
            self.v_gcn = GCN(self.n_users, self.v_feat.size(1), self.dim_latent, self.aggr_mode)
        if self.t_feat is not None:
            self.t_gcn = GCN(self.n_users, self.t_feat.size(1), self.dim_latent, self.aggr_mode)
        self.result_embed = nn.init.xavier_normal_(
            torch.tensor(np.random.randn(self.n_users + self.n_items, dim_x))).float().to(self.device)

    def forward(self):
        v_rep, t_rep = self._modal()
        U = self.n_users
        if v_rep is not None and t_rep is not None:
            rep = torch.cat((v_rep, t_rep), dim=1)
            user_rep = torch.cat((v_rep[:U] * self.weight_u[:, 0], t_rep[:U] * self.weight_u[:, 1]), dim=1)
        else:
            rep = v_rep if v_rep is not None else t_rep
            user_rep = rep[:U]
        item_rep = rep[U:].contiguous()
        h = item_rep if self.n_layers else 2.0 * item_rep
        for layer in range(self.n_layers):
            last = layer == self.n_layers - 1
            h = hip_ops.spmm(self.mm_adj, h, item_rep if last else None)         # item_rep + mm_adj^n item_rep
        user_rep = hip_ops.spmm(self.user_csr, user_rep.contiguous(), user_rep)  # user_rep + h_u1
        result = torch.cat((user_rep, h), dim=0)
        self.result_embed = result.detach()
        return result

    def calculate_loss(self, interaction):
        loss, reg = self._bpr_and_pref_reg(self.forward(), interaction)
        reg = reg + (self.weight_u ** 2).mean()
        return loss + self.reg_weight * reg
