"""SELFCF_ed with the LightGCN encoder on the HIP hot path (reference: models/selfcfed_lgn.py,
common/encoders.py:12-139).

encoder : mean_l(A_hat^l E0) with A_hat = sparse_dropout(norm_adj, rate ~ U[0,1)) drawn per batch
          (encoders.py:77-90): the kept entries scaled by 1/(1-rate).  The CSR structure never changes,
          only the per-entry values do, so one `DynGraph` (structure + transpose permutation, built once)
          serves every batch and the dropped entries are zeros of the value vector; the masked matrix is
          not symmetric, the backward runs on the transposed CSR with the same values
loss    : predictor Linear(64, 64) on the batch's rows (fp32 MFMA projection kernel), negative cosine
          similarity against dropped-out detached targets, L2 regulariser (selfcfed_lgn.py:57-68)
eval    : score = p(u).i + u.p(i)  ==  <[p(u), u], [i, p(i)]>: ONE fused score + mask + top-K at row
          width 128 (selfcfed_lgn.py:70-77); no dropout (encoders.py:118-139, plain norm_adj CSR)
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from mmrec_amd import hip_ops
from mmrec_amd.common.encoders import LightGCN_Encoder
from mmrec_amd.models._base import FusedEvalMixin, GeneralRecommender


class SELFCFED_LGN(FusedEvalMixin, GeneralRecommender):
    graph_capturable = False      # the encoder's edge-dropout rate is a host-side numpy draw per batch: a capture would freeze it

    def __init__(self, config, dataset):
        super().__init__(config, dataset)
        self.user_count, self.item_count = self.n_users, self.n_items
        self.latent_size = config['embedding_size']
        self.dropout = config['dropout']
        self.reg_weight = config['reg_weight']
        self.online_encoder = LightGCN_Encoder(config, dataset)
        self.predictor = nn.Linear(self.latent_size, self.latent_size)

    def _predict(self, x):
        return hip_ops.linear(x.contiguous(), self.predictor.weight, self.predictor.bias)

    def forward(self, inputs):
        u_online, i_online = self.online_encoder(inputs)
        with torch.no_grad():
            u_target = F.dropout(u_online.clone(), self.dropout)
            i_target = F.dropout(i_online.clone(), self.dropout)
        return u_online, u_target, i_online, i_target

    @torch.no_grad()
    def get_embedding(self):
        u_online, i_online = self.online_encoder.get_embedding()
        return self._predict(u_online), u_online, self._predict(i_online), i_online

    @staticmethod
    def loss_fn(p, z):      # negative cosine similarity, fused (selfcfed_lgn.py:57-58)
        return -hip_ops.cosine_mean(p.contiguous(), None, z.detach().contiguous(), None)

    def calculate_loss(self, interaction):
        u_online, u_target, i_online, i_target = self.forward(interaction)
        reg_loss = 0.5 * (torch.sum(u_online ** 2) + torch.sum(i_online ** 2))      # L2Loss, common/loss.py:54-62
        u_online, i_online = self._predict(u_online), self._predict(i_online)
        loss_ui = self.loss_fn(u_online, i_target) / 2
        loss_iu = self.loss_fn(i_online, u_target) / 2
        return loss_ui + loss_iu + self.reg_weight * reg_loss

    def eval_embeddings(self):
        pu, u, pi, i = self.get_embedding()
        return torch.cat([pu, u], dim=1), torch.cat([i, pi], dim=1)
