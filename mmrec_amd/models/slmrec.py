"""SLMRec on the HIP hot path (reference: models/slmrec.py), ssl_task 'FAC' (the shipped configuration).

Three LightGCN propagations over the same normalised user-item graph -- id, projected image and projected text item
tables, each stacked under the shared user table -- then Linear fusion, an in-batch InfoNCE main loss and the FAC
self-supervised InfoNCE terms between projected id / image / text item views.

Kernels: fp32 MFMA projection (features -> 64, the 192 -> 64 fusion layers and the 64 -> 64 / 32 FAC heads), fused
layer-mean CSR SpMM, the fused in-batch InfoNCE (row-normalised views, temperature, diagonal positives ==
CrossEntropy(logits / temp, arange)), fused score + mask + top-K evaluation (sigmoid is monotone: same ranking).
`batched_propagation` (new key, default off until it has run on the device): the three tables are propagated as ONE
192-wide SpMM per layer, so the CSR is read once instead of three times.

Reference behaviour kept: item features are L2-normalised once at load; evaluation scores with the embeddings of
the LAST training forward; `reg` is read by nothing; `g_a_iva` is created (and saved) but unused without audio.
Not carried over: ssl_task 'FD' / 'FM' / 'FD+FM' -- outside the 'kwai' dataset the reference itself fails there
(they read audio tensors that are never created, slmrec.py:115-117).
"""
import numpy as np
import scipy.sparse as sp
import torch
import torch.nn as nn
import torch.nn.functional as F

from mmrec_amd import hip_ops
from mmrec_amd.models._base import FusedEvalMixin, GeneralRecommender


def slmrec_adjacency(inter_csr, n_users, n_items, adj_type):
    """create_adj_mat (slmrec.py:436-478): (COO indices [2, nnz], fp32 values) of the chosen normalisation"""
    u, i = inter_csr.nonzero()
    n = n_users + n_items
    half = sp.csr_matrix((np.ones(u.shape[0], dtype=np.float32), (u, i + n_users)), shape=(n, n))
    adj = half + half.T

    def row_normalised(a):                              # D^-1 a, empty rows stay empty
        deg = np.asarray(a.sum(1)).flatten()
        with np.errstate(divide='ignore'):
            inv = np.power(deg, -1)
        inv[np.isinf(inv)] = 0.0
        return sp.diags(inv).dot(a)
    if adj_type == 'plain':
        out = adj
    elif adj_type == 'norm':
        out = row_normalised(adj + sp.eye(n))
    elif adj_type == 'gcmc':
        out = row_normalised(adj)
    elif adj_type == 'pre':                             # D^-1/2 A D^-1/2
        deg = np.asarray(adj.sum(1)) + 1e-08
        dis = np.power(deg, -0.5).flatten()
        dis[np.isinf(dis)] = 0.0
        out = sp.diags(dis).dot(adj).dot(sp.diags(dis))
    else:
        out = row_normalised(adj) + sp.eye(n)
    out = out.tocoo()
    return np.stack([out.row.astype(np.int64), out.col.astype(np.int64)]), out.data.astype(np.float32)


def _lin(layer, x):
    """nn.Linear on the MFMA projection kernel when its shape is one the kernel takes (64 outputs)"""
    if layer.out_features == hip_ops.EMB_DIM and layer.in_features % 4 == 0:
        return hip_ops.linear(x.contiguous(), layer.weight, layer.bias)
    return layer(x)


class SLMRec(FusedEvalMixin, GeneralRecommender):
    def __init__(self, config, dataset):
        super().__init__(config, dataset)
        self.a_feat = None
        self.config = config
        self.num_users, self.num_items = self.n_users, self.n_items
        self.latent_dim = config['recdim']
        self.n_layers = config['layer_num']
        self.mm_fusion_mode = config['mm_fusion_mode']
        self.temp = config['temp']
        self.ssl_task = config['ssl_task']
        if self.ssl_task != 'FAC':
            raise NotImplementedError("SLMRec: ssl_task %r -- the reference only runs 'FAC' outside its 'kwai' dataset"
                                      % (self.ssl_task,))
        if self.mm_fusion_mode != 'concat':
            # the fusion layers are sized for the concatenation (slmrec.py:418-423); 'mean' hands them latent_dim-wide
            # rows and fails in the reference's first forward as well
            raise NotImplementedError("SLMRec: mm_fusion_mode %r (only 'concat' runs in the reference)"
                                      % (self.mm_fusion_mode,))
        self.batched_propagation = bool(config['batched_propagation'])
        self._create_tables(config)
        self.all_items = self.all_users = None
        idx, val = slmrec_adjacency(dataset.inter_matrix(form='csr').astype(np.float32), self.n_users, self.n_items,
                                    config['adj_type'])
        n = self.n_users + self.n_items
        symmetric = config['adj_type'] in ('plain', 'pre')
        self.norm_adj = hip_ops.CsrGraph.from_coo_host(idx, val, n, n, self.device, symmetric=symmetric)
        if not symmetric:
            self.norm_adj.transpose()
        d = self.latent_dim
        self.g_i_iv, self.g_v_iv = nn.Linear(d, d), nn.Linear(d, d)
        self.g_iv_iva, self.g_a_iva = nn.Linear(d, d), nn.Linear(d, d)
        self.g_iva_ivat, self.g_t_ivat = nn.Linear(d, d // 2), nn.Linear(d, d // 2)
        for layer in (self.g_i_iv, self.g_v_iv, self.g_iv_iva, self.g_a_iva, self.g_iva_ivat, self.g_t_ivat):
            nn.init.xavier_uniform_(layer.weight)
        self.ssl_temp = config['ssl_temp']

    def _create_tables(self, config):
        d = self.latent_dim
        self.embedding_user = nn.Embedding(self.n_users, d)
        self.embedding_item = nn.Embedding(self.n_items, d)
        if config['init'] == 'xavier':
            nn.init.xavier_uniform_(self.embedding_user.weight, gain=1)
            nn.init.xavier_uniform_(self.embedding_item.weight, gain=1)
        elif config['init'] == 'normal':
            nn.init.normal_(self.embedding_user.weight, std=0.1)
            nn.init.normal_(self.embedding_item.weight, std=0.1)
        n_modal = 0
        if self.v_feat is not None:
            self.v_feat = F.normalize(self.v_feat, dim=1)
            self.v_dense = nn.Linear(self.v_feat.shape[1], d)
            nn.init.xavier_uniform_(self.v_dense.weight)
            n_modal += 1
        if self.t_feat is not None:
            self.t_feat = F.normalize(self.t_feat, dim=1)
            self.t_dense = nn.Linear(self.t_feat.shape[1], d)
            nn.init.xavier_uniform_(self.t_dense.weight)
            n_modal += 1
        if self.v_feat is None or self.t_feat is None:
            raise ValueError("SLMRec needs image and text features (its forward reads both, slmrec.py:96-109)")
        self.item_feat_dim = d * (n_modal + 1)
        self.embedding_item_after_GCN = nn.Linear(self.item_feat_dim, d)
        self.embedding_user_after_GCN = nn.Linear(self.item_feat_dim, d)
        nn.init.xavier_uniform_(self.embedding_item_after_GCN.weight)
        nn.init.xavier_uniform_(self.embedding_user_after_GCN.weight)

    def mm_fusion(self, reps):
        return torch.cat(reps, dim=1)

    def compute(self):
        users = self.embedding_user.weight
        tables = (self.embedding_item.weight, _lin(self.v_dense, self.v_feat), _lin(self.t_dense, self.t_feat))
        U, d = self.n_users, self.latent_dim
        if self.batched_propagation:
            wide = torch.cat([torch.cat((users, t), dim=0) for t in tables], dim=1)          # [N, 3 d]
            out = hip_ops.lightgcn_mean(self.norm_adj, wide, self.n_layers)
            outs = [out[:, j * d:(j + 1) * d] for j in range(3)]
        else:
            outs = [hip_ops.lightgcn_mean(self.norm_adj, torch.cat((users, t), dim=0), self.n_layers) for t in tables]
        (self.i_emb_u, self.i_emb_i), (self.v_emb_u, self.v_emb_i), (self.t_emb_u, self.t_emb_i) = \
            [(o[:U], o[U:]) for o in outs]
        user = _lin(self.embedding_user_after_GCN, self.mm_fusion([self.i_emb_u, self.v_emb_u, self.t_emb_u]))
        item = _lin(self.embedding_item_after_GCN, self.mm_fusion([self.i_emb_i, self.v_emb_i, self.t_emb_i]))
        return user, item

    def eval_embeddings(self):
        if self.all_users is None:          # the reference cannot evaluate before a training step; compute instead
            u, i = self.compute()
            return u.detach(), i.detach()
        return self.all_users.detach(), self.all_items.detach()

    def full_sort_predict(self, interaction):
        return torch.sigmoid(super().full_sort_predict(interaction))

    def _in_batch_ce(self, a, b, temp):
        """CrossEntropy(a b^T / temp, arange): plain logits, not normalised (the FAC heads)"""
        logits = torch.mm(a, b.t()) / temp
        return F.cross_entropy(logits, torch.arange(a.shape[0], device=a.device))

    def infonce(self, users, pos):
        all_users, all_items = self.compute()
        self.all_users, self.all_items = all_users.detach(), all_items.detach()     # what the evaluation reuses: values only
        ids = torch.arange(users.shape[0], device=users.device)
        return hip_ops.infonce(all_users[users].contiguous(), all_items[pos].contiguous(), ids, self.temp)

    def fac(self, idx):
        x_i_iv = _lin(self.g_i_iv, self.i_emb_i[idx])
        x_v_iv = _lin(self.g_v_iv, self.v_emb_i[idx])
        v_loss = self._in_batch_ce(x_i_iv, x_v_iv, self.ssl_temp)
        x_iva_ivat = self.g_iva_ivat(_lin(self.g_iv_iva, x_i_iv))
        x_t_ivat = self.g_t_ivat(self.t_emb_i[idx])
        return v_loss + self._in_batch_ce(x_iva_ivat, x_t_ivat, self.ssl_temp)

    def calculate_loss(self, interaction):
        users, pos = interaction[0], interaction[1]
        main_loss = self.infonce(users, pos)
        loss = main_loss + self.config['ssl_alpha'] * self.fac(pos)
        # nothing on `self` keeps this step's autograd graph alive after it: a later step captured as a hipGraph would meet the
        # gradient accumulators of this one, bound to another stream (the capture then ended in a segmentation fault)
        self.i_emb_u = self.i_emb_i = self.v_emb_u = self.v_emb_i = self.t_emb_u = self.t_emb_i = None
        return loss
