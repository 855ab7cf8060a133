"""DualGNN on the HIP hot path (reference: models/dualgnn.py, which needs torch_geometric).

Per modality: features -> MLP (F -> 256 -> 64, fp32 MFMA projection kernels) -> row-normalise together with a
trainable user preference table -> two hops of D^-1/2 A D^-1/2 over the user-item graph, x + A x + A^2 x (PyG
`Base_gcn(aggr='add')` twice; here the fused layer-accumulating CSR SpMM).  `aggr_mode: 'mean'` is the same SpMM with
1 / in-degree values on raw messages, `'max'` two calls of the neighbour-max kernel (`hip_ops.neighbor_max`).  The user side is then smoothed over a
user-user co-occurrence graph: every user averages (softmax-of-count weights) the representations of k = 40
neighbours -- the reference gathers a [U, 40, 64] tensor and batch-multiplies it; that is an SpMM with a [U, U]
CSR of 40 entries per row, and its backward the SpMM with the transposed CSR.

Reference quirks kept on purpose:
  * `representation = self.v_rep; representation += self.t_rep` adds IN PLACE, so the "visual" user
    representation that enters the modality fusion is already v + t (dualgnn.py:143-151,155-163);
  * `self.v_preference = preference` re-registers the GCN's table under a second top-level name, so state dicts
    written after the first step carry `v_preference` / `t_preference` next to `v_gcn.preference`;
  * the edge-dropped copies of the graph are built but never used (GCN.forward ignores `edge_index_drop`): they
    are not built here, only the numpy RNG draw behind them is consumed so that the epoch shuffles stay aligned;
  * evaluation scores with the `result_embed` of the last training forward (dualgnn.py:190-197);
  * MLP_v / MLP_t / MLP_user are created (and saved) but never called.
"""
import math
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from mmrec_amd import hip_ops
from mmrec_amd.models._base import FusedEvalMixin, GeneralRecommender
from mmrec_amd.models.mmgcn import _lin64
from mmrec_amd.utils.user_graph import pack_user_graph_dict


def sym_norm_graph(inter_coo, n_users, n_items, device):
    """D^-1/2 A D^-1/2 over cat(edges, flipped edges), degrees counted on that list (Base_gcn.message,
    dualgnn.py:331-339); no epsilon: isolated nodes have no edges to scale."""
    u = inter_coo.row.astype(np.int64)
    i = inter_coo.col.astype(np.int64) + n_users
    src, dst = np.concatenate([u, i]), np.concatenate([i, u])
    n = n_users + n_items
    deg = np.bincount(src, minlength=n).astype(np.float32)
    with np.errstate(divide='ignore'):
        dis = np.power(deg, np.float32(-0.5)).astype(np.float32)
    val = (dis[src] * dis[dst]).astype(np.float32)
    return hip_ops.CsrGraph.from_coo_host(np.stack([dst, src]), val, n, n, device, symmetric=True)


AGGR_MODES = ('add', 'mean', 'max')


def mean_graph(inter_coo, n_users, n_items, device):
    """the same cat(edges, flipped edges) list with values 1 / in-degree of the target (PyG `aggr='mean'` on raw messages,
    Base_gcn.message returns x_j as it is); not symmetric: the transpose is built once, here"""
    u = inter_coo.row.astype(np.int64)
    i = inter_coo.col.astype(np.int64) + n_users
    src, dst = np.concatenate([u, i]), np.concatenate([i, u])
    n = n_users + n_items
    deg = np.bincount(dst, minlength=n).astype(np.float32)
    g = hip_ops.CsrGraph.from_coo_host(np.stack([dst, src]), (np.float32(1.0) / deg[dst]).astype(np.float32), n, n, device)
    g.transpose()
    return g


def max_graph(inter_coo, n_users, n_items, device):
    """the structure of the same list, targets as rows, for `hip_ops.neighbor_max` (PyG `aggr='max'` on raw messages): both
    CSR forms and their permutations, built once"""
    u = torch.from_numpy(inter_coo.row.astype(np.int64))
    i = torch.from_numpy(inter_coo.col.astype(np.int64)) + n_users
    src, dst = torch.cat([u, i]).to(device), torch.cat([i, u]).to(device)
    n = n_users + n_items
    return hip_ops.DynGraph(dst, src, n, n)


def check_aggr_mode(aggr_mode, who):
    if aggr_mode not in AGGR_MODES:
        raise ValueError("%s: aggr_mode %r is not one of 'add', 'mean', 'max'" % (who, aggr_mode))
    return aggr_mode


def aggr_graph(aggr_mode, inter_coo, n_users, n_items, device, who):
    """the user-item graph in the form Base_gcn's aggregation wants (dualgnn.py:318-345, dragon.py:387-410)"""
    check_aggr_mode(aggr_mode, who)
    build = {'add': sym_norm_graph, 'mean': mean_graph, 'max': max_graph}[aggr_mode]
    return build(inter_coo, n_users, n_items, device)


def np_xavier_normal(*shape):
    """nn.init.xavier_normal_(torch.tensor(np.random.randn(*shape), dtype=float32)): the numpy draw is
    overwritten, but it advances the global numpy stream the epoch shuffles read from"""
    return nn.init.xavier_normal_(torch.tensor(np.random.randn(*shape), dtype=torch.float32))


class GCN(nn.Module):
    """reference GCN(dim_latent=64): preference table + 2-layer MLP, x + A x + A A x; `aggr_mode` is Base_gcn's aggregation
    and decides what `graph` is (`aggr_graph`): 'add' the D^-1/2 A D^-1/2 CSR, 'mean' the 1 / in-degree CSR, 'max' a DynGraph"""

    def __init__(self, num_user, dim_feat, dim_latent, aggr_mode='add'):
        super().__init__()
        self.aggr_mode = check_aggr_mode(aggr_mode, "GCN")
        self.last_arg = None         # 'max': the (detached) argmax of the two hops of the last forward, for tests and debugging
        self.preference = nn.Parameter(np_xavier_normal(num_user, dim_latent))
        self.MLP = nn.Linear(dim_feat, 4 * dim_latent)
        self.MLP_1 = nn.Linear(4 * dim_latent, dim_latent)

    def forward(self, graph, features):
        temp = _lin64(self.MLP_1, F.leaky_relu(_lin64(self.MLP, features)))
        x = F.normalize(torch.cat((self.preference, temp), dim=0))
        if self.aggr_mode == 'max':
            h, a1 = hip_ops.neighbor_max(x, graph)
            h_1, a2 = hip_ops.neighbor_max(h, graph)
            self.last_arg = (a1.detach(), a2.detach())
            return h + x + h_1, self.preference
        return hip_ops.lightgcn_mean(graph, x, 2) * 3.0, self.preference     # h + x + h_1


class UserGraphMixin:
    """What DualGNN and DRAGON share.  `user_graph_dict.npy` -> per-epoch [U, U] CSR with k entries per row (topk_sample, dualgnn.py:199-243)."""

    def load_user_graph(self, config, k):
        path = os.path.join(os.path.abspath(config['data_path'] + config['dataset']), config['user_graph_dict_file'])
        if not os.path.exists(path):
            raise FileNotFoundError(path + ": build it with tools/gen_user_graph.py -d " + str(config['dataset']))
        d = np.load(path, allow_pickle=True).item()
        if len(d) != self.n_users:
            raise ValueError("user_graph_dict has %d users, the dataset %d" % (len(d), self.n_users))
        self.k = k
        self._ug_ids, self._ug_cnt, self._ug_len = pack_user_graph_dict(d, k)

    def topk_sample(self, k):
        """-> (ids int64 [U, k], weights float32 [U, k]).  Rows with fewer than k neighbours are padded by
        resampling what they have, one `np.random.randint` per slot in the reference's order; users without
        neighbours get all-zero rows."""
        ids, cnt, length = self._ug_ids.copy(), self._ug_cnt.copy(), self._ug_len
        for u in np.nonzero((length > 0) & (length < k))[0]:
            for m in range(int(length[u]), k):
                r = np.random.randint(0, m)
                ids[u, m], cnt[u, m] = ids[u, r], cnt[u, r]
        w = torch.softmax(torch.from_numpy(cnt), dim=1)
        w[torch.from_numpy(length == 0)] = 0.0
        return ids, w.numpy()

    def pre_epoch_processing(self):
        ids, w = self.topk_sample(self.k)
        self.epoch_user_graph, self.user_weight_matrix = ids, torch.from_numpy(w).to(self.device)
        keep = np.repeat(self._ug_len > 0, self.k)
        rows = np.repeat(np.arange(self.n_users, dtype=np.int32), self.k)[keep]
        dev = self.device
        rows, cols = torch.from_numpy(rows).to(dev), torch.from_numpy(ids.reshape(-1)[keep].astype(np.int32)).to(dev)
        vals = torch.from_numpy(w.reshape(-1)[keep]).to(dev)
        # forward and transposed CSR by the device sort (stable: a row keeps its neighbour order), once per epoch
        self.user_csr = hip_ops.CsrGraph.from_coo_device(rows, cols, vals, self.n_users, self.n_users)
        t = hip_ops.CsrGraph.from_coo_device(cols, rows, vals, self.n_users, self.n_users)
        self.user_csr._t, t._t = t, self.user_csr

    # ---- shared by DualGNN and DRAGON
    def _apply(self, fn, *a, **k):
        out = super()._apply(fn, *a, **k)
        self.result_embed = fn(self.result_embed)
        return out

    def _modal(self):
        v_rep = t_rep = None
        if self.v_feat is not None:
            v_rep, self.v_preference = self.v_gcn(self.graph, self.v_feat)
        if self.t_feat is not None:
            t_rep, self.t_preference = self.t_gcn(self.graph, self.t_feat)
        return v_rep, t_rep

    def eval_embeddings(self):
        res = self.result_embed
        return res[:self.n_users], res[self.n_users:]

    def _bpr_and_pref_reg(self, result, interaction):
        users = interaction[0]
        pos, neg = interaction[1] + self.n_users, interaction[2] + self.n_users
        # -mean log2 sigmoid(pos - neg)
        loss = hip_ops.bpr_loss(result, result, users, pos, neg, hip_ops.BPR_LOGSIG, 'mean') / math.log(2.0)
        denom = float(users.numel() * self.dim_latent)
        reg = 0.0
        if self.v_preference is not None:
            reg = reg + hip_ops.gather_sqnorm(self.v_preference, users) / denom
        if self.t_preference is not None:
            reg = reg + hip_ops.gather_sqnorm(self.t_preference, users) / denom
        return loss, reg


class DualGNN(UserGraphMixin, FusedEvalMixin, GeneralRecommender):
    def __init__(self, config, dataset):
        super().__init__(config, dataset)
        dim_x = config['embedding_size']
        self.num_user, self.num_item = self.n_users, self.n_items
        self.aggr_mode = check_aggr_mode(config['aggr_mode'], "DualGNN")
        self.construction = 'weighted_sum'
        self.reg_weight = config['reg_weight']
        self.drop_rate = 0.1
        self.dim_latent = 64
        self.MLP_v = nn.Linear(self.dim_latent, self.dim_latent, bias=False)
        self.MLP_t = nn.Linear(self.dim_latent, self.dim_latent, bias=False)
        self.load_user_graph(config, 40)
        inter = dataset.inter_matrix(form='coo').astype(np.float32)
        self.graph = aggr_graph(self.aggr_mode, inter, self.n_users, self.n_items, self.device, "DualGNN")
        self.weight_u = nn.Parameter(np_xavier_normal(self.n_users, 2, 1))
        self.weight_u.data = F.softmax(self.weight_u.data, dim=1)
        self.weight_i = nn.Parameter(np_xavier_normal(self.n_items, 2, 1))
        self.weight_i.data = F.softmax(self.weight_i.data, dim=1)
        np.random.choice(self.n_items, int(self.n_items * self.drop_rate), replace=False)   # the unused item drop
        self.MLP_user = nn.Linear(self.dim_latent * 3, self.dim_latent)
        self.v_preference = self.t_preference = None
        if self.v_feat is not None:
            self.v_gcn = GCN(self.n_users, self.v_feat.size(1), self.dim_latent, self.aggr_mode)
        if self.t_feat is not None:
            self.t_gcn = GCN(self.n_users, self.t_feat.size(1), self.dim_latent, self.aggr_mode)
        # float64 in the reference, and only ever read if evaluation precedes the first training step
        self.result_embed = nn.init.xavier_normal_(
            torch.tensor(np.random.randn(self.n_users + self.n_items, dim_x))).float().to(self.device)

    def forward(self):
        v_rep, t_rep = self._modal()
        U = self.n_users
        if v_rep is not None and t_rep is not None:
            rep = v_rep + t_rep                       # the in-place sum: it IS the v_rep the fusion sees
            user_rep = rep[:U] * self.weight_u[:, 0] + t_rep[:U] * self.weight_u[:, 1]
        else:
            rep = v_rep if v_rep is not None else t_rep
            user_rep = rep[:U]
        user_rep = hip_ops.spmm(self.user_csr, user_rep.contiguous(), user_rep)      # user_rep + h_u1
        result = torch.cat((user_rep, rep[U:]), dim=0)
        self.result_embed = result.detach()
        return result

    def calculate_loss(self, interaction):
        loss, reg = self._bpr_and_pref_reg(self.forward(), interaction)
        reg = reg + (self.weight_u ** 2).mean() + (self.weight_i ** 2).mean()
        return loss + self.reg_weight * reg
