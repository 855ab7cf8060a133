"""DAMRS on the HIP hot path (reference: models/damrs.py).

LightGCN over the user-item graph plus three frozen item-item graphs -- text kNN, image kNN (both restricted to
pairs that are above the mean similarity in BOTH modalities) and a "session" graph read from
`item_graph_dict_file` -- each propagating the item id embeddings.  Every propagation is the HIP CSR SpMM (fused
layer mean for LightGCN); evaluation is the fused score + mask + top-K.  The pseudo-label machinery of the loss
(row softmaxes / top-10 over [batch items, all items] similarity blocks, the neighbour-discrimination and KL terms,
the confidence-weighted BPR) is dense row-wise work on those blocks and stays in torch; the positive scores of the
discrimination term are read out of the similarity block instead of being re-computed from a gathered [b, 10, 64]
tensor.  With the config key `fused_labels: True` (absent / False: that path, untouched) the neighbour term holds no
[b, I] block: the labels come from `hip_ops.pseudo_labels` (csrc/tri_topk.hip: one sweep over the three tables for the
three mixed top-10 lists, the second lists out of the top-20 cosines), the row totals from `hip_ops.score_lse` and the
twenty positive cosines per row from `hip_ops.edge_dot`; the KL term's [users, items] blocks stay.  With `fused_kl: True`
(absent / False: the composition, untouched) they go too: the KL term is `hip_ops.mutual_kl` (csrc/mutual_kl.hip: the two
divergences collapse to (p_g - p_m)(logit p_g - logit p_m), swept on the fp32 MFMA, forward and backward) on the gathered user
rows and the two row-normalised item gathers; with both keys on the loss holds no two-dimensional block.  The composition is
NaN once a logit saturates fp32's sigmoid; the collapsed form stays finite.

Reference behaviour kept: image_trs / text_trs exist (and are saved) but take no part in anything; the weights stored
in the item-graph file are ignored (a 0/1 adjacency is normalised); items missing from the file keep only their self
loop.  `torch.unique(sorted=False)` orders differently on CPU and device in the reference; the loss does not depend
on that order, a sorted unique is used here.
"""
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from mmrec_amd import hip_ops
from mmrec_amd.graph import norm_adj_graph
from mmrec_amd.models._base import FusedEvalMixin, GeneralRecommender


def sym_normalised_graph(rows, cols, n, device):
    """compute_normalized_laplacian (damrs.py:108-115): 0/1 entries scaled by rowsum^-1/2 at both ends"""
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    deg = np.float32(1e-7) + np.bincount(rows, minlength=n).astype(np.float32)
    dis = np.power(deg, np.float32(-0.5)).astype(np.float32)
    g = hip_ops.CsrGraph.from_coo_host(np.stack([rows, cols]), (dis[rows] * dis[cols]).astype(np.float32), n, n, device)
    g.transpose()
    return g


def mutual_knn_edges(v_feat, t_feat, knn_k, block=2048):
    """-> (rows, image neighbours, text neighbours) as host arrays (damrs.py:58-104).  Similarities below the global
    mean of EITHER modality are zeroed in both; an item keeps min(knn_k, #surviving pairs) neighbours per modality."""
    vn = v_feat / torch.norm(v_feat, p=2, dim=-1, keepdim=True)
    tn = t_feat / torch.norm(t_feat, p=2, dim=-1, keepdim=True)
    n = vn.shape[0]
    # global means of the two similarity matrices without holding them: sum_ij <a_i, a_j> = |sum_i a_i|^2
    v_mean = (vn.sum(0).double() ** 2).sum() / float(n * n)
    t_mean = (tn.sum(0).double() ** 2).sum() / float(n * n)
    k = min(knn_k, n)
    rows, v_ind, t_ind = [], [], []
    for r0 in range(0, n, block):
        v_sim, t_sim = vn[r0:r0 + block] @ vn.t(), tn[r0:r0 + block] @ tn.t()
        drop = (v_sim < v_mean) | (t_sim < t_mean)
        v_sim, t_sim = v_sim.masked_fill(drop, 0.0), t_sim.masked_fill(drop, 0.0)
        keep = torch.clamp((t_sim != 0).sum(1), max=k)                       # neighbours kept per item
        sel = torch.arange(k, device=keep.device)[None, :] < keep[:, None]
        rows.append((torch.arange(r0, r0 + v_sim.shape[0], device=keep.device)[:, None].expand(-1, k))[sel])
        v_ind.append(torch.topk(v_sim, k, dim=-1).indices[sel])
        t_ind.append(torch.topk(t_sim, k, dim=-1).indices[sel])
    cat = lambda xs: torch.cat(xs).cpu().numpy()                              # noqa: E731
    return cat(rows), cat(v_ind), cat(t_ind)


class DAMRS(FusedEvalMixin, GeneralRecommender):
    graph_capturable = False      # torch.unique of the batch ids: data-dependent shapes inside the step

    def __init__(self, config, dataset):
        super().__init__(config, dataset)
        self.embedding_dim = config['embedding_size']
        self.knn_k = config['knn_k']
        self.n_layers = config['n_mm_layers']
        self.n_ui_layers = config['n_ui_layers']
        self.reg_weight = config['reg_weight']
        self.kl_weight = config['kl_weight']
        self.neighbor_weight = config['neighbor_weight']
        self.n_nodes = self.n_users + self.n_items
        if self.v_feat is None or self.t_feat is None:
            raise ValueError("DAMRS needs image and text features (both kNN graphs are built in its constructor)")
        self.interaction_matrix = dataset.inter_matrix(form='coo').astype(np.float32)
        self.norm_adj = norm_adj_graph(self.interaction_matrix, self.n_users, self.n_items, self.device)
        self.user_embedding = nn.Embedding(self.n_users, self.embedding_dim)
        self.item_id_embedding = nn.Embedding(self.n_items, self.embedding_dim)
        nn.init.xavier_uniform_(self.user_embedding.weight)
        nn.init.xavier_uniform_(self.item_id_embedding.weight)
        self.image_embedding = nn.Embedding.from_pretrained(self.v_feat, freeze=True)
        self.image_trs = nn.Linear(self.v_feat.shape[1], self.embedding_dim)
        self.text_embedding = nn.Embedding.from_pretrained(self.t_feat, freeze=True)
        self.text_trs = nn.Linear(self.t_feat.shape[1], self.embedding_dim)
        rows, v_nb, t_nb = mutual_knn_edges(self.v_feat, self.t_feat, self.knn_k)
        self.image_adj = sym_normalised_graph(rows, v_nb, self.n_items, self.device)
        self.text_adj = sym_normalised_graph(rows, t_nb, self.n_items, self.device)
        path = os.path.join(os.path.abspath(config['data_path'] + config['dataset']), config['item_graph_dict_file'])
        item_graph = np.load(path, allow_pickle=True).item()
        s_rows, s_cols = [np.arange(self.n_items, dtype=np.int64)], [np.arange(self.n_items, dtype=np.int64)]
        for i in range(self.n_items):
            if i in item_graph:
                nb = np.asarray(item_graph[i][0], dtype=np.int64)
                s_rows.append(np.full(nb.shape[0], i, dtype=np.int64))
                s_cols.append(nb)
        self.session_adj = sym_normalised_graph(np.concatenate(s_rows), np.concatenate(s_cols), self.n_items, self.device)
        self.fused_labels = bool(config['fused_labels']) if 'fused_labels' in config else False    # new key, default off
        self.fused_kl = bool(config['fused_kl']) if 'fused_kl' in config else False                # new key, default off

    # ---- propagation
    def _item_graph(self, graph):
        h = self.item_id_embedding.weight
        for _ in range(self.n_layers):
            h = hip_ops.spmm(graph, h)
        return h

    def forward(self):
        ego = torch.cat((self.user_embedding.weight, self.item_id_embedding.weight), dim=0)
        out = hip_ops.lightgcn_mean(self.norm_adj, ego, self.n_ui_layers)
        return (out[:self.n_users], out[self.n_users:], self._item_graph(self.text_adj),
                self._item_graph(self.image_adj), self._item_graph(self.session_adj))

    def eval_embeddings(self):
        u, i, h_t, h_v, h_s = self.forward()
        return u, i + (h_v + h_t + h_s) / 3.0

    # ---- loss pieces (dense [batch items, all items] blocks)
    @staticmethod
    def _cosine_block(emb, aug):
        return torch.mm(F.normalize(emb, dim=1), F.normalize(aug, dim=1).t())

    @staticmethod
    def _pseudo_labels(p1, p2, p3):
        mm_pos = torch.topk(p1 + p2 + p3 + p3, 10, dim=-1).indices
        single_pos = torch.topk(p3.scatter(1, mm_pos, 0.0), 10, dim=-1).indices
        return mm_pos, single_pos

    @staticmethod
    def _neighbour_discrimination(mm_pos, s_pos, cos, temperature=0.2):
        e = torch.exp(cos / temperature)
        mm, s, ttl = e.gather(1, mm_pos).sum(1), e.gather(1, s_pos).sum(1), e.sum(1)
        return torch.mean(-torch.log(mm / ttl + 10e-10) - torch.log(s / (ttl - mm) + 10e-10))

    @staticmethod
    def _kl(p1, p2):
        return p1 * torch.log(p1) - p1 * torch.log(p2) + (1 - p1) * torch.log(1 - p1) - (1 - p1) * torch.log(1 - p2)

    def _kl_term(self, n_u, items_g, items_m):
        """the symmetric KL between the user-item probabilities of the graph view and of the modal view; `fused_kl`: no
        [users, items] block (hip_ops.mutual_kl on the row-normalised gathers)"""
        if self.fused_kl:
            return hip_ops.mutual_kl(n_u, hip_ops.row_normalize(items_g), hip_ops.row_normalize(items_m))
        p_g = torch.sigmoid(torch.mm(n_u, F.normalize(items_g, dim=-1).t()))
        p_m = torch.sigmoid(torch.mm(n_u, F.normalize(items_m, dim=-1).t()))
        return torch.mean(self._kl(p_g, p_m) + self._kl(p_m, p_g))

    @staticmethod
    def _modal_weights(u, h_t, h_v, h_s, pos_items, neg_items):
        with torch.no_grad():
            def probs(items):
                return torch.sigmoid(torch.stack([(u * F.normalize(h[items], dim=-1)).sum(1) for h in (h_t, h_s, h_v)]))
            p, n_mean = probs(pos_items), probs(neg_items).mean()
            p_mean = p.mean(0)
            pos_w = torch.clamp(p_mean * torch.exp(-torch.var(p, dim=0)) ** 2, 0, 1)
            neg_w = torch.clamp((p.max(0).values - n_mean) * (p_mean < n_mean).to(p.dtype), 0, 1)
        return pos_w, neg_w

    def _neighbour_fused(self, i_id, tables, k=10, temperature=0.2):
        """the neighbour-discrimination term of the three modalities without a [b, I] block: labels from
        hip_ops.pseudo_labels, log of the row total by score_lse, the 2 k positive cosines per row by edge_dot"""
        hn = [hip_ops.row_normalize(h) for h in tables]
        mm_pos, s_pos = hip_ops.pseudo_labels([x.detach() for x in hn], i_id, k)
        rows = i_id.repeat_interleave(2 * k)
        total = 0.0
        for m, x in enumerate(hn):
            log_ttl = hip_ops.score_lse(x[i_id], x, 1.0 / temperature)
            cols = torch.cat((mm_pos[m], s_pos[m]), dim=1).reshape(-1)
            e = torch.exp(hip_ops.edge_dot(x, x, rows, cols).view(-1, 2 * k) / temperature)
            mm, s, ttl = e[:, :k].sum(1), e[:, k:].sum(1), torch.exp(log_ttl)
            total = total + torch.mean(-torch.log(mm / ttl + 10e-10) - torch.log(s / (ttl - mm) + 10e-10))
        return total / 3.0

    def _calculate_loss_fused(self, interaction):
        """calculate_loss with `fused_labels`: only the neighbour term differs, the KL and BPR terms are those below"""
        users, pos_items, neg_items = interaction[0], interaction[1], interaction[2]
        user_emb, item_emb, h_t, h_v, h_s = self.forward()
        u_id = torch.unique(users)
        i_id = torch.unique(torch.cat((pos_items, neg_items)))
        neighbour = self._neighbour_fused(i_id, (h_t, h_v, h_s))
        n_u = user_emb[u_id]
        it_emb = (h_t + h_s + h_v) / 3.0
        kl = self._kl_term(n_u, item_emb[i_id], it_emb[i_id])
        u = user_emb[users]
        pos_w, neg_w = self._modal_weights(u, h_t, h_v, h_s, pos_items, neg_items)
        ia = item_emb + (h_t + h_v + h_s) / 3.0
        diff = (u * ia[pos_items]).sum(1) - (u * ia[neg_items]).sum(1)
        mf = -torch.mean(torch.log(torch.sigmoid(diff)) * pos_w + torch.log(torch.sigmoid(-diff)) * neg_w)
        return mf + self.neighbor_weight * neighbour + kl * self.kl_weight

    def calculate_loss(self, interaction):
        if self.fused_labels:
            return self._calculate_loss_fused(interaction)
        users, pos_items, neg_items = interaction[0], interaction[1], interaction[2]
        user_emb, item_emb, h_t, h_v, h_s = self.forward()
        u_id = torch.unique(users)
        i_id = torch.unique(torch.cat((pos_items, neg_items)))
        cos_t, cos_v, cos_s = (self._cosine_block(h[i_id], h) for h in (h_t, h_v, h_s))
        with torch.no_grad():
            p_t, p_v, p_s = (F.softmax(c, dim=1) for c in (cos_t, cos_v, cos_s))
            labels_s = self._pseudo_labels(p_t, p_v, p_s)
            labels_v = self._pseudo_labels(p_t, p_s, p_v)
            labels_t = self._pseudo_labels(p_v, p_s, p_t)
        neighbour = (self._neighbour_discrimination(*labels_s, cos_s) + self._neighbour_discrimination(*labels_v, cos_v)
                     + self._neighbour_discrimination(*labels_t, cos_t)) / 3.0
        n_u = user_emb[u_id]
        it_emb = (h_t + h_s + h_v) / 3.0
        kl = self._kl_term(n_u, item_emb[i_id], it_emb[i_id])
        u = user_emb[users]
        pos_w, neg_w = self._modal_weights(u, h_t, h_v, h_s, pos_items, neg_items)
        ia = item_emb + (h_t + h_v + h_s) / 3.0
        diff = (u * ia[pos_items]).sum(1) - (u * ia[neg_items]).sum(1)
        mf = -torch.mean(torch.log(torch.sigmoid(diff)) * pos_w + torch.log(torch.sigmoid(-diff)) * neg_w)
        return mf + self.neighbor_weight * neighbour + kl * self.kl_weight
