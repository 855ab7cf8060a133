"""MVGAE on the HIP hot path (reference: models/mvgae.py, which needs torch_geometric).

Three variational graph encoders (image, text, collaborative) of the same shape: features -> 128 -> row-normalise with
a user preference table -> `n_layers` graph convolutions -> a mean head and a log-variance head; the modal posteriors
are merged by a product of experts, then merged again with the collaborative posterior.  A convolution is
x W -> MEAN over the neighbours and the node itself (PyG MessagePassing(aggr='mean') with self loops) -> + bias ->
row-normalise -> dropout.  The mean aggregation is the HIP CSR SpMM with values 1/(deg + 1) over
cat(edges, flipped edges, self loops) -- 64 columns per call; its backward uses the transposed CSR.  The 64-output
Linears run on the fp32 MFMA projection kernels.

The reconstruction term compares each user with the HARDEST of the batch's negatives: the reference materialises a
[B, B, 64] tensor for that (1 GiB at B = 2048); here it is the [B, B] product of the two gathered blocks followed by a
row maximum -- the same values and the same (argmax-routed) gradient.

Reference quirks kept on purpose:
  * `preference` (per encoder) and `collaborative` are plain tensors, not Parameters: never trained, never saved;
  * the positive edge is decoded as z[user] . z[pos_item] WITHOUT the item offset, and the negatives likewise index
    z by raw item id (mvgae.py:84-86,164-170) -- i.e. mostly user rows of z;
  * linear_layer1 / linear_layer2 feed an `x_hat` that is dropped when `concate` is False: they exist (and are saved)
    but receive no gradient;
  * evaluation scores with sigmoid(mu) of the LAST training forward.

Everything after the three encoders -- two products of experts, four reparametrisations, four KL terms, four full-table
sigmoids and sigmoid(mu) for the evaluation table -- is, by default, a composition of about 140 element-wise launches
over [users + items, 64] temporaries, mirrored by autograd.  With the config key `fused_posterior: True` (absent /
False: that path, untouched) `calculate_loss` makes one `hip_ops.posterior_fusion` call (csrc/posterior.hip: two
launches forward, one backward, every intermediate recomputed) for the four z tables, the four KL terms and
`result_embed`; the four noise tables are drawn in the composition's order (pd, v, t, c); and the four reconstruction
terms become one batched term: the 3 B rows of cat(user, pos, neg) are gathered from the four z tables FIRST, the sigmoid
runs on those [4, 3 B, 64] rows only, then one bmm and one row maximum.  The loss is the same sum.

With the config key `fused_heads: True` (absent / False: the four lines at the end of `GCN.forward`, untouched; independent of
`fused_posterior`) every encoder ends with ONE aggregation AX = spmm(graph, x) for both heads -- the aggregation is linear, so
spmm(graph, x W) = AX W -- and one `hip_ops.encoder_heads` call (csrc/encoder_heads.hip: one launch forward, two backward) for
the two normalised convolutions, their dropouts (two masks drawn in the composition's order, mu then logvar), the four
leaky-ReLUs and the four 64 x 64 Linears.  The trunk convolutions stay as they are: conv_embed_1 is 128 wide.

With the config key `fused_recon: True` (absent / False: `recon_loss` and the batched lines of `_fused_loss`, untouched;
independent of the other two keys) the reconstruction terms are `hip_ops.hardest_negative_loss` (csrc/hardest_neg.hip: three
launches forward, one backward and the sorted row scatter): with `fused_posterior` on, ONE call on the stacked z [4, N, 64];
with it off, four calls on z.unsqueeze(0).  No squashed table, no gathered rows, no [B, B] block; the maximum's gradient goes
to the LOWEST position that attains it.
"""
import math

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from mmrec_amd import hip_ops
from mmrec_amd.models._base import FusedEvalMixin, GeneralRecommender
from mmrec_amd.models.mmgcn import _lin64

MAX_LOGVAR = 10


def self_loop_mean_graph(inter_coo, n_users, n_items, device):
    """rows = message targets; values 1 / (in-degree incl. the self loop)"""
    u = inter_coo.row.astype(np.int64)
    i = inter_coo.col.astype(np.int64) + n_users
    n = n_users + n_items
    loop = np.arange(n, dtype=np.int64)
    dst, src = np.concatenate([i, u, loop]), np.concatenate([u, i, loop])
    deg = np.bincount(dst, minlength=n).astype(np.float32)
    g = hip_ops.CsrGraph.from_coo_host(np.stack([dst, src]), (1.0 / deg)[dst].astype(np.float32), n, n, device)
    g.transpose()
    return g


class BaseModel(nn.Module):
    """x W, mean aggregation, + bias, row-normalise, dropout(0.1)"""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.in_channels = in_channels
        self.weight = nn.Parameter(torch.empty(in_channels, out_channels))
        self.bias = nn.Parameter(torch.empty(out_channels))
        bound = 1.0 / math.sqrt(in_channels)
        self.weight.data.uniform_(-bound, bound)
        self.bias.data.uniform_(-bound, bound)

    def forward(self, x, graph):
        if self.weight.shape[1] == hip_ops.EMB_DIM and self.in_channels % 4 == 0:
            xw = hip_ops.linear(x.contiguous(), self.weight.t().contiguous(), None)
        else:
            xw = torch.matmul(x, self.weight)
        out = F.normalize(hip_ops.spmm(graph, xw) + self.bias, p=2, dim=-1)
        return F.dropout(out, p=0.1, training=self.training)


class GCN(nn.Module):
    def __init__(self, features, num_user, dim_id, num_layer, dim_latent, device, fused_heads=False):
        super().__init__()
        self.features, self.num_layer, self.fused_heads = features, num_layer, fused_heads
        self.preference = nn.init.xavier_normal_(torch.rand((num_user, dim_latent))).to(device)    # not a Parameter
        self.MLP = nn.Linear(features.size(1), dim_latent)
        nn.init.xavier_normal_(self.MLP.weight)
        self.conv_embed_1 = BaseModel(dim_latent, dim_id)
        nn.init.xavier_normal_(self.conv_embed_1.weight)
        self.linear_layer1 = nn.Linear(dim_latent, dim_id)
        nn.init.xavier_normal_(self.linear_layer1.weight)
        self.g_layer1 = nn.Linear(dim_id, dim_id)
        nn.init.xavier_normal_(self.g_layer1.weight)
        self.conv_embed_2 = BaseModel(dim_id, dim_id)
        nn.init.xavier_normal_(self.conv_embed_2.weight)
        self.linear_layer2 = nn.Linear(dim_id, dim_id)
        nn.init.xavier_normal_(self.linear_layer2.weight)
        self.g_layer2 = nn.Linear(dim_id, dim_id)                      # (left at its default init by the reference)
        for j in (4, 5):                                               # (creation order = the reference's RNG order)
            conv = BaseModel(dim_id, dim_id)
            nn.init.xavier_normal_(conv.weight)
            lin = nn.Linear(dim_id, dim_id)
            nn.init.xavier_normal_(lin.weight)
            gl = nn.Linear(dim_id, dim_id)
            nn.init.xavier_normal_(gl.weight)
            setattr(self, 'conv_embed_%d' % j, conv)
            setattr(self, 'linear_layer%d' % j, lin)
            setattr(self, 'g_layer%d' % j, gl)

    def forward(self, graph):
        x = F.normalize(torch.cat((self.preference, self.MLP(self.features)), dim=0))
        if self.num_layer > 0:
            x = F.leaky_relu(_lin64(self.g_layer1, F.leaky_relu(self.conv_embed_1(x, graph))))
        if self.num_layer > 1:
            x = F.leaky_relu(_lin64(self.g_layer2, F.leaky_relu(self.conv_embed_2(x, graph))))
        if self.fused_heads:
            return self._fused_heads(x.contiguous(), graph)
        mu = F.leaky_relu(self.conv_embed_4(x, graph))
        mu = _lin64(self.g_layer4, mu) + F.leaky_relu(_lin64(self.linear_layer4, x))
        logvar = F.leaky_relu(self.conv_embed_5(x, graph))
        logvar = _lin64(self.g_layer5, logvar) + F.leaky_relu(_lin64(self.linear_layer5, x))
        return mu, logvar

    def _fused_heads(self, x, graph):
        """the four lines below it in `forward` with the `fused_heads` key on: one aggregation for both heads, then one op"""
        ax = hip_ops.spmm(graph, x)
        scale = None
        if self.training:                                              # the composition's call order: mu, then logvar
            scale = torch.stack([F.dropout(torch.ones_like(ax), p=0.1, training=True) for _ in range(2)])
        heads = [(getattr(self, 'conv_embed_%d' % j), getattr(self, 'g_layer%d' % j), getattr(self, 'linear_layer%d' % j))
                 for j in (4, 5)]
        stack = lambda ts: torch.stack(list(ts))                       # noqa: E731
        out = hip_ops.encoder_heads(ax, x, stack(c.weight for c, _, _ in heads), stack(c.bias for c, _, _ in heads),
                                    stack(g.weight for _, g, _ in heads), stack(g.bias for _, g, _ in heads),
                                    stack(l.weight for _, _, l in heads), stack(l.bias for _, _, l in heads), scale)
        return out[0], out[1]


def product_of_experts(mu, logvar, eps=1e-8):
    T = 1.0 / (torch.exp(logvar) + eps)
    pd_var = 1.0 / torch.sum(T, dim=0)
    return torch.sum(mu * T, dim=0) * pd_var, torch.log(pd_var)


class MVGAE(FusedEvalMixin, GeneralRecommender):
    graph_capturable = False      # dropout masks and reparametrisation noise are drawn inside the step

    def __init__(self, config, dataset):
        super().__init__(config, dataset)
        self.num_user, self.num_item = self.n_users, self.n_items
        self.dim_x = config['embedding_size']
        self.beta = config['beta']
        self.fused_posterior = bool(config['fused_posterior']) if 'fused_posterior' in config else False    # new key, default off
        self.fused_heads = bool(config['fused_heads']) if 'fused_heads' in config else False                # new key, default off
        self.fused_recon = bool(config['fused_recon']) if 'fused_recon' in config else False                # new key, default off
        num_layer = config['n_layers']
        if self.v_feat is None or self.t_feat is None:
            raise ValueError("MVGAE needs image and text features (its forward reads both encoders)")
        self.collaborative = nn.init.xavier_normal_(torch.rand((self.n_items, self.dim_x))).to(self.device)
        inter = dataset.inter_matrix(form='coo').astype(np.float32)
        self.graph = self_loop_mean_graph(inter, self.n_users, self.n_items, self.device)
        self.v_gcn = GCN(self.v_feat, self.n_users, self.dim_x, num_layer, 128, self.device, self.fused_heads)
        self.t_gcn = GCN(self.t_feat, self.n_users, self.dim_x, num_layer, 128, self.device, self.fused_heads)
        self.c_gcn = GCN(self.collaborative, self.n_users, self.dim_x, num_layer, 128, self.device, self.fused_heads)
        n = self.n_users + self.n_items
        self.result_embed = nn.init.xavier_normal_(torch.rand((n, self.dim_x))).to(self.device)

    def _apply(self, fn, *a, **k):
        out = super()._apply(fn, *a, **k)
        self.collaborative, self.result_embed = fn(self.collaborative), fn(self.result_embed)
        self.c_gcn.features = self.collaborative
        for gcn in (self.v_gcn, self.t_gcn, self.c_gcn):
            gcn.preference = fn(gcn.preference)
        return out

    def reparametrize(self, mu, logvar):
        logvar = logvar.clamp(max=MAX_LOGVAR)
        if self.training:
            return mu + torch.randn_like(logvar) * 0.1 * torch.exp(logvar.mul(0.5))
        return mu

    def forward(self):
        v_mu, v_logvar = self.v_gcn(self.graph)
        t_mu, t_logvar = self.t_gcn(self.graph)
        c_mu, c_logvar = self.c_gcn(self.graph)
        pd_mu, pd_logvar = product_of_experts(torch.stack([v_mu, t_mu]), torch.stack([v_logvar, t_logvar]))
        pd_mu, pd_logvar = product_of_experts(torch.stack([pd_mu, c_mu]), torch.stack([pd_logvar, c_logvar]))
        z = self.reparametrize(pd_mu, pd_logvar)
        self.result_embed = torch.sigmoid(pd_mu).detach()
        return pd_mu, pd_logvar, z, v_mu, v_logvar, t_mu, t_logvar, c_mu, c_logvar

    def eval_embeddings(self):
        return self.result_embed[:self.n_users], self.result_embed[self.n_users:]

    def recon_loss(self, z, user, pos_items, neg_items):
        z = torch.sigmoid(z)
        zu = z[user]
        pos = torch.sigmoid((zu * z[pos_items]).sum(dim=1))
        hardest = torch.mm(zu, z[neg_items].t()).max(dim=-1).values          # == max_j <z[user_b], z[neg_j]>
        return -torch.sum(torch.log2(torch.sigmoid(pos - torch.sigmoid(hardest))))

    def _fused_recon_loss(self, z, user, pos_items, neg_items):
        """recon_loss with the `fused_recon` key on: one latent of the op"""
        return hip_ops.hardest_negative_loss(z.unsqueeze(0), user, pos_items, neg_items)[0]

    def kl_loss(self, mu, logvar):
        logvar = logvar.clamp(max=MAX_LOGVAR)
        return -0.5 * torch.mean(torch.sum(1 + logvar - mu ** 2 - logvar.exp(), dim=1))

    def _fused_loss(self, user, pos_items, neg_items):
        """calculate_loss with the `fused_posterior` key on: the same sum, the posterior tail as one op"""
        v_mu, v_logvar = self.v_gcn(self.graph)
        t_mu, t_logvar = self.t_gcn(self.graph)
        c_mu, c_logvar = self.c_gcn(self.graph)
        ops = [t.contiguous() for t in (v_mu, v_logvar, t_mu, t_logvar, c_mu, c_logvar)]
        noise = [torch.randn_like(ops[1]) for _ in range(4)] if self.training else None     # the composition's order: pd, v, t, c
        z, kl, self.result_embed = hip_ops.posterior_fusion(*ops, noise)
        if self.fused_recon:                                          # the four reconstruction terms: one call, no [4, 3 B, 64] rows
            return hip_ops.hardest_negative_loss(z, user, pos_items, neg_items).sum() + self.beta * kl.sum()
        b = user.shape[0]
        rows = torch.sigmoid(z.index_select(1, torch.cat((user, pos_items, neg_items))))    # [4, 3 B, 64]
        zu, zp, zn = rows[:, :b], rows[:, b:2 * b], rows[:, 2 * b:]
        pos = torch.sigmoid((zu * zp).sum(dim=2))
        hardest = torch.bmm(zu, zn.transpose(1, 2)).max(dim=-1).values                      # [4, B]
        recon = -torch.sum(torch.log2(torch.sigmoid(pos - torch.sigmoid(hardest))))
        return recon + self.beta * kl.sum()

    def calculate_loss(self, interaction):
        user, pos_items, neg_items = interaction[0], interaction[1], interaction[2]
        if self.fused_posterior:
            return self._fused_loss(user, pos_items, neg_items)
        pd_mu, pd_logvar, z, v_mu, v_logvar, t_mu, t_logvar, c_mu, c_logvar = self.forward()
        z_v = self.reparametrize(v_mu, v_logvar)
        z_t = self.reparametrize(t_mu, t_logvar)
        z_c = self.reparametrize(c_mu, c_logvar)
        recon_loss = self._fused_recon_loss if self.fused_recon else self.recon_loss
        loss = recon_loss(z, user, pos_items, neg_items) + self.beta * self.kl_loss(pd_mu, pd_logvar)
        for zz, mu, lv in ((z_v, v_mu, v_logvar), (z_t, t_mu, t_logvar), (z_c, c_mu, c_logvar)):
            loss = loss + recon_loss(zz, user, pos_items, neg_items) + self.beta * self.kl_loss(mu, lv)
        return loss
