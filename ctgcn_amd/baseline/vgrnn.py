"""VGRNN (variational graph recurrent network, https://arxiv.org/abs/1908.09710) with the constructor, forward signature and
state_dict keys of the reference's baseline/vgrnn.py (conv_type 'GCN'), so checkpoints move both ways.

What a GCNConv means, read from the reference: edge weights are ignored and every listed entry counts 1; a self loop of weight 2
(improved=True) is appended for every node on top of whatever the list holds; Â = D^-1/2 (P + 2 I) D^-1/2 with D the row sums of
P + 2 I; output row edge_index[0] gathers from edge_index[1].  Â is built once per snapshot as an ops.GcnAdj (coalesce, then the fp64
ops.gcn_normalize) and cached: the window is constant over the epochs.  The backward reads GcnAdj.transposed(), so the pattern need
not be symmetric.

The aggregation is linear, so the six convolutions of a graph-GRU step need two gathers (ops.ggru_gates, ops.ggru_blend,
ctgcn_vgrnn.hip), each finishing its rows in registers:
    [g_z | g_r | c] = Â (x [W_xz | W_xr | W_xh] + h [W_hz | W_hr | 0]) + biases,   z = σ(g_z),  q = σ(g_r) ⊙ h
    h̃ = tanh(c + Â (q W_hh)),   h' = z ⊙ h + (1 − z) ⊙ h̃
and enc_mean / enc_std, which read the same input over the same Â, one gather of width 2 · output_dim whose epilogue also forms
z = mean + noise ⊙ std (ops.vgrnn_heads); enc itself is ops.gcn_conv with its ReLU epilogue.  The decoder returns a
LazyInnerProduct holding z_t; metrics.VAELoss turns it into the loss with ops.vae_nll (ctgcn_vgrnn.hip), which never forms z zᵀ.
fused=False is the same model composed of stock torch ops: six sparse products a step and the dense [N, N] logits.

Departures from the reference, each on purpose: the initial h has N = the row count of x (the reference reads x.size(1), the same
number for its identity features); hx is detached on entry (Variable(hx) does not detach, so a second batch would back-propagate
through the first batch's freed graph); rnn_layer_num > 1 is the math as it reads (the reference's in-place h_out[i] fails in
autograd); 'SAGE' and 'GIN' are not built and raise NotImplementedError."""
import math

import torch
from torch import nn
from torch.nn import functional as F

from .. import layers, ops


def glorot(tensor):
    if tensor is not None:
        stdv = math.sqrt(6.0 / (tensor.size(0) + tensor.size(1)))
        tensor.data.uniform_(-stdv, stdv)


def zeros(tensor):
    if tensor is not None:
        tensor.data.fill_(0)


def _identity(x):
    return x


def gcn_conv_adjacency(edge_index, num_nodes, improved=True, long_threshold=None):
    """The GcnAdj of Â = D^-1/2 (P + w I) D^-1/2 for a [2, E] index tensor (w = 2 with improved); a GcnAdj is handed back as it is.
    Built once per index tensor and kept on that tensor, so it lives exactly as long as the tensor does (an in-place change of the
    tensor makes a new one)."""
    if isinstance(edge_index, ops.GcnAdj):
        if edge_index.n != num_nodes:
            raise ValueError("adjacency of %d rows for %d nodes" % (edge_index.n, num_nodes))
        return edge_index
    if not (isinstance(edge_index, torch.Tensor) and not edge_index.is_sparse and edge_index.dim() == 2 and edge_index.shape[0] == 2):
        raise TypeError("a [2, E] index tensor or a prepared GcnAdj expected")
    ops._need_cuda(edge_index)
    cache = edge_index.__dict__.setdefault("_gcn_conv_adjacency", {})
    key = (edge_index._version, int(num_nodes), bool(improved), long_threshold)
    hit = cache.get(key)
    if hit is None:
        cache.clear()                                               # an entry of an earlier version of the tensor is of no use
        dev = edge_index.device
        loops = torch.arange(num_nodes, device=dev, dtype=torch.int64)
        idx = torch.cat([edge_index.to(torch.int64), torch.stack((loops, loops))], dim=1)
        if edge_index.numel() and (int(edge_index.min()) < 0 or int(edge_index.max()) >= num_nodes):
            raise ValueError("edge index outside [0, %d)" % num_nodes)
        val = torch.cat([torch.ones(edge_index.shape[1], device=dev), torch.full((num_nodes,), 2.0 if improved else 1.0, device=dev)])
        pattern = torch.sparse_coo_tensor(idx, val, (num_nodes, num_nodes)).coalesce()      # row-major order, duplicates summed
        row_ptr = torch.zeros(num_nodes + 1, dtype=torch.int64, device=dev)
        row_ptr[1:] = torch.bincount(pattern.indices()[0], minlength=num_nodes).cumsum(0)
        row_ptr, col = row_ptr.to(torch.int32), pattern.indices()[1].to(torch.int32)
        adj = ops.GcnAdj(row_ptr, col, ops.gcn_normalize(row_ptr, col, pattern.values(), row_norm=False), long_threshold)
        hit = cache[key] = adj
    return hit


def _sparse(adj):
    """Â of a GcnAdj as a torch sparse tensor, for the composed path; kept on the GcnAdj"""
    t = getattr(adj, "_sparse_tensor", None)
    if t is None:
        t = adj._sparse_tensor = adj.to_sparse_tensor().coalesce()
    return t


def _cat_bias(*parts):
    return None if parts[0] is None else torch.cat(parts)


class GCNConv(nn.Module):
    def __init__(self, in_channels, out_channels, act=F.relu, improved=True, bias=False):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.improved = improved
        self.act = act
        self.weight = nn.Parameter(torch.empty(in_channels, out_channels))
        if bias:
            self.bias = nn.Parameter(torch.empty(out_channels))
        else:
            self.register_parameter('bias', None)
        self.reset_parameters()

    def reset_parameters(self):
        glorot(self.weight)
        zeros(self.bias)

    def forward(self, x, edge_index, edge_weight=None, fused=True):
        """act(Â (x W) + b); edge_weight is accepted and ignored, as the reference's callers never pass one"""
        ops._need_cuda(x)
        adj = gcn_conv_adjacency(edge_index, x.shape[0], self.improved)
        S = torch.matmul(x, self.weight)
        if not fused:
            out = torch.sparse.mm(_sparse(adj), S)
            return self.act(out if self.bias is None else out + self.bias)
        if self.act is F.relu:
            return ops.gcn_conv(S, adj, self.bias, ops.GCN_EPI_RELU)
        return self.act(ops.gcn_conv(S, adj, self.bias))

    def __repr__(self):
        return '{}({}, {})'.format(self.__class__.__name__, self.in_channels, self.out_channels)


class graph_gru_gcn(nn.Module):
    def __init__(self, input_size, hidden_size, n_layer, bias=True):
        super().__init__()
        self.hidden_size = hidden_size
        self.n_layer = n_layer
        for name in ('weight_xz', 'weight_hz', 'weight_xr', 'weight_hr', 'weight_xh', 'weight_hh'):
            setattr(self, name, nn.ModuleList())
        for i in range(n_layer):
            width = input_size if i == 0 else hidden_size
            for name in ('weight_xz', 'weight_xr', 'weight_xh'):
                getattr(self, name).append(GCNConv(width, hidden_size, act=_identity, bias=bias))
            for name in ('weight_hz', 'weight_hr', 'weight_hh'):
                getattr(self, name).append(GCNConv(hidden_size, hidden_size, act=_identity, bias=bias))

    def packed(self):
        """per layer ([W_xz | W_xr | W_xh], [W_hz | W_hr], the summed biases or None): what the fused step multiplies by, formed once per
        forward and shared by its snapshots"""
        out = []
        for i in range(self.n_layer):
            xz, xr, xh, hz, hr, hh = (m[i] for m in (self.weight_xz, self.weight_xr, self.weight_xh, self.weight_hz, self.weight_hr, self.weight_hh))
            bias = None if xz.bias is None else torch.cat([xz.bias + hz.bias, xr.bias + hr.bias, xh.bias + hh.bias])
            out.append((torch.cat([xz.weight, xr.weight, xh.weight], dim=1), torch.cat([hz.weight, hr.weight], dim=1), bias))
        return out

    def cell(self, i, x, h, adj, packed):
        """one layer's step in two gathers (see the module's docstring)"""
        w_x, w_h, bias = packed[i]
        U = torch.matmul(x, w_x)
        U[:, :2 * self.hidden_size].addmm_(h, w_h)                   # in place: no second N x 3H tensor
        z, q, c = ops.ggru_gates(U, h, adj, bias)
        return ops.ggru_blend(torch.matmul(q, self.weight_hh[i].weight), c, z, h, adj)

    def cell_composed(self, i, x, h, adj, packed=None):
        """the reference's six convolutions, in stock torch ops"""
        z = torch.sigmoid(self.weight_xz[i](x, adj, fused=False) + self.weight_hz[i](h, adj, fused=False))
        r = torch.sigmoid(self.weight_xr[i](x, adj, fused=False) + self.weight_hr[i](h, adj, fused=False))
        h_tilde = torch.tanh(self.weight_xh[i](x, adj, fused=False) + self.weight_hh[i](r * h, adj, fused=False))
        return z * h + (1 - z) * h_tilde

    def forward(self, inp, edgidx, h, fused=True, packed=None):
        ops._need_cuda(inp, h)
        adj = gcn_conv_adjacency(edgidx, inp.shape[0])
        step = self.cell if fused else self.cell_composed
        if fused and packed is None:
            packed = self.packed()
        outs = []
        for i in range(self.n_layer):
            outs.append(step(i, inp if i == 0 else outs[i - 1], h[i], adj, packed))
        h_out = torch.stack(outs, dim=0)
        return h_out, h_out


class InnerProductDecoder(nn.Module):
    """act(z zᵀ) as a dense [N, N] matrix: the reference's decoder, kept for the composed path and for small graphs"""

    def __init__(self, act=torch.sigmoid, dropout=0.):
        super().__init__()
        self.act = act
        self.dropout = dropout

    def forward(self, inp):
        inp = F.dropout(inp, self.dropout, training=self.training)
        return self.act(torch.mm(inp, inp.t()))


class LazyInnerProduct(object):
    """The decoder's logits z zᵀ, not formed: metrics.VAELoss reads z; dense() materialises the [N, N] matrix."""

    def __init__(self, z):
        self.z = z

    def dense(self):
        return torch.mm(self.z, self.z.t())

    def size(self):
        return torch.Size((self.z.shape[0], self.z.shape[0]))


class VGRNN(nn.Module):
    def __init__(self, input_dim, hidden_dim, output_dim, rnn_layer_num, conv_type='GCN', bias=True, fused=True):
        super().__init__()
        self.input_dim, self.hidden_dim, self.output_dim = input_dim, hidden_dim, output_dim
        self.rnn_layer_num = rnn_layer_num
        self.conv_type = conv_type
        self.bias = bias
        self.fused = fused
        self.method_name = 'VGRNN'
        assert conv_type in ['GCN', 'SAGE', 'GIN']
        if conv_type != 'GCN':
            raise NotImplementedError("VGRNN conv_type %r is not built: only 'GCN' is" % conv_type)
        assert rnn_layer_num >= 1
        self.phi_x = nn.Sequential(nn.Linear(input_dim, hidden_dim, bias=bias), nn.ReLU())
        self.phi_z = nn.Sequential(nn.Linear(output_dim, hidden_dim, bias=bias), nn.ReLU())
        self.enc = GCNConv(hidden_dim + hidden_dim, hidden_dim, bias=bias)
        self.enc_mean = GCNConv(hidden_dim, output_dim, act=_identity, bias=bias)
        self.enc_std = GCNConv(hidden_dim, output_dim, act=F.softplus, bias=bias)
        self.prior = nn.Sequential(nn.Linear(hidden_dim, hidden_dim, bias=bias), nn.ReLU())
        self.prior_mean = nn.Sequential(nn.Linear(hidden_dim, output_dim, bias=bias))
        self.prior_std = nn.Sequential(nn.Linear(hidden_dim, output_dim, bias=bias), nn.Softplus())
        self.rnn = graph_gru_gcn(hidden_dim + hidden_dim, hidden_dim, rnn_layer_num, bias=bias)
        self.dec = InnerProductDecoder(act=_identity)

    def _phi_x(self, x):
        lin = self.phi_x[0]
        if x.is_sparse:
            if layers._is_identity(x) and x.shape[1] == lin.in_features:
                return F.relu(ops.linear_of_identity(lin.weight, lin.bias))
            out = torch.sparse.mm(x, lin.weight.t())
            return F.relu(out if lin.bias is None else out + lin.bias)
        return self.phi_x(x)

    def forward(self, x_list, edge_idx_list, hx=None, noise_list=None, fused=None):
        """(embedding_list, h, loss_data_list) as the reference returns them, embedding_list[t] = enc_mean_t.  x_list: a list or a
        stacked tensor of features, the sparse identity included; edge_idx_list[t]: the [2, E] index tensor the reference passes, or a
        GcnAdj from gcn_conv_adjacency; noise_list[t]: the [N, output_dim] standard-normal draw of snapshot t (default: torch.randn on
        the device, so torch.manual_seed reproduces a run).  loss_data_list[4][t] is a LazyInnerProduct on the fused path and the dense
        logits on the composed one."""
        assert len(x_list) == len(edge_idx_list) and len(x_list) > 0
        fused = self.fused if fused is None else fused
        steps = len(x_list)
        first = x_list[0]
        ops._need_cuda(first, hx)
        n, dev = first.shape[0], first.device
        if hx is None:
            h = torch.zeros(self.rnn_layer_num, n, self.hidden_dim, device=dev)
        else:
            h = hx.detach()
        loss_data_list = [[], [], [], [], []]
        embedding_list = []
        if fused:                                                   # the concatenated weights, once for the window
            packed = self.rnn.packed()
            w_heads = torch.cat([self.enc_mean.weight, self.enc_std.weight], dim=1)
            b_heads = _cat_bias(self.enc_mean.bias, self.enc_std.bias)
        for t in range(steps):
            adj = gcn_conv_adjacency(edge_idx_list[t], n)
            phi_x_t = self._phi_x(x_list[t])
            noise = torch.randn(n, self.output_dim, device=dev) if noise_list is None else noise_list[t]
            ops._need_cuda(noise)
            if fused:
                W = self.enc.weight
                S = torch.matmul(phi_x_t, W[:self.hidden_dim]) + torch.matmul(h[-1], W[self.hidden_dim:])
                enc_t = ops.gcn_conv(S, adj, self.enc.bias, ops.GCN_EPI_RELU)
                enc_mean_t, enc_std_t, z_t = ops.vgrnn_heads(torch.matmul(enc_t, w_heads), adj, b_heads, noise)
            else:
                enc_t = self.enc(torch.cat([phi_x_t, h[-1]], 1), adj, fused=False)
                enc_mean_t = self.enc_mean(enc_t, adj, fused=False)
                enc_std_t = self.enc_std(enc_t, adj, fused=False)
                z_t = noise.mul(enc_std_t).add(enc_mean_t)
            prior_t = self.prior(h[-1])
            prior_mean_t = self.prior_mean(prior_t)
            prior_std_t = self.prior_std(prior_t)
            phi_z_t = self.phi_z(z_t)
            dec_t = LazyInnerProduct(z_t) if fused else self.dec(z_t)
            _, h = self.rnn(torch.cat([phi_x_t, phi_z_t], 1), adj, h, fused=fused, packed=packed if fused else None)
            embedding_list.append(enc_mean_t)
            for k, v in enumerate((enc_mean_t, enc_std_t, prior_mean_t, prior_std_t, dec_t)):
                loss_data_list[k].append(v)
        return embedding_list, h, loss_data_list

    def reset_parameters(self, stdv=1e-1):
        for weight in self.parameters():
            weight.data.normal_(0, stdv)

    @staticmethod
    def _reparameterized_sample(mean, std):
        return torch.randn(std.size(), device=mean.device).mul(std).add_(mean)
