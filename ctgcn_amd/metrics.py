"""NegativeSamplingLoss and ReconstructionLoss with the reference's constructor / forward signatures (reference metrics.py:18-123).

The reference walks over the batch nodes in Python, drawing positives with random.sample per node (metrics.py:68-84) —
the bottleneck of real training once the model is fast.  Here the draws are one HIP kernel
(ctgcn_neg_sampling_indices); the scores and the BCE terms are the reference's own formulas in torch.

epoch_loss() of both losses is the epoch-fused path of embedding.UnsupervisedEmbedding: every batch of an epoch scored
against ONE forward's embeddings, losses and the gradient of their sum by the kernels of ctgcn_epoch.hip.

ClassificationLoss and StructureClassificationLoss are the supervised trainer's losses (reference metrics.py:169-229): cross entropy
(or BCE with logits for 1-D scores), accuracy and ROC AUC per snapshot, by the loss pass of ctgcn_supervised.hip.

VAELoss and VAEClassificationLoss are the VGRNN baseline's losses (reference metrics.py:126-161, :232-247): the KL divergence of the
posterior from the prior plus the decoder's weighted BCE against the adjacency, which ops.vae_nll (ctgcn_vgrnn.hip) computes from z
without the [N, N] matrices when the model hands over its lazy decoder output.
"""
import ctypes
import itertools
import os

import numpy as np
import torch
from torch import nn
from torch.nn import functional as F

from . import _lib, ops
from ._lib import check, ptr
from .walks import WalkPairs

# seed=None streams: a per-process base drawn from OS entropy (the reference calls random.seed() — OS entropy — on every
# forward, metrics.py:69) advanced by a counter, so runs, and the ranks of one job, draw different samples
_seed_base = int.from_bytes(os.urandom(8), "little")
_seed_counter = itertools.count(1)
_M64 = 2 ** 64 - 1
_GOLDEN = 0x9E3779B97F4A7C15


def _splitmix64(z):
    z = (z + _GOLDEN) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def epoch_batch_seed(base, epoch, batch, snapshot):
    """The sample seed of (epoch, batch, snapshot) under a run's base seed: the same in the fused and the per-batch trainer."""
    z = _splitmix64(base & _M64)
    for v in (epoch, batch, snapshot):
        z = _splitmix64(z ^ (v & _M64))
    return z


def _seed_tensor(seeds, device):
    """uint64 seeds as the bits of an int64 device tensor."""
    return torch.from_numpy(np.asarray([int(x) & _M64 for x in seeds], dtype=np.uint64).view(np.int64)).to(device)


def _rows(mat, what):
    """(pointer, leading dimension) of a [N, d] fp32 CUDA view whose rows are unit-stride (a [T, N, d] view of [N, T, d] qualifies)."""
    ops._need_cuda(mat)
    if mat.dim() != 2 or mat.dtype != torch.float32 or (mat.shape[1] > 1 and mat.stride(1) != 1):
        raise ValueError("%s must be a float32 [N, d] view with unit column stride" % what)
    return mat.data_ptr(), max(mat.stride(0), mat.shape[1])


def _as_list(x):
    return [x] if not isinstance(x, list) and x.dim() == 2 else list(x)


class NegativeSamplingLoss(nn.Module):
    def __init__(self, node_pair_list, neg_freq_list, neg_num=20, Q=10, seed=None):
        super().__init__()
        self.node_pair_list = node_pair_list        # per snapshot: WalkPairs, or the reference's array of python lists
        self.neg_freq_list = neg_freq_list          # per snapshot: the negative table (list / array / tensor of node ids)
        self.neg_sample_num = neg_num
        self.Q = Q
        self.seed = seed                            # None: a fresh stream per call (the reference reseeds from the OS)
        self.shared_base = None                     # snapshot_parallel.share_loss_seed: one entropy-drawn stream for all ranks of a job
        self._shared_calls = 0
        self._cache = {}

    def _device_inputs(self, i, device):
        hit = self._cache.get((i, str(device)))
        if hit is None:
            pairs = self.node_pair_list[i]
            if not isinstance(pairs, WalkPairs):
                pairs = WalkPairs.from_lists(pairs, device)
            elif pairs.device != device:
                pairs = WalkPairs(pairs.row_ptr.to(device), pairs.col.to(device))
            table = self.neg_freq_list[i]
            table = table if isinstance(table, torch.Tensor) else torch.as_tensor(np.asarray(table, dtype=np.int32))
            hit = self._cache[(i, str(device))] = (pairs, table.to(device=device, dtype=torch.int32).contiguous())
        return hit

    def sample_indices(self, i, batch_indices, seed=None):
        """(sample_num, node_indices, pos_indices, neg_indices) — metrics.py:62-93 for snapshot i.  seed: an explicit draw seed
        (the trainer's per-(epoch, batch, snapshot) seed); None: the loss's own stream."""
        device = batch_indices.device
        ops._need_cuda(batch_indices)
        pairs, table = self._device_inputs(i, device)
        num = int(self.neg_sample_num)
        batch = batch_indices.to(torch.int64).contiguous()
        deg = (pairs.row_ptr[1:] - pairs.row_ptr[:-1]).long()[batch]
        take = torch.clamp(deg, max=num)
        offsets = torch.cumsum(take, 0) - take
        sample_num = int(take.sum().item())
        if sample_num == 0:
            return 0, None, None, None
        node_idx = torch.empty(sample_num, dtype=torch.int64, device=device)
        pos_idx = torch.empty(sample_num, dtype=torch.int64, device=device)
        neg_idx = torch.empty(num, dtype=torch.int64, device=device)
        scratch = torch.empty(num, dtype=torch.int64, device=device)
        if seed is not None:
            pass
        elif self.seed is not None:
            seed = self.seed * 1000003 + i
        elif self.shared_base is not None:          # every rank makes the same sequence of calls: the same draws everywhere
            self._shared_calls += 1
            seed = self.shared_base + self._shared_calls * 0x9E3779B97F4A7C15
        else:
            seed = _seed_base + next(_seed_counter) * 0x9E3779B97F4A7C15
        with torch.cuda.device(device):
            check(_lib.load().ctgcn_neg_sampling_indices(batch.numel(), ptr(batch), ptr(pairs.row_ptr), ptr(pairs.col), num, table.numel(),
                                                         ptr(table), ctypes.c_uint64(seed & (2 ** 64 - 1)), ptr(offsets), ptr(node_idx),
                                                         ptr(pos_idx), ptr(neg_idx), ptr(scratch), ops._stream()),
                  "ctgcn_neg_sampling_indices")
        dt = batch_indices.dtype
        return sample_num, node_idx.to(dt), pos_idx.to(dt), neg_idx.to(dt)

    def forward(self, input_list, seeds=None):
        """seeds (optional): one explicit draw seed per snapshot (see sample_indices)."""
        assert len(input_list) == 2
        node_embedding, batch_indices = input_list[0], input_list[1]
        if not isinstance(node_embedding, list) and node_embedding.dim() == 2:
            node_embedding = [node_embedding]
        bce = nn.BCEWithLogitsLoss()
        loss = torch.zeros(1, device=batch_indices.device)
        for i in range(len(node_embedding)):
            emb = node_embedding[i]
            sample_num, node_idx, pos_idx, neg_idx = self.sample_indices(i, batch_indices, None if seeds is None else seeds[i])
            if sample_num == 0:
                continue
            pos_score = torch.sum(emb[node_idx].mul(emb[pos_idx]), dim=1)
            neg_score = torch.sum(emb[node_idx].matmul(torch.transpose(emb[neg_idx], 1, 0)), dim=1)
            loss = loss + bce(pos_score, torch.ones_like(pos_score)) + self.Q * bce(neg_score, torch.zeros_like(neg_score))
        return loss

    def batched_sample_indices(self, i, node_indices, batch_size, seeds):
        """The draws of every batch of an epoch for snapshot i in two launches and one host read (the total, for allocation).
        node_indices: the epoch permutation (int64, CUDA); batch b = node_indices[b*batch_size : (b+1)*batch_size] draws with
        seeds[b] exactly what sample_indices(i, batch, seed=seeds[b]) draws.  Returns (total, offsets int64[P+1] per position,
        batch_offsets int64[B+1], node_idx int64[total], pos_idx int64[total], neg_idx int64[B, num]); node_idx / pos_idx are
        None when total == 0."""
        device = node_indices.device
        ops._need_cuda(node_indices)
        pairs, table = self._device_inputs(i, device)
        num = int(self.neg_sample_num)
        perm = node_indices.to(torch.int64).contiguous()
        P = perm.numel()
        B = -(-P // batch_size)
        if len(seeds) != B:
            raise ValueError("one seed per batch: %d batches, %d seeds" % (B, len(seeds)))
        lib = _lib.load()
        offsets = torch.empty(P + 1, dtype=torch.int64, device=device)
        batch_off = torch.empty(B + 1, dtype=torch.int64, device=device)
        neg_idx = torch.empty(B, num, dtype=torch.int64, device=device)
        scratch = torch.empty(B, num, dtype=torch.int64, device=device)
        seed_t = _seed_tensor(seeds, device)
        with torch.cuda.device(device):
            ws = torch.empty(max(lib.ctgcn_epoch_scan_workspace_bytes(P), 1), dtype=torch.uint8, device=device)
            check(lib.ctgcn_neg_sampling_offsets_batched(P, ptr(perm), ptr(pairs.row_ptr), num, batch_size, ptr(offsets), ptr(batch_off),
                                                         ptr(ws), ws.numel(), ops._stream()), "ctgcn_neg_sampling_offsets_batched")
            total = int(offsets[P].item())
            node_idx = torch.empty(total, dtype=torch.int64, device=device) if total else None
            pos_idx = torch.empty(total, dtype=torch.int64, device=device) if total else None
            check(lib.ctgcn_neg_sampling_indices_batched(P, ptr(perm), batch_size, ptr(seed_t), ptr(pairs.row_ptr), ptr(pairs.col), num,
                                                         table.numel(), ptr(table), ptr(offsets), ptr(node_idx), ptr(pos_idx), ptr(neg_idx),
                                                         ptr(scratch), ops._stream()), "ctgcn_neg_sampling_indices_batched")
        return total, offsets, batch_off, node_idx, pos_idx, neg_idx

    def epoch_loss(self, embeddings, node_indices, batch_size, seeds, grads):
        """Every batch of an epoch against one set of embeddings: returns the per-batch losses float64 [T, B] (the reference's
        forward of batch b, snapshot t, on these embeddings) and ACCUMULATES d(Σ losses)/dE into grads.  embeddings / grads: a
        [T, N, d] tensor (a strided view is read in place) or a list of [N, d]; seeds[t][b]: the draw seed of batch b, snapshot t."""
        emb, grd = _as_list(embeddings), _as_list(grads)
        if len(emb) != len(grd) or len(seeds) != len(emb):
            raise ValueError("embeddings, grads and seeds must cover the same snapshots")
        device = node_indices.device
        P = node_indices.numel()
        B = -(-P // batch_size)
        losses = torch.zeros(len(emb), B, dtype=torch.float64, device=device)
        lib = _lib.load()
        for t, (e, g) in enumerate(zip(emb, grd)):
            e = e.detach()
            if e.shape != g.shape or e.shape[0] < P:
                raise ValueError("snapshot %d: embedding %s / gradient %s" % (t, tuple(e.shape), tuple(g.shape)))
            pe, lde = _rows(e, "embedding")
            pg, ldg = _rows(g, "gradient")
            total, offsets, _, node_idx, pos_idx, neg_idx = self.batched_sample_indices(t, node_indices, batch_size, seeds[t])
            pos_sorted, pos_order = torch.sort(pos_idx, stable=True) if total else (None, None)
            neg_sorted, neg_order = torch.sort(neg_idx.view(-1), stable=True)
            d = e.shape[1]
            with torch.cuda.device(device):
                ws = torch.empty(lib.ctgcn_negsampling_loss_workspace_bytes(P, total, batch_size, d), dtype=torch.uint8, device=device)
                check(lib.ctgcn_negsampling_loss_fwd_bwd_f32(P, batch_size, total, d, int(self.neg_sample_num), float(self.Q), pe, lde,
                                                             ptr(offsets), ptr(node_idx), ptr(pos_idx), ptr(neg_idx), ptr(pos_sorted),
                                                             ptr(pos_order), ptr(neg_sorted), ptr(neg_order), ptr(losses[t]), pg, ldg,
                                                             ptr(ws), ws.numel(), ops._stream()), "ctgcn_negsampling_loss_fwd_bwd_f32")
        return losses


class ReconstructionLoss(nn.Module):
    """Reconstruction loss of CGCN-S / CTGCN-S (reference metrics.py:97-123): Σ_t MSE(structure_t[batch], embedding_t[batch])."""

    def __init__(self):
        super().__init__()

    def forward(self, input_list):
        assert len(input_list) == 3
        node_embedding, structure_embedding, batch_indices = input_list[0], input_list[1], input_list[2]
        node_embedding = _as_list(node_embedding)
        structure_embedding = _as_list(structure_embedding)
        mse_loss = nn.MSELoss()
        structure_loss = 0
        for embedding_mat, structure_mat in zip(node_embedding, structure_embedding):
            if batch_indices is not None:
                structure_loss = structure_loss + mse_loss(structure_mat[batch_indices], embedding_mat[batch_indices])
            else:
                structure_loss = structure_loss + mse_loss(structure_mat, embedding_mat)
        return structure_loss

    def epoch_loss(self, embeddings, structures, node_indices, batch_size, grad_embeddings, grad_structures):
        """Every batch of an epoch at once: per-batch losses float64 [T, B]; the gradients of their sum are ACCUMULATED into
        grad_embeddings / grad_structures (same layouts as the inputs; a [T, N, d] strided view is read in place).  node_indices
        must hold distinct rows."""
        emb, st, ge, gs = _as_list(embeddings), _as_list(structures), _as_list(grad_embeddings), _as_list(grad_structures)
        if not (len(emb) == len(st) == len(ge) == len(gs)):
            raise ValueError("embeddings, structures and gradients must cover the same snapshots")
        device = node_indices.device
        ops._need_cuda(node_indices)
        rows = node_indices.to(torch.int64).contiguous()
        P = rows.numel()
        B = -(-P // batch_size)
        losses = torch.zeros(len(emb), B, dtype=torch.float64, device=device)
        lib = _lib.load()
        with torch.cuda.device(device):
            ws = torch.empty(max(lib.ctgcn_reconstruction_loss_workspace_bytes(P), 1), dtype=torch.uint8, device=device)
            for t in range(len(emb)):
                e, s = emb[t].detach(), st[t].detach()
                if not (e.shape == s.shape == ge[t].shape == gs[t].shape):
                    raise ValueError("snapshot %d: shapes differ" % t)
                pe, lde = _rows(e, "embedding")
                ps, lds = _rows(s, "structure")
                pge, ldge = _rows(ge[t], "embedding gradient")
                pgs, ldgs = _rows(gs[t], "structure gradient")
                check(lib.ctgcn_reconstruction_loss_fwd_bwd_f32(P, batch_size, e.shape[1], ptr(rows), ps, lds, pe, lde, ptr(losses[t]), pgs, ldgs,
                                                                pge, ldge, ptr(ws), ws.numel(), ops._stream()),
                      "ctgcn_reconstruction_loss_fwd_bwd_f32")
        return losses


class ClassificationLoss(nn.Module):
    """(total_loss, total_acc, total_auc) of per-snapshot predictions against per-snapshot labels (reference metrics.py:169-209):
    the loss is summed over the snapshots, accuracy and AUC are their means.

    2-D predictions [items, n_class]: CrossEntropyLoss, accuracy = (first argmax == label), AUC = sklearn's micro one-vs-rest
    roc_auc_score over the ravelled one-hot labels and softmax probabilities.  For n_class == 2 the reference's sklearn call fails
    on the shape; here it is the binary AUC of the class-1 probability.
    1-D predictions z (InnerProduct): BCEWithLogitsLoss, prediction z > 0 (the argmax of (1 - σ(z), σ(z)), first on ties).  The
    reference takes its AUC of sigmoid(sigmoid(z)), whose two saturating sigmoids tie large scores in floating point; this AUC
    ranks by z, the ranking that expression has in exact arithmetic.
    Loss, count and probabilities come from one kernel pass (ops.cls_loss_autograd); fused=False (attribute) computes them with
    stock torch ops.  Both take the AUC from evaluation._logreg.roc_auc on the device."""

    def __init__(self, n_class):
        super().__init__()
        self.n_class = n_class
        self.fused = True

    def forward(self, input_list, batch_labels):
        cls_res = input_list
        if not isinstance(cls_res, (list, tuple)) and cls_res.dim() == 2:
            cls_res = [cls_res]
        return self._classification_loss(cls_res, batch_labels)

    def _snapshot(self, preds, labels):
        dot = preds.dim() == 1
        if not dot:
            assert preds.shape[1] == self.n_class
        if self.fused:
            loss, correct, prob = ops.cls_loss_autograd(preds, labels, dot=dot)
            acc = correct[0].double() / labels.numel()
        elif dot:
            loss = F.binary_cross_entropy_with_logits(preds, labels.to(preds.dtype))
            prob = torch.sigmoid(preds.detach())
            acc = ((preds.detach() > 0).to(labels.dtype) == labels).double().sum() / labels.numel()
        else:
            loss = F.cross_entropy(preds, labels.long())
            prob = torch.softmax(preds.detach(), dim=1)
            acc = (preds.detach().max(1)[1] == labels).double().sum() / labels.numel()
        from .evaluation._logreg import roc_auc
        if dot:
            auc = roc_auc(labels, preds.detach())
        elif self.n_class == 2:
            auc = roc_auc(labels, prob[:, 1])
        else:
            onehot = labels.long().unsqueeze(1) == torch.arange(self.n_class, device=labels.device).unsqueeze(0)
            auc = roc_auc(onehot.reshape(-1), prob.reshape(-1))
        return loss, acc, auc

    def _classification_loss(self, cls_res, batch_labels):
        total_loss, total_acc, total_auc = 0, 0, 0
        timestamp_num = len(cls_res)
        for i in range(timestamp_num):
            loss_val, acc_val, auc_val = self._snapshot(cls_res[i], batch_labels[i])
            total_loss = total_loss + loss_val
            total_acc = total_acc + acc_val
            total_auc = total_auc + auc_val
        total_acc /= timestamp_num
        total_auc /= timestamp_num
        return total_loss, total_acc, total_auc


class StructureClassificationLoss(nn.Module):
    """ReconstructionLoss([embeddings, structures, None]) + ClassificationLoss for CGCN-S / CTGCN-S (reference metrics.py:214-229)."""

    def __init__(self, n_class):
        super().__init__()
        self.reconstruction_loss = ReconstructionLoss()
        self.classification_loss = ClassificationLoss(n_class)

    @property
    def fused(self):
        return self.classification_loss.fused

    @fused.setter
    def fused(self, value):
        self.classification_loss.fused = bool(value)

    def forward(self, input_list, batch_labels):
        assert len(input_list) == 3
        cls_res, node_embedding, structure_embedding = input_list[0], input_list[1], input_list[2]
        structure_loss = self.reconstruction_loss([node_embedding, structure_embedding, None])
        cls_loss, total_acc, total_auc = self.classification_loss(cls_res, batch_labels)
        return structure_loss + cls_loss, total_acc, total_auc


class VAELoss(nn.Module):
    """Σ_t KLD(enc_t ‖ prior_t) + NLL(dec_t, adj_t) of the VGRNN (reference metrics.py:126-161).  input_list = [enc_mean, enc_std,
    prior_mean, prior_std, dec, adj], one entry per snapshot each.  dec[t] is the model's lazy decoder output (an object holding z_t:
    the loss is ops.vae_nll, no [N, N] matrix) or a dense [N, N] logit matrix (the reference's expression in stock torch ops);
    adj[t] is a torch sparse tensor or an ops.GcnAdj of the target adjacency, weights included.  The KLD is elementwise torch work,
    summed in fp64; the result is a fp64 scalar.  An adjacency whose values sum to 0 raises ValueError (the reference divides by zero)."""

    def __init__(self, eps=1e-10):
        super().__init__()
        self.eps = eps

    def forward(self, input_list):
        assert len(input_list) == 6
        enc_mean_list, enc_std_list, prior_mean_list, prior_std_list, dec_list, adj_list = input_list
        kld_loss, nll_loss = 0, 0
        for t in range(len(adj_list)):
            kld_loss = kld_loss + self._kld_gauss(enc_mean_list[t], enc_std_list[t], prior_mean_list[t], prior_std_list[t])
            nll_loss = nll_loss + self._nll_bernoulli(dec_list[t], adj_list[t])
        return kld_loss + nll_loss

    def _kld_gauss(self, mean_1, std_1, mean_2, std_2):
        num_nodes = mean_1.size()[0]
        kld_element = (2 * torch.log(std_2 + self.eps) - 2 * torch.log(std_1 + self.eps)
                       + (torch.pow(std_1 + self.eps, 2) + torch.pow(mean_1 - mean_2, 2)) / torch.pow(std_2 + self.eps, 2) - 1)
        return (0.5 / num_nodes) * torch.mean(torch.sum(kld_element.double(), dim=1), dim=0)

    @staticmethod
    def _nll_bernoulli(dec, adj):
        if not isinstance(dec, torch.Tensor):                  # the lazy decoder output: z, never z zᵀ
            from .layers import as_gcn_adj
            return ops.vae_nll(dec.z, as_gcn_adj(adj, dec.z.device, symmetric=False))
        target = (adj.to_sparse_tensor() if isinstance(adj, ops.GcnAdj) else adj).to_dense().to(dec.dtype)
        n = target.size()[0]
        total = target.sum()
        if float(total) == 0.0:
            raise ValueError("the adjacency's values sum to 0: pos_weight = (n² − S) / S is undefined")
        posw = (n * n - total) / total
        norm = n * n / ((n * n - total) * 2)
        return norm * torch.mean(F.binary_cross_entropy_with_logits(input=dec, target=target, pos_weight=posw, reduction='none'), dim=[0, 1])


class VAEClassificationLoss(nn.Module):
    """VAELoss(input_list[:-1]) + ClassificationLoss(input_list[-1], labels) for a supervised VGRNN (reference metrics.py:232-247)."""

    def __init__(self, n_class, eps=1e-10):
        super().__init__()
        self.vae_loss = VAELoss(eps=eps)
        self.classification_loss = ClassificationLoss(n_class)

    @property
    def fused(self):
        return self.classification_loss.fused

    @fused.setter
    def fused(self, value):
        self.classification_loss.fused = bool(value)

    def forward(self, input_list, batch_labels):
        assert len(input_list) == 7
        vae_loss = self.vae_loss(input_list[:-1])
        classification_loss, total_acc, total_auc = self.classification_loss(input_list[-1], batch_labels)
        return vae_loss + classification_loss, total_acc, total_auc
