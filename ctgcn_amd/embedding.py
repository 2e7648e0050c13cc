"""UnsupervisedEmbedding: the reference's unsupervised trainer (reference embedding.py:13-89, 293-368) for CTGCN-C/-S and CGCN-C/-S.

The reference runs, per epoch, one full-graph forward + loss(batch) + backward for each of the ceil(N / batch_size) batches of a
shuffled node order and steps Adam once after the last batch (gradient accumulation).  The weights do not change inside an epoch
and the forward is deterministic, so every batch sees the same embeddings and the accumulated gradient is the gradient of
Σ_b loss_b.  fused=True (default) computes exactly that from ONE forward and ONE backward per epoch: the losses of all batches and
d(Σ loss)/d(output) come from the kernels of ctgcn_epoch.hip (metrics.*.epoch_loss).  fused=False is the reference's loop step
for step.  Both modes draw the same samples: batch b of epoch e, snapshot t uses metrics.epoch_batch_seed(base, e, b, t), and the
node order is the reference's all_nodes[torch.randperm(N)] from torch's CPU generator.
"""
import os
import time

import torch

from ._lib import CtgcnHipError
from .export import save_embedding
from .metrics import NegativeSamplingLoss, ReconstructionLoss, _seed_base, epoch_batch_seed

_S_MODELS = ('CGCN-S', 'CTGCN-S')
_SUPPORTED = ('CGCN-C', 'CGCN-S', 'CTGCN-C', 'CTGCN-S')


def batch_count(node_num, batch_size):
    """ceil(node_num / batch_size): reference embedding.py:322-326."""
    return -(-node_num // batch_size)


def batch_bounds(node_num, batch_size):
    """[(start, end)] of the batches of one epoch, the last one partial."""
    return [(j * batch_size, min(node_num, (j + 1) * batch_size)) for j in range(batch_count(node_num, batch_size))]


def epoch_order(node_num, shuffle=True):
    """The reference's node order of one epoch (embedding.py:340): torch.randperm from torch's CPU generator, or 0..N-1."""
    return torch.randperm(node_num) if shuffle else torch.arange(node_num)


def snapshot_file_stem(timestamp_list, start_idx, i):
    """Name of snapshot i's export file without '.csv' (reference embedding.py:84)."""
    return timestamp_list[start_idx + i].split('.')[0]


class UnsupervisedEmbedding(object):
    def __init__(self, base_path, origin_folder, embedding_folder, node_list, model, loss, model_folder='model', has_cuda=False):
        if not has_cuda:
            raise CtgcnHipError("UnsupervisedEmbedding runs on the MI355X only (has_cuda=True); there is no CPU fallback")
        self.base_path = base_path
        self.origin_base_path = os.path.abspath(os.path.join(base_path, origin_folder))
        self.embedding_base_path = os.path.abspath(os.path.join(base_path, embedding_folder))
        self.model_base_path = os.path.abspath(os.path.join(base_path, model_folder))
        self.has_cuda = has_cuda
        self.device = torch.device('cuda', torch.cuda.current_device())
        self.model = model
        self.loss = loss
        self.file_sep = '\t'
        self.full_node_list = node_list
        self.node_num = len(node_list)
        self.timestamp_list = sorted(os.listdir(self.origin_base_path))
        self.last_epoch_losses = []         # per-batch losses of the last epoch (the reference prints them per batch)
        self.sample_seed_base = None        # base of the per-(epoch, batch, snapshot) sample seeds of the last run
        os.makedirs(self.embedding_base_path, exist_ok=True)
        os.makedirs(self.model_base_path, exist_ok=True)

    def prepare(self, load_model, model_file, lr=1e-3, weight_decay=0.):
        """reference embedding.py:49-69"""
        if load_model:
            model_path = os.path.join(self.model_base_path, model_file)
            if os.path.exists(model_path):
                self.model.load_state_dict(torch.load(model_path, map_location='cpu'))
                self.model.eval()
        self.model = self.model.to(self.device)
        self.loss = self.loss.to(self.device)
        optimizer = torch.optim.Adam(self.model.parameters(), lr=lr, weight_decay=weight_decay)
        optimizer.zero_grad()
        return self.model, self.loss, optimizer

    def get_batch_info(self, batch_size):
        return batch_count(self.node_num, batch_size)

    def _check_model(self, model):
        name = getattr(model, 'method_name', None)
        if name not in _SUPPORTED:
            raise NotImplementedError("UnsupervisedEmbedding covers %s, not %r" % (', '.join(_SUPPORTED), name))
        want = ReconstructionLoss if name in _S_MODELS else NegativeSamplingLoss
        if not isinstance(self.loss, want):
            raise ValueError("%s trains with %s, got %s" % (name, want.__name__, type(self.loss).__name__))
        return name

    def _seed_base(self):
        if isinstance(self.loss, NegativeSamplingLoss) and self.loss.seed is not None:
            return int(self.loss.seed)
        return _seed_base + int.from_bytes(os.urandom(8), 'little')     # reference: random.seed() from OS entropy per forward

    @staticmethod
    def _split(name, res):
        """(loss embeddings, structures or None, export list) of a forward: reference embedding.py:298-320."""
        if name in _S_MODELS:
            emb, struct = res
            return emb, struct, struct
        return res, None, res

    def _epoch_fused(self, model, name, x_list, adj_list, node_indices, batch_size, epoch_idx, base):
        res = model(x_list, adj_list)
        emb, struct, output_list = self._split(name, res)
        B = batch_count(self.node_num, batch_size)
        if struct is None:
            T = len(emb) if isinstance(emb, list) or emb.dim() == 3 else 1
            seeds = [[epoch_batch_seed(base, epoch_idx, b, t) for b in range(B)] for t in range(T)]
            grad = [torch.zeros_like(e) for e in emb] if isinstance(emb, list) else torch.zeros_like(emb)   # strided like out: [T, N, d] of [N, T, d]
            losses = self.loss.epoch_loss(emb, node_indices, batch_size, seeds, grad)
            outs, grads = (emb, grad) if isinstance(emb, list) else ([emb], [grad])
        else:
            ge = [torch.zeros_like(e) for e in emb] if isinstance(emb, list) else torch.zeros_like(emb)
            gs = [torch.zeros_like(s) for s in struct] if isinstance(struct, list) else torch.zeros_like(struct)
            losses = self.loss.epoch_loss(emb, struct, node_indices, batch_size, ge, gs)
            outs = (list(emb) if isinstance(emb, list) else [emb]) + (list(struct) if isinstance(struct, list) else [struct])
            grads = (list(ge) if isinstance(ge, list) else [ge]) + (list(gs) if isinstance(gs, list) else [gs])
        pairs = [(o, g) for o, g in zip(outs, grads) if o.requires_grad]
        torch.autograd.backward([o for o, _ in pairs], [g for _, g in pairs])
        return losses.sum(0).tolist(), output_list

    def _epoch_per_batch(self, model, name, x_list, adj_list, node_indices, batch_size, epoch_idx, base):
        losses, output_list = [], None
        for j, (lo, hi) in enumerate(batch_bounds(self.node_num, batch_size)):
            batch_indices = node_indices[lo:hi]
            res = model(x_list, adj_list)
            emb, struct, output_list = self._split(name, res)
            if struct is None:
                T = len(emb) if isinstance(emb, list) or emb.dim() == 3 else 1
                loss = self.loss([emb, batch_indices], seeds=[epoch_batch_seed(base, epoch_idx, j, t) for t in range(T)])
            else:
                loss = self.loss([emb, struct, batch_indices])
            if isinstance(loss, torch.Tensor) and loss.requires_grad:
                loss.backward()
            losses.append(float(loss))
            del res, emb, struct, loss
        return losses, output_list

    def learn_embedding(self, adj_list, x_list, edge_list=None, node_dist_list=None, epoch=50, batch_size=1024, lr=1e-3, start_idx=0,
                        weight_decay=0., model_file='ctgcn', load_model=False, shuffle=True, export=True, fused=True):
        """reference embedding.py:329-368; edge_list / node_dist_list are the VGRNN / PGNN inputs and unused here."""
        model, loss_model, optimizer = self.prepare(load_model, model_file, lr=lr, weight_decay=weight_decay)
        name = self._check_model(model)
        all_nodes = torch.arange(self.node_num, device=self.device)
        base = self.sample_seed_base = self._seed_base()
        run = self._epoch_fused if fused else self._epoch_per_batch
        output_list = []
        st = time.time()
        model.train()
        for i in range(epoch):
            node_indices = all_nodes[epoch_order(self.node_num, shuffle).to(self.device)]
            t1 = time.time()
            self.last_epoch_losses, output_list = run(model, name, x_list, adj_list, node_indices, batch_size, i, base)
            optimizer.step()            # gradient accumulation over the epoch's batches (embedding.py:349-352)
            model.zero_grad()
            print('epoch', i + 1, ', batches =', len(self.last_epoch_losses), ', loss:', sum(self.last_epoch_losses),
                  ', cost time: ', time.time() - t1, ' seconds!')
        cost_time = time.time() - st
        if export and len(output_list):
            save_embedding([o.detach() for o in output_list] if isinstance(output_list, list) else output_list.detach(),
                           self.timestamp_list, start_idx, self.embedding_base_path, self.full_node_list, sep=self.file_sep)
        if model_file:
            torch.save(model.state_dict(), os.path.join(self.model_base_path, model_file))
        del output_list
        torch.cuda.empty_cache()
        return cost_time
