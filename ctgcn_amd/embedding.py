"""UnsupervisedEmbedding: the reference's unsupervised trainer (reference embedding.py:13-89, 293-368) for CTGCN-C/-S, CGCN-C/-S and the
EvolveGCN, GCRN, GCN, GAT, GIN, SAGE, PGNN, TgGCN, TgGAT, TgSAGE and TgGIN baselines (single-output models: trained like the -C models), and
for the VGRNN baseline.

The reference runs, per epoch, one full-graph forward + loss(batch) + backward for each of the ceil(N / batch_size) batches of a
shuffled node order and steps Adam once after the last batch (gradient accumulation).  The weights do not change inside an epoch
and the forward is deterministic, so every batch sees the same embeddings and the accumulated gradient is the gradient of
Σ_b loss_b.  fused=True (default) computes exactly that from ONE forward and ONE backward per epoch: the losses of all batches and
d(Σ loss)/d(output) come from the kernels of ctgcn_epoch.hip (metrics.*.epoch_loss).  fused=False is the reference's loop step
for step.  Both modes draw the same samples: batch b of epoch e, snapshot t uses metrics.epoch_batch_seed(base, e, b, t), and the
node order is the reference's all_nodes[torch.randperm(N)] from torch's CPU generator.

A PGNN takes (x_list, dists_max, dists_argmax), drawn by baseline.pgnn.preselect_anchor from node_dist_list before each forward, as the
reference's get_model_res does.  The fused epoch makes one forward per epoch and so draws anchor sets once per epoch; fused=False draws
them per batch, as the reference does.  Under torch.manual_seed the fused paths repeat a run bit for bit; the unfused paths gather rows
with torch's indexing, whose backward adds with float atomics, and repeat bit for bit under torch.use_deterministic_algorithms(True).

A VGRNN takes (x_list, edge_list, hx) and trains with metrics.VAELoss on its own loss data plus adj_list (U-own).  Its loss covers
all nodes, so a batch is a full forward and the full loss: the reference's loop is run as it stands, hx carried from batch to batch
(detached on entry by the model) and Adam stepped once per epoch.  fused selects the model's kernel path or its composed stock-torch
path.

SupervisedEmbedding is the reference's supervised trainer (embedding.py:93-290) for the learning types S-node, S-edge, S-link-st
and S-link-dy on the same models; its classifier head and loss run the kernels of ctgcn_supervised.hip.
"""
import math
import os
import time

import torch

from ._lib import CtgcnHipError
from .export import save_embedding
from .metrics import (ClassificationLoss, NegativeSamplingLoss, ReconstructionLoss, StructureClassificationLoss, VAEClassificationLoss,
                      VAELoss, _seed_base, epoch_batch_seed)

_S_MODELS = ('CGCN-S', 'CTGCN-S')
_TG_MODELS = ('TgGCN', 'TgGAT', 'TgSAGE', 'TgGIN')              # the PyG variants: model(x_list, edge_list) on raw [2, E] indices, no adjacency
_SUPPORTED = ('CGCN-C', 'CGCN-S', 'CTGCN-C', 'CTGCN-S', 'EvolveGCN', 'GCRN', 'GAT', 'GIN', 'SAGE', 'PGNN', 'VGRNN') + _TG_MODELS      # the baselines: single-output, trained like the -C models
# trained too, but only as this package's own class (the driver sends GCN through the trainers like every other method); not in _SUPPORTED:
# another module that carries the name is still refused as an unsupported method
_MODULE_TRAINED = ('GCN',)


def _supported_name(trainer, model):
    """the model's method_name when the trainer covers it, NotImplementedError otherwise"""
    name = getattr(model, 'method_name', None)
    if name in _MODULE_TRAINED:
        from . import baseline
        if isinstance(model, getattr(baseline, name)):
            return name
    elif name in _SUPPORTED:
        return name
    raise NotImplementedError("%s covers %s, and %s as ctgcn_amd.baseline's own module, not %r (%s)"
                              % (trainer, ', '.join(_SUPPORTED), ', '.join(_MODULE_TRAINED), name, type(model).__name__))


def _check_own_baseline(trainer, model, name):
    """GIN, SAGE, PGNN, VGRNN and the four PyG variants are trained as this package's own modules, whose passes run in ctgcn_pool.hip,
    ctgcn_pgnn.hip, ctgcn_vgrnn.hip and ctgcn_tg.hip.  Another module
    that carries the name (the reference's classes with their dense masks and Python loops, or a model relabelled by hand) has no such
    path and is refused, not run through whatever forward it happens to have."""
    if name in ('GIN', 'SAGE', 'PGNN', 'VGRNN') + _TG_MODELS:
        from . import baseline
        cls = getattr(baseline, name)
        if not isinstance(model, cls):
            raise NotImplementedError("%s trains %s as ctgcn_amd.baseline.%s, got %s" % (trainer, name, name, type(model).__name__))


def model_forward(model, x_list, adj_list, node_dist_list, node_num, device, edge_list=None):
    """model(x_list, adj_list); for a PyG variant model(x_list, edge_list) (adj_list may be None); for a PGNN one draw of anchor sets
    and model(x_list, dists_max, dists_argmax) (reference embedding.py:209-212); dist_argmax holds node ids when the model carries
    anchor_node_ids = True"""
    name = getattr(model, 'method_name', None)
    if name in _TG_MODELS:
        return model(x_list, edge_list)
    if name != 'PGNN':
        return model(x_list, adj_list)
    from .baseline.pgnn import preselect_anchor
    dists_max, dists_argmax = preselect_anchor(node_num, node_dist_list, device, node_ids=bool(getattr(model, 'anchor_node_ids', False)))
    return model(x_list, dists_max, dists_argmax)


def _check_edge_list(name, edge_list, steps):
    if name == 'VGRNN' and (edge_list is None or len(edge_list) != steps):
        raise ValueError("a VGRNN needs edge_list: one [2, E] index tensor (or prepared adjacency) per snapshot")
    if name in _TG_MODELS and (edge_list is None or len(edge_list) != steps):
        raise ValueError("%s needs edge_list: one [2, E] index tensor (or prepared ops.TgGraph) per snapshot, got %s for %d snapshots"
                         % (name, "none" if edge_list is None else len(edge_list), steps))


def _check_node_dist(name, node_dist_list):
    if name == 'PGNN' and node_dist_list is None:
        raise ValueError("a PGNN needs node_dist_list (baseline.pgnn.precompute_dist_data of the snapshots' edge lists)")


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
        name = _supported_name("UnsupervisedEmbedding", model)
        _check_own_baseline("UnsupervisedEmbedding", model, name)
        want = VAELoss if name == 'VGRNN' else ReconstructionLoss if name in _S_MODELS else NegativeSamplingLoss
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

    def _epoch_fused(self, model, name, x_list, adj_list, node_indices, batch_size, epoch_idx, base, node_dist_list=None, edge_list=None):
        res = model_forward(model, x_list, adj_list, node_dist_list, self.node_num, self.device, edge_list)
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

    def _epoch_per_batch(self, model, name, x_list, adj_list, node_indices, batch_size, epoch_idx, base, node_dist_list=None, edge_list=None):
        losses, output_list = [], None
        for j, (lo, hi) in enumerate(batch_bounds(self.node_num, batch_size)):
            batch_indices = node_indices[lo:hi]
            res = model_forward(model, x_list, adj_list, node_dist_list, self.node_num, self.device, edge_list)
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

    def _epoch_vgrnn(self, model, x_list, adj_list, edge_list, batch_size, fused):
        """the reference's batch loop for a VGRNN (embedding.py:342-352): every batch a full forward and the full loss"""
        losses, output_list, hx = [], None, None
        for _ in batch_bounds(self.node_num, batch_size):
            output_list, hx, loss_data_list = model(x_list, edge_list, hx, fused=fused)
            loss = self.loss(loss_data_list + [adj_list])
            loss.backward()
            losses.append(float(loss))
            del loss_data_list, loss
        return losses, output_list

    def learn_embedding(self, adj_list, x_list, edge_list=None, node_dist_list=None, epoch=50, batch_size=1024, lr=1e-3, start_idx=0,
                        weight_decay=0., model_file='ctgcn', load_model=False, shuffle=True, export=True, fused=True):
        """reference embedding.py:329-368; edge_list is the input of a VGRNN and of the PyG variants (required for them, unused otherwise;
        adj_list may then be None for the PyG variants, as the reference's train.py passes it); node_dist_list is what a
        PGNN draws its anchor distances from (required for it, unused otherwise)."""
        model, loss_model, optimizer = self.prepare(load_model, model_file, lr=lr, weight_decay=weight_decay)
        name = self._check_model(model)
        _check_node_dist(name, node_dist_list)
        _check_edge_list(name, edge_list, len(x_list))
        all_nodes = torch.arange(self.node_num, device=self.device)
        base = self.sample_seed_base = self._seed_base()
        run = self._epoch_fused if fused else self._epoch_per_batch
        output_list = []
        st = time.time()
        model.train()
        for i in range(epoch):
            node_indices = all_nodes[epoch_order(self.node_num, shuffle).to(self.device)]
            t1 = time.time()
            if name == 'VGRNN':
                self.last_epoch_losses, output_list = self._epoch_vgrnn(model, x_list, adj_list, edge_list, batch_size, fused)
            else:
                self.last_epoch_losses, output_list = run(model, name, x_list, adj_list, node_indices, batch_size, i, base, node_dist_list, edge_list)
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


LEARNING_TYPES = ('S-node', 'S-edge', 'S-link-st', 'S-link-dy')


def supervised_split_counts(item_num, train_ratio, val_ratio, test_ratio):
    """floor(item_num * ratio) per split, as the reference takes them (embedding.py:121-123, :168-170)."""
    return tuple(int(math.floor(item_num * r)) for r in (train_ratio, val_ratio, test_ratio))


def label_splits(labels, train_ratio, val_ratio, test_ratio):
    """The reference's S-node / S-edge splits (embedding.py:111-142) of per-snapshot label tensors ([rows, 2]: node, label, or
    [rows, 3]: from, to, label): the first floor(rows * train_ratio) rows in file order, then val, then test; no shuffle.
    Returns (idx_train, label_train, idx_val, label_val, idx_test, label_test), node items [n], edge items [2, n]."""
    out = [[] for _ in range(6)]
    for cur in labels:
        assert cur.dim() == 2 and cur.shape[1] in (2, 3)
        counts = supervised_split_counts(cur.shape[0], train_ratio, val_ratio, test_ratio)
        lo = 0
        for k, cnt in enumerate(counts):
            rows = cur[lo:lo + cnt]
            lo += cnt
            out[2 * k].append(rows[:, 0] if cur.shape[1] == 2 else rows[:, :2].transpose(0, 1))
            out[2 * k + 1].append(rows[:, -1])
    return tuple(out)


def _distinct_negatives(keys, node_num, count, seed, snapshot, dev):
    """count negatives [count, 2] no two of which are the same pair in either direction (the reference rejects such draws,
    utils.py:120): the sampler's slots in order, a pair already seen dropped, further rounds drawn until count are kept."""
    from .evaluation.link_prediction import sample_negatives
    kept = torch.empty(0, 2, dtype=torch.int64, device=dev)
    rnd = 0
    while kept.shape[0] < count:
        need = count - kept.shape[0]
        draw = sample_negatives(keys, node_num, need + need // 8 + 16, epoch_batch_seed(seed, 1, rnd, snapshot), dev)
        cand = torch.cat([kept, draw])
        pair = torch.minimum(cand[:, 0], cand[:, 1]) * node_num + torch.maximum(cand[:, 0], cand[:, 1])
        order = torch.sort(pair, stable=True).indices
        first = torch.ones_like(pair, dtype=torch.bool)
        first[order[1:]] = pair[order[1:]] != pair[order[:-1]]
        kept = cand[first][:count]
        rnd += 1
    return kept


def link_splits(edge_list, node_num, learning_type, train_ratio, val_ratio, test_ratio, seed):
    """S-link-st / S-link-dy splits.  Per snapshot (S-link-dy: from snapshot 1 on, scored against the previous snapshot's embedding)
    the positives are the columns of the [2, E] edge list as given, self-loops dropped, shuffled by a torch generator seeded with
    (seed, snapshot); the first floor(E * train_ratio) are train, then val, then test.  Each split is followed by as many negatives
    from the link-prediction evaluation's GPU sampler (evaluation.link_prediction.sample_negatives): pairs u != v that are no
    edge of the snapshot in either direction, no pair twice in either direction within a snapshot.  The reference draws them one by one from numpy's global stream
    (embedding.py:155-190), so the draws differ by construction.  Labels are float (1 then 0), as the reference's."""
    from .evaluation.link_prediction import membership_keys
    out = [[] for _ in range(6)]
    first = 1 if learning_type == 'S-link-dy' else 0
    for i in range(first, len(edge_list)):
        cur = edge_list[i]
        assert cur.shape[0] == 2
        if not cur.is_cuda:
            raise CtgcnHipError("the link splits are drawn by the GPU sampler: edge lists must be CUDA tensors (no CPU fallback)")
        dev = cur.device
        pos = cur.to(torch.int64).t()
        pos = pos[pos[:, 0] != pos[:, 1]]
        snap_seed = epoch_batch_seed(seed, 0, 0, i)
        gen = torch.Generator(device=dev)
        gen.manual_seed(snap_seed & 0x7FFFFFFFFFFFFFFF)
        pos = pos[torch.randperm(pos.shape[0], generator=gen, device=dev)]
        counts = supervised_split_counts(pos.shape[0], train_ratio, val_ratio, test_ratio)
        keys = membership_keys(torch.cat([pos, pos.flip(1)]), node_num)
        neg = _distinct_negatives(keys, node_num, sum(counts), seed, i, dev)
        lo = 0
        for k, cnt in enumerate(counts):
            both = torch.cat([pos[lo:lo + cnt], neg[lo:lo + cnt]]).t().contiguous()
            lo += cnt
            out[2 * k].append(both)
            out[2 * k + 1].append(torch.cat([torch.ones(cnt, device=dev), torch.zeros(cnt, device=dev)]))
    return tuple(out)


class SupervisedEmbedding(object):
    """The reference's SupervisedEmbedding (embedding.py:93-290) for CGCN-C / CGCN-S / CTGCN-C / CTGCN-S.

    Kept from the reference: Adam covers the embedding model only, so the classifier stays the fixed random head it was built as
    (embedding.py:69); splits are taken in label-file order with no shuffle, batch_size and shuffle are accepted and unused; per
    epoch one train forward, loss, backward and Adam step, from the second epoch on a forward on the val items, a checkpoint
    whenever acc_val improves, and a test forward on the reloaded best checkpoint.
    Departures, each on purpose: train_classifier=True adds the classifier's parameters to the same Adam (the reference never
    trains it); the val and test forwards run under torch.no_grad(); when no checkpoint was written (epoch < 2, or acc_val never
    above 0) the current weights are kept where the reference fails to load; the S-link splits come from the GPU sampler
    (link_splits; `seed` fixes them, None draws a fresh stream); the 1-D AUC ranks by z (metrics.ClassificationLoss).

    fused=True runs the head and the loss on the kernels of ctgcn_supervised.hip; fused=False is the reference's expression in
    stock torch ops (E[idx], Linear, cross_entropy, index_put backward).  After a run: history (per epoch a dict of loss / acc / auc
    for train and, from epoch 2, val), test_result (loss, acc, auc), best_epoch (1-based, None without a checkpoint)."""

    def __init__(self, base_path, origin_folder, embedding_folder, node_list, model, loss, classifier, model_folder='model', has_cuda=False):
        if not has_cuda:
            raise CtgcnHipError("SupervisedEmbedding runs on the MI355X only (has_cuda=True); there is no CPU fallback")
        self.base_path = base_path
        self.origin_base_path = os.path.abspath(os.path.join(base_path, origin_folder))
        self.embedding_base_path = os.path.abspath(os.path.join(base_path, embedding_folder))
        self.model_base_path = os.path.abspath(os.path.join(base_path, model_folder))
        self.has_cuda = has_cuda
        self.device = torch.device('cuda', torch.cuda.current_device())
        self.model, self.loss, self.classifier = model, loss, classifier
        self.file_sep = '\t'
        self.full_node_list = node_list
        self.node_num = len(node_list)
        self.timestamp_list = sorted(os.listdir(self.origin_base_path))
        self.history, self.test_result, self.best_epoch = [], None, None
        self.split_seed = None              # seed of the S-link splits of the last run
        self.on_backward = None             # optional callback(epoch index, model, classifier) between backward and the Adam step
        os.makedirs(self.embedding_base_path, exist_ok=True)
        os.makedirs(self.model_base_path, exist_ok=True)

    def prepare(self, load_model, model_file, classifier_file=None, lr=1e-3, weight_decay=0., train_classifier=False):
        """reference embedding.py:50-71"""
        classifier = self.classifier
        if load_model:
            model_path = os.path.join(self.model_base_path, model_file)
            if os.path.exists(model_path):
                self.model.load_state_dict(torch.load(model_path, map_location='cpu'))
                self.model.eval()
            if classifier_file and classifier is not None:
                classifier.load_state_dict(torch.load(os.path.join(self.model_base_path, classifier_file), map_location='cpu'))
                classifier.eval()
        self.model = self.model.to(self.device)
        self.loss = self.loss.to(self.device)
        if classifier is not None:
            self.classifier = classifier = classifier.to(self.device)
        params = list(self.model.parameters())
        if train_classifier and classifier is not None:
            params += list(classifier.parameters())
        optimizer = torch.optim.Adam(params, lr=lr, weight_decay=weight_decay)
        optimizer.zero_grad()
        return self.model, self.loss, optimizer, classifier

    def get_batch_info(self, learning_type, node_labels, edge_labels, edge_list, batch_size, shuffle, train_ratio, val_ratio, test_ratio,
                       seed=None):
        """(idx_train, label_train, idx_val, label_val, idx_test, label_test), one entry per scored snapshot (embedding.py:99-191)."""
        if learning_type not in LEARNING_TYPES:
            raise ValueError("learning_type must be one of %s, got %r" % (', '.join(LEARNING_TYPES), learning_type))
        if learning_type == 'S-node':
            assert node_labels
            return label_splits(node_labels, train_ratio, val_ratio, test_ratio)
        if learning_type == 'S-edge':
            assert edge_labels
            return label_splits(edge_labels, train_ratio, val_ratio, test_ratio)
        assert edge_list
        if seed is None:
            seed = _seed_base + int.from_bytes(os.urandom(8), 'little')
        self.split_seed = int(seed)
        return link_splits(edge_list, self.node_num, learning_type, train_ratio, val_ratio, test_ratio, self.split_seed)

    def get_model_res(self, learning_type, adj_list, x_list, edge_list, node_dist_list, batch_indices, model, classifier, hx=None, fused=True):
        """(loss_input_list, output_list, hx): reference embedding.py:193-226 for the k-core models."""
        if model.method_name in _S_MODELS:
            embedding_list, structure_list = model(x_list, adj_list)
            embedding_list = embedding_list[:-1] if learning_type == 'S-link-dy' else embedding_list
            cls_list = classifier(embedding_list, batch_indices)
            return [cls_list, embedding_list, structure_list], structure_list, hx
        if model.method_name == 'VGRNN':
            embedding_list, _, loss_data_list = model(x_list, edge_list, hx, fused=fused)
            embedding_list = embedding_list[:-1] if learning_type == 'S-link-dy' else embedding_list
            return loss_data_list + [adj_list, classifier(embedding_list, batch_indices)], embedding_list, hx
        embedding_list = model_forward(model, x_list, adj_list, node_dist_list, self.node_num, self.device, edge_list)
        embedding_list = embedding_list[:-1] if learning_type == 'S-link-dy' else embedding_list
        return classifier(embedding_list, batch_indices), embedding_list, hx

    def _check_model(self, model):
        name = _supported_name("SupervisedEmbedding", model)
        _check_own_baseline("SupervisedEmbedding", model, name)
        want = VAEClassificationLoss if name == 'VGRNN' else StructureClassificationLoss if name in _S_MODELS else ClassificationLoss
        if not isinstance(self.loss, want):
            raise ValueError("%s trains with %s, got %s" % (name, want.__name__, type(self.loss).__name__))
        return name

    def learn_embedding(self, adj_list, x_list, node_labels=None, edge_labels=None, edge_list=None, node_dist_list=None,
                        learning_type='S-node', epoch=50, batch_size=1024, lr=1e-3, start_idx=0, weight_decay=0., train_ratio=0.5,
                        val_ratio=0.3, test_ratio=0.2, model_file='ctgcn', classifier_file='ctgcn_cls', load_model=False, shuffle=True,
                        export=True, train_classifier=False, seed=None, fused=True, batch_info=None):
        """reference embedding.py:230-290.  train_classifier departs from the reference (see the class).  batch_info: a precomputed
        (idx_train, label_train, idx_val, label_val, idx_test, label_test) used in place of get_batch_info."""
        assert train_ratio + val_ratio + test_ratio <= 1.0
        name = self._check_model(self.model)
        _check_node_dist(name, node_dist_list)
        _check_edge_list(name, edge_list, len(x_list))
        model, loss_model, optimizer, classifier = self.prepare(load_model, model_file, classifier_file, lr, weight_decay, train_classifier)
        if batch_info is None:
            batch_info = self.get_batch_info(learning_type, node_labels, edge_labels, edge_list, batch_size, shuffle, train_ratio, val_ratio,
                                             test_ratio, seed=seed)
        idx_train, label_train, idx_val, label_val, idx_test, label_test = batch_info
        loss_model.fused = classifier.fused = bool(fused)
        cls_params = [p for p in classifier.parameters() if p.requires_grad]
        if not train_classifier:            # not in the optimizer: no dW / db pass for gradients nobody reads
            for p in cls_params:
                p.requires_grad_(False)
        model_path = os.path.join(self.model_base_path, model_file) if model_file else None
        cls_path = os.path.join(self.model_base_path, classifier_file) if classifier_file else None
        self.history, self.test_result, self.best_epoch = [], None, None
        best_acc, output_list = 0, []
        torch.cuda.empty_cache()
        st = time.time()
        model.train()
        try:
            for i in range(epoch):
                t1 = time.time()
                loss_input_list, output_list, _ = self.get_model_res(learning_type, adj_list, x_list, edge_list, node_dist_list, idx_train,
                                                                     model, classifier, fused=bool(fused))
                loss_train, acc_train, auc_train = loss_model(loss_input_list, label_train)
                loss_train.backward()
                if self.on_backward is not None:
                    self.on_backward(i, model, classifier)
                optimizer.step()
                model.zero_grad()
                classifier.zero_grad()
                rec = {'loss_train': float(loss_train.detach()), 'acc_train': float(acc_train), 'auc_train': float(auc_train),
                       'loss_val': None, 'acc_val': None, 'auc_val': None}
                del loss_input_list, loss_train
                if i > 0:
                    with torch.no_grad():
                        loss_input_list, output_list, _ = self.get_model_res(learning_type, adj_list, x_list, edge_list, node_dist_list,
                                                                             idx_val, model, classifier, fused=bool(fused))
                        loss_val, acc_val, auc_val = loss_model(loss_input_list, label_val)
                    rec.update(loss_val=float(loss_val), acc_val=float(acc_val), auc_val=float(auc_val))
                    if rec['acc_val'] > best_acc:
                        best_acc, self.best_epoch = rec['acc_val'], i + 1
                        if model_path:
                            torch.save(model.state_dict(), model_path)
                        if cls_path:
                            torch.save(classifier.state_dict(), cls_path)
                    del loss_input_list
                self.history.append(rec)
                print('Epoch: ' + str(i + 1), ' '.join('%s: %.4f' % (k, v) for k, v in rec.items() if v is not None),
                      'cost time: {:.4f}s'.format(time.time() - t1))
            if self.best_epoch is not None:     # no checkpoint written: keep the current weights (the reference fails to load)
                if model_path:
                    model.load_state_dict(torch.load(model_path, map_location=self.device))
                if cls_path:
                    classifier.load_state_dict(torch.load(cls_path, map_location=self.device))
            model.eval()
            classifier.eval()
            with torch.no_grad():
                loss_input_list, output_list, _ = self.get_model_res(learning_type, adj_list, x_list, edge_list, node_dist_list, idx_test,
                                                                     model, classifier, fused=bool(fused))
                loss_test, acc_test, auc_test = loss_model(loss_input_list, label_test)
            self.test_result = (float(loss_test), float(acc_test), float(auc_test))
            print('Test set results:', 'loss= {:.4f}'.format(self.test_result[0]), 'accuracy= {:.4f}'.format(self.test_result[1]),
                  'auc= {:.4f}'.format(self.test_result[2]))
        finally:
            if not train_classifier:
                for p in cls_params:
                    p.requires_grad_(True)
        cost_time = time.time() - st
        if export and len(output_list):
            save_embedding([o.detach() for o in output_list] if isinstance(output_list, list) else output_list.detach(),
                           self.timestamp_list, start_idx, self.embedding_base_path, self.full_node_list, sep=self.file_sep)
        del output_list
        torch.cuda.empty_cache()
        print('training total time: ', cost_time, ' seconds!')
        return cost_time
