"""Edge-classification evaluation with the reference's interface and file contract (evaluation/edge_classification.py), on the GPU.

DataGenerator / EdgeClassifier / aggregate_results / edge_classification(args) keep the reference's constructor and method signatures,
config keys and file formats: edgecls-data written by either implementation is read by the other.  A row is an edge and its feature
is the Hadamard product E[from] ⊙ E[to]; the kernels form it while they stage a tile (the pair table of _ovr.py), so no
[edges, d] matrix is built.  What runs differently from the reference:
  - files are walked in sorted order, the snapshot files and the label files alike (the reference uses os.listdir order, which
    depends on the filesystem); "the first label file", whose labels fix the classes, is the first in sorted order.  Under
    np.random.seed(s) the split files are then identical to the reference's;
  - the reference's DataGenerator cannot be constructed: its __init__ reads self.node_num before assigning it and raises
    AttributeError.  Ours simply works, and writes what the reference writes once node_num is supplied to it;
  - labels must be exactly the integers 0..K-1 (K >= 2), else ValueError: the reference scores a row as correct when the argmax
    index equals the label value, which is meaningless for other label sets.  A split label outside the classes, an endpoint index
    outside [0, N) and a node missing from the node file raise ValueError too;
  - the |C| x K one-vs-rest models of every date of a method (K = 2: one model per C) are fitted together by the batched Newton
    solver of _ovr.py to tol (default 1e-6 on sklearn's scaled gradient, where the reference's lbfgs stops at 1e-4); max_iter caps
    Newton iterations at min(max_iter, 100).  `worker` is accepted and ignored.
Predictions are the first argmax of fp64 expit(z) over a C's models (K = 2: class 1 iff p > 1 - p) and accuracies are exact counts
over the split size.  evaluate() is the in-memory entry point for one split; evaluate_window() fits rep_num x T problems at once.
"""
import os
import time
from functools import partial

import numpy as np
import pandas as pd
import torch

from . import _common, _ovr
from ._common import aggregate_stats, method_snapshots, read_embedding, read_nodes, select_C
from ._ovr import Problem
from .node_classification import _accuracy, check_classes, shuffle_split, split_counts  # noqa: F401

TASK = "edge-classification"
_device = partial(_common.device, task=TASK)
require_cuda = partial(_common.require_cuda, task=TASK)


def _check_split(arr, K, N, what):
    """arr: [n, 3] (from, to, label), numpy or tensor; ValueError for a label outside 0..K-1 or an endpoint outside [0, N)."""
    if arr.shape[0] == 0:
        return
    if int(arr[:, 2].min()) < 0 or int(arr[:, 2].max()) >= K:
        raise ValueError("%s has a label outside the classes 0..%d" % (what, K - 1))
    if int(arr[:, :2].min()) < 0 or int(arr[:, :2].max()) >= N:
        raise ValueError("%s has an endpoint index outside [0, %d)" % (what, N))


def _as_split(x, K, N, what):
    """[n, 3] (from, to, label) CUDA -> (from, to, y) int64 / int64 / int32, checked."""
    require_cuda(x, what)
    x = x.to(torch.int64).reshape(-1, 3)
    _check_split(x, K, N, what)
    return x[:, 0].contiguous(), x[:, 1].contiguous(), x[:, 2].to(torch.int32).contiguous()


def evaluate_batch(E, splits, C_list, K, max_iter=100, tol=1e-6, hess_max=1 << 17):
    """Fit and score many problems at once on one float32 CUDA embedding E [R, d].  splits: one (train, val, test) per problem, each a
    (from, to, y) triple of CUDA tensors (from / to index E, y in [0, K)).  Returns one dict per problem (see evaluate) and the
    FitReports."""
    C_list = [float(c) for c in C_list]
    require_cuda(E, "embedding")
    for s in splits:
        for part in s:
            for x in part:
                require_cuda(x, "split")
    table = _ovr.Table(E, [Problem(s[0][0], s[0][2], K, rows2=s[0][1]) for s in splits], C_list, hess_max=hess_max)
    theta, reports = _ovr.fit(table, tol=tol, max_iter=max_iter)
    scored = {}
    for part in (1, 2):
        probs = [Problem(s[part][0], s[part][2], K, rows2=s[part][1]) for s in splits]
        pred, correct = table.predict(theta, probs)
        scored[part] = (pred, correct.cpu().numpy(), [p.rows.numel() for p in probs])
    G, D1 = len(C_list), E.shape[1] + 1
    mpg = _ovr.models_per_group(K)
    offs = {part: np.concatenate([[0], np.cumsum(scored[part][2])]) for part in (1, 2)}
    out = []
    for i in range(len(splits)):
        val_acc = [_accuracy(int(c), scored[1][2][i]) for c in scored[1][1][i]]
        test_acc = [_accuracy(int(c), scored[2][2][i]) for c in scored[2][1][i]]
        idx = select_C(val_acc)
        m0 = int(table.model_start_h[i])
        out.append({"val_acc": val_acc, "test_acc": test_acc, "C": C_list[idx], "C_index": idx % G, "acc": test_acc[idx],
                    "theta": theta[m0:m0 + G * mpg].reshape(G, mpg, D1),
                    "report": [r for r in reports if r.problem == i],
                    "val_pred": scored[1][0][offs[1][i]:offs[1][i + 1]], "test_pred": scored[2][0][offs[2][i]:offs[2][i + 1]]})
    return out, reports


def evaluate(embedding, train, val, test, C_list, classes, max_iter=100, tol=1e-6, hess_max=1 << 17):
    """In-memory edge classification of one split.  embedding: float32 CUDA [N, d]; train / val / test: [n, 3] int64 CUDA (from index,
    to index, label); classes: the class values (must be 0..K-1) or K.  For every C a one-vs-rest set of balanced logistic regressions
    is fitted on the features E[from] ⊙ E[to] of train; the C with the best validation accuracy (the last of ties) is kept and its
    test accuracy reported.  Returns the dict of node_classification.evaluate: val_acc, test_acc, C, C_index, acc, val_pred,
    test_pred, theta, report."""
    require_cuda(embedding, "embedding")
    K = classes if isinstance(classes, int) else len(check_classes(classes))
    E = embedding.to(torch.float32).contiguous()
    splits = [tuple(_as_split(x, K, E.shape[0], name) for x, name in ((train, "train"), (val, "val"), (test, "test")))]
    return evaluate_batch(E, splits, C_list, K, max_iter=max_iter, tol=tol, hess_max=hess_max)[0][0]


def evaluate_window(embeddings, edge_labels, C_list, rep_num=10, train_ratio=0.7, val_ratio=0.2, test_ratio=0.1, seed=0, classes=None,
                    max_iter=100, tol=1e-6, hess_max=1 << 17):
    """Edge classification over a window, all rep_num x T problems fitted together.  embeddings: CUDA [N, T, d] (as the model returns
    them) or a list of T [N, d]; edge_labels: T triples (from_idx, to_idx, label) of 1-D arrays.  Splits are drawn on the host with
    the reference's rule (shuffle of np.arange(n), consecutive slices) from np.random.RandomState(seed), in (rep, snapshot) order.
    classes default to those of snapshot 0 (the reference's first label file).  Returns a dict: acc [rep, T] (test accuracy at the
    chosen C), C [rep, T], val_acc / test_acc [rep, T, |C|], results (the evaluate() dict of each problem, rep-major), reports."""
    if isinstance(embeddings, torch.Tensor) and embeddings.dim() == 3:
        require_cuda(embeddings, "embeddings")
        N, T, d = embeddings.shape
        E = embeddings.to(torch.float32).permute(1, 0, 2).reshape(T * N, d).contiguous()
    else:
        for e in embeddings:
            require_cuda(e, "embedding")
        T, N = len(embeddings), embeddings[0].shape[0]
        E = torch.cat([e.to(torch.float32) for e in embeddings]).contiguous()
    if len(edge_labels) != T:
        raise ValueError("need one (from_idx, to_idx, label) triple per snapshot")
    lab = [np.stack([np.asarray(a.cpu() if isinstance(a, torch.Tensor) else a, np.int64).reshape(-1) for a in trip], 1)
           for trip in edge_labels]
    K = len(check_classes(lab[0][:, 2] if classes is None else classes))
    for t, arr in enumerate(lab):
        _check_split(arr, K, N, "snapshot %d" % t)
    rng = np.random.RandomState(seed)
    dev = E.device
    splits = []
    for _ in range(rep_num):
        for t, arr in enumerate(lab):
            splits.append(tuple((torch.from_numpy(arr[ix, 0] + t * N).to(dev), torch.from_numpy(arr[ix, 1] + t * N).to(dev),
                                 torch.from_numpy(arr[ix, 2].astype(np.int32)).to(dev))
                                for ix in shuffle_split(arr.shape[0], train_ratio, val_ratio, test_ratio, rng)))
    res, reports = evaluate_batch(E, splits, C_list, K, max_iter=max_iter, tol=tol, hess_max=hess_max)
    shape = (rep_num, T)
    return {"acc": np.array([r["acc"] for r in res]).reshape(shape), "C": np.array([r["C"] for r in res]).reshape(shape),
            "val_acc": np.array([r["val_acc"] for r in res]).reshape(shape + (-1,)),
            "test_acc": np.array([r["test_acc"] for r in res]).reshape(shape + (-1,)), "results": res, "reports": reports}


class DataGenerator(object):
    """Reference DataGenerator: <date>_{train,val,test}.csv (columns from_id, to_id, label) per snapshot file, drawn with the global
    np.random.shuffle, snapshot files in sorted order."""

    def __init__(self, base_path, input_folder, output_folder, node_file, label_folder, file_sep='\t', train_ratio=0.7, val_ratio=0.2,
                 test_ratio=0.1):
        self.base_path = base_path
        self.input_base_path = os.path.abspath(os.path.join(base_path, input_folder))
        self.output_base_path = os.path.abspath(os.path.join(base_path, output_folder))
        self.label_base_path = os.path.abspath(os.path.join(base_path, label_folder))
        self.file_sep = file_sep
        self.full_node_list = read_nodes(os.path.join(base_path, node_file))
        self.node_num = len(self.full_node_list)
        self.node2idx_dict = dict(zip(self.full_node_list, np.arange(self.node_num)))
        assert train_ratio + test_ratio + val_ratio <= 1.0
        self.train_ratio, self.val_ratio, self.test_ratio = train_ratio, val_ratio, test_ratio
        os.makedirs(self.input_base_path, exist_ok=True)
        os.makedirs(self.output_base_path, exist_ok=True)

    def generate_edge_samples(self, file_name, sep='\t'):
        date = file_name.split('.')[0]
        df_edges = pd.read_csv(os.path.join(self.label_base_path, file_name), sep=sep, header=0, names=['from_id', 'to_id', 'label'])
        missing = [x for col in ('from_id', 'to_id') for x in df_edges[col] if x not in self.node2idx_dict]
        if missing:
            raise ValueError("label file %s names %d node(s) missing from the node file, e.g. %r" % (file_name, len(missing), missing[0]))
        edge_arr = np.stack([df_edges[col].map(self.node2idx_dict).values for col in ('from_id', 'to_id')], 1).reshape(-1, 2)
        label_arr = df_edges['label'].values
        splits = shuffle_split(df_edges.shape[0], self.train_ratio, self.val_ratio, self.test_ratio)
        for part, ix in zip(('train', 'val', 'test'), splits):
            pd.DataFrame({'from_id': edge_arr[ix, 0], 'to_id': edge_arr[ix, 1], 'label': label_arr[ix]}).to_csv(
                os.path.join(self.output_base_path, date + '_' + part + '.csv'), sep=self.file_sep, index=False)

    def generate_edge_samples_all_time(self, sep='\t', worker=-1):
        for file_name in sorted(os.listdir(self.input_base_path)):
            self.generate_edge_samples(file_name, sep)


class EdgeClassifier(object):
    """Reference EdgeClassifier: <method>_acc_record.csv (columns date, acc; sep ',') under output_folder.  Every date of a method is
    fitted in one batched solve.  tol: the solver's stopping tolerance on max |∇f|; max_iter caps Newton iterations at
    min(max_iter, 100)."""

    def __init__(self, base_path, origin_folder, embedding_folder, edgeclas_folder, output_folder, node_file, label_folder, file_sep='\t',
                 C_list=None, max_iter=5000, tol=1e-6, device=None):
        self.base_path = base_path
        self.origin_base_path = os.path.abspath(os.path.join(base_path, origin_folder))
        self.embedding_base_path = os.path.abspath(os.path.join(base_path, embedding_folder))
        self.edgeclas_base_path = os.path.abspath(os.path.join(base_path, edgeclas_folder))
        self.output_base_path = os.path.abspath(os.path.join(base_path, output_folder))
        self.file_sep = file_sep
        self.full_node_list = read_nodes(os.path.join(base_path, node_file))
        self.label_base_path = os.path.abspath(os.path.join(base_path, label_folder))
        f_list = sorted(os.listdir(self.label_base_path))
        assert len(f_list) > 0
        df_label = pd.read_csv(os.path.join(self.label_base_path, f_list[0]), sep=file_sep)
        self.unique_labels = df_label['label'].unique()
        self.classes = check_classes(self.unique_labels)
        self.C_list = C_list
        self.max_iter = max_iter
        self.tol = tol
        self.device = device
        self.reports = {}
        for p in (self.embedding_base_path, self.origin_base_path, self.output_base_path):
            os.makedirs(p, exist_ok=True)

    def _read_split(self, date, part):
        return pd.read_csv(os.path.join(self.edgeclas_base_path, date + '_' + part + '.csv'), sep=self.file_sep).values.astype(np.int64)

    def edge_classification_all_time(self, method):
        print('method = ', method)
        dev = _device(self.device)
        K, N = len(self.classes), len(self.full_node_list)

        def read_splits(date):
            return [self._read_split(date, p) for p in ('train', 'val', 'test')]

        dates, embs, splits = [], [], []
        for date, _, cur_embedding_path, parts in method_snapshots(self.origin_base_path, self.embedding_base_path, method, first=read_splits):
            t = len(embs)
            embs.append(torch.from_numpy(read_embedding(cur_embedding_path, self.file_sep, self.full_node_list, np.float32)))
            prob = []
            for name, arr in zip(('train', 'val', 'test'), parts):
                arr = arr.reshape(-1, 3)
                _check_split(arr, K, N, "%s_%s.csv" % (date, name))
                prob.append((torch.from_numpy(arr[:, 0] + t * N).to(dev), torch.from_numpy(arr[:, 1] + t * N).to(dev),
                             torch.from_numpy(arr[:, 2].astype(np.int32)).to(dev)))
            dates.append(date)
            splits.append(tuple(prob))
        rows = []
        if dates:
            E = torch.cat(embs).to(dev).contiguous()
            res, _ = evaluate_batch(E, splits, self.C_list, K, max_iter=min(self.max_iter, 100), tol=self.tol)
            for date, r in zip(dates, res):
                self.reports[(method, date)] = r
                rows.append([date, r["acc"]])
        df_output = pd.DataFrame(rows, columns=['date', 'acc'])
        print(df_output)
        print('method = ', method, ', average accuracy: ', df_output['acc'].mean())
        df_output.to_csv(os.path.join(self.output_base_path, method + '_acc_record.csv'), sep=',', index=False)

    def edge_classification_all_method(self, method_list=None, worker=-1):
        if method_list is None:
            method_list = os.listdir(self.embedding_base_path)
        for method in method_list:
            self.edge_classification_all_time(method)


def aggregate_results(base_path, edgecls_res_folder, start_idx, rep_num, method_list):
    """Per method: <method>_acc_record.csv under edgecls_res_folder with date, one column acc_<i> per repetition, then avg, max, min."""
    if rep_num <= 0:
        return
    for method in method_list:
        def read(i):
            return pd.read_csv(os.path.join(base_path, edgecls_res_folder + '_' + str(i), method + '_acc_record.csv'), sep=',', header=0,
                               names=['date', 'acc_' + str(i)])
        df_method = read(start_idx)
        for i in range(start_idx + 1, start_idx + rep_num):
            df_method = pd.concat([df_method, read(i).iloc[:, [1]]], axis=1)
        output_base_path = os.path.join(base_path, edgecls_res_folder)
        os.makedirs(output_base_path, exist_ok=True)
        acc_list = ['acc_' + str(i) for i in range(start_idx, start_idx + rep_num)]
        aggregate_stats(df_method, acc_list).to_csv(os.path.join(output_base_path, method + '_acc_record.csv'), sep=',', index=False)


def edge_classification(args):
    """The reference's edge_cls driver: the same config keys ('worker' ignored; optional 'tol')."""
    base_path = args['base_path']
    start_idx, rep_num = args['start_idx'], args['rep_num']
    t1 = time.time()
    if args['do_edgecls']:
        for i in range(start_idx, start_idx + rep_num):
            print('idx = ', i)
            data_generator = DataGenerator(base_path=base_path, input_folder=args['origin_folder'],
                                           output_folder=args['edgecls_data_folder'] + '_' + str(i), node_file=args['node_file'],
                                           label_folder=args['elabel_folder'], file_sep=args['file_sep'], train_ratio=args['train_ratio'],
                                           val_ratio=args['val_ratio'], test_ratio=args['test_ratio'])
            if args['generate']:
                data_generator.generate_edge_samples_all_time(sep=args['file_sep'])
            edge_classifier = EdgeClassifier(base_path=base_path, origin_folder=args['origin_folder'], embedding_folder=args['embed_folder'],
                                             edgeclas_folder=args['edgecls_data_folder'] + '_' + str(i),
                                             output_folder=args['edgecls_res_folder'] + '_' + str(i), node_file=args['node_file'],
                                             label_folder=args['elabel_folder'], file_sep=args['file_sep'], C_list=args['c_list'],
                                             max_iter=args['max_iter'], tol=args.get('tol', 1e-6))
            edge_classifier.edge_classification_all_method(method_list=args['method_list'])
    print('edge classification cost time: ', time.time() - t1, ' seconds!')
    if args['aggregate']:
        aggregate_results(base_path, args['edgecls_res_folder'], start_idx, rep_num, args['method_list'])
