"""Node-classification evaluation with the reference's interface and file contract (evaluation/node_classification.py), on the GPU.

DataGenerator / NodeClassifier / aggregate_results / node_classification(args) keep the reference's constructor and method signatures,
config keys and file formats: nodecls-data written by either implementation is read by the other.  What runs differently:
  - files are walked in sorted order, the snapshot files and the label files alike (the reference uses os.listdir order, which
    depends on the filesystem); "the first label file", whose labels fix the classes, is the first in sorted order.  Under
    np.random.seed(s) the split files are then identical to the reference's;
  - labels must be exactly the integers 0..K-1 (K >= 2), else ValueError: the reference scores a row as correct when the argmax
    index equals the label value, which is meaningless for other label sets.  A split label outside the classes and a node missing
    from the node file raise ValueError too;
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
from ._ovr import Problem, require_cuda


_device = partial(_common.device, task="node-classification")


def split_counts(node_num, train_ratio, val_ratio, test_ratio):
    """(train_num, val_num, test_num) of a label file with node_num rows, as the reference computes them."""
    return (int(np.floor(node_num * train_ratio)), int(np.floor(node_num * val_ratio)), int(np.floor(node_num * test_ratio)))


def shuffle_split(node_num, train_ratio, val_ratio, test_ratio, rng=np.random):
    """The reference's split of one label file: np.arange(node_num) shuffled by rng.shuffle, then consecutive train, val and test
    slices.  Returns the three index arrays."""
    idx = np.arange(node_num)
    rng.shuffle(idx)
    tr, va, te = split_counts(node_num, train_ratio, val_ratio, test_ratio)
    return idx[:tr], idx[tr:tr + va], idx[tr + va:tr + va + te]


def check_classes(labels):
    """The sorted class values of `labels` (LabelBinarizer's classes_); ValueError unless they are exactly 0..K-1 with K >= 2."""
    classes = np.unique(np.asarray(labels))
    if len(classes) < 2 or not np.issubdtype(classes.dtype, np.integer) or not np.array_equal(classes, np.arange(len(classes))):
        raise ValueError("node labels must be the integers 0..K-1 with K >= 2 (got classes %s): the reference counts a row as correct "
                         "when the predicted class index equals the label value" % (list(classes[:10]),))
    return [int(c) for c in classes]


def _as_split(x, dev, K, what):
    """[n, 2] (node, label) -> (rows, y) CUDA int64 / int32, labels checked against 0..K-1."""
    require_cuda(x, what)
    x = x.to(torch.int64).reshape(-1, 2)
    if x.shape[0] and (int(x[:, 1].min()) < 0 or int(x[:, 1].max()) >= K):
        raise ValueError("%s has a label outside the classes 0..%d" % (what, K - 1))
    return x[:, 0].contiguous(), x[:, 1].to(torch.int32).contiguous()


def _accuracy(correct, n):
    return correct / n if n else float('nan')


def evaluate_batch(E, splits, C_list, K, max_iter=100, tol=1e-6, hess_max=1 << 17):
    """Fit and score many problems at once on one float32 CUDA embedding E [R, d].  splits: one (train, val, test) per problem, each a
    (rows, y) pair of CUDA tensors (rows index E, y in [0, K)).  Returns one dict per problem (see evaluate) and the FitReports."""
    C_list = [float(c) for c in C_list]
    tr = [Problem(s[0][0], s[0][1], K) for s in splits]
    table = _ovr.Table(E, tr, C_list, hess_max=hess_max)
    theta, reports = _ovr.fit(table, tol=tol, max_iter=max_iter)
    out = []
    scored = {}
    for part in (1, 2):
        probs = [Problem(s[part][0], s[part][1], K) for s in splits]
        pred, correct = table.predict(theta, probs)
        scored[part] = (pred, correct.cpu().numpy(), [p.rows.numel() for p in probs])
    G, D1 = len(C_list), E.shape[1] + 1
    mpg = _ovr.models_per_group(K)
    for i in range(len(splits)):
        val_acc = [_accuracy(int(c), scored[1][2][i]) for c in scored[1][1][i]]
        test_acc = [_accuracy(int(c), scored[2][2][i]) for c in scored[2][1][i]]
        idx = select_C(val_acc)
        m0 = int(table.model_start_h[i])
        out.append({"val_acc": val_acc, "test_acc": test_acc, "C": C_list[idx], "C_index": idx % G, "acc": test_acc[idx],
                    "theta": theta[m0:m0 + G * mpg].reshape(G, mpg, D1),
                    "report": [r for r in reports if r.problem == i]})
    offs = {part: np.concatenate([[0], np.cumsum(scored[part][2])]) for part in (1, 2)}
    for i, o in enumerate(out):
        o["val_pred"] = scored[1][0][offs[1][i]:offs[1][i + 1]]
        o["test_pred"] = scored[2][0][offs[2][i]:offs[2][i + 1]]
    return out, reports


def evaluate(embedding, train, val, test, C_list, classes, max_iter=100, tol=1e-6, hess_max=1 << 17):
    """In-memory node classification of one split.  embedding: float32 CUDA [N, d]; train / val / test: [n, 2] int64 CUDA (node index,
    label); classes: the class values (must be 0..K-1) or K.  For every C a one-vs-rest set of balanced logistic regressions is fitted
    on train; the C with the best validation accuracy (the last of ties) is kept and its test accuracy reported.  Returns a dict:
      val_acc, test_acc   accuracy per C on val / test
      C, C_index          the chosen C
      acc                 its test accuracy
      val_pred, test_pred predicted class per row and C (int32 CUDA [n, |C|])
      theta               the fitted parameters (double [|C|, models per C, d+1], w then b)
      report              the solver's FitReport of every model"""
    require_cuda(embedding, "embedding")
    K = classes if isinstance(classes, int) else len(check_classes(classes))
    E = embedding.to(torch.float32).contiguous()
    splits = [tuple(_as_split(x, E.device, K, name) for x, name in ((train, "train"), (val, "val"), (test, "test")))]
    return evaluate_batch(E, splits, C_list, K, max_iter=max_iter, tol=tol, hess_max=hess_max)[0][0]


def evaluate_window(embeddings, labels, C_list, rep_num=10, train_ratio=0.7, val_ratio=0.2, test_ratio=0.1, seed=0, classes=None,
                    max_iter=100, tol=1e-6, hess_max=1 << 17):
    """Node classification over a window, all rep_num x T problems fitted together.  embeddings: CUDA [N, T, d] (as the model returns
    them) or a list of T [N, d]; labels: T pairs (node_idx, label) of 1-D arrays.  Splits are drawn on the host with the reference's
    rule (shuffle of np.arange(n), consecutive slices) from np.random.RandomState(seed), in (rep, snapshot) order.  classes default to
    those of snapshot 0 (the reference's first label file).  Returns a dict: acc [rep, T] (test accuracy at the chosen C), C [rep, T],
    val_acc / test_acc [rep, T, |C|], results (the evaluate() dict of each problem, rep-major), reports."""
    if isinstance(embeddings, torch.Tensor) and embeddings.dim() == 3:
        require_cuda(embeddings, "embeddings")
        N, T, d = embeddings.shape
        E = embeddings.to(torch.float32).permute(1, 0, 2).reshape(T * N, d).contiguous()
    else:
        for e in embeddings:
            require_cuda(e, "embedding")
        T, N = len(embeddings), embeddings[0].shape[0]
        E = torch.cat([e.to(torch.float32) for e in embeddings]).contiguous()
    if len(labels) != T:
        raise ValueError("need one (node_idx, label) pair per snapshot")
    lab = [(np.asarray(a.cpu() if isinstance(a, torch.Tensor) else a, np.int64),
            np.asarray(b.cpu() if isinstance(b, torch.Tensor) else b, np.int64)) for a, b in labels]
    K = len(check_classes(lab[0][1] if classes is None else classes))
    for nodes, y in lab:
        if len(y) and (y.min() < 0 or y.max() >= K):
            raise ValueError("a label lies outside the classes 0..%d" % (K - 1))
        if len(nodes) and (nodes.min() < 0 or nodes.max() >= N):
            raise ValueError("a node index lies outside [0, %d)" % N)
    rng = np.random.RandomState(seed)
    dev = E.device
    host = []
    for _ in range(rep_num):
        for t, (nodes, y) in enumerate(lab):
            host.append([(nodes[ix] + t * N, y[ix]) for ix in shuffle_split(len(nodes), train_ratio, val_ratio, test_ratio, rng)])
    splits = [tuple((torch.from_numpy(r).to(dev), torch.from_numpy(y.astype(np.int32)).to(dev)) for r, y in s) for s in host]
    res, reports = evaluate_batch(E, splits, C_list, K, max_iter=max_iter, tol=tol, hess_max=hess_max)
    shape = (rep_num, T)
    return {"acc": np.array([r["acc"] for r in res]).reshape(shape), "C": np.array([r["C"] for r in res]).reshape(shape),
            "val_acc": np.array([r["val_acc"] for r in res]).reshape(shape + (-1,)),
            "test_acc": np.array([r["test_acc"] for r in res]).reshape(shape + (-1,)), "results": res, "reports": reports}


class DataGenerator(object):
    """Reference DataGenerator: <date>_{train,test,val}.csv (columns node, label) per snapshot file, drawn with the global
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

    def generate_node_samples(self, file_name, sep='\t'):
        date = file_name.split('.')[0]
        df_nodes = pd.read_csv(os.path.join(self.label_base_path, file_name), sep=sep, header=0, names=['node', 'label'])
        missing = [x for x in df_nodes['node'] if x not in self.node2idx_dict]
        if missing:
            raise ValueError("label file %s names %d node(s) missing from the node file, e.g. %r" % (file_name, len(missing), missing[0]))
        node_arr = df_nodes['node'].map(self.node2idx_dict).values
        label_arr = df_nodes['label'].values
        splits = shuffle_split(df_nodes.shape[0], self.train_ratio, self.val_ratio, self.test_ratio)
        for part, ix in zip(('train', 'test', 'val'), (splits[0], splits[2], splits[1])):
            pd.DataFrame({'node': node_arr[ix], 'label': label_arr[ix]}).to_csv(
                os.path.join(self.output_base_path, date + '_' + part + '.csv'), sep=self.file_sep, index=False)

    def generate_node_samples_all_time(self, sep='\t', worker=-1):
        for file_name in sorted(os.listdir(self.input_base_path)):
            self.generate_node_samples(file_name, sep)


class NodeClassifier(object):
    """Reference NodeClassifier: <method>_acc_record.csv (columns date, acc; sep ',') under output_folder.  Every date of a method is
    fitted in one batched solve.  tol: the solver's stopping tolerance on max |∇f|; max_iter caps Newton iterations at
    min(max_iter, 100)."""

    def __init__(self, base_path, origin_folder, embedding_folder, nodeclas_folder, output_folder, node_file, label_folder, file_sep='\t',
                 C_list=None, max_iter=5000, tol=1e-6, device=None):
        self.base_path = base_path
        self.origin_base_path = os.path.abspath(os.path.join(base_path, origin_folder))
        self.embedding_base_path = os.path.abspath(os.path.join(base_path, embedding_folder))
        self.nodecls_base_path = os.path.abspath(os.path.join(base_path, nodeclas_folder))
        self.output_base_path = os.path.abspath(os.path.join(base_path, output_folder))
        self.file_sep = file_sep
        self.full_node_list = read_nodes(os.path.join(base_path, node_file))
        label_base_path = os.path.abspath(os.path.join(base_path, label_folder))
        f_list = sorted(os.listdir(label_base_path))
        assert len(f_list) > 0
        df_label = pd.read_csv(os.path.join(label_base_path, f_list[0]), sep=file_sep)
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
        return pd.read_csv(os.path.join(self.nodecls_base_path, date + '_' + part + '.csv'), sep=self.file_sep).values.astype(np.int64)

    def node_classification_all_time(self, method):
        print('method = ', method)
        dev = _device(self.device)
        K = len(self.classes)

        def read_splits(date):
            return [self._read_split(date, p) for p in ('train', 'val', 'test')]

        dates, embs, splits = [], [], []
        for date, _, cur_embedding_path, parts in method_snapshots(self.origin_base_path, self.embedding_base_path, method, first=read_splits):
            t = len(embs)
            embs.append(torch.from_numpy(read_embedding(cur_embedding_path, self.file_sep, self.full_node_list, np.float32)))
            prob = []
            for name, arr in zip(('train', 'val', 'test'), parts):
                if arr.shape[0] and (arr[:, 1].min() < 0 or arr[:, 1].max() >= K):
                    raise ValueError("%s_%s.csv has a label outside the classes %s" % (date, name, self.classes))
                prob.append((torch.from_numpy(arr[:, 0] + t * len(self.full_node_list)).to(dev),
                             torch.from_numpy(arr[:, 1].astype(np.int32)).to(dev)))
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

    def node_classification_all_method(self, method_list=None, worker=-1):
        if method_list is None:
            method_list = os.listdir(self.embedding_base_path)
        for method in method_list:
            self.node_classification_all_time(method)


def aggregate_results(base_path, nodecls_res_folder, start_idx, rep_num, method_list):
    """Per method: <method>_acc_record.csv under nodecls_res_folder with date, one column acc_<i> per repetition, then avg, max, min."""
    if rep_num <= 0:
        return
    for method in method_list:
        def read(i):
            return pd.read_csv(os.path.join(base_path, nodecls_res_folder + '_' + str(i), method + '_acc_record.csv'), sep=',', header=0,
                               names=['date', 'acc_' + str(i)])
        df_method = read(start_idx)
        for i in range(start_idx + 1, start_idx + rep_num):
            df_method = pd.concat([df_method, read(i).iloc[:, [1]]], axis=1)
        output_base_path = os.path.join(base_path, nodecls_res_folder)
        os.makedirs(output_base_path, exist_ok=True)
        acc_list = ['acc_' + str(i) for i in range(start_idx, start_idx + rep_num)]
        aggregate_stats(df_method, acc_list).to_csv(os.path.join(output_base_path, method + '_acc_record.csv'), sep=',', index=False)


def node_classification(args):
    """The reference's node_cls driver: the same config keys ('worker' ignored; optional 'tol')."""
    base_path = args['base_path']
    start_idx, rep_num = args['start_idx'], args['rep_num']
    t1 = time.time()
    if args['do_nodecls']:
        for i in range(start_idx, start_idx + rep_num):
            print('idx = ', i)
            data_generator = DataGenerator(base_path=base_path, input_folder=args['origin_folder'],
                                           output_folder=args['nodecls_data_folder'] + '_' + str(i), node_file=args['node_file'],
                                           label_folder=args['nlabel_folder'], file_sep=args['file_sep'], train_ratio=args['train_ratio'],
                                           val_ratio=args['val_ratio'], test_ratio=args['test_ratio'])
            if args['generate']:
                data_generator.generate_node_samples_all_time(sep=args['file_sep'])
            node_classifier = NodeClassifier(base_path=base_path, origin_folder=args['origin_folder'], embedding_folder=args['embed_folder'],
                                             nodeclas_folder=args['nodecls_data_folder'] + '_' + str(i),
                                             output_folder=args['nodecls_res_folder'] + '_' + str(i), node_file=args['node_file'],
                                             label_folder=args['nlabel_folder'], file_sep=args['file_sep'], C_list=args['c_list'],
                                             max_iter=args['max_iter'], tol=args.get('tol', 1e-6))
            node_classifier.node_classification_all_method(method_list=args['method_list'])
    print('node classification cost time: ', time.time() - t1, ' seconds!')
    if args['aggregate']:
        aggregate_results(base_path, args['nodecls_res_folder'], start_idx, rep_num, args['method_list'])
